"""CPU: running reward scaling (PPO --normalize_reward) without a GPU -- the numpy reference against exact
rational arithmetic, the scan's affine-composition rule against the sequential walk, the refusals of the two entry points that
return before any HIP call, the option table, the weights file's reward_rms.* and the state file's presence rule."""
import ctypes as C
import fractions
import os
import types

import numpy as np
import pytest
import torch

from fly_bproject_amd import options, train_state
from tests import reward_norm_cases as cases
from tests import reward_norm_ref as R


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    """g = 0.5 and dyadic rewards: every op is exact.  Env 0 ends at t = 1 and comes in with 8; env 1 never ends."""
    reward = np.array([[1, 2], [2, 0], [4, 1], [-8, 0.5]], dtype=np.float32)
    reset = np.array([[0, 0], [7, 0], [0, 0], [0, 0]], dtype=np.int64)
    w = R.walk(reward, reset, 0.5, carry=[8.0, 0.0])
    assert w.G.tolist() == [[5.0, 2.0], [4.5, 1.0], [4.0, 1.5], [-6.0, 1.25]]       # the end row's G counts, then G = 0
    assert w.carry.tolist() == [-6.0, 1.25]
    assert w.mag.tolist() == [[5.0, 2.0], [4.5, 1.0], [4.0, 1.5], [10.0, 1.25]]
    assert w.smax.tolist() == [10.0, 2.0]
    assert R.moments(w.G) == (8.0, 1.65625, float(np.mean((w.G - 1.65625) ** 2)))
    tab = R.table((8.0, 0.0, 4.0 - 1e-5))
    assert tab.tolist() == [0.0, 2.0, 0.5, 0.0]
    x = np.array([1.0, -30.0, np.nan, np.inf, -np.inf, 0.0], dtype=np.float32)
    out = R.scale(x, tab[2], 10.0)
    assert out.dtype == np.float32 and out[[0, 1, 3, 4, 5]].tolist() == [0.5, -10.0, 10.0, -10.0, 0.0] and np.isnan(out[2])
    assert R.discount(0.99) == np.float64(np.float32(0.99)) != 0.99


@pytest.mark.parametrize("gamma", [0.99, 0.5])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_reference_against_exact_fractions(gamma, seed):
    """The sequential float64 walk against fractions.Fraction: every G within its first-order bound 2 u / (1 - g) max M, and
    every carry under a TENTH of the scan bound (so the bound is the scan's to use, not the reference's)."""
    T, N = 37, 7
    reward, reset, cin = cases.case(T, N, seed, carry=bool(seed & 1), huge=False, lanes=4)
    w = R.walk(reward, reset, gamma, cin)
    exact, exact_carry = R.exact_walk(reward, reset, gamma, cin)
    g = float(R.discount(gamma))
    worst = 0.0
    for e in range(N):
        for t in range(T):
            err = abs(fractions.Fraction(float(w.G[t, e])) - exact[t][e])
            assert err <= 1.001 * 2 * R.U / (1 - g) * max(w.mag[:t + 1, e].max(), abs(cin[e]))
        err = float(abs(fractions.Fraction(float(w.carry[e])) - exact_carry[e]))
        bound = float(R.scan_bound(gamma, w.smax[e]))
        assert err <= bound / 10, (e, err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    print("reward_norm reference vs exact: worst carry |error| / scan bound %.3g (gamma %g, seed %d)" % (worst, gamma, seed))
    ended_last = reset[T - 1] != 0
    assert (w.carry[ended_last] == 0).all() and (w.smax[ended_last] == 0).all()


def test_exact_inputs_are_reproduced_exactly():
    """g = 0.5, small dyadic rewards, short episodes: no rounding anywhere, so walk, scan and fractions agree exactly."""
    rng = np.random.default_rng(0)
    T, N = 20, 5
    reward = (rng.integers(-8, 9, (T, N)) / 4).astype(np.float32)
    reset = (rng.random((T, N)) < 0.2).astype(np.int64)
    w = R.walk(reward, reset, 0.5)
    exact, exact_carry = R.exact_walk(reward, reset, 0.5)
    assert all(fractions.Fraction(float(w.G[t, e])) == exact[t][e] for t in range(T) for e in range(N))
    G, carry = R.scan_walk(reward, reset, 0.5, lanes=4)
    assert np.array_equal(G, w.G) and np.array_equal(carry, w.carry)
    assert [fractions.Fraction(float(c)) for c in carry] == exact_carry


# ---- the scan's composition rule ----------------------------------------------------------------------------------------------------
def test_composition_is_associative_and_has_an_identity():
    rng = np.random.default_rng(1)
    for _ in range(200):
        m = [(fractions.Fraction(int(a), 8) * int(k), fractions.Fraction(int(b), 16))
             for a, b, k in zip(rng.integers(1, 8, 3), rng.integers(-50, 50, 3), rng.integers(0, 2, 3))]   # a = 0: an end

        def comp(p, q):
            return p[0] * q[0], q[0] * p[1] + q[1]
        assert comp(comp(m[0], m[1]), m[2]) == comp(m[0], comp(m[1], m[2]))
        one = (fractions.Fraction(1), fractions.Fraction(0))
        assert comp(one, m[0]) == m[0] == comp(m[0], one)
        x = fractions.Fraction(int(rng.integers(-9, 9)), 4)
        first = m[0][0] * x + m[0][1]
        assert comp(m[0], m[1])[0] * x + comp(m[0], m[1])[1] == m[1][0] * first + m[1][1]       # composing = applying in turn


@pytest.mark.parametrize("gamma", [0.99, 0.5])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129, 200])
def test_scan_rule_against_the_sequential_walk(T, gamma):
    """The scan restated in numpy (64 chunks, Kogge-Stone, second walk) against the walk: ends on chunk boundaries, at t = 0,
    at t = T - 1, on consecutive rows, in every row and nowhere (the six patterns, each on a column of its own), zero and
    non-zero carry-in.  Carries within the documented bound, G row by row within the same bound on the row's own S."""
    N = 8
    worst = 0.0
    for seed, carry in ((T, False), (T + 1, True)):
        reward, reset, cin = cases.case(T, N, seed, carry=carry)
        reset[:, 6:] = 0
        reset[::3, 7] = 1
        w = R.walk(reward, reset, gamma, cin)
        G, out = R.scan_walk(reward, reset, gamma, cin)
        bound = R.scan_bound(gamma, w.smax)
        err = np.abs(out - w.carry)
        assert (err <= bound).all(), (err, bound)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        # every G: its S is the running maximum of M inside the row's open episode, at most the maximum up to the row
        run = np.maximum.accumulate(np.maximum(w.mag, np.abs(cin)[None]), axis=0)
        assert (np.abs(G - w.G) <= R.scan_bound(gamma, run)).all()
        every = [k for k in range(6) if cases.PATTERNS[(seed + k) % 6] == "every"]
        first = 1 if carry else 0                           # (row 0 holds the carry-in too)
        assert every and all(out[k] == 0.0 and np.array_equal(G[first:, k], reward[first:, k].astype(np.float64)) for k in every)
    print("reward_norm scan rule vs walk: worst |error| / bound %.3g (T %d, gamma %g)" % (worst, T, gamma))


def test_scan_rule_keeps_a_nan_behind_its_end():
    T, N = 130, 3
    reward, reset, cin = cases.case(T, N, 11, carry=True)
    reset[:] = 0
    reward[5, 0] = np.nan                                   # env 0: an end later on, in another chunk
    reset[40, 0] = 1
    reward[50, 1] = np.inf                                  # env 1: no end behind it
    w = R.walk(reward, reset, 0.99, cin)
    G, out = R.scan_walk(reward, reset, 0.99, cin)
    assert np.isfinite(w.carry[0]) and np.isfinite(out[0]) and abs(out[0] - w.carry[0]) <= R.scan_bound(0.99, w.smax[0])
    assert np.array_equal(np.isnan(G), np.isnan(w.G)) and np.isnan(G[5:41, 0]).all() and not np.isnan(G[41:, 0]).any()
    assert out[1] == w.carry[1] == np.inf and np.isfinite(out[2])


def test_the_bound_has_the_documented_terms():
    for gamma in (0.99, 0.5):
        g = float(np.float32(gamma))
        assert R.scan_c(gamma) == 4 / (1 - g) + g / (1 - g) + 1 / (np.e * np.log(1 / g)) + 80
    assert 615 < R.scan_c(0.99) < 616 and 89 < R.scan_c(0.5) < 90
    assert R.scan_bound(0.99, 0.0) == 0.0


# ---- the entry points' refusals (they return before any HIP call) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    _lib.build()
    return _lib.load()


def test_returns_refusals(lib):
    f = lib.ppo_reward_returns
    r, rs, ci, co, sets = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    good = (r, rs, 0.99, 8, 64, ci, co, sets, 0, None)
    for i in (0, 1, 5, 6, 7):
        args = list(good)
        args[i] = None
        assert f(*args) == -1 and b"null pointer" in lib.fly_last_error(), i
    for T, N in ((0, 64), (-1, 64), (8, 0), (8, -5)):
        assert f(r, rs, 0.99, T, N, ci, co, sets, 0, None) == -1 and b"T and N must be > 0" in lib.fly_last_error()
    for mode in (1, 2, 3, 5, 8, -1):
        assert f(r, rs, 0.99, 8, 64, ci, co, sets, mode, None) == -1 and b"mode_flags must be 0 or PPO_GAE_SCAN" in lib.fly_last_error()
    assert f(r, rs, 0.99, 1 << 40, 1 << 40, ci, co, sets, 0, None) == -1 and b"overflow" in lib.fly_last_error()
    assert f(r + 2, rs, 0.99, 8, 64, ci, co, sets, 0, None) == -1 and b"4-byte aligned" in lib.fly_last_error()
    for i in (1, 5, 6, 7):
        args = list(good)
        args[i] += 4
        assert f(*args) == -1 and b"8-byte aligned" in lib.fly_last_error(), i
    for other in (ci + 8, ci - 8, ci + 8 * 63):
        assert f(r, rs, 0.99, 8, 64, ci, other, sets, 0, None) == -1 and b"carry_out must be carry_in or not overlap" in lib.fly_last_error()


def test_scale_refusals(lib):
    f = lib.ppo_reward_scale
    r, tab, out = 0x10000, 0x20000, 0x30000
    for args in ((None, 4, tab, 10.0, out, None), (r, 4, None, 10.0, out, None), (r, 4, tab, 10.0, None, None)):
        assert f(*args) == -1 and b"null pointer" in lib.fly_last_error()
    for n in (0, -3):
        assert f(r, n, tab, 10.0, out, None) == -1 and b"n must be > 0" in lib.fly_last_error()
    for clip in (0.0, -1.0, float("nan")):
        assert f(r, 4, tab, clip, out, None) == -1 and b"clip must be > 0" in lib.fly_last_error()
    for args in ((r + 2, 4, tab, 10.0, out, None), (r, 4, tab + 1, 10.0, out, None), (r, 4, tab, 10.0, out + 3, None)):
        assert f(*args) == -1 and b"4-byte aligned" in lib.fly_last_error()
    for other in (r + 4, r - 4, r + 12):
        assert f(r, 4, tab, 10.0, other, None) == -1 and b"must be the reward buffer or not overlap" in lib.fly_last_error()


def test_extension_header_and_its_binding_table(lib, monkeypatch):
    """include/flyhip_ext.h (which flyhip.h includes at its end) against _lib.SYMBOLS_EXT, as tests/test_abi_cpu.py holds
    flyhip.h against _lib.SYMBOLS: the same names, per parameter the ctypes type its C type binds to, the declared restype after
    load(), one checked callable each on ext() -- and nothing of it in SYMBOLS or on api(), whose version stays 13."""
    from fly_bproject_amd import _lib
    from tests import abi_header
    main = open(abi_header.HEADER).read()
    assert main.count('#include "flyhip_ext.h"') == 1 and "ppo_reward_" not in abi_header.header_text()
    monkeypatch.setattr(abi_header, "HEADER", os.path.join(abi_header.REPO, "include", "flyhip_ext.h"))
    protos = abi_header.prototypes()
    assert protos == {
        "ppo_reward_returns": ("int", ["const float*", "const int64_t*", "float", "int64_t", "int64_t", "const double*", "double*",
                                       "double*", "int", "void*"]),
        "ppo_reward_scale": ("int", ["const float*", "int64_t", "const float*", "float", "float*", "void*"])}
    assert set(protos) == set(_lib.SYMBOLS_EXT) and not set(protos) & set(_lib.SYMBOLS)
    for name, (ret, params) in protos.items():
        want = [abi_header.ctype_of(t, {}) for t in params]
        fn = getattr(lib, name)
        assert _lib.SYMBOLS_EXT[name] == want == list(fn.argtypes) and fn.restype is abi_header.RETURNS[ret], name
    ext = _lib.ext()
    assert ext is _lib.ext() and set(vars(ext)) == set(_lib.SYMBOLS_EXT) and not set(vars(ext)) & set(vars(_lib.api()))
    with pytest.raises(_lib.FlyHipError, match=r"ppo_reward_scale failed \(-1\): ppo_reward_scale: null pointer"):
        ext.ppo_reward_scale(None, 4, None, 10.0, None, None)
    assert _lib.ABI_VERSION == 13 == lib.fly_abi_version()  # no existing argument list changed


# ---- option, flag, weights file, state file -----------------------------------------------------------------------------------------------
def ns(**kw):
    return types.SimpleNamespace(**dict(dict(num_envs=1000), **kw))


def test_option_table_and_flags():
    import trainer
    on, clip = options.BY_NAME["normalize_reward"], options.BY_NAME["reward_clip"]
    assert (on.default, on.choices, on.env) == (False, None, None) and (clip.default, clip.choices, clip.env) == (10.0, None, None)
    a = trainer.parse_args([])
    assert a.normalize_reward is False and a.reward_clip == 10.0
    a = trainer.parse_args(["--normalize_reward", "--reward_clip", "2.5"])
    assert a.normalize_reward is True and a.reward_clip == 2.5
    rec = options.resolve(a, os.environ)
    assert rec.normalize_reward is True and rec.reward_clip == 2.5 and type(rec.reward_clip) is float
    rec = options.resolve(ns(), os.environ)
    assert rec.normalize_reward is False and rec.reward_clip == 10.0
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="reward_clip must be > 0"):
            options.resolve(ns(normalize_reward=True, reward_clip=bad), os.environ)
        options.resolve(ns(reward_clip=bad), os.environ)    # the clip means nothing without the flag
    assert "--normalize_reward" in trainer.__doc__ and "--reward_clip" in trainer.__doc__


def test_the_meta_blocks_do_not_name_the_options():
    for args in (ns(), ns(normalize_reward=True, reward_clip=3.0)):
        rec = options.resolve(args, os.environ)
        for block in (options.projection(rec), train_state.expected_meta(args), train_state.expected_meta_ext(args)):
            assert "normalize_reward" not in block and "reward_clip" not in block
    assert train_state.expected_meta(ns()) == train_state.expected_meta(ns(normalize_reward=True, reward_clip=3.0))
    assert train_state.expected_meta_ext(ns(normalize_reward=True)) == {"lambda_returns": False}
    assert train_state.FORMAT == 1 and train_state.META_EXT_FIELDS == ("lambda_returns",) and len(train_state.META_FIELDS) == 22


def test_a_bad_clip_is_refused_before_the_env(monkeypatch):
    from fly_bproject_amd import ppo

    def no_env(args):
        raise AssertionError("the env was built before the argument was validated")
    monkeypatch.setattr(ppo, "Fly", no_env)
    with pytest.raises(ValueError, match="reward_clip must be > 0"):
        ppo.PPO(ns(normalize_reward=True, reward_clip=0.0))
    with pytest.raises(AssertionError, match="before the argument"):
        ppo.PPO(ns(normalize_reward=True, reward_clip=0.5))


def _rms(prefix):
    return {prefix + ".mean": torch.zeros((), dtype=torch.float64), prefix + ".var": torch.ones((), dtype=torch.float64),
            prefix + ".count": torch.zeros((), dtype=torch.float64)}


def test_split_rms_for_the_reward_statistics():
    """The four combinations of (the file holds reward_rms.*, the flag is on), and an incomplete set."""
    from fly_bproject_amd import ppo
    assert ppo.REWARD_RMS_KEYS == ("reward_rms.mean", "reward_rms.var", "reward_rms.count")
    net = {"fc1.weight": torch.zeros(2, 2)}
    sd = dict(net, **_rms("reward_rms"))
    got = ppo.split_reward_rms(sd, True)                                            # holds them, flag on: split off
    assert sorted(got) == sorted(ppo.REWARD_RMS_KEYS) and list(sd) == ["fc1.weight"]
    sd = dict(net, **_rms("reward_rms"))
    with pytest.raises(ValueError, match=r"trained with reward normalisation .*run with --normalize_reward"):
        ppo.split_reward_rms(sd, False)                                             # holds them, flag off: refused
    for on in (True, False):                                                        # a reference checkpoint: nothing, either way
        sd = dict(net)
        assert ppo.split_reward_rms(sd, on) == {} and list(sd) == ["fc1.weight"]
    sd = dict(net, **_rms("reward_rms"))
    del sd["reward_rms.var"]
    with pytest.raises(ValueError, match="incomplete reward statistics"):
        ppo.split_reward_rms(sd, True)
    # the three families do not see each other's keys
    sd = dict(net, **_rms("reward_rms"), **_rms("value_rms"))
    assert sorted(ppo.split_value_rms(sd, True)) == sorted(ppo.VALUE_RMS_KEYS) and "reward_rms.var" in sd
    assert sorted(ppo.split_reward_rms(sd, True)) == sorted(ppo.REWARD_RMS_KEYS) and list(sd) == ["fc1.weight"]


def _block():
    return {"stats": torch.tensor([8.0, 0.5, 2.0], dtype=torch.float64), "table": torch.zeros(4),
            "stats_next": torch.tensor([8.0, 0.5, 2.0], dtype=torch.float64), "table_next": torch.zeros(4),
            "carry": torch.zeros(1000, dtype=torch.float64), "carry_next": torch.zeros(1000, dtype=torch.float64)}


def _state(args, with_block):
    agent = {"run_step": 160, "optim_step": 75}
    if with_block:
        agent["reward_norm"] = _block()
    return {"format": train_state.FORMAT, "meta": train_state.expected_meta(args), "meta_ext": train_state.expected_meta_ext(args),
            "policy": {}, "agent": agent, "env": {}}


def test_state_block_presence_rule():
    assert train_state.REWARD_NORM_KEYS == ("stats", "table", "stats_next", "table_next", "carry", "carry_next")
    train_state.check_reward_norm(_state(ns(), True), True)
    train_state.check_reward_norm(_state(ns(), False), False)
    with pytest.raises(ValueError, match=r"saved with normalize_reward .*run with --normalize_reward"):
        train_state.check_reward_norm(_state(ns(), True), False)
    with pytest.raises(ValueError, match=r"saved without normalize_reward .*run without --normalize_reward"):
        train_state.check_reward_norm(_state(ns(), False), True)
    bad = _state(ns(), True)
    bad["agent"]["reward_norm"] = torch.zeros(3)
    with pytest.raises(ValueError, match="agent.reward_norm is no block"):
        train_state.check_reward_norm(bad, True)


@pytest.mark.parametrize("saved_with,run_with", [(True, False), (False, True), (True, True), (False, False)])
def test_resume_checks_the_block_before_the_env(tmp_path, monkeypatch, saved_with, run_with):
    """Files built by hand, through PPO.__init__: a mismatch is a ValueError raised where check_meta runs, before an env exists;
    a match (with another reward_clip) gets as far as the env."""
    from fly_bproject_amd import ppo
    for k in ("FLY_GEMM", "FLY_STEP_GEMM", "FLY_PERSISTENT_ROLLOUT"):
        monkeypatch.delenv(k, raising=False)

    def no_env(args):
        raise AssertionError("as far as the env")
    monkeypatch.setattr(ppo, "Fly", no_env)
    weights = str(tmp_path / "w_75.pth")
    torch.save(_state(ns(normalize_reward=saved_with), saved_with), train_state.training_state_path(weights, 0))
    args = ns(resume=True, resume_path=weights, normalize_reward=run_with, reward_clip=3.0)
    if saved_with == run_with:
        with pytest.raises(AssertionError, match="as far as the env"):
            ppo.PPO(args)
    else:
        with pytest.raises(ValueError, match="saved with%s normalize_reward" % ("" if saved_with else "out")):
            ppo.PPO(args)
