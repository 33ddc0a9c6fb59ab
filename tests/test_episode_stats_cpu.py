"""Episode statistics (PPO --episode_stats), the part that needs no GPU: the binding against the header, the
entry points' argument checks, the option and the flag, the untouched state-file meta, and the reference's own invariants."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest

from fly_bproject_amd import options, train_state
from tests import episode_stats_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    _lib.build()
    return _lib.load()


# ---- the binding -------------------------------------------------------------------------------------------------------------
def test_binding_and_header_agree_and_the_abi_version_stays_13(lib):
    from fly_bproject_amd import _lib
    P, L, I = C.c_void_p, C.c_int64, C.c_int
    assert _lib.ABI_VERSION == 13 and lib.fly_abi_version() == 13
    assert _lib.SYMBOLS["ppo_episode_stats"] == [P, P, P, L, L, L, P, P, P, I, P]
    assert _lib.SYMBOLS["ppo_episode_stats_merge"] == [P, L, P, P, P]
    for name in ("ppo_episode_stats", "ppo_episode_stats_merge"):
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name] and getattr(lib, name).restype is C.c_int
    header = open(os.path.join(REPO, "include", "flyhip.h")).read()
    assert ("int ppo_episode_stats(const float* reward, const int64_t* reset, const int64_t* progress, int64_t max_episode_length,\n"
            "                      int64_t T, int64_t N, double* carry_ret, int64_t* carry_len, double* sets, int mode, void* stream);") in header
    assert "int ppo_episode_stats_merge(const double* sets, int64_t nsets, double* window, double* total, void* stream);" in header
    macros = dict(re.findall(r"^#define (FLY_EPISODE_SETS?)\s+(\d+)", header, flags=re.M))
    assert (int(macros["FLY_EPISODE_SET"]), int(macros["FLY_EPISODE_SETS"])) == (_lib.EPISODE_SET, _lib.EPISODE_SETS) == (10, 256)
    assert R.SET == _lib.EPISODE_SET


def test_argument_checks_come_before_any_launch(lib):
    """FLY_E_ARG (-1) for a NULL pointer, a non-positive or overflowing size, an unknown mode and a misaligned buffer: all
    decided on the host, so they hold without a GPU.  The addresses are never dereferenced."""
    r, rs, pg, cr, cl, sets = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    f = lib.ppo_episode_stats
    good = [r, rs, pg, 1000, 8, 64, cr, cl, sets, 0, None]
    for i in (0, 1, 2, 6, 7, 8):
        args = list(good)
        args[i] = None
        assert f(*args) == -1 and b"null pointer" in lib.fly_last_error(), i
    for i, bad in ((3, 0), (3, -5), (4, 0), (4, -1), (5, 0), (5, -64)):
        args = list(good)
        args[i] = bad
        assert f(*args) == -1 and b"must be > 0" in lib.fly_last_error(), (i, bad)
    for mode in (1, 2, 3, 5, 8, -1):
        assert f(*(good[:9] + [mode, None])) == -1 and b"mode_flags" in lib.fly_last_error()
    assert f(r, rs, pg, 1000, 1 << 40, 1 << 40, cr, cl, sets, 0, None) == -1 and b"overflow" in lib.fly_last_error()
    assert f(r + 2, rs, pg, 1000, 8, 64, cr, cl, sets, 0, None) == -1 and b"4-byte aligned" in lib.fly_last_error()
    for i in (1, 2, 6, 7, 8):
        args = list(good)
        args[i] += 4
        assert f(*args) == -1 and b"8-byte aligned" in lib.fly_last_error(), i
    g = lib.ppo_episode_stats_merge
    w, t = 0x70000, 0x80000
    for args in ((None, 4, w, t, None), (sets, 4, None, t, None), (sets, 4, w, None, None)):
        assert g(*args) == -1 and b"null pointer" in lib.fly_last_error()
    for n in (0, -1):
        assert g(sets, n, w, t, None) == -1 and b"nsets must be > 0" in lib.fly_last_error()
    assert g(sets, 1 << 62, w, t, None) == -1 and b"overflow" in lib.fly_last_error()
    for args in ((sets + 4, 4, w, t, None), (sets, 4, w + 4, t, None), (sets, 4, w, t + 4, None)):
        assert g(*args) == -1 and b"8-byte aligned" in lib.fly_last_error()
    for args in ((sets, 4, w, w, None), (sets, 4, w, w + 8 * 9, None), (sets, 4, w + 8 * 9, w, None)):
        assert g(*args) == -1 and b"overlap" in lib.fly_last_error()


# ---- option, flag, state file ----------------------------------------------------------------------------------------------------
def test_option_flag_and_an_untouched_state_meta():
    import trainer
    opt = options.BY_NAME["episode_stats"]
    assert opt.default is False and opt.choices is None and opt.env is None
    assert trainer.parse_args([]).episode_stats is False
    assert trainer.parse_args(["--episode_stats"]).episode_stats is True
    for args, want in ((trainer.parse_args([]), False), (trainer.parse_args(["--episode_stats"]), True),
                       (types.SimpleNamespace(num_envs=1000), False), (types.SimpleNamespace(num_envs=1000, episode_stats=1), True)):
        rec = options.resolve(args, os.environ)
        assert rec.episode_stats is want
        assert "episode_stats" not in options.projection(rec)
        assert "episode_stats" not in train_state.expected_meta(args) and "episode_stats" not in train_state.expected_meta_ext(args)
    assert "--episode_stats" in trainer.__doc__
    # the option decides nothing a state depends on: both tuples and the format are what they were
    assert train_state.FORMAT == 1
    assert train_state.META_FIELDS == (
        "num_envs", "rollout_size", "variant", "reward", "world_size", "rank", "gae", "minibatch", "minibatch_seed", "action_noise",
        "noise_rho", "normalize_obs", "obs_clip", "normalize_value", "normalize_advantage", "randomize", "dr_ranges", "dr_seed",
        "gemm", "step_gemm", "persistent_rollout", "dp_mode")
    assert train_state.META_EXT_FIELDS == ("lambda_returns",)
    # so a state saved without the flag passes both checks of a run with it, and the other way round
    on, off = types.SimpleNamespace(num_envs=1000, episode_stats=True), types.SimpleNamespace(num_envs=1000)
    assert train_state.expected_meta(on) == train_state.expected_meta(off)
    train_state.check_meta(train_state.expected_meta(off), on)
    train_state.check_meta_ext(train_state.expected_meta_ext(on), off)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    """Two envs, five steps, limit 3 (max_episode_length 4).  Env 0 ends at t = 1 (progress 2: a fall) and t = 4 (progress 3:
    a time-out); env 1 never ends and comes in with (10.5, 7)."""
    reward = np.array([[1, .5], [2, .25], [4, 1], [8, 2], [16, 4]], dtype=np.float32)
    reset = np.array([[0, 0], [1, 0], [0, 0], [0, 0], [5, 0]], dtype=np.int64)
    progress = np.array([[1, 8], [2, 9], [1, 10], [2, 11], [3, 12]], dtype=np.int64)
    w = R.walk(reward, reset, progress, 4, carry_ret=[0.0, 10.5], carry_len=[0, 7])
    assert [(e.env, e.t, e.ret, e.exact, e.length, e.timeout, e.abs_sum, e.terms) for e in w.episodes] == [
        (0, 1, 3.0, 3.0, 2, False, 3.0, 2), (0, 4, 28.0, 28.0, 3, True, 28.0, 3)]
    assert w.carry_ret.tolist() == [0.0, 18.25] and w.carry_len.tolist() == [0, 12]
    assert w.carry_exact.tolist() == [0.0, 18.25] and w.carry_abs.tolist() == [0.0, 18.25] and w.carry_terms.tolist() == [0, 6]
    s = R.set_of(w.episodes, 10)
    assert s.tolist() == [2.0, 15.5, 312.5, 3.0, 28.0, 5.0, 2.0, 3.0, 1.0, 10.0]
    assert R.set_of([], 7).tolist() == [0, 0, 0, np.inf, -np.inf, 0, np.inf, 0, 0, 7]
    # env 1 alone under the limit's rule: progress >= 3 everywhere, so an end there is a time-out whatever else happened
    reset[2, 1] = 1
    w = R.walk(reward, reset, progress, 4, carry_ret=[0.0, 10.5], carry_len=[0, 7])
    ep = [e for e in w.episodes if e.env == 1]
    assert len(ep) == 1 and (ep[0].ret, ep[0].length, ep[0].timeout, ep[0].terms) == (12.25, 10, True, 4)
    assert w.carry_ret[1] == 6.0 and w.carry_len[1] == 2


def _progress_of(reset):
    """progress as the env counts it from scratch: steps since the reset, read after the step (an end row holds the length)."""
    T, N = reset.shape
    progress, p = np.zeros((T, N), np.int64), np.zeros(N, np.int64)
    for t in range(T):
        p = p + 1
        progress[t] = p
        p[reset[t] != 0] = 0
    return progress


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_invariants_on_random_flags(seed):
    """From scratch (zero carries) a closed episode's length is `progress` at its end row; with any carry-in, per env the closed
    returns plus carry out minus carry in are the float64 sum of the env's rewards, to the roundings of those sums; the
    lengths conserve the rows exactly; the sequentially rounded return is within the summation bound of the exact one."""
    rng = np.random.default_rng(seed)
    T, N = 200, 23
    reward = rng.uniform(-2, 2, (T, N)).astype(np.float32)
    reset = (rng.random((T, N)) < 1 / 7).astype(np.int64) * rng.integers(1, 4, (T, N))
    reset[:, 0] = 0                                                   # one env that never ends
    progress = _progress_of(reset)
    w = R.walk(reward, reset, progress, 9)
    assert len(w.episodes) == int((reset != 0).sum()) > 100
    for ep in w.episodes:
        assert ep.length == progress[ep.t, ep.env] and ep.timeout == (ep.length >= 8)
        assert abs(ep.ret - ep.exact) <= R.return_bound(ep) and ep.terms == ep.length
    assert any(ep.timeout for ep in w.episodes) and not all(ep.timeout for ep in w.episodes)
    rows_to_last_end = np.array([np.flatnonzero(np.append(1, reset[:, e]))[-1] for e in range(N)])      # 0: no end at all
    assert w.carry_len[0] == T and (w.carry_len == T - rows_to_last_end).all()
    gap, bound = R.conservation_gap(reward, w)
    assert (gap <= bound).all() and bound.max() < 1e-10
    # with carries coming in: lengths and returns shift by exactly that much in each env's first episode, conservation holds
    cin, lin = rng.normal(0, 50, N), rng.integers(0, 90, N)
    w2 = R.walk(reward, reset, progress, 9, carry_ret=cin, carry_len=lin)
    gap, bound = R.conservation_gap(reward, w2, cin)
    assert (gap <= bound).all()
    per_env = sum(ep.length for ep in w2.episodes) + int(w2.carry_len.sum())
    assert per_env == T * N + int(lin.sum())
    first = {}
    for a, b in zip(w.episodes, w2.episodes):
        assert (a.env, a.t, a.timeout) == (b.env, b.t, b.timeout)
        if a.env not in first:
            first[a.env] = True
            assert b.length == a.length + lin[a.env] and b.terms == a.terms + 1
        else:
            assert (b.length, b.ret, b.exact) == (a.length, a.ret, a.exact)
    # pooling the sets of any split of the episodes gives the set of all of them
    all_set = R.set_of(w.episodes, T * N)
    parts = [R.set_of(w.episodes[:40], 100), R.empty_set(5), R.set_of(w.episodes[40:41], T * N - 200), R.set_of(w.episodes[41:], 95)]
    pooled = R.pool(parts)
    ints = [R.N_, R.RMIN, R.RMAX, R.LSUM, R.LMIN, R.LMAX, R.TIMEOUTS, R.ROWS]
    assert np.array_equal(pooled[ints], all_set[ints])
    assert math.isclose(pooled[R.MEAN], all_set[R.MEAN], rel_tol=0, abs_tol=1e-13)
    assert math.isclose(pooled[R.M2], all_set[R.M2], rel_tol=1e-13)
