"""lambda-return critic targets (PPO --lambda_returns), the part that needs no GPU: the reference against
hand-computed cases, the binding and the entry point's argument checks, the flag / table / record agreement, and the state
file's `meta_ext` block."""
import ctypes as C
import io
import os
import types

import numpy as np
import pytest
import torch

from fly_bproject_amd import options, train_state
from tests import gae_episodic_ref as E
from tests import value_norm_ref as VN
from tests import value_target_ref as R
from tests.test_resume_cpu import FULL, _args


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_lambda_one_gives_the_discounted_reward_sum_plus_the_bootstrap():
    """lambda = 1, no ends, done = 1 and v_next[t] = v[t + 1]: the deltas telescope, so A_t + V(s_t) is the discounted sum of
    the rewards from t to the end of the rollout plus gamma^(T - t) v(s_T).  Both sides in float64: sums of at most 2 T + 1
    terms of magnitude <= 10, so they agree to a few hundred float64 roundings of 10 -- 1e-12 leaves a factor 10^3."""
    T, N, gamma = 9, 5, 0.99
    rng = np.random.default_rng(0)
    r = rng.normal(0, 3, (T, N))
    ring = rng.normal(0, 3, (T + 1, N))
    adv = R.gae64(r, ring[:T], ring[1:], np.ones((T, N)), gamma, 1.0)
    got = R.lambda_targets64(adv, ring[:T])
    want = np.empty((T, N))
    for t in range(T):
        want[t] = sum(gamma ** k * r[t + k] for k in range(T - t)) + gamma ** (T - t) * ring[T]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # lambda = 0 is the other end: A_t = delta_t, and the lambda-return is the one-step TD target
    adv0 = R.gae64(r, ring[:T], ring[1:], np.ones((T, N)), gamma, 0.0)
    np.testing.assert_allclose(R.lambda_targets64(adv0, ring[:T]), r + gamma * ring[1:], rtol=0, atol=1e-12)


def _episodic_case(seed, T=12, N=40, L=6):
    rng = np.random.default_rng(seed)
    r, v, vn = (rng.normal(0, 1, (T, N)).astype(np.float32) for _ in range(3))
    reset = (rng.random((T, N)) < 0.25).astype(np.int64)
    progress = rng.integers(0, L + 2, (T, N))
    ended_prev = (rng.random(N) < 0.5).astype(np.int64)
    return r, v, vn, reset, progress, ended_prev, L


@pytest.mark.parametrize("tab", [None, VN.table((1000.0, 37.5, 44444.0))], ids=["plain", "table"])
def test_episodic_stale_rows_give_vd_and_falls_have_no_bootstrap(tab):
    r, v, vn, reset, progress, ended_prev, L = _episodic_case(3)
    ended, timeout, stale = E.flags_of(reset, progress, ended_prev, L)
    fall = ended & ~timeout & ~stale
    assert stale.sum() > 20 and fall.sum() > 20 and (~stale & ~ended).sum() > 20
    td, adv = E.episodic32(r, v, vn, reset, progress, ended_prev, L, table=tab)
    got = R.lambda_targets(adv, v, tab)
    vd = v if tab is None else VN.denormalize(v, tab)
    assert (adv[stale] == 0).all()
    assert np.array_equal(got[stale], vd[stale]) and np.array_equal(got[stale], td[stale])      # the stale TD target is vd too
    # a fall: the carry is cut and nothing is bootstrapped, so adv = r - vd and the lambda-return is the reward (float64: to
    # two roundings of |r| + |vd| <= 1e3)
    e64 = E.episodic64(r, v, vn, reset, progress, ended_prev, L, np.float32(0.99), np.float32(0.99 * 0.95), table=tab)
    got64 = R.lambda_targets64(e64.adv, v, tab)
    np.testing.assert_allclose(got64[fall], r.astype(np.float64)[fall], rtol=0, atol=1e-12)
    # and the float32 statement is the float64 one to its own three roundings
    u = 2.0 ** -24
    s, m = (1.0, 0.0) if tab is None else (float(tab[1]), float(tab[0]))
    v64, a64 = v.astype(np.float64), adv.astype(np.float64)
    bound = u * (np.abs(v64 * s) + np.abs(v64 * s + m) + np.abs(a64 + v64 * s + m)) * 1.01
    assert (np.abs(got - R.lambda_targets64(adv, v, tab)) <= bound).all()


def test_reference_moments_and_combine():
    rng = np.random.default_rng(1)
    x = (1e3 + 1e-2 * rng.standard_normal(5000)).astype(np.float32)
    n, mean, m2 = R.moments(x)
    assert n == 5000 and R.moments(np.zeros(0)) == (0.0, 0.0, 0.0)
    sets = [R.moments(part) for part in (x[:7], x[7:7], x[7:3000], x[3000:])]
    cn, cmean, cm2 = R.combine(sets)
    assert cn == n
    np.testing.assert_allclose(cmean, mean, rtol=1e-14)
    np.testing.assert_allclose(cm2, m2, rtol=1e-10)
    assert VN.moments(x)[2] == pytest.approx(m2 / n, rel=1e-14)          # M2 = count * population variance


# ---- the binding -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_binding_exists_and_the_abi_version_stays_13(lib):
    from fly_bproject_amd import _lib
    assert _lib.ABI_VERSION == 13 and lib.fly_abi_version() == 13
    assert _lib.SYMBOLS["ppo_lambda_targets"] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.ppo_lambda_targets.argtypes == _lib.SYMBOLS["ppo_lambda_targets"] and lib.ppo_lambda_targets.restype is C.c_int
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flyhip.h")).read()
    assert "int ppo_lambda_targets(const float* adv, const float* v, const float* table, int64_t n, float* target_out, double* sets," in header


def test_argument_checks_come_before_any_launch(lib):
    """FLY_E_ARG (-1) for n < 0, a NULL required pointer, misaligned buffers and aliasing: all decided on the host, so they hold
    without a GPU.  The addresses are never dereferenced."""
    a, v, out, sets, tab = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    f = lib.ppo_lambda_targets
    assert f(a, v, tab, -1, out, sets, None) == -1 and b"n must be >= 0" in lib.fly_last_error()
    for args in ((None, v, tab, 4, out, sets, None), (a, None, tab, 4, out, sets, None), (a, v, tab, 4, None, sets, None)):
        assert f(*args) == -1 and b"null pointer" in lib.fly_last_error()
    assert f(a + 2, v, None, 4, out, None, None) == -1 and b"4-byte aligned" in lib.fly_last_error()
    assert f(a, v, None, 4, out, sets + 4, None) == -1 and b"8-byte aligned" in lib.fly_last_error()
    for args in ((a, v, None, 4, a, None, None), (a, v, None, 4, v + 12, None, None), (a, v, None, 4, a - 12, None, None)):
        assert f(*args) == -1 and b"alias" in lib.fly_last_error()
    assert f(a, v, None, 0, out, None, None) == 0                       # n == 0 without sets: nothing to write, no launch


# ---- option, flag, record ------------------------------------------------------------------------------------------------------
def test_flag_table_and_record_agree():
    import trainer
    opt = options.BY_NAME["lambda_returns"]
    assert opt.default is False and opt.choices is None and opt.env is None
    assert trainer.parse_args([]).lambda_returns is False
    assert trainer.parse_args(["--lambda_returns"]).lambda_returns is True
    for args, want in ((trainer.parse_args([]), False), (trainer.parse_args(["--lambda_returns"]), True),
                       (types.SimpleNamespace(num_envs=1000), False), (types.SimpleNamespace(num_envs=1000, lambda_returns=1), True)):
        rec = options.resolve(args, os.environ)
        assert rec.lambda_returns is want
        assert options.projection(rec)["lambda_returns"] is want
        assert train_state.expected_meta_ext(args) == {"lambda_returns": want}
        assert "lambda_returns" not in train_state.expected_meta(args)              # the format-1 meta block is as it was
    assert train_state.META_EXT_FIELDS == ("lambda_returns",) and train_state.FORMAT == 1
    assert "lambda_returns" not in train_state.META_FIELDS
    assert "--lambda_returns" in trainer.__doc__


# ---- meta_ext --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("held,run", [(True, False), (False, True)])
def test_meta_ext_refuses_a_difference_in_both_directions(held, run):
    with pytest.raises(ValueError) as e:
        train_state.check_meta_ext({"lambda_returns": held}, _args(lambda_returns=run))
    msg = str(e.value)
    assert (" lambda_returns is %r in the state file and %r in this run" % (held, run)) in msg and "--load_path" in msg
    train_state.check_meta_ext({"lambda_returns": held}, _args(lambda_returns=held))
    train_state.check_meta_ext({"lambda_returns": held}, _args(**dict(FULL, lambda_returns=held)))


def test_a_file_without_the_block_is_a_run_with_the_option_off():
    for absent in (None, {}):
        train_state.check_meta_ext(absent, _args())
        train_state.check_meta_ext(absent, _args(lambda_returns=False))
        with pytest.raises(ValueError, match=" lambda_returns is False in the state file and True in this run"):
            train_state.check_meta_ext(absent, _args(lambda_returns=True))
    with pytest.raises(ValueError, match="lambda_returns is 1 in the state file and True"):      # strict: a bool, as in meta
        train_state.check_meta_ext({"lambda_returns": 1}, _args(lambda_returns=True))
    with pytest.raises(ValueError, match="meta_ext is no block"):
        train_state.check_meta_ext([True], _args())


def test_meta_ext_round_trips_through_the_weights_only_loader():
    ext = train_state.expected_meta_ext(_args(lambda_returns=True))
    f = io.BytesIO()
    torch.save({"format": train_state.FORMAT, "meta": train_state.expected_meta(_args()), "meta_ext": ext}, f)
    f.seek(0)
    back = torch.load(f, weights_only=True)
    assert back["meta_ext"] == {"lambda_returns": True} and type(back["meta_ext"]["lambda_returns"]) is bool
    train_state.check_meta_ext(back["meta_ext"], _args(lambda_returns=True))


def _state_file(tmp_path, name, meta_ext):
    weights = str(tmp_path / (name + ".pth"))
    state = {"format": train_state.FORMAT, "meta": train_state.expected_meta(_args())}
    if meta_ext is not None:
        state["meta_ext"] = meta_ext
    torch.save(state, train_state.training_state_path(weights, 0))
    return weights


def test_the_constructor_checks_the_block_before_the_env_exists(tmp_path, monkeypatch):
    from fly_bproject_amd import ppo

    def no_env(args):
        raise AssertionError("the env was built")

    monkeypatch.setattr(ppo, "Fly", no_env)
    for k in ("FLY_GEMM", "FLY_STEP_GEMM", "FLY_PERSISTENT_ROLLOUT"):
        monkeypatch.delenv(k, raising=False)
    old, off, on = (_state_file(tmp_path, n, e) for n, e in (("old", None), ("off", {"lambda_returns": False}),
                                                              ("on", {"lambda_returns": True})))
    for weights, flag in ((old, True), (off, True), (on, False)):
        with pytest.raises(ValueError, match=" lambda_returns is "):
            ppo.PPO(_args(resume=True, resume_path=weights, lambda_returns=flag))
    for weights, flag in ((old, False), (off, False), (on, True)):
        with pytest.raises(AssertionError, match="the env was built"):          # accepted: it gets as far as the env
            ppo.PPO(_args(resume=True, resume_path=weights, lambda_returns=flag))
