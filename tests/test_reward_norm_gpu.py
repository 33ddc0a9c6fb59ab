"""GPU (-m gpu): the reward-scaling kernels (csrc/reward_norm.hip) through the C ABI against tests/reward_norm_ref.py.

Every buffer a kernel writes sits between two sentinel guards (tests/test_rollout_kernels_gpu.py's Guarded), so a ragged tail
that writes past its array fails here without any fault.  The lane = env form is held to the reference's carries bit for bit;
the scan form to the bound the reference module derives (c(gamma) u S, nothing of it from what the kernel returns), and each
scan case prints its worst |error| / bound (`-s`).  Statistics after ppo_value_norm_merge sit against numpy two-pass float64
moments of the reference's G at the suite's standing bounds (rtol 1e-10, atol 1e-12 on the mean)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import reward_norm_cases as cases
from tests import reward_norm_ref as R
from tests.test_rollout_kernels_gpu import SENTINEL, Guarded, _dev, _p, lib    # noqa: F401  (lib: the module's fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCAN = 4
INITIAL = (0.0, 0.0, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_carries(got, want):
    """== on the float64 bit patterns; NaN envs compared as NaN."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def run_returns(lib, reward, reset, gamma, cin, mode, in_place=False, expect=0, override=None):
    """-> (carry_out [N], sets [k][3]) through guarded buffers; carry_in is checked to be untouched (or is carry_out itself
    with `in_place`).  With expect != 0: asserts the return code and that nothing was written."""
    T, N = reward.shape
    sets = Guarded(lib.VALUE_NORM_SETS * lib.VALUE_NORM_SET, dtype=torch.float64)
    dcin = Guarded(N, dtype=torch.float64, init=cin)
    cout = dcin if in_place else Guarded(N, dtype=torch.float64)
    dr, ds = _dev(reward), _dev(reset)
    args = dict(reward=_p(dr), reset=_p(ds), gamma=gamma, T=T, N=N, carry_in=dcin.ptr, carry_out=cout.ptr, sets=sets.ptr, mode=mode)
    args.update(override or {})
    rc = lib.load().ppo_reward_returns(*args.values(), None)
    assert rc == expect, lib.load().fly_last_error()
    out, s = cout.get(), sets.get()
    if expect != 0:
        assert (s == SENTINEL).all() and (out == (np.asarray(cin) if in_place else SENTINEL)).all()
        return None
    if not in_place:
        assert np.array_equal(_bits(dcin.get()), _bits(cin)), "carry_in was written"
    return out, s.reshape(-1, 3)


def run_merge(lib, stats, sets):
    """-> (stats_out (count, mean, var), table f32 [4]) of ppo_value_norm_merge over `sets`."""
    so, to = Guarded(3, dtype=torch.float64), Guarded(4)
    dsi, dsets = _dev(np.asarray(stats, dtype=np.float64)), _dev(np.ascontiguousarray(sets, dtype=np.float64))
    lib.check(lib.load().ppo_value_norm_merge(_p(dsi), _p(dsets), dsets.shape[0], so.ptr, to.ptr, None), "ppo_value_norm_merge")
    return tuple(float(x) for x in so.get()), to.get()


def _assert_stats(got, want):
    """The bounds tests/test_value_norm_gpu.py and tests/test_obs_norm_gpu.py hold their statistics to."""
    (c, mu, var), (wc, wmu, wvar) = got, want
    print("return statistics: count %r (want %r)  mean %.17g (want %.17g)  var %.17g (want %.17g)" % (c, wc, mu, wmu, var, wvar))
    assert c == wc
    np.testing.assert_allclose(mu, wmu, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(var, wvar, rtol=1e-10, atol=0)


def _assert_sets(lib, sets, T, N, mode):
    """Counts add to T * N exactly; a workgroup's count is its envs times T; workgroups without envs hold 0 | 0 | 0."""
    k = lib.VALUE_NORM_SETS
    assert sets.shape == (k, 3) and sets[:, 0].sum() == T * N
    e = np.arange(N)
    owner = e % k if mode & SCAN else (e // 64) % k        # scan: env e -> workgroup e mod k; lane form: its 64-block mod k
    envs = np.bincount(owner, minlength=k)
    assert np.array_equal(sets[:, 0], envs * float(T))
    assert (sets[envs == 0] == 0.0).all()


def _assert_scan_carries(got, w, gamma, what):
    bound = R.scan_bound(gamma, w.smax)
    nan = np.isnan(w.carry)
    assert np.array_equal(np.isnan(got), nan)
    err = np.abs(got - w.carry)
    inf = np.isinf(w.carry)
    assert np.array_equal(got[inf], w.carry[inf])
    ok = ~nan & ~inf
    assert (err[ok] <= bound[ok]).all(), (what, err[ok].max(), bound[ok])
    pos = ok & (bound > 0)
    worst = float(np.max(err[pos] / bound[pos], initial=0.0))
    print("reward_norm scan carry_out: worst |error| / bound %.3g (%s)" % (worst, what))
    return worst


def _check(lib, T, N, mode, gamma, seed, carry, nan=False, huge=True):
    reward, reset, cin = cases.case(T, N, seed, carry=carry, nan=nan, huge=huge)
    w = R.walk(reward, reset, gamma, cin)
    out, sets = run_returns(lib, reward, reset, gamma, cin, mode)
    if mode & SCAN:
        _assert_scan_carries(out, w, gamma, "T %d N %d gamma %g seed %d" % (T, N, gamma, seed))
    else:
        _same_carries(out, w.carry)                                                                 # (1)
    _assert_sets(lib, sets, T, N, mode)                                                             # (3)
    if nan:
        col = N // 2
        t_nan = int(np.flatnonzero(np.isnan(reward[:, col]))[0])
        ends_after = np.flatnonzero(reset[t_nan:, col] != 0)
        assert np.isnan(w.carry[col]) == (len(ends_after) == 0)              # poisoned only until the env's next end
        assert not np.isnan(np.delete(out, col)).any()                       # and only its own env
        return out, sets
    stats, table = run_merge(lib, INITIAL, sets)                                                    # (4)
    _assert_stats(stats, R.moments(w.G))
    assert np.array_equal(table.view(np.uint32), R.table(stats).view(np.uint32))
    return out, sets


# ---- ppo_reward_returns, lane = env ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.99, 0.5])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 33])
def test_lane_form_around_the_unroll(lib, T, gamma):
    for N in (1, 63, 64, 65, 130):
        _check(lib, T, N, 0, gamma, seed=T + N, carry=bool((T + N) & 1))
        _check(lib, T, N, 0, gamma, seed=T + N + 1, carry=bool((T + N) & 1), huge=False)      # statistics of unit scale too


def test_lane_form_takes_a_second_trip_over_the_envs(lib):
    N = 256 * 64 + 65
    out, sets = _check(lib, 3, N, 0, 0.99, seed=5, carry=True)
    assert sets[0, 0] == (64 + 64) * 3 and sets[1, 0] == (64 + 1) * 3 and sets[2, 0] == 64 * 3


@pytest.mark.parametrize("mode", [0, SCAN])
def test_a_nan_reward_poisons_only_its_env_until_its_next_end(lib, mode):
    for seed in (0, 1, 2, 3):
        _check(lib, 33 if mode == 0 else 129, 65 if mode == 0 else 3, mode, 0.99, seed=seed, carry=True, nan=True)


# ---- ppo_reward_returns, scan --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.99, 0.5])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129, 200])
def test_scan_form_within_the_derived_bound(lib, T, gamma):
    """L = 1 with empty lanes, L = 1 exact, L = 2 with a ragged last chunk and lanes past T, L = 3, L = 4; 257 envs: one more
    than sets.  The ratio printed here is the figure DESIGN.md 3.3i quotes; above 1 the kernel or the derivation is wrong."""
    for N in (1, 3, 257):
        _check(lib, T, N, SCAN, gamma, seed=T + N, carry=bool((T + N) & 1))
        _check(lib, T, N, SCAN, gamma, seed=T + N + 1, carry=bool((T + N) & 1), huge=False)   # statistics of unit scale too


# ---- two launches, both forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,T,N", [(0, 18, 130), (SCAN, 130, 3)])
def test_two_launches_chained_through_the_carry(lib, mode, T, N):
    """Halves of a rollout chained through the carry, one merge of both launches' sets: the carries of one launch over the
    whole (bit for bit in the lane form, within the bound in the scan form) and its statistics."""
    gamma = 0.99
    reward, reset, cin = cases.case(T, N, 21, carry=True)
    h = T // 2
    w = R.walk(reward, reset, gamma, cin)
    whole, whole_sets = run_returns(lib, reward, reset, gamma, cin, mode)
    mid, sets_a = run_returns(lib, reward[:h], reset[:h], gamma, cin, mode)
    end, sets_b = run_returns(lib, reward[h:], reset[h:], gamma, mid, mode, in_place=True)       # carry_out == carry_in
    if mode & SCAN:
        _assert_scan_carries(whole, w, gamma, "whole")
        _assert_scan_carries(end, w, gamma, "two halves")
    else:
        _same_carries(whole, w.carry)
        _same_carries(end, w.carry)
    assert sets_a[:, 0].sum() + sets_b[:, 0].sum() == T * N
    prior = (1000.0, 0.25, 4.0)
    want = R.merge(prior, w.G)
    _assert_stats(run_merge(lib, prior, np.concatenate((sets_a, sets_b)))[0], want)
    _assert_stats(run_merge(lib, prior, whole_sets)[0], want)


@pytest.mark.parametrize("T,N", [(65, 3), (9, 130), (200, 65)])
def test_both_forms_on_the_same_input(lib, T, N):
    gamma = 0.99
    reward, reset, cin = cases.case(T, N, 31, carry=True)
    w = R.walk(reward, reset, gamma, cin)
    lane, lane_sets = run_returns(lib, reward, reset, gamma, cin, 0)
    scan, scan_sets = run_returns(lib, reward, reset, gamma, cin, SCAN)
    assert lane_sets[:, 0].sum() == scan_sets[:, 0].sum() == T * N
    _same_carries(lane, w.carry)
    _assert_scan_carries(scan, w, gamma, "both forms")
    a, b = run_merge(lib, INITIAL, lane_sets)[0], run_merge(lib, INITIAL, scan_sets)[0]
    want = R.moments(w.G)
    _assert_stats(a, want)
    _assert_stats(b, want)


# ---- ppo_reward_scale ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_scale_is_numpy_float32_bit_for_bit(lib, n, offset):
    rng = np.random.default_rng(n + offset)
    x = (rng.standard_normal(n) * 40).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, cases.HUGE, -cases.HUGE], dtype=np.float32)
    x[rng.permutation(n)[:min(n, 6)]] = special[:min(n, 6)]
    table = R.table((100.0, 3.0, 7.5))
    clip = 10.0
    want = R.scale(x, table[2], clip)
    src, out = Guarded(n, offset=offset, init=x), Guarded(n, offset=offset)
    dt = _dev(table)
    lib.check(lib.load().ppo_reward_scale(src.ptr, n, _p(dt), clip, out.ptr, None), "ppo_reward_scale")
    got = out.get()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(src.get().view(np.uint32), x.view(np.uint32))                  # the rewards are only read
    nan, pinf, ninf = np.isnan(x), x == np.inf, x == -np.inf
    assert np.isnan(got[nan]).all() and (got[pinf] == clip).all() and (got[ninf] == -clip).all()
    # in place
    lib.check(lib.load().ppo_reward_scale(src.ptr, n, _p(dt), clip, src.ptr, None), "ppo_reward_scale")
    assert np.array_equal(src.get().view(np.uint32), want.view(np.uint32))
    # a mixed alignment takes the scalar path with the same bits
    if n > 1:
        mixed, dx = Guarded(n, offset=1 - offset), _dev(x)
        lib.check(lib.load().ppo_reward_scale(_p(dx), n, _p(dt), clip, mixed.ptr, None), "ppo_reward_scale")
        assert np.array_equal(mixed.get().view(np.uint32), want.view(np.uint32))


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(lib):
    reward, reset, cin = cases.case(9, 65, 3, carry=True)
    for override in (dict(reward=None), dict(reset=None), dict(carry_in=None), dict(carry_out=None), dict(sets=None),
                     dict(T=0), dict(T=-1), dict(N=0), dict(mode=1), dict(mode=2), dict(mode=6), dict(mode=8)):
        run_returns(lib, reward, reset, 0.99, cin, 0, expect=-1, override=override)
    x = np.ones(8, dtype=np.float32)
    dt = _dev(R.table(INITIAL))
    for kw in (dict(reward=None), dict(table=None), dict(out=None), dict(n=0), dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan"))):
        src, out = Guarded(8, init=x), Guarded(8)
        a = dict(reward=src.ptr, n=8, table=_p(dt), clip=10.0, out=out.ptr)
        a.update(kw)
        assert lib.load().ppo_reward_scale(*a.values(), None) == -1
        assert (out.get() == SENTINEL).all() and (src.get() == 1.0).all()
    src = Guarded(8, init=x)
    assert lib.load().ppo_reward_scale(src.ptr, 4, _p(dt), 10.0, C.c_void_p(src.ptr.value + 8), None) == -1      # a partial overlap
    assert (src.get() == 1.0).all()
