"""GPU (-m gpu): the episode-statistics kernels (PPO --episode_stats) through the C ABI on synthetic rows,
against tests/episode_stats_ref.py: both forms at the shapes and flag patterns where they can go wrong, two chained launches
against one, the two forms against each other, determinism, the merge, and a NaN reward.

Bounds (U = 2^-53, all from the reference's own values):
  a return or a carry     terms * U * sum|summand| of the episode / env concerned against the correctly rounded sum: the
                          recursive-summation bound, which holds for every order of adding the summands (the lane = env form adds
                          them in time order, the scan form chunk by chunk).  `d` below is its largest value over the episodes;
  ret_min, ret_max        d: an extreme of values that are each within d_i moves by at most max d_i;
  ret_mean                8 n U max|ret| + d: Welford / Chan in float64 plus the mean of the returns' own errors;
  ret_M2                  8 n U sum ret^2 + 4 d sum|ret| + n d^2: the same for M2, and M2's first-order change
                          2 sum (ret_i - mean) d_i with sum|ret_i - mean| <= 2 sum|ret_i|.
A float32 accumulation anywhere would miss them by about nine decimal orders.  Integer fields, carry_len and rows are exact; in
the lane = env form the carries and the extremes are also the reference's sequential float64 sums bit for bit (same additions,
same order)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import episode_stats_ref as R
from tests.hip_helpers import cuda

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEL = 1000                                            # max_episode_length: a time-out is progress >= 999
SETS = 256
U = R.U
INTS = [R.N_, R.LSUM, R.LMIN, R.LMAX, R.TIMEOUTS]
LANE_SHAPES = [(1, 1), (2, 63), (7, 64), (5, 65), (9, 130), (2, 64 * SETS + 1)]
SCAN_T, SCAN_N = [1, 63, 64, 65, 129, 1000], [1, 3, 16]
PATTERNS = ("none", "every", "first", "last", "edge_before", "edge_at", "span", "random")
WORST = {}                                            # field -> the largest |error| / bound seen (printed per case)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _lib():
    from fly_bproject_amd import _lib as L
    assert (L.EPISODE_SET, L.EPISODE_SETS) == (R.SET, SETS)
    return L, L.load()


def _flags(pattern, T, N, rng):
    """The end flags of a pattern; non-zero values vary, some with only high bits set (the rule is != 0 on an int64)."""
    L = (T + 63) // 64
    on = np.zeros((T, N), bool)
    if pattern == "every":
        on[:] = True
    elif pattern == "first":
        on[0] = True
    elif pattern == "last":
        on[T - 1] = True
    elif pattern == "edge_before":                    # the last step of every chunk of the scan form
        on[L - 1::L] = True
    elif pattern == "edge_at":                        # the first step of every chunk but the first
        on[L::L] = True
    elif pattern == "span":                           # one episode over more than two whole chunks, between two ends
        first = min(L // 2, T - 1)
        on[first] = True
        if first + 3 * L + 1 < T:
            on[first + 3 * L + 1] = True
    elif pattern == "random":
        on = rng.random((T, N)) < 1 / 7
    else:
        assert pattern == "none"
    values = rng.choice(np.array([1, 1, 2, -1, 1 << 32, 1 << 62], dtype=np.int64), (T, N))
    return np.where(on, values, 0).astype(np.int64)


def _case(T, N, pattern, carry, seed=0):
    rng = np.random.default_rng([seed, T, N, PATTERNS.index(pattern), int(carry)])
    reward = rng.uniform(-2, 2, (T, N)).astype(np.float32)
    reset = _flags(pattern, T, N, rng)
    progress = rng.integers(MEL - 4, MEL + 3, (T, N)).astype(np.int64)          # both sides of max_episode_length - 1
    cr = rng.normal(0, 30, N) if carry else np.zeros(N)
    cl = rng.integers(1, 700, N).astype(np.int64) if carry else np.zeros(N, np.int64)
    return reward, reset, progress, cr, cl


def _launch(reward, reset, progress, cr, cl, mode, mel=MEL):
    """One ppo_episode_stats launch on host arrays -> (sets [SETS][SET], carry_ret, carry_len) as numpy.  Every output sits
    inside a larger buffer of sentinels that must come back untouched."""
    L, lib = _lib()
    T, N = reward.shape
    r, rs, pg = cuda(reward), cuda(reset), cuda(progress)
    dcr = torch.full((N + 16,), -7.0, dtype=torch.float64, device=DEV)
    dcl = torch.full((N + 16,), -7, dtype=torch.long, device=DEV)
    dsets = torch.full((SETS + 2, R.SET), -7.0, dtype=torch.float64, device=DEV)
    dcr[8:8 + N] = cuda(np.asarray(cr, np.float64))
    dcl[8:8 + N] = cuda(np.asarray(cl, np.int64))
    L.check(lib.ppo_episode_stats(_p(r), _p(rs), _p(pg), mel, T, N, _p(dcr[8:]), _p(dcl[8:]), _p(dsets[1:]), mode, None),
            "ppo_episode_stats")
    torch.cuda.synchronize()
    hcr, hcl, hsets = dcr.cpu().numpy(), dcl.cpu().numpy(), dsets.cpu().numpy()
    assert (hcr[:8] == -7).all() and (hcr[8 + N:] == -7).all() and (hcl[:8] == -7).all() and (hcl[8 + N:] == -7).all()
    assert (hsets[0] == -7).all() and (hsets[-1] == -7).all()
    return hsets[1:-1], hcr[8:8 + N], hcl[8:8 + N]


def _ratio(name, err, bound):
    """err <= bound, and the ratio kept for the record; 0 <= 0 passes (bounds can be exactly zero: no summand at all)."""
    err, bound = float(err), float(bound)
    assert err <= bound, (name, err, bound)
    if bound > 0:
        WORST[name] = max(WORST.get(name, 0.0), err / bound)


def _float_bounds(w):
    """(d, mean bound, M2 bound) of the module docstring for the walk's episodes."""
    ret = np.array([ep.exact for ep in w.episodes])
    n = len(ret)
    d = max(R.return_bound(ep) for ep in w.episodes)
    return d, 8 * n * U * np.abs(ret).max() + d, 8 * n * U * (ret ** 2).sum() + 4 * d * np.abs(ret).sum() + n * d * d


def _check_set(got, w, rows, tag):
    """A set (pooled or persistent) against the reference's set of the walk's episodes."""
    want = R.set_of(w.episodes, rows)
    assert np.array_equal(got[INTS], want[INTS]), (tag, got, want)
    assert got[R.ROWS] == rows, (tag, got[R.ROWS], rows)
    if not w.episodes:
        assert np.array_equal(got, R.empty_set(rows)), (tag, got)
        return
    d, mean_bound, m2_bound = _float_bounds(w)
    _ratio("ret_min", abs(got[R.RMIN] - want[R.RMIN]), d)
    _ratio("ret_max", abs(got[R.RMAX] - want[R.RMAX]), d)
    _ratio("ret_mean", abs(got[R.MEAN] - want[R.MEAN]), mean_bound)
    _ratio("ret_M2", abs(got[R.M2] - want[R.M2]), m2_bound)
    assert got[R.M2] >= 0


def _check_carries(cr, cl, w, tag):
    assert np.array_equal(cl, w.carry_len), tag
    for e in range(len(cr)):
        _ratio("carry_ret", abs(cr[e] - w.carry_exact[e]), R.return_bound(int(w.carry_terms[e]), w.carry_abs[e]))


def _check_sets_shape(sets, T, N, mode):
    """Every workgroup's own set: whole numbers where whole numbers belong, the rows it walked, empty where it had no env."""
    assert np.array_equal(sets[:, INTS + [R.ROWS]], np.floor(sets[:, INTS + [R.ROWS]]))          # (len_min of an empty set: +inf)
    assert sets[:, R.ROWS].sum() == T * N
    busy = min(SETS, N if mode else (N + 63) // 64)
    for s in sets[busy:]:
        assert np.array_equal(s, R.empty_set(0))
    for s in sets[sets[:, R.N_] == 0]:
        assert np.array_equal(s[:R.ROWS], R.empty_set(0)[:R.ROWS])


def _run_patterns(T, N, mode):
    for pattern in PATTERNS:
        for carry in (False, True):
            tag = (T, N, mode, pattern, carry)
            reward, reset, progress, cr, cl = _case(T, N, pattern, carry)
            w = R.walk(reward, reset, progress, MEL, cr, cl)
            sets, cr_out, cl_out = _launch(reward, reset, progress, cr, cl, mode)
            _check_sets_shape(sets, T, N, mode)
            _check_set(R.pool(sets), w, T * N, tag)
            _check_carries(cr_out, cl_out, w, tag)
            if pattern == "none":
                assert not w.episodes and np.array_equal(cl_out, cl + T)                 # the carries grow by exactly T
            if pattern in ("last", "every"):
                assert (cr_out == 0).all() and (cl_out == 0).all()                      # an end in the last row: nothing is open
            if pattern == "every":
                assert R.pool(sets)[R.N_] == T * N and R.pool(sets)[R.LMAX] == (1 + cl.max() if carry else 1)
            if mode == 0 and w.episodes:
                # same float64 additions in the same order: the sequential reference, bit for bit
                seq = R.set_of(w.episodes, T * N, key="ret")
                assert np.array_equal(cr_out, w.carry_ret), tag
                assert R.pool(sets)[R.RMIN] == seq[R.RMIN] and R.pool(sets)[R.RMAX] == seq[R.RMAX], tag
            timeouts = sum(ep.timeout for ep in w.episodes)
            if pattern == "every" and T * N >= 63:
                assert 0 < timeouts < len(w.episodes)                                   # both sides of the limit were met
    print("T %d N %d mode %d: worst |error| / bound so far %s" % (T, N, mode, {k: "%.3g" % v for k, v in sorted(WORST.items())}))


@pytest.mark.parametrize("T,N", LANE_SHAPES)
def test_lane_form(T, N):
    _run_patterns(T, N, 0)


@pytest.mark.parametrize("N", SCAN_N)
@pytest.mark.parametrize("T", SCAN_T)
def test_scan_form(T, N):
    _run_patterns(T, N, 4)


def _merge(sets, window, total):
    """ppo_episode_stats_merge of host sets into host window / total -> the new (window, total)."""
    L, lib = _lib()
    s = cuda(np.ascontiguousarray(sets, dtype=np.float64).reshape(-1, R.SET))
    buf = torch.full((4, R.SET), -7.0, dtype=torch.float64, device=DEV)
    buf[1], buf[2] = cuda(np.asarray(window, np.float64)), cuda(np.asarray(total, np.float64))
    L.check(lib.ppo_episode_stats_merge(_p(s), s.shape[0], _p(buf[1]), _p(buf[2]), None), "ppo_episode_stats_merge")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[0] == -7).all() and (h[3] == -7).all()
    return h[1], h[2]


@pytest.mark.parametrize("T,N,mode", [(9, 130, 0), (129, 3, 4), (64, 16, 4)])
def test_two_chained_launches_and_the_merge_equal_one_launch(T, N, mode):
    """A rollout of 2 T rows in two launches over its halves, the carries handed on, each launch merged into window / total:
    the integers, carry_len and rows of one launch over the whole, the float fields within the whole's bounds."""
    for pattern in ("random", "span", "edge_at", "none"):
        reward, reset, progress, cr, cl = _case(2 * T, N, pattern, True, seed=5)
        w = R.walk(reward, reset, progress, MEL, cr, cl)
        window = total = R.empty_set(0)
        c1, l1 = cr, cl
        for half in (slice(0, T), slice(T, 2 * T)):
            sets, c1, l1 = _launch(reward[half], reset[half], progress[half], c1, l1, mode)
            window, total = _merge(sets, window, total)
        assert np.array_equal(window, total)                          # both started empty and saw the same sets
        _check_set(total, w, 2 * T * N, (T, N, mode, pattern, "chained"))
        _check_carries(c1, l1, w, (T, N, mode, pattern, "chained"))
        sets, c2, l2 = _launch(reward, reset, progress, cr, cl, mode)
        _, whole = _merge(sets, R.empty_set(0), R.empty_set(0))
        assert np.array_equal(whole[INTS + [R.ROWS]], total[INTS + [R.ROWS]]) and np.array_equal(l1, l2)
        _check_set(whole, w, 2 * T * N, (T, N, mode, pattern, "whole"))


@pytest.mark.parametrize("T,N", [(65, 3), (129, 16), (1000, 16), (64, 1)])
def test_the_two_forms_agree_on_every_integer(T, N):
    for pattern in ("random", "edge_before", "edge_at", "span", "every"):
        reward, reset, progress, cr, cl = _case(T, N, pattern, True, seed=9)
        lane, scan = _launch(reward, reset, progress, cr, cl, 0), _launch(reward, reset, progress, cr, cl, 4)
        a, b = R.pool(lane[0]), R.pool(scan[0])
        assert np.array_equal(a[INTS + [R.ROWS]], b[INTS + [R.ROWS]]) and np.array_equal(lane[2], scan[2]), (T, N, pattern)


@pytest.mark.parametrize("T,N,mode", [(9, 130, 0), (2, 64 * SETS + 1, 0), (129, 16, 4), (1000, 3, 4)])
def test_a_repeat_launch_gives_the_same_bits(T, N, mode):
    reward, reset, progress, cr, cl = _case(T, N, "random", True, seed=3)
    a, b = _launch(reward, reset, progress, cr, cl, mode), _launch(reward, reset, progress, cr, cl, mode)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.mark.parametrize("nsets", [1, 3, 64, 65, 300])
def test_merge_folds_the_sets_into_window_and_total(nsets):
    """Sets made by the reference from random episodes, every third one empty, folded onto a window and a total that already
    hold episodes: the reference's pooled statistics -- integers and extremes exactly, mean within 8 n U max|ret| and M2
    within 8 n U sum ret^2 (the inputs are given, so the returns bring no error of their own).  Empty sets are neutral."""
    rng = np.random.default_rng(nsets)

    def some_set(k, rows):
        eps = [R.Episode(0, 0, x, x, int(l), bool(t), abs(x), 1)
               for x, l, t in zip(rng.normal(3, 40, k), rng.integers(1, 999, k), rng.random(k) < 0.3)]
        return R.set_of(eps, rows)

    sets = np.stack([some_set(0 if i % 3 == 1 else int(rng.integers(1, 9)), int(rng.integers(0, 500))) for i in range(nsets)])
    window, total = some_set(5, 77), some_set(900, 123456)
    got_w, got_t = _merge(sets, window, total)
    for got, prior in ((got_w, window), (got_t, total)):
        want = R.pool(np.vstack([prior[None], sets]))
        exact = INTS + [R.ROWS, R.RMIN, R.RMAX]
        assert np.array_equal(got[exact], want[exact])
        n, big = want[R.N_], max(abs(want[R.RMIN]), abs(want[R.RMAX]))
        _ratio("merge_mean", abs(got[R.MEAN] - want[R.MEAN]), 8 * n * U * big)
        _ratio("merge_M2", abs(got[R.M2] - want[R.M2]), 8 * n * U * (want[R.M2] + n * want[R.MEAN] ** 2))
    # empty sets alone: only rows move
    empties = np.stack([R.empty_set(i) for i in range(nsets)])
    got_w, got_t = _merge(empties, window, R.empty_set(4))
    rows = sum(range(nsets))
    assert np.array_equal(got_w[:R.ROWS].view(np.int64), window[:R.ROWS].view(np.int64)) and got_w[R.ROWS] == window[R.ROWS] + rows
    assert np.array_equal(got_t, R.empty_set(4 + rows))
    print("merge nsets %d: worst |error| / bound so far %s" % (nsets, {k: "%.3g" % v for k, v in sorted(WORST.items())}))


@pytest.mark.parametrize("T,N,mode", [(9, 130, 0), (129, 16, 4)])
def test_a_nan_reward_stays_in_its_env(T, N, mode):
    reward, reset, progress, cr, cl = _case(T, N, "random", True, seed=13)
    clean = _launch(reward, reset, progress, cr, cl, mode)
    bad, e = reward.copy(), N // 2
    bad[T // 3, e] = np.nan
    got = _launch(bad, reset, progress, cr, cl, mode)
    a, b = R.pool(clean[0]), R.pool(got[0])
    assert np.array_equal(a[INTS + [R.ROWS]], b[INTS + [R.ROWS]])
    assert np.array_equal(clean[0][:, INTS + [R.ROWS]], got[0][:, INTS + [R.ROWS]])     # set by set, too
    assert np.array_equal(clean[2], got[2])
    others = np.arange(N) != e
    assert np.array_equal(clean[1][others].view(np.int64), got[1][others].view(np.int64))
    ends_after = np.flatnonzero(reset[T // 3:, e])
    assert np.isnan(got[1][e]) == (len(ends_after) == 0)               # the carry is NaN only while the NaN's episode is open
    assert np.isnan(got[0][:, R.MEAN]).any() == (len(ends_after) > 0)
