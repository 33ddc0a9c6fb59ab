"""GPU (-m gpu): the update-diagnostics kernels (csrc/update_stats.hip) through the C ABI against tests/update_stats_ref.py.

The sets sit between sentinel guards (tests/test_rollout_kernels_gpu.py's Guarded).  Counts, the clipped count and both maxima
are exact (the cases keep every finite ratio outside its rounding margin of the clip edges: tests/update_stats_cases.py, asserted
on the CPU); moments at the suite's float64 bar (rtol 1e-10, atol 1e-12 on the mean); the four sums and the ratio extremes within
the bounds the reference derives from the op count (nothing of them from what the kernel returns).  Every case prints its
measured / bound per field (`-s`; profiles/update_stats_error.txt holds one run): a ratio above 1 means the kernel or the
derivation is wrong, not the tolerance."""
import numpy as np
import pytest
import torch

from tests import update_stats_cases as cases
from tests import update_stats_ref as R
from tests.test_rollout_kernels_gpu import SENTINEL, Guarded, _dev, _p, lib    # noqa: F401  (lib: the module's fixture)

pytestmark = pytest.mark.gpu
MOMENTS = ((R.TN, R.TMEAN, R.TM2), (R.EN, R.EMEAN, R.EM2))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_stats(lib, c, offset=0):
    """-> sets [256][17] of ppo_update_stats on case `c`; offset shifts the bases of mu and action by that many floats off their
    16-byte alignment (1, 2: the scalar path), and that of the per-row arrays with them."""
    n = c.mu.shape[0]
    sets = Guarded(R.SETS * R.SET, dtype=torch.float64)
    bufs = [Guarded(a.size, offset=offset, init=a) for a in (c.mu, c.action, c.old_logp, c.adv, c.v, c.target)]
    assert all((b.ptr.value % 16 == 0) == (offset % 4 == 0) and b.ptr.value % 4 == 0 for b in bufs)
    dvar = _dev(c.var)
    rc = lib.load().ppo_update_stats(*[b.ptr for b in bufs], _p(dvar), c.clip, n, sets.ptr, None)
    assert rc == 0, lib.load().fly_last_error()
    out = sets.get().reshape(R.SETS, R.SET)
    for b, a in zip(bufs, (c.mu, c.action, c.old_logp, c.adv, c.v, c.target)):
        assert np.array_equal(b.get().view(np.uint32), np.ascontiguousarray(a).reshape(-1).view(np.uint32)), "an input was written"
    return out


def run_merge(lib, sets, last, window, total):
    """-> (last, window, total) after ppo_update_stats_merge over `sets`."""
    g = [Guarded(R.SET, dtype=torch.float64, init=x) for x in (last, window, total)]
    dsets = _dev(np.ascontiguousarray(sets, dtype=np.float64))
    rc = lib.load().ppo_update_stats_merge(_p(dsets), dsets.shape[0], g[0].ptr, g[1].ptr, g[2].ptr, None)
    assert rc == 0, lib.load().fly_last_error()
    return tuple(x.get() for x in g)


_REFERENCE = {}


def _reference(key):
    """The case, its per-row terms and its set, computed once and shared (never written)."""
    if key not in _REFERENCE:
        c = cases.case(*key)
        t = R.row_terms(*c[:8])
        assert R.clip_margin_ok(t)
        _REFERENCE[key] = (c, t, R.set_from_terms(t, c.adv, c.v, c.target))
    return _REFERENCE[key]


def _check_sets_shape(sets, n):
    """One set per workgroup: workgroup g owns the tiles g, g + 256, ...; without a tile it holds the empty set."""
    assert sets.shape == (R.SETS, R.SET) and sets[:, R.ROWS].sum() == n
    tiles = (n + 255) // 256
    rows = np.zeros(R.SETS)
    for tile in range(tiles):
        rows[tile % R.SETS] += min(256, n - 256 * tile)
    assert np.array_equal(sets[:, R.ROWS], rows)
    for g in np.flatnonzero(rows == 0):
        assert np.array_equal(_bits(sets[g]), _bits(R.empty_set())), g


def _check_against_reference(got, t, want, label, near=0):
    """`got`: the kernel's sets folded into one (by the reference merge, or by the merge kernel).  `near`: how many finite rows
    lie within their margin of a clip edge (0 for the seeded cases; rows of a real rollout may), each of which may fall on
    either side in fp32: the clipped count then agrees to that many, everything else is held as before (the policy term is
    continuous across the edges, so its bound does not move)."""
    exact = [k for k in R.EXACT if k != R.CLIPPED]
    assert np.array_equal(got[exact], want[exact]), (label, got[exact], want[exact])
    assert abs(got[R.CLIPPED] - want[R.CLIPPED]) <= near and got[R.CLIPPED] == int(got[R.CLIPPED]), (label, got[R.CLIPPED], want[R.CLIPPED], near)
    for n_, mean, m2 in MOMENTS:
        np.testing.assert_allclose(got[mean], want[mean], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(got[m2], want[m2], rtol=1e-10, atol=0)
    line = []
    for k, name in ((R.K1, "k1"), (R.K3, "k3"), (R.POL, "pol"), (R.HUB, "hub")):
        err, bound = abs(got[k] - want[k]), R.sum_bound(t, k)
        line.append("%s %.3g" % (name, err / bound if bound > 0 else (np.inf if err > 0 else 0.0)))
        assert err <= bound, (label, name, err, bound)
    for k, name in ((R.RMIN, "ratio_min"), (R.RMAX, "ratio_max")):
        err, bound = abs(got[k] - want[k]), R.extreme_bound(t)
        line.append("%s %.3g" % (name, err / bound if bound > 0 else (np.inf if err > 0 else 0.0)))
        assert err <= bound, (label, name, err, bound)
    print("update_stats %s: measured / bound  %s" % (label, "  ".join(line)))


@pytest.mark.parametrize("key", cases.GPU_CASES, ids=lambda k: "R%d" % k[0])
def test_kernel_against_the_reference(lib, key):
    c, t, want = _reference(key)
    n = key[0]
    sets = run_stats(lib, c)
    _check_sets_shape(sets, n)
    _check_against_reference(R.merge_all(sets), t, want, "R=%d" % n)
    again = run_stats(lib, c)
    assert np.array_equal(_bits(sets), _bits(again))                  # no atomics: two launches, the same bits


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("key", [cases.GPU_CASES[1], cases.GPU_CASES[6], cases.GPU_CASES[7]], ids=lambda k: "R%d" % k[0])
def test_scalar_path_gives_the_same_bits(lib, key, offset):
    """Bases that are only 4-byte aligned: identical results."""
    c, t, want = _reference(key)
    aligned, shifted = run_stats(lib, c), run_stats(lib, c, offset=offset)
    assert np.array_equal(_bits(aligned), _bits(shifted))
    _check_against_reference(R.merge_all(shifted), t, want, "R=%d, bases + %d floats" % (key[0], offset))


def test_a_bad_variance_makes_every_row_nonfinite(lib):
    c, _, _ = _reference(cases.GPU_CASES[4])
    for bad in (0.0, -1.0, float("nan")):
        var = c.var.copy()
        var[11] = bad
        got = R.merge_all(run_stats(lib, c._replace(var=var)))
        want = R.empty_set()
        want[R.ROWS] = want[R.NONFINITE] = c.mu.shape[0]
        assert np.array_equal(_bits(got), _bits(want)), bad


def test_merge_kernel(lib):
    """Against the reference merge in the same order: sums, counts and extremes bit for bit, moments at 1e-10; `last` is
    overwritten, `window` and `total` accumulate over two calls; empty sets are skipped."""
    c1, _, _ = _reference(cases.GPU_CASES[7])
    c2, _, _ = _reference(cases.GPU_CASES[4])
    s1, s2 = run_stats(lib, c1), run_stats(lib, c2)
    assert (s1[:, R.ROWS] == 0).sum() > 200                           # most workgroups had no tile: empty sets among the 256
    empty = R.empty_set()
    plain = [k for k in range(R.SET) if k not in (R.TMEAN, R.TM2, R.EMEAN, R.EM2)]

    def same(got, want):
        assert np.array_equal(_bits(got[plain]), _bits(want[plain])), (got, want)
        np.testing.assert_allclose(got[[R.TMEAN, R.EMEAN]], want[[R.TMEAN, R.EMEAN]], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(got[[R.TM2, R.EM2]], want[[R.TM2, R.EM2]], rtol=1e-10, atol=0)

    junk = np.arange(R.SET, dtype=np.float64) + 0.5                   # whatever `last` held goes
    last, window, total = run_merge(lib, s1, junk, empty, empty)
    b1 = R.merge_all(s1)
    for got in (last, window, total):
        same(got, b1)
    # the second call: two ranks' worth of sets (s2 then s1) onto what the first left
    both = np.concatenate((s2, s1))
    last2, window2, total2 = run_merge(lib, both, last, window, total)
    b2 = R.merge_all(both)
    same(last2, b2)
    same(window2, R.merge(window, b2))
    same(total2, R.merge(total, b2))
    assert last2[R.ROWS] == 255 + 1027
    assert total2[R.ROWS] == 1027 + 1027 + 255
    # nothing but empty sets: `last` is the empty set, the persistent sets stay as they are, bit for bit
    last3, window3, total3 = run_merge(lib, np.tile(empty, (5, 1)), last2, window2, total2)
    assert np.array_equal(_bits(last3), _bits(empty))
    assert np.array_equal(_bits(window3), _bits(window2)) and np.array_equal(_bits(total3), _bits(total2))
    # a single set, and a count that is no multiple of the 64 the kernel stages at a time
    one = run_merge(lib, s1[:1], junk, empty, empty)
    same(one[0], s1[0])
    odd = run_merge(lib, np.concatenate((s1, s2[:7])), junk, empty, empty)
    same(odd[0], R.merge_all(np.concatenate((s1, s2[:7]))))
