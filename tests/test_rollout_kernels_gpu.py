"""GPU (-m gpu): the rollout's PPO kernels (csrc/ppo_kernels.hip, its value-normalising GAE instances included) through the C ABI
against the float64 references of tests/rollout_ref.py, at ragged shapes and at the edges of their index arithmetic.

Every buffer a kernel writes sits between two guards of 64 elements pre-filled with a sentinel, and reading a result back
asserts that both guards are untouched: a ragged tail that writes past its array fails here without any fault.  Outputs are
pre-filled with the sentinel as well, so an element a kernel skips cannot pass a value check.

Bounds (u = 2^-24; derived in tests/rollout_ref.py, none of them from what the kernels return):
  sampling      action within 1 ulp of its float32 specification; log-prob within 1e-5 + 2e-6 |logp| (the suite's bar) plus
                the cancellation term sum_j |x_j| 2^-23 (|mu_j| + |a_j|) / L_j
  GAE           target within 2^-23 (|gamma v'| + |tg|); advantage within 2 x the first-order bound of the six rounded
                intermediates per step (the factor 2 covers the second-order terms)
  scan GAE      advantage within 4 x (that bound + the re-associated carries: the zero-carry pass, six tree levels of two
                roundings, the repeated-product multipliers)
  normalisation rtol = atol = 2e-4 against float64 at every mean / std ratio
  bookkeeping   score within (n / 1024 + 16) u sum|r| / n |scale| + 2 u |score| per row; variance chain bit-exact
Each test prints its largest error / bound (`-s`)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import rollout_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = 12345.0
U = R.U


@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    _lib.load()
    return _lib


class Guarded:
    """A device array of n elements between two sentinel guards; `offset` shifts its first element (alignment cases)."""

    def __init__(self, n, dtype=torch.float32, offset=0, init=None):
        self.n, self.lo = int(n), GUARD + offset
        self.full = torch.full((self.lo + self.n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        assert self.full.data_ptr() % 16 == 0
        self.t = self.full[self.lo:self.lo + self.n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(DEV))

    @property
    def ptr(self):
        return C.c_void_p(self.full.data_ptr() + self.lo * self.full.element_size())

    def get(self):
        torch.cuda.synchronize()
        full = self.full.cpu().numpy()
        assert (full[:self.lo] == SENTINEL).all(), "a kernel wrote in front of its array"
        assert (full[self.lo + self.n:] == SENTINEL).all(), "a kernel wrote past the end of its array"
        return full[self.lo:self.lo + self.n].copy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _ratio(err, bound):
    """Largest err / bound over the elements (a zero bound admits only a zero error)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


# ------------------------------------------------------------------------------------------------------------- launches
def run_sample(lib, mu, var, eps):
    n = mu.shape[0]
    act, logp = Guarded(n * 18), Guarded(n)
    dmu, dvar, deps = _dev(mu), _dev(var), _dev(eps)
    lib.check(lib.load().ppo_sample_logprob(_p(dmu), _p(dvar), _p(deps), act.ptr, logp.ptr, n, None), "ppo_sample_logprob")
    return act.get().reshape(n, 18), logp.get()


def run_gae(lib, r, v, vn, d, mode, expect=0):
    T, N = r.shape
    tgt, adv = Guarded(T * N), Guarded(T * N)
    dr, dv, dvn, dd = _dev(r), _dev(v), _dev(vn), _dev(d)
    rc = lib.load().ppo_td_gae(_p(dr), _p(dv), _p(dvn), _p(dd), 0.99, 0.95, T, N, tgt.ptr, adv.ptr, mode, None)
    assert rc == expect, (rc, lib.load().fly_last_error())
    return tgt.get().reshape(T, N), adv.get().reshape(T, N)


def run_gae_vnorm(lib, r, v, vn, d, mode):
    T, N = r.shape
    tgt, adv = Guarded(T * N), Guarded(T * N)
    sets = Guarded(lib.VALUE_NORM_SETS * lib.VALUE_NORM_SET, dtype=torch.float64)
    table = _dev(np.array([0.0, 1.0, 1.0, 0.0], np.float32))                   # the identity: vd = v * 1 + 0
    dr, dv, dvn, dd = _dev(r), _dev(v), _dev(vn), _dev(d)
    lib.check(lib.load().ppo_td_gae_vnorm(_p(dr), _p(dv), _p(dvn), _p(dd), _p(table), 0.99, 0.95, T, N, tgt.ptr, adv.ptr,
                                          sets.ptr, mode, None), "ppo_td_gae_vnorm")
    return tgt.get().reshape(T, N), adv.get().reshape(T, N), sets.get().reshape(-1, 3)


def run_adv_stats(lib, buf):
    stats = Guarded(514)
    lib.check(lib.load().ppo_adv_stats(buf.ptr, buf.n, stats.ptr, None), "ppo_adv_stats")
    return stats


def run_adv_apply(lib, buf, totals_ptr, count):
    lib.check(lib.load().ppo_adv_apply(buf.ptr, buf.n, totals_ptr, float(count), 1e-8, None), "ppo_adv_apply")
    return buf.get()


def run_adv_normalise(lib, a):
    buf = Guarded(a.size, init=a)
    stats = run_adv_stats(lib, buf)
    out = run_adv_apply(lib, buf, stats.ptr, a.size)
    return out, stats.get()[:2]


def run_rollout_book(lib, reward, rows, n, score0, scale, var0, decay, var_min):
    """reward: a Guarded holding [rows][n]."""
    terms, score = Guarded(max(rows, 1)), Guarded(1, init=np.float32([score0]))
    var = Guarded(len(var0), init=np.float32(var0))
    applied = Guarded(1, dtype=torch.int32, init=np.int32([5]))
    lib.check(lib.load().ppo_rollout_bookkeeping(reward.ptr, rows, n, terms.ptr, score.ptr, C.c_float(scale), var.ptr, len(var0),
                                                 C.c_float(decay), C.c_float(var_min), applied.ptr, None), "ppo_rollout_bookkeeping")
    return score.get()[0], var.get(), int(applied.get()[0]), terms.get()


def run_step_book(lib, reward, rows, n, score0, scale, var0, decay, var_min):
    score, var = Guarded(1, init=np.float32([score0])), Guarded(len(var0), init=np.float32(var0))
    for r in range(rows):
        row = C.c_void_p(reward.ptr.value + 4 * r * n)
        lib.check(lib.load().ppo_step_bookkeeping(row, n, score.ptr, C.c_float(scale), var.ptr, len(var0), C.c_float(decay),
                                                  C.c_float(var_min), None), "ppo_step_bookkeeping")
    return score.get()[0], var.get()


# -------------------------------------------------------------------------------------------------------------- sampling
def sample_case(n, mu_scale):
    """var log-spaced over the schedule's range [var_min = 0.01, 1]; mu wide enough that both clips fire; eps with exact 0 and
    +-4; entries with eps = 0 and mu = +-1 land exactly on the clip, entries with mu = +-1.3 exactly behind it."""
    rng = np.random.default_rng(1000 + n)
    var = np.geomspace(0.01, 1.0, 18).astype(np.float32)
    mu = rng.uniform(-mu_scale, mu_scale, (n, 18)).astype(np.float32)
    eps = rng.normal(0, 1, (n, 18)).astype(np.float32)
    k = np.arange(n * 18).reshape(n, 18)
    eps[k % 11 == 3], eps[k % 11 == 6], eps[k % 11 == 8] = 0.0, 4.0, -4.0
    for rem, m in ((0, 1.0), (5, -1.0), (7, 1.3), (9, -1.3)):
        mu[k % 23 == rem], eps[k % 23 == rem] = m, 0.0
    return mu, var, eps


@pytest.mark.parametrize("mu_scale", [1.5, 50.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 209])
def test_sample_logprob_against_float64(lib, n, mu_scale):
    mu, var, eps = sample_case(n, mu_scale)
    act, logp = run_sample(lib, mu, var, eps)
    a64, clip64, logp64 = R.sample_logprob64(mu, var, eps)
    want = R.sample_action32(mu, var, eps)
    assert (want == 1.0).any() and (want == -1.0).any() and (np.abs(a64) > 1.0).any()
    assert (np.abs(act.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()          # 1 ulp of the float32 value
    L = np.sqrt(var.astype(np.float64))
    assert (np.abs(act - clip64) <= U * (2 * np.abs(L * eps) + np.abs(a64)) + 1e-12).all()     # and three roundings off float64
    k = np.arange(n * 18).reshape(n, 18)
    assert (act[k % 23 == 0] == 1.0).all() and (act[k % 23 == 5] == -1.0).all()
    canc = R.logprob_cancellation64(mu, var, eps)
    bar = 1e-5 + 2e-6 * np.abs(logp64)
    err = np.abs(logp - logp64)
    print("sample n=%d |mu|<=%g: max logp error / bound %.3f (cancellation term up to %.1f x the bar)"
          % (n, mu_scale, _ratio(err, bar + canc), (canc / bar).max()))
    if mu_scale > 10 and n > 1:
        assert (canc > bar).any()                                   # the wide set exists so that this term dominates
    assert (err <= bar + canc).all()


# ------------------------------------------------------------------------------------------------------------------- GAE
@functools.lru_cache(maxsize=None)
def gae_case(T, N, mode):
    """Inputs and their float64 reference, computed once per shape.  Env patterns of `done`, cycled over the envs starting at
    T mod 5 (so N = 1 meets all of them over the T list): random, all zero, all one, a single zero at t = 0, a single zero
    at t = T - 1 (the last two per step only)."""
    rng = np.random.default_rng(7 * T + N)
    r = rng.normal(0.5, 1, (T, N)).astype(np.float32)
    v, vn = rng.normal(0, 1, (T, N)).astype(np.float32), rng.normal(0, 1, (T, N)).astype(np.float32)
    d = (rng.random((T, N)) < 0.9).astype(np.float32)
    for e in range(N):
        pat = (e + T) % 5
        if pat in (1, 2):
            d[:, e] = pat - 1
        elif pat == 3:
            d[:, e] = 1; d[0, e] = 0
        elif pat == 4:
            d[:, e] = 1; d[T - 1, e] = 0
    if not mode & 1:
        d = d[T // 2].copy()
    gamma, gl = R.gamma_gl32()
    ref = R.td_gae64(r, v, vn, d, gamma, gl, mode)
    return r, v, vn, d, ref


def check_target(tgt, ref):
    assert (np.abs(tgt - ref.target) <= R.target_bound64(ref)).all()


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("T,N", [(1, 1), (1, 65), (9, 63), (9, 64), (17, 129)])
def test_td_gae_against_float64(lib, T, N, mode):
    r, v, vn, d, ref = gae_case(T, N, mode)
    tgt, adv = run_gae(lib, r, v, vn, d, mode)
    check_target(tgt, ref)
    err = np.abs(adv - ref.adv)
    print("gae T=%d N=%d mode=%d: max advantage error / first-order bound %.3f" % (T, N, mode, _ratio(err, ref.bound)))
    assert (err <= 2 * ref.bound).all()


SCAN_T = [1, 2, 63, 64, 65, 127, 128, 129, 200, 4097]
SCAN_MARGIN = 4


def check_scan(tag, T, N, mode, tgt, adv, ref, where=None):
    """`where`: a function of the bool [T][N] of the rows that miss -> what the failing assertion says about them."""
    check_target(tgt, ref)
    bound = ref.bound + R.scan_carry_bound64(ref.delta, R.gamma_gl32()[1])
    err = np.abs(adv - ref.adv)
    print("%s T=%d N=%d mode=%d: max advantage error / bound %.3f (the carries are up to %.2f of the bound)"
          % (tag, T, N, mode, _ratio(err, bound), float(np.max(1 - ref.bound / bound))))
    miss = ~(err <= SCAN_MARGIN * bound)
    assert not miss.any(), where(miss) if where else None


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("T", SCAN_T)
def test_td_gae_scan_against_float64(lib, T, N, mode):
    r, v, vn, d, ref = gae_case(T, N, mode)
    tgt, adv = run_gae(lib, r, v, vn, d, mode | R.GAE_SCAN)
    check_scan("scan", T, N, mode, tgt, adv, ref)


def test_td_gae_scan_rejects_the_masked_recurrence(lib):
    r, v, vn, d, _ = gae_case(9, 63, 3)
    tgt, adv = run_gae(lib, r, v, vn, d, R.GAE_SCAN | 3, expect=-1)
    assert (tgt == SENTINEL).all() and (adv == SENTINEL).all()                 # rejected before any launch


@pytest.mark.parametrize("T", SCAN_T)
def test_td_gae_vnorm_scan_copy_against_float64(lib, T):
    """The value-normalising instance of the scan (ppo_td_gae_vnorm_scan_kernel, once a copy in value_norm.hip, now the same
    td_gae_scan_env in another grid mapping): under the identity table it is held to the same reference and bound, equals
    ppo_td_gae's scan bit for bit, and counts every target exactly once in its moment sets."""
    N, mode = 3, T % 2
    r, v, vn, d, ref = gae_case(T, N, mode)
    tgt, adv, sets = run_gae_vnorm(lib, r, v, vn, d, mode | R.GAE_SCAN)
    check_scan("vnorm scan", T, N, mode, tgt, adv, ref)
    t0, a0 = run_gae(lib, r, v, vn, d, mode | R.GAE_SCAN)
    assert np.array_equal(tgt, t0) and np.array_equal(adv, a0)
    assert sets[:, 0].sum() == T * N
    np.testing.assert_allclose((sets[:, 0] * sets[:, 1]).sum() / (T * N), ref.target.mean(), rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ advantage normalisation
ADV_CASES = [(0, 1.0), (3, 1.0), (30, 1.0), (100, 1.0), (300, 1.0), (0, 1e-3), (30, 1e-3), (0, 1e3), (30, 1e3)]


@pytest.mark.parametrize("n", [2, 7, 255, 256, 257, 65537, 655360])
def test_advantage_normalisation_against_float64(lib, n):
    z = np.random.default_rng(n).normal(0, 1, n)
    worst = {}
    for ratio, std in ADV_CASES:
        a = (std * (ratio + z)).astype(np.float32)
        out, stats = run_adv_normalise(lib, a)
        want, total, mean, sd = R.adv_normalise64(a)
        err = np.abs(out - want)
        worst[(ratio, std)] = _ratio(err, 2e-4 + 2e-4 * np.abs(want))
        np.testing.assert_allclose(out, want, rtol=2e-4, atol=2e-4, err_msg="mean/std %g at std %g" % (ratio, std))
        np.testing.assert_allclose(float(stats[0]), total, rtol=1e-4, atol=1e-2)            # stats[0] stays the sum
        np.testing.assert_allclose(float(stats[0]), total, rtol=2 ** -23, atol=0)            # accumulated in float64, rounded once
        np.testing.assert_allclose(float(stats[1]), sd * sd * (n - 1), rtol=1e-6, atol=0)    # the centred second moment
    print("adv normalise n=%d: max error / bar per (mean/std, std): %s"
          % (n, ", ".join("(%g, %g) %.4f" % (k + (x,)) for k, x in worst.items())))


@pytest.mark.parametrize("n", [4099, 65537])
def test_advantage_normalisation_two_ranks(lib, n):
    """Two ranks at kernel level: halves of mean 0 and 50, statistics per half, combined by ppo.py's own combine_adv_stats,
    applied to both halves with the global count == float64 on the whole array."""
    from fly_bproject_amd.ppo import combine_adv_stats
    rng = np.random.default_rng(n)
    halves = [rng.normal(m, 1.0, n).astype(np.float32) for m in (0.0, 50.0)]
    bufs = [Guarded(n, init=h) for h in halves]
    pairs = [run_adv_stats(lib, b) for b in bufs]
    ranks = torch.stack([s.t[:2] for s in pairs])
    totals = Guarded(2, init=np.zeros(2, np.float32))
    totals.t.copy_(combine_adv_stats(ranks, n))
    want = R.adv_normalise64(np.concatenate(halves))[0]
    out = np.concatenate([run_adv_apply(lib, b, totals.ptr, 2 * n) for b in bufs])
    for s in pairs + [totals]:
        s.get()
    print("adv normalise, two ranks n=%d: max error / bar %.4f" % (n, _ratio(np.abs(out - want), 2e-4 + 2e-4 * np.abs(want))))
    np.testing.assert_allclose(out, want, rtol=2e-4, atol=2e-4)


def test_adv_stats_rejects_a_misaligned_scratch(lib):
    buf, stats = Guarded(8, init=np.ones(8, np.float32)), Guarded(516)
    assert lib.load().ppo_adv_stats(buf.ptr, 8, C.c_void_p(stats.ptr.value + 4), None) == -1
    stats.get()


# ------------------------------------------------------------------------------------------------------------ bookkeeping
BOOK_PAIRS = [(1e-5, 0.2), (1e-3, 0.0105), (0.0, 0.2)]         # (decay, starting variance); var_min = 0.01 clamps the second


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099, 8190])
def test_bookkeeping_against_float64(lib, n):
    """Both ABI entries: the score against the float64 mean (rewards of mean 1 / std 1, so a dropped tail element is far
    outside the bound), the variance chain bit for bit, rows_applied; reward rows 16-byte aligned and off by one float (with
    n % 4 != 0 and rows = 3 every other row is misaligned anyway, as in training at 4099 or 8190 envs)."""
    rng = np.random.default_rng(n)
    worst = 0.0
    for rows in (1, 3):
        rew = rng.normal(1.0, 1.0, (rows, n)).astype(np.float32)
        for offset in (0, 1):
            reward = Guarded(rows * n, offset=offset, init=rew)
            assert (reward.ptr.value % 16 == 0) == (offset == 0)
            for nvar in (0, 18, 63, 256):
                for decay, v0 in BOOK_PAIRS:
                    var0 = np.linspace(v0, 1.5 * v0, nvar).astype(np.float32)
                    score, tol, var = R.bookkeeping64(rew, 0.25, 0.01, var0, decay, 0.01)
                    s1, v1 = run_step_book(lib, reward, rows, n, 0.25, 0.01, var0, decay, 0.01)
                    assert abs(s1 - score) <= tol, ("step", rows, offset, nvar, decay, s1, score, tol)
                    assert np.array_equal(v1, var)
                    worst = max(worst, abs(s1 - score) / tol)
                    if nvar > 63:
                        continue                                     # the row-block form takes at most 63
                    s2, v2, applied, terms = run_rollout_book(lib, reward, rows, n, 0.25, 0.01, var0, decay, 0.01)
                    assert abs(s2 - score) <= tol, ("rollout", rows, offset, nvar, decay, s2, score, tol)
                    assert np.array_equal(v2, var) and applied == 5 + rows
                    np.testing.assert_allclose(terms, rew.astype(np.float64).mean(axis=1) * float(np.float32(0.01)), rtol=0,
                                               atol=tol)
                    worst = max(worst, abs(s2 - score) / tol)
            reward.get()
    print("bookkeeping n=%d: max score error / bound %.3f" % (n, worst))


def test_rollout_bookkeeping_of_no_rows_is_a_no_op(lib):
    reward = Guarded(8, init=np.ones(8, np.float32))
    var0 = np.full(18, 0.2, np.float32)
    score, var, applied, terms = run_rollout_book(lib, reward, 0, 8, 0.25, 0.01, var0, 1e-3, 0.01)
    assert score == np.float32(0.25) and np.array_equal(var, var0) and applied == 5 and (terms == SENTINEL).all()
