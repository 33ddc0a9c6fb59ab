"""PPO update diagnostics (PPO --update_stats) restated in numpy from the definitions in
include/flyhip_update_stats.h, not from the kernels.

M is formed in float32 in the kernel's op order (so it is the kernel's M bit for bit); everything behind it is float64 arithmetic
on the fp32 inputs.  The kernel's fp32 log-ratio then differs from this file's by rounding alone, and `row_terms` returns, per row,
a bound b_i on that difference and what follows from it for every sum -- derived below from the definition's op count, never
from a measured error.

The bound.  u = 2^-24 (unit roundoff of fp32); a correctly rounded op has relative error <= u (+, -, *, 1/x and sqrtf are:
hipcc's default is correctly rounded division and square root); logf and expf are documented by the HIP math API at 1 ulp
= 2u relative.  With C = 33.08... (gauss_logp's constant), S = sum_d |ln L_d| (= |hld| when every var_d is on one side of 1) and first
order in u:
    L_d = sqrtf(var_d)                     relative u          -> |ln L_d| moves by u
    logf(L_d)                              relative 2u         -> 2u |ln L_d|
    17 additions of the d-ordered sum      each u |partial|    -> 17 u S
  so |hld32 - hld64| <= 18 u + 19 u S.
    the constant C as a float              0.5 u C             (it enters through the factor -0.5)
    C + M                                  0.5 u (C + M)
    * -0.5                                 exact
    - hld                                  u |logp| <= u (0.5 (C + M) + S)
    - old_logp                             u |lr|   <= u (0.5 (C + M) + S + |old_logp|)
  With B_i = 0.5 (C + M_i) + S + |old_logp_i| and 18 u <= 1.09 u 0.5 C, the sum is at most
    u (0.5 (C + M_i) (1 + 1 + 1 + 1 + 1.09) + S (19 + 1 + 1) + |old_logp_i|) <= 21 u B_i,
  and K = 22 leaves the second-order terms their room:   b_i = 22 u (0.5 (33.08 + M_i) + S + |old_logp_i|).
From it:  ratio32 = expf(lr32) against exp(lr64):  rb_i = ratio64 (expm1(b_i) (1 + 2u) + 2u);  a k3 term rb_i + b_i;
    pol = -min(ratio A, clamp(ratio) A): min is 1-Lipschitz in the pair, each product rounds once:  |A| (rb_i + u (ratio64 + rb_i));
    hub: dv = v - target rounds once (u |dv|), huber is 1-Lipschitz and rounds once more (u hub; the 0.5 factor is exact):
         u (|dv| + hub) (1 + 1e-6).
Float64 accumulation (the kernel's tree, this file's pairwise sums) adds at most n 2^-52 sum |x_i|, included in `sum_bound`.
"""
import collections

import numpy as np

NA = 18
SET = 17
SETS = 256
U = 2.0 ** -24
K = 22.0
# the loss head's constant (csrc/loss_head.inc GAUSS_DIM_LOG_2PI = 33.08178959434617f, its "18 ln 2 pi") as the float it is: the
# definition of gauss_logp, so an input here; the bound keeps its 0.5 u C term for it all the same
LOG_2PI_18 = float(np.float32(33.08178959434617))
(ROWS, K1, K3, CLIPPED, RMIN, RMAX, POL, HUB, TN, TMEAN, TM2, EN, EMEAN, EM2, NONFINITE, AMAX, TMAX) = range(SET)
COUNTS = (ROWS, CLIPPED, TN, EN, NONFINITE)
EXACT = (ROWS, CLIPPED, TN, EN, NONFINITE, AMAX, TMAX)   # what the kernel must reproduce exactly under the case condition
SUMS = (K1, K3, POL, HUB)

Rows = collections.namedtuple("Rows", "M lr ratio finite clipped k1 k3 pol hub b rb b_k3 b_pol b_hub lo hi")


def empty_set():
    s = np.zeros(SET)
    s[RMIN], s[RMAX] = np.inf, -np.inf
    return s


def mahalanobis32(mu, action, var):
    """M in float32 in the kernel's op order: inv_var = 1 / var, ((a - mu) * (a - mu)) * inv_var, summed d = 0 .. 17 from 0."""
    mu, action, var = (np.asarray(x, dtype=np.float32) for x in (mu, action, var))
    with np.errstate(all="ignore"):
        inv_var = (np.float32(1.0) / var).astype(np.float32)
        M = np.zeros(mu.shape[0], dtype=np.float32)
        for d in range(NA):
            diff = (action[:, d] - mu[:, d]).astype(np.float32)
            e = ((diff * diff).astype(np.float32) * inv_var[d]).astype(np.float32)
            M = (M + e).astype(np.float32)
    return M


def clip_edges(clip):
    """The loss head's closed interval: 1 -+ clip formed in float32, as float64 numbers."""
    c = np.float32(clip)
    return float(np.float32(1.0) - c), float(np.float32(1.0) + c)


def row_terms(mu, action, old_logp, adv, v, target, var, clip):
    """Per row: the float64 terms of the set from the fp32 inputs (M the kernel's), the non-finite rule, and the bounds."""
    old_logp, adv, v, target = (np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64) for x in (old_logp, adv, v, target))
    var64 = np.asarray(var, dtype=np.float32).astype(np.float64)
    M = mahalanobis32(mu, action, var).astype(np.float64)
    lo, hi = clip_edges(clip)
    with np.errstate(all="ignore"):
        logs = np.log(np.sqrt(var64))
        hld, S = logs.sum(), np.abs(logs).sum()
        lr = -0.5 * (LOG_2PI_18 + M) - hld - old_logp
        ratio = np.exp(lr)
        # float32 overflow of expf is part of the rule: an lr whose fp32 ratio is inf (above ~88.72) is non-finite
        finite = (np.isfinite(lr) & np.isfinite(ratio) & (ratio <= np.finfo(np.float32).max) & np.isfinite(adv) & np.isfinite(v)
                  & np.isfinite(target))
        clipped = ~((ratio >= lo) & (ratio <= hi))
        s1, s2 = ratio * adv, np.clip(ratio, lo, hi) * adv
        pol = -np.minimum(s1, s2)
        dv = v - target
        hub = np.where(np.abs(dv) < 1.0, 0.5 * dv * dv, np.abs(dv) - 0.5)
        b = K * U * (0.5 * (LOG_2PI_18 + M) + S + np.abs(old_logp))
        rb = ratio * (np.expm1(b) * (1 + 2 * U) + 2 * U)
        b_pol = np.abs(adv) * (rb + U * (ratio + rb))
        b_hub = U * (np.abs(dv) + hub) * (1 + 1e-6)
    return Rows(M, lr, ratio, finite, clipped, -lr, ratio - 1.0 - lr, pol, hub, b, rb, rb + b, b_pol, b_hub, lo, hi)


def moments(x):
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0.0, 0.0, 0.0
    mean = x.mean()
    return float(x.size), float(mean), float(((x - mean) ** 2).sum())


def set_of(mu, action, old_logp, adv, v, target, var, clip):
    """The set of all given rows."""
    t = row_terms(mu, action, old_logp, adv, v, target, var, clip)
    return set_from_terms(t, adv, v, target)


def set_from_terms(t, adv, v, target):
    adv, v, target = (np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64) for x in (adv, v, target))
    f = t.finite
    s = empty_set()
    s[ROWS], s[NONFINITE] = f.size, f.size - f.sum()
    if f.any():
        s[K1], s[K3], s[CLIPPED] = t.k1[f].sum(), t.k3[f].sum(), t.clipped[f].sum()
        s[RMIN], s[RMAX] = t.ratio[f].min(), t.ratio[f].max()
        s[POL], s[HUB] = t.pol[f].sum(), t.hub[f].sum()
        s[TN], s[TMEAN], s[TM2] = moments(target[f])
        s[EN], s[EMEAN], s[EM2] = moments(target[f] - v[f])
        s[AMAX], s[TMAX] = np.abs(adv[f]).max(), np.abs(target[f]).max()
    return s


def sum_bound(t, field):
    """The bound on |kernel's sum - this file's| for one of SUMS: the per-row bounds of the finite rows, plus float64 accumulation."""
    f = t.finite
    per_row, terms = {K1: (t.b, t.k1), K3: (t.b_k3, t.k3), POL: (t.b_pol, t.pol), HUB: (t.b_hub, t.hub)}[field]
    n = int(f.sum())
    return float(per_row[f].sum() + n * 2.0 ** -52 * (np.abs(terms[f]).sum() + per_row[f].sum()))


def extreme_bound(t):
    """The bound on the ratio extremes: the largest per-row ratio bound among the finite rows."""
    return float(t.rb[t.finite].max()) if t.finite.any() else 0.0


def clip_margin_ok(t):
    """The condition on the cases: no finite row's float64 ratio lies within its rb_i of an edge of the clip interval.  Under it
    the kernel's fp32 ratio falls on the same side of both edges as this file's, so the clipped count must match exactly."""
    f = t.finite
    near = (np.abs(t.ratio - t.lo) <= t.rb) | (np.abs(t.ratio - t.hi) <= t.rb)
    return not bool((near & f).any())


def moments_merge(n, mean, m2, nb, mb, qb):
    """Chan et al.'s merge as csrc/value_norm.h writes it; an empty side leaves the other as it is."""
    if not nb > 0.0:
        return n, mean, m2
    if not n > 0.0:
        return nb, mb, qb
    t, d = n + nb, mb - mean
    inv = 1.0 / t
    return t, mean + d * (nb * inv), m2 + (qb + d * d * (n * nb * inv))


def merge(a, b):
    """a + b by the fold rule: sums and counts add, extremes combine, moments by Chan's merge; a set without rows is skipped."""
    a, b = np.array(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not b[ROWS] > 0.0:
        return a
    for k in (ROWS, K1, K3, CLIPPED, POL, HUB, NONFINITE):
        a[k] = a[k] + b[k]
    a[RMIN], a[RMAX] = min(a[RMIN], b[RMIN]), max(a[RMAX], b[RMAX])
    a[TN], a[TMEAN], a[TM2] = moments_merge(a[TN], a[TMEAN], a[TM2], b[TN], b[TMEAN], b[TM2])
    a[EN], a[EMEAN], a[EM2] = moments_merge(a[EN], a[EMEAN], a[EM2], b[EN], b[EMEAN], b[EM2])
    a[AMAX], a[TMAX] = max(a[AMAX], b[AMAX]), max(a[TMAX], b[TMAX])
    return a


def merge_all(sets):
    """sets[0 .. k) folded in index order into one set."""
    out = empty_set()
    for s in np.asarray(sets, dtype=np.float64).reshape(-1, SET):
        out = merge(out, s)
    return out
