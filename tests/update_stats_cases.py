"""Seeded cases for the PPO update diagnostics (tests/update_stats_ref.py has the definitions).  Every case has
  - a var that differs in all 18 columns (a wrong column index in the kernel's flat layout shows in M),
  - ratios on both sides of both clip edges (0.7, 0.79 | 0.81, ~1, 1.19 | 1.21, 1.4, and a spread around 1),
  - advantages of both signs and exactly 0,
  - |v - target| below, exactly at and above 1 (dyadic targets and offsets: the fp32 difference is exact),
  - distinct rows,
  - with bad=True (R >= 8): one row with a NaN mu, one with a +inf target and one with lr = 100 (> 88: expf overflows).
No finite row's ratio lies within its rounding margin of a clip edge: `case` nudges such rows (ref.clip_margin_ok is then
asserted by the CPU tests for every case the GPU tests use)."""
import collections

import numpy as np

from tests import update_stats_ref as ref

CLIP = 0.2
LR_TARGETS = np.log(np.array([0.7, 0.79, 0.81, 1.0, 1.19, 1.21, 1.4]))
DV = np.array([0.25, 1.0, 1.75, -0.5, -1.0, -2.5, 0.0])             # v - target: below, at, above the Huber kink, both signs
KINK = np.array([False, True, False, False, True, False, True])     # these stay exactly as they are (no jitter)

Case = collections.namedtuple("Case", "mu action old_logp adv v target var clip bad_rows")


def case(R, seed, bad=False):
    rng = np.random.default_rng(1000 * seed + R)
    var = (np.linspace(0.06, 0.45, ref.NA) * (1.0 + 0.01 * (seed % 7)))[rng.permutation(ref.NA)].astype(np.float32)
    assert len(set(var.tolist())) == ref.NA and (var < 1).all()
    mu = (0.3 * rng.standard_normal((R, ref.NA))).astype(np.float32)
    action = (mu + np.sqrt(var) * rng.standard_normal((R, ref.NA))).astype(np.float32)
    i = np.arange(R)
    # the log-ratio each row should have: the seven edge values in turn, every eighth row a draw around 0
    want = np.where(i % 8 == 7, 0.15 * rng.standard_normal(R), LR_TARGETS[i % 8 % 7] + 1e-3 * rng.standard_normal(R))
    M = ref.mahalanobis32(mu, action, var).astype(np.float64)
    logp = -0.5 * (ref.LOG_2PI_18 + M) - np.log(np.sqrt(var.astype(np.float64))).sum()
    old_logp = (logp - want).astype(np.float32)
    adv = (rng.standard_normal(R) * np.array([1.0, -1.0, 0.0])[(i // 2) % 3]).astype(np.float32)     # +, +, -, -, 0, 0, ...
    target = (np.round(2.0 * rng.standard_normal(R) * 64) / 64).astype(np.float32)
    k = (i // 3) % 7
    jitter = np.where(KINK[k], 0.0, rng.integers(-64, 65, R) / 1024.0)
    v = (target.astype(np.float64) + DV[k] + jitter).astype(np.float32)
    bad_rows = ()
    if bad:
        assert R >= 8
        bad_rows = (R // 7, R // 2, R - 1)
        mu[bad_rows[0], 3] = np.nan
        target[bad_rows[1]] = np.inf
        old_logp[bad_rows[2]] = np.float32(logp[bad_rows[2]] - 100.0)
    # nudge what sits within its margin of a clip edge (four margins, so the condition holds with room)
    for _ in range(8):
        t = ref.row_terms(mu, action, old_logp, adv, v, target, var, CLIP)
        with np.errstate(invalid="ignore"):
            near = t.finite & ((np.abs(t.ratio - t.lo) <= 4 * t.rb) | (np.abs(t.ratio - t.hi) <= 4 * t.rb))
        if not near.any():
            break
        old_logp[near] += np.float32(0.01)
    assert len({r.tobytes() for r in mu}) == R
    return Case(mu, action, old_logp, adv, v, target, var, CLIP, bad_rows)


# what tests/test_update_stats_gpu.py runs: (R, seed, bad).  256 workgroups x 256 rows is one full grid stride.
FULL_STRIDE = 256 * 256
GPU_CASES = [(1, 0, False), (63, 1, True), (64, 2, False), (65, 3, True), (255, 4, True), (256, 5, False), (257, 6, True),
             (1027, 7, True), (FULL_STRIDE + 257, 8, True)]
