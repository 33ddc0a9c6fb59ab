/*
 * flyhip_update_stats.h -- PPO update diagnostics (opt-in, PPO --update_stats): two entry points of
 * libflyhip.so added after the prototype lists of flyhip.h and flyhip_ext.h were fixed.
 *
 * flyhip.h includes this file at its end, behind flyhip_ext.h, so C and C++ callers include flyhip.h alone; the FLY_* codes
 * used here are flyhip.h's.  The Python binding keeps a third list for it (fly_bproject_amd/_lib.py: SYMBOLS_UPDATE_STATS,
 * reached through _lib.update_stats_api()), held to this header prototype by prototype by the tests.  FLY_ABI_VERSION does not
 * move: no existing argument list or structure changes.
 */
#ifndef FLYHIP_UPDATE_STATS_H
#define FLYHIP_UPDATE_STATS_H

#include <stdint.h>

#define FLY_UPDATE_STATS_SET 17    /* one set of update statistics (f64), the table below */
#define FLY_UPDATE_STATS_SETS 256  /* sets ppo_update_stats writes (one per workgroup) */

#ifdef __cplusplus
extern "C" {
#endif

/* How far an update moved the policy, how much of the surrogate was clipped and how well the critic fits its targets: a
 * probe BEHIND the finished update.  The caller evaluates the updated network on the rollout's R rows (mlp_forward: mu f32
 * [R][18], v f32 [R]) and hands them in with the rollout's action f32 [R][18], old_logp / adv / target f32 [R], the action
 * variance var f32 [18] and the clip range.  Per row, in fp32 with separately rounded ops (no fma):
 *     L_d = sqrtf(var_d),  hld = sum_d logf(L_d) in d order,  inv_var_d = 1.0f / var_d      once per launch, as ppo_sample_logprob
 *     M     = sum_d ((a_d - mu_d)^2 * inv_var_d)          d = 0 .. 17 in order, from 0: float32 numpy reproduces M bit for bit
 *     logp  = -0.5f * (33.08178959434617f + M) - hld;   lr = logp - old_logp;   ratio = expf(lr)
 *     pol   = -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A),   hub = smooth_l1(v - target)      the update kernels' own
 *                                                                  loss lines (csrc/loss_head.inc), with inv_batch = 1
 *     clipped = !(ratio >= 1 - clip && ratio <= 1 + clip)          the loss head's CLOSED interval, 1 -+ clip formed in fp32
 * A row is NON-FINITE when any of lr, ratio, A, v, target is NaN or +-inf (an lr above about 88 makes ratio inf; a var that
 * is 0, negative or NaN makes every row non-finite): it counts in `rows` and `nonfinite` and in nothing else.  Finite rows
 * accumulate in float64.  A set is FLY_UPDATE_STATS_SET doubles:
 *      0      rows                               every row, finite or not
 *      1      sum of -lr                         k1: its mean over the finite rows estimates KL(old || new)
 *      2      sum of (double)ratio - 1 - (double)lr      Schulman's k3, each term >= 0 up to rounding: `approx_kl`
 *      3      clipped                            count
 *      4, 5   ratio min, max
 *      6      sum of pol
 *      7      sum of hub
 *      8-10   n | mean | M2 of target            float64 Welford updates and Chan et al.'s merge (csrc/value_norm.h)
 *      11-13  n | mean | M2 of the residual (double)target - (double)v        explained variance = 1 - M2_res / M2_target
 *      14     nonfinite                          count
 *      15     max |A|
 *      16     max |target|
 * The empty set is 0 | 0 | 0 | 0 | +inf | -inf | 0 | 0 | 0 0 0 | 0 0 0 | 0 | 0 | 0.  Counts are exact integers.
 * ppo_update_stats writes sets f64 [FLY_UPDATE_STATS_SETS][FLY_UPDATE_STATS_SET]: always that many workgroups, grid-stride
 *   over tiles of 256 rows, one set each; a workgroup without rows writes the empty set; the sets' `rows` sum to R.  Every
 *   reduction is a fixed tree, no atomics: the same input gives the same bits.  mu and action are read as flat arrays, with
 *   16-byte loads when both bases are 16-byte aligned and a scalar path with identical results otherwise (4-byte alignment
 *   is all that is required).  One launch, no host sync, graph-capturable.  Nothing but `sets` is written.
 * ppo_update_stats_merge: one workgroup folds sets[0 .. nsets) in index order (all ranks' sets in rank order) into one set,
 *   writes that set to `last` and folds it into the persistent sets `window` (since the caller last reset it) and `total`,
 *   in place.  The fold: sums and counts add, min and max combine, the moments go through Chan et al.'s merge, and a set
 *   without rows is skipped.  `last`, `window` and `total` must not overlap each other.
 * FLY_E_ARG, before any HIP call and with nothing written: a NULL pointer, R < 1, nsets < 1, a clip that is not in (0, 1)
 *   (a NaN included), a float buffer that is not 4-byte aligned or a double buffer that is not 8-byte aligned, an R * 18 or an
 *   nsets * FLY_UPDATE_STATS_SET that overflows a byte offset, and persistent sets that overlap. */
int ppo_update_stats(const float* mu, const float* action, const float* old_logp, const float* adv, const float* v,
                     const float* target, const float* var, float clip, int64_t R, double* sets, void* stream);
int ppo_update_stats_merge(const double* sets, int64_t nsets, double* last, double* window, double* total, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLYHIP_UPDATE_STATS_H */
