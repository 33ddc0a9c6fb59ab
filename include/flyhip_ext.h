/*
 * flyhip_ext.h -- entry points added to libflyhip.so since the prototype list of flyhip.h was fixed at ABI version 13.
 *
 * flyhip.h includes this file at its end, so C and C++ callers include flyhip.h alone and see everything; the types and the
 * FLY_* / PPO_GAE_* macros used here are flyhip.h's.  The Python binding keeps the two lists apart in the same way
 * (fly_bproject_amd/_lib.py: SYMBOLS for flyhip.h, SYMBOLS_EXT for this file, reached through _lib.ext()), each held to its
 * header, prototype by prototype, by the tests.  An entry point added here does not move FLY_ABI_VERSION: that moves only when
 * an existing argument list or structure changes.
 */
#ifndef FLYHIP_EXT_H
#define FLYHIP_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Running reward scaling (opt-in, PPO --normalize_reward): rewards divided by the running standard
 * deviation of the discounted return (gymnasium's NormalizeReward, SB3's VecNormalize(norm_reward=True)), in front of the
 * unchanged GAE entry points.  Per env e, with the carry G[e] (f64, the discounted return of the env's open episode) living
 * across rollouts, t = 0 .. T-1, from the reward row and the int64 reset-flag row the rollout writes:
 *     G = fl(fl(g * G) + (double)reward[t][e])      g = (double)gamma; two separately rounded float64 ops, no fma
 *     the moments take G                            every (t, e) counts, the step that performs a reset too
 *     reset[t][e] != 0:  G = 0                      ppo_episode_stats' end rule: the end row's reward belongs to the closing episode
 * ppo_reward_returns reads carry_in f64 [N] and writes carry_out f64 [N] (the same buffer, or one that does not overlap it)
 *   and the float64 moments (count | mean | M2) of all T x N values of G, one set per workgroup in
 *   sets f64 [FLY_VALUE_NORM_SETS][FLY_VALUE_NORM_SET] (workgroups with no env write 0 | 0 | 0): what ppo_value_norm_merge
 *   folds into the running statistics S_r = count | mean | var (initially 0 | 0 | 1), whose table entry r = (float)(1 /
 *   sqrt(var + 1e-5)) scales the rewards; the mean is tracked and not used.  Per-lane Welford updates and a fixed
 *   combination tree, no atomics: deterministic.  mode_flags: 0 (lane = env, t walks forward: numpy float64 reproduces the
 *   carries bit for bit) or PPO_GAE_SCAN (one wave per env, time on lanes: the chunks' affine maps G_out = a G_in + b
 *   composed by a shuffle scan, for few envs x very long rollouts; the counts are identical, the carries agree to float64
 *   rounding, and an end passes on exactly nothing from before it).  A NaN reward makes its env's G NaN until that env's next
 *   end; the other envs' carries do not see it.  Anything else, a NULL pointer, T < 1, N < 1, a misaligned buffer, a
 *   carry_out that partly overlaps carry_in or a T * N that overflows: FLY_E_ARG, and nothing is written.
 * ppo_reward_scale: out[i] = clamp(reward[i] * table[2], -clip, +clip) for n elements, one rounded fp32 multiply and a clamp
 *   by comparisons (float32 numpy reproduces it bit for bit; NaN passes through, +-inf lands on +-clip).  `table` is the
 *   m | s | r | 0 table ppo_value_norm_merge writes.  out may be `reward` itself, but must not partly overlap it.  16-byte
 *   accesses when both are 16-byte aligned, a scalar path with identical results otherwise.  A NULL pointer, n < 1, a clip
 *   that is not > 0 or a misaligned buffer: FLY_E_ARG. */
int ppo_reward_returns(const float* reward, const int64_t* reset, float gamma, int64_t T, int64_t N, const double* carry_in,
                       double* carry_out, double* sets, int mode_flags, void* stream);
int ppo_reward_scale(const float* reward, int64_t n, const float* table, float clip, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLYHIP_EXT_H */
