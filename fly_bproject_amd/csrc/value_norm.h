// value_norm.h — running value normalisation (PPO --normalize_value): the layouts, the two maps and the float64 moments (Welford
// update, Chan merge, the wave and workgroup reductions) shared by value_norm.hip and every kernel that writes moment sets.
//
//   table   f32 [VALUE_NORM_TABLE]: m | s | r | 0        vd = v * s + m (critic output -> reward units), y = (tg - m) * r
//   stats   f64 [VALUE_NORM_SET]:   count | mean | var   the running statistics S_v of the TD targets (population variance)
//   moments f64 [k][VALUE_NORM_SET]: count | mean | M2   batch moments, one set per workgroup of the GAE pass
#ifndef VALUE_NORM_H
#define VALUE_NORM_H

#include "flyhip.h"

#define VALUE_NORM_SETS FLY_VALUE_NORM_SETS
#define VALUE_NORM_SET FLY_VALUE_NORM_SET
#define VALUE_NORM_TABLE FLY_VALUE_NORM_TABLE

#ifdef __HIPCC__
// Separately rounded fp32 ops (no fma), so numpy / torch in float32 reproduce both maps bit for bit.  Under the identity
// table (m = 0, s = r = 1) both return their argument.
__device__ __forceinline__ float value_denorm(float v, float m, float s)
{
    return __fadd_rn(__fmul_rn(v, s), m);
}

// No clamp: a clamped regression target is biased, and the Huber loss already bounds the critic's gradient.
__device__ __forceinline__ float value_norm_apply(float tg, float m, float r)
{
    return __fmul_rn(__fsub_rn(tg, m), r);
}

// One more value into the moments (n, mean, M2): Welford's update in float64.
__device__ __forceinline__ void value_moments_add(double& n, double& mean, double& m2, float x)
{
    n += 1.0;
    const double d = (double)x - mean;
    mean += d / n;
    m2 += d * ((double)x - mean);
}

// The same update for a value that is a float64 already (reward_norm.hip's discounted returns): not rounded to float first.
__device__ __forceinline__ void value_moments_add(double& n, double& mean, double& m2, double x)
{
    n += 1.0;
    const double d = x - mean;
    mean += d / n;
    m2 += d * (x - mean);
}

// (n, mean, M2) <- (n, mean, M2) + (nb, mb, qb): Chan et al.'s parallel update; an empty side leaves the other as it is.
__device__ __forceinline__ void value_moments_merge(double& n, double& mean, double& m2, double nb, double mb, double qb)
{
    if (!(nb > 0.0)) return;
    if (!(n > 0.0)) { n = nb; mean = mb; m2 = qb; return; }
    const double t = n + nb, d = mb - mean, inv = 1.0 / t;
    mean += d * (nb * inv);
    m2 += qb + d * d * (n * nb * inv);
    n = t;
}

// The wave's 64 per-lane moments -> its lane 0, by a fixed shuffle tree (the other lanes are left with partial merges).
__device__ __forceinline__ void value_moments_to_lane0(double& n, double& mean, double& m2)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double nb = __shfl_down(n, o, 64), mb = __shfl_down(mean, o, 64), qb = __shfl_down(m2, o, 64);
        value_moments_merge(n, mean, m2, nb, mb, qb);
    }
}

// The moments of a 256-thread workgroup -> its thread 0: the tree per wave, lane 0 of each wave through LDS, and thread 0
// folds waves 1..3 into its own in wave order.  Every thread of the workgroup calls it (it holds a barrier).
__device__ __forceinline__ void value_moments_to_thread0(double& n, double& mean, double& m2)
{
    __shared__ double part[4][VALUE_NORM_SET];
    value_moments_to_lane0(n, mean, m2);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = n; part[wave][1] = mean; part[wave][2] = m2; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) value_moments_merge(n, mean, m2, part[w][0], part[w][1], part[w][2]);
}

// One set: count | mean | M2, M2 not below zero.
__device__ __forceinline__ void value_store_set(double n, double mean, double m2, double* __restrict__ set)
{
    set[0] = n;
    set[1] = mean;
    set[2] = m2 > 0.0 ? m2 : 0.0;
}

// A one-wave workgroup's moments -> lane 0, which writes the workgroup's set.
__device__ __forceinline__ void value_write_set(double n, double mean, double m2, double* __restrict__ set)
{
    value_moments_to_lane0(n, mean, m2);
    if (threadIdx.x == 0) value_store_set(n, mean, m2, set);
}
#endif

#endif
