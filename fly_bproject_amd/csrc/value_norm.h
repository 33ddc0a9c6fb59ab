// value_norm.h — running value normalisation (PPO --normalize_value): the layouts shared by the kernels of value_norm.hip.
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

// The wave's 64 per-lane moments -> lane 0, by a fixed shuffle tree; lane 0 writes the workgroup's set.
__device__ __forceinline__ void value_write_set(double n, double mean, double m2, double* __restrict__ set)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double nb = __shfl_down(n, o, 64), mb = __shfl_down(mean, o, 64), qb = __shfl_down(m2, o, 64);
        value_moments_merge(n, mean, m2, nb, mb, qb);
    }
    if (threadIdx.x == 0) {
        set[0] = n;
        set[1] = mean;
        set[2] = m2 > 0.0 ? m2 : 0.0;
    }
}
#endif

#endif
