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
#endif

#endif
