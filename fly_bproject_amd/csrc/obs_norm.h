// obs_norm.h — running observation normalisation (PPO --normalize_obs): the layouts shared by the statistics kernels
// (obs_norm.hip), the NORM instantiations of the rollout kernels (mlp_mfma.hip) and the handle (flyhip_abi.hip).
//
//   table   f32 [OBS_NORM_TABLE]: m[73] | r[73] | clip        what the kernels read: y = clamp((x - m_j) * r_j, -clip, clip)
//   stats   f64 [OBS_NORM_SET]:   count | mean[73] | var[73]   the running statistics S (population variance)
//   moments f64 [k][OBS_NORM_SET]: count | mean[73] | M2[73]   batch moments, one set per workgroup of the pass
#ifndef OBS_NORM_H
#define OBS_NORM_H

#include "flyhip.h"

#define OBS_NORM_COLS FLY_NUM_OBS
#define OBS_NORM_TABLE (2 * OBS_NORM_COLS + 1)
#define OBS_NORM_SET (1 + 2 * OBS_NORM_COLS)

// The handle's device copy of FlyConfig is followed by one pointer slot: the table fly_set_obs_norm registered (NULL = off).
// The NORM kernels read it through the config pointer they already receive, so no launch gains an argument.
constexpr unsigned long OBS_NORM_SLOT = (sizeof(FlyConfig) + 15) & ~15UL;

#ifdef __HIPCC__
__device__ __forceinline__ const float* obs_norm_table(const FlyConfig* c)
{
    return *reinterpret_cast<const float* const*>(reinterpret_cast<const char*>(c) + OBS_NORM_SLOT);
}

// Separately rounded fp32 ops, so torch's ((x - m) * r).clamp(-clip, clip) reproduces it bit for bit.  The clamp is written as
// comparisons: a NaN fails both and passes through (fminf / fmaxf would turn it into a bound).
__device__ __forceinline__ float obs_norm_apply(float x, float m, float r, float clip)
{
    const float y = __fmul_rn(__fsub_rn(x, m), r);
    return y < -clip ? -clip : (y > clip ? clip : y);
}

// table (global) -> LDS, OBS_NORM_TABLE floats; the caller's barrier publishes it
__device__ __forceinline__ void obs_norm_load(float* lds_tab, const FlyConfig* c)
{
    if (threadIdx.x < OBS_NORM_TABLE) lds_tab[threadIdx.x] = obs_norm_table(c)[threadIdx.x];
}
#endif

#endif
