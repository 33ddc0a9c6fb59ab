// value_target.hip — λ-return critic targets for PPO (--lambda_returns).
//
//   lambda_targets_kernel      target = adv + vd elementwise, vd = v * s + m under the value-normalisation table (or v without
//                              one), plus -- when asked for -- the float64 moments (count, mean, M2) of the targets, one set per
//                              workgroup: the contract ppo_td_gae_vnorm_kernel (ppo_kernels.hip) gives ppo_value_norm_merge
//
// A stand-alone pass behind the unchanged GAE kernels: it reads the advantages and critic outputs they read or wrote and
// overwrites the TD targets (and their moment sets).  Deterministic: per-lane Welford updates, a fixed combination tree, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "launch.h"

namespace {

constexpr int TARGET_THREADS = 256;         // value_moments_to_thread0's workgroup

// Separately rounded fp32 ops in this order, no fma: the denormalisation of ppo_td_gae_vnorm, then one add.  NaN passes through.
template <bool TABLE>
__device__ __forceinline__ float lambda_target(float adv, float v, float m, float s)
{
    return __fadd_rn(adv, TABLE ? value_denorm(v, m, s) : v);
}

// Grid-stride over n elements: 16-byte accesses where all three buffers allow it (float4_map.h's split, here with two inputs and
// the moments), a scalar tail; element by element the same ops either way.  Every lane keeps Welford moments of the targets it
// wrote; value_moments_to_thread0 (value_norm.h) reduces the four waves', and thread 0 writes the workgroup's set.
template <bool TABLE, bool SETS>
__global__ __launch_bounds__(TARGET_THREADS) void lambda_targets_kernel(const float* __restrict__ adv, const float* __restrict__ v,
                                                                         const float* __restrict__ table, long n,
                                                                         float* __restrict__ target_out, double* __restrict__ sets)
{
    float m = 0.0f, s = 1.0f;
    if (TABLE) { m = table[0]; s = table[1]; }
    double cn = 0.0, cm = 0.0, cq = 0.0;
    const long stride = (long)gridDim.x * TARGET_THREADS, first = (long)blockIdx.x * TARGET_THREADS + threadIdx.x;
    const bool aligned = ((reinterpret_cast<uintptr_t>(adv) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(target_out)) & 15) == 0;
    const long n4 = aligned ? n >> 2 : 0;
    const float4* adv4 = reinterpret_cast<const float4*>(adv);
    const float4* v4 = reinterpret_cast<const float4*>(v);
    float4* out4 = reinterpret_cast<float4*>(target_out);
    for (long i = first; i < n4; i += stride) {
        const float4 a = adv4[i], x = v4[i];
        const float4 t = make_float4(lambda_target<TABLE>(a.x, x.x, m, s), lambda_target<TABLE>(a.y, x.y, m, s),
                                     lambda_target<TABLE>(a.z, x.z, m, s), lambda_target<TABLE>(a.w, x.w, m, s));
        out4[i] = t;
        if (SETS) {
            value_moments_add(cn, cm, cq, t.x);
            value_moments_add(cn, cm, cq, t.y);
            value_moments_add(cn, cm, cq, t.z);
            value_moments_add(cn, cm, cq, t.w);
        }
    }
    for (long i = 4 * n4 + first; i < n; i += stride) {
        const float t = lambda_target<TABLE>(adv[i], v[i], m, s);
        target_out[i] = t;
        if (SETS) value_moments_add(cn, cm, cq, t);
    }
    if (!SETS) return;
    value_moments_to_thread0(cn, cm, cq);
    if (threadIdx.x == 0) value_store_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

}  // namespace

extern "C" hipError_t flyhip_launch_lambda_targets(const float* adv, const float* v, const float* table, int64_t n,
                                                   float* target_out, double* sets, void* stream)
{
    // always FLY_VALUE_NORM_SETS workgroups: one set each, and those with no element write an empty set
    return with_bools([&](auto has_table, auto has_sets) {
        return launch_kernel<lambda_targets_kernel<has_table.value, has_sets.value>>(VALUE_NORM_SETS, TARGET_THREADS, 0, stream, adv, v,
                                                                                     table, (long)n, target_out, sets);
    }, table != nullptr, sets != nullptr);
}
