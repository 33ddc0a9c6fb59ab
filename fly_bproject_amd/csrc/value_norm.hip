// value_norm.hip — running value normalisation for the PPO critic (--normalize_value).
//
//   value_norm_merge_kernel    one workgroup: the sets combined in order (Chan et al.'s parallel update), folded into a COPY
//                              of the running statistics, and the fp32 table of that copy -- the inputs are never written
//   value_norm_apply_kernel    y = (tg - m) * r, elementwise, into a second buffer
//
// The sets come from the GAE pass (ppo_td_gae_vnorm_kernel and its scan form, ppo_kernels.hip; gae_episodic.hip), from
// lambda_targets_kernel (value_target.hip) or from the reward returns (reward_norm.hip).
// All deterministic: every combination runs in a fixed order and there are no atomics, so two runs on the same data are
// bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "float4_map.h"
#include "launch.h"

namespace {

constexpr int MERGE_THREADS = 256;          // sets staged per round of the merge

// One workgroup.  The k sets are staged through LDS 256 at a time (coalesced loads) and thread 0 combines them in index order,
// skipping empty ones; the result is folded into a copy of stats_in (whose M2 is var * count), and stats_out / table_out are
// written from that copy.  stats_in is only read: the caller commits by copying stats_out over it when it chooses to.
__global__ __launch_bounds__(MERGE_THREADS) void value_norm_merge_kernel(const double* __restrict__ stats_in,
                                                                         const double* __restrict__ sets, long k,
                                                                         double* __restrict__ stats_out,
                                                                         float* __restrict__ table_out)
{
    __shared__ double stage[MERGE_THREADS][VALUE_NORM_SET];
    const int tid = threadIdx.x;
    double na = 0.0, ma = 0.0, qa = 0.0;
    for (long base = 0; base < k; base += MERGE_THREADS) {
        const long left = k - base;
        const int cnt = left < MERGE_THREADS ? (int)left : MERGE_THREADS;
        if (tid < cnt) {
#pragma unroll
            for (int j = 0; j < VALUE_NORM_SET; ++j) stage[tid][j] = sets[(base + tid) * VALUE_NORM_SET + j];
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < cnt; ++i) value_moments_merge(na, ma, qa, stage[i][0], stage[i][1], stage[i][2]);
        __syncthreads();
    }
    if (tid != 0) return;
    double n = stats_in[0], mean = stats_in[1], q = stats_in[2] * stats_in[0];
    value_moments_merge(n, mean, q, na, ma, qa);
    const double var = na > 0.0 ? q / n : stats_in[2];
    stats_out[0] = n;
    stats_out[1] = mean;
    stats_out[2] = var;
    const double sd = sqrt(var + 1e-5);
    table_out[0] = (float)mean;
    table_out[1] = (float)sd;
    table_out[2] = (float)(1.0 / sd);
    table_out[3] = 0.0f;
}

// out[i] = (tg[i] - m) * r, elementwise (float4_map.h).  NaN passes through.
__global__ __launch_bounds__(FLOAT4_MAP_THREADS) void value_norm_apply_kernel(const float* __restrict__ tg, long n,
                                                                              const float* __restrict__ table,
                                                                              float* __restrict__ out)
{
    const float m = table[0], r = table[2];
    float4_map(tg, n, out, [=](float x) { return value_norm_apply(x, m, r); });
}

}  // namespace

extern "C" hipError_t flyhip_launch_value_norm_merge(const double* stats_in, const double* sets, int64_t k, double* stats_out,
                                                     float* table_out, void* stream)
{
    return launch_kernel<value_norm_merge_kernel>(1, MERGE_THREADS, 0, stream, stats_in, sets, (long)k, stats_out, table_out);
}

extern "C" hipError_t flyhip_launch_value_norm_apply(const float* target, int64_t n, const float* table, float* out, void* stream)
{
    return launch_kernel<value_norm_apply_kernel>(float4_map_grid(n), FLOAT4_MAP_THREADS, 0, stream, target, (long)n, table, out);
}
