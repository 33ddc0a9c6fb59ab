// value_norm.hip — running value normalisation for the PPO critic (--normalize_value).
//
//   value_td_gae_kernel        ppo_td_gae_kernel (ppo_kernels.hip) with v / v_next mapped to reward units under the table, plus
//   value_td_gae_scan_kernel   the float64 moments (count, mean, M2) of the TD targets, one set per workgroup
//   value_norm_merge_kernel    one workgroup: the sets combined in order (Chan et al.'s parallel update), folded into a COPY
//                              of the running statistics, and the fp32 table of that copy -- the inputs are never written
//   value_norm_apply_kernel    y = (tg - m) * r, elementwise, into a second buffer
//
// All deterministic: every combination runs in a fixed order and there are no atomics, so two runs on the same data are
// bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "launch.h"

namespace {

constexpr int GAE_BLOCK = 64;               // one wave per workgroup, as ppo_td_gae: envs spread over the CUs
constexpr int MERGE_THREADS = 256;          // sets staged per round of the merge
constexpr int APPLY_THREADS = 256;

// lane = env, t walks backwards: the loop of ppo_td_gae_kernel, per element the same ops in the same order, with v and v_next
// replaced by their denormalised values.  Workgroup g takes the env blocks g, g + gridDim.x, ... (one block for N <= 16384), and
// every lane keeps Welford moments of the targets it wrote -- not raw sums: targets of mean 1e3 / std 1e-2 keep their digits.
template <int MODE>
__global__ __launch_bounds__(GAE_BLOCK) void value_td_gae_kernel(
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,
    const float* __restrict__ done, const float* __restrict__ table, float gamma, float gl, long T, long N,
    float* __restrict__ target_out, float* __restrict__ adv_out, double* __restrict__ sets)
{
    const float m = table[0], s = table[1];
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long e = (long)blockIdx.x * GAE_BLOCK + threadIdx.x; e < N; e += (long)gridDim.x * GAE_BLOCK) {
        float d_row = (MODE & PPO_GAE_DONE_PER_STEP) ? 0.0f : done[e];
        float a = 0.0f;
#pragma unroll 8
        for (long t = T - 1; t >= 0; --t) {
            const long i = t * N + e;
            float d = (MODE & PPO_GAE_DONE_PER_STEP) ? done[i] : d_row;
            const float vn = value_denorm(v_next[i], m, s), vv = value_denorm(v[i], m, s);
            float tg = __fadd_rn(reward[i], __fmul_rn(__fmul_rn(gamma, vn), d));          // ppo.py:160, reward units
            float delta = __fsub_rn(tg, vv);                                               // ppo.py:161
            float carry = (MODE & PPO_GAE_MASK_RECURRENCE) ? __fmul_rn(a, d) : a;
            a = __fadd_rn(__fmul_rn(gl, carry), delta);                                    // ppo.py:167
            target_out[i] = tg;
            adv_out[i] = a;
            value_moments_add(cn, cm, cq, tg);
        }
    }
    value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

// ppo_td_gae_scan_kernel with the same replacement: one wave per env, the 64 lanes own 64 consecutive chunks of the time axis
// (see ppo_kernels.hip for the scan).  Workgroup g takes envs g, g + gridDim.x, ...; the moments are taken in pass 2, where
// every target is written exactly once.
template <int MODE>
__global__ __launch_bounds__(GAE_BLOCK) void value_td_gae_scan_kernel(
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,
    const float* __restrict__ done, const float* __restrict__ table, float gamma, float gl, long T, long N,
    float* __restrict__ target_out, float* __restrict__ adv_out, double* __restrict__ sets)
{
    const float tm = table[0], ts = table[1];
    const int lane = threadIdx.x;
    const long L = (T + 63) / 64;
    const long t_hi = T - (long)lane * L;                 // exclusive; lane 0 owns the LAST chunk
    const long t_lo = (t_hi - L > 0) ? t_hi - L : 0;
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long e = blockIdx.x; e < N; e += gridDim.x) {
        const float d_row = (MODE & PPO_GAE_DONE_PER_STEP) ? 0.0f : done[e];
        auto delta_at = [&](long t, float& tg) {
            const long i = t * N + e;
            const float d = (MODE & PPO_GAE_DONE_PER_STEP) ? done[i] : d_row;
            const float vn = value_denorm(v_next[i], tm, ts), vv = value_denorm(v[i], tm, ts);
            tg = __fadd_rn(reward[i], __fmul_rn(__fmul_rn(gamma, vn), d));
            return __fsub_rn(tg, vv);
        };
        // pass 1: chunk contribution and multiplier
        float S = 0.0f, m = 1.0f;
        for (long t = t_hi - 1; t >= t_lo && t_hi > 0; --t) {
            float tg;
            const float dl = delta_at(t, tg);
            S = __fadd_rn(__fmul_rn(gl, S), dl);
            m *= gl;
        }
        if (t_hi <= 0) { S = 0.0f; m = 1.0f; }
        // inclusive scan over lanes:  X_l = S_l + m_l * X_{l-1}
        float sm = m, sv = S;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float pm = __shfl_up(sm, o, 64), pv = __shfl_up(sv, o, 64);
            if (lane >= o) { sv = sv + sm * pv; sm = sm * pm; }
        }
        float carry = __shfl_up(sv, 1, 64);               // advantage entering this chunk
        if (lane == 0) carry = 0.0f;
        // pass 2: the real recurrence from the true carry
        float a = carry;
        for (long t = t_hi - 1; t >= t_lo && t_hi > 0; --t) {
            float tg;
            const float dl = delta_at(t, tg);
            a = __fadd_rn(__fmul_rn(gl, a), dl);
            target_out[t * N + e] = tg;
            adv_out[t * N + e] = a;
            value_moments_add(cn, cm, cq, tg);
        }
    }
    value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

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

// out[i] = (tg[i] - m) * r: 16-byte accesses where both buffers allow it, a scalar tail.  NaN passes through.
__global__ __launch_bounds__(APPLY_THREADS) void value_norm_apply_kernel(const float* __restrict__ tg, long n,
                                                                         const float* __restrict__ table, float* __restrict__ out)
{
    const float m = table[0], r = table[2];
    const long stride = (long)gridDim.x * APPLY_THREADS, first = (long)blockIdx.x * APPLY_THREADS + threadIdx.x;
    const bool aligned = ((reinterpret_cast<uintptr_t>(tg) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long n4 = aligned ? n >> 2 : 0;
    const float4* in4 = reinterpret_cast<const float4*>(tg);
    float4* out4 = reinterpret_cast<float4*>(out);
    for (long i = first; i < n4; i += stride) {
        const float4 x = in4[i];
        out4[i] = make_float4(value_norm_apply(x.x, m, r), value_norm_apply(x.y, m, r), value_norm_apply(x.z, m, r),
                              value_norm_apply(x.w, m, r));
    }
    for (long i = 4 * n4 + first; i < n; i += stride) out[i] = value_norm_apply(tg[i], m, r);
}

}  // namespace

extern "C" hipError_t flyhip_launch_td_gae_vnorm(const float* reward, const float* v, const float* v_next, const float* done,
                                                 const float* table, float gamma, float lambda, int64_t T, int64_t N,
                                                 float* target_out, float* adv_out, double* sets, int mode, void* stream)
{
    const float gl = (float)((double)gamma * (double)lambda);   // python double product, ppo.py:167
    // always FLY_VALUE_NORM_SETS workgroups: one set each, and those with no env write an empty set
    if (mode & PPO_GAE_SCAN)
        return with_int<0, 1>(mode & PPO_GAE_DONE_PER_STEP ? 1 : 0, [&](auto m) {
            return launch_kernel<value_td_gae_scan_kernel<m.value>>(VALUE_NORM_SETS, GAE_BLOCK, 0, stream, reward, v, v_next, done, table,
                                                                    gamma, gl, (long)T, (long)N, target_out, adv_out, sets);
        });
    return with_int<0, 1, 2, 3>(mode & 3, [&](auto m) {
        return launch_kernel<value_td_gae_kernel<m.value>>(VALUE_NORM_SETS, GAE_BLOCK, 0, stream, reward, v, v_next, done, table, gamma,
                                                           gl, (long)T, (long)N, target_out, adv_out, sets);
    });
}

extern "C" hipError_t flyhip_launch_value_norm_merge(const double* stats_in, const double* sets, int64_t k, double* stats_out,
                                                     float* table_out, void* stream)
{
    hipLaunchKernelGGL(value_norm_merge_kernel, dim3(1), dim3(MERGE_THREADS), 0, (hipStream_t)stream, stats_in, sets, (long)k,
                       stats_out, table_out);
    return hipGetLastError();
}

extern "C" hipError_t flyhip_launch_value_norm_apply(const float* target, int64_t n, const float* table, float* out, void* stream)
{
    const long per = 4L * APPLY_THREADS;
    long grid = (n + per - 1) / per;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(value_norm_apply_kernel, dim3((unsigned)grid), dim3(APPLY_THREADS), 0, (hipStream_t)stream, target,
                       (long)n, table, out);
    return hipGetLastError();
}
