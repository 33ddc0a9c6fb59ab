// ppo_kernels.hip — gfx950 kernels for the PPO rollout math around the policy network.
//
//   ppo_sample_logprob_kernel   ppo.py:213-220  a = mu + sqrt(var) eps; log N(a; mu, diag var); clip
//   ppo_td_gae_kernel           ppo.py:157-171  TD target + delta + reverse GAE recurrence, lane = env
//   ppo_td_gae_scan_kernel                      the same as a wave scan: one wave per env, time on lanes (PPO_GAE_SCAN)
//   ppo_td_gae_vnorm_kernel                     both with v / v_next mapped to reward units under the value-normalisation table,
//   ppo_td_gae_vnorm_scan_kernel                plus the float64 moments (count, mean, M2) of the TD targets, one set per workgroup
//   ppo_adv_stats / _totals / _apply_kernel     advantage normalisation (opt-in)
//   ppo_bookkeeping_kernel, ppo_row_terms_kernel + ppo_rows_apply_kernel   the score and the action variance's decay
//
// The four GAE kernels are grid mappings around one row (td_gae_row), one backward walk (td_gae_walk) and one scan
// (td_gae_scan_env): what they compute alike is written once.
//
// All are streaming kernels (HBM-bound by construction): rows of the row-major [n][18] operands
// are staged through LDS so that global traffic is 16-byte coalesced while each lane walks its
// own row; the [T][N] rollout tensors are walked with lane = env, so every time step is one
// coalesced 256-byte line per wave and the recurrence lives in a register.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "time_scan.h"
#include "launch.h"

namespace {

#include "loss_head.inc"

constexpr int NA = FLY_NUM_DOF;
constexpr int SL_BLOCK = 64;            // rows per workgroup (one wave)
constexpr int SL_PAD = NA + 1;          // 19-word row pitch: conflict-free column walks

__global__ __launch_bounds__(SL_BLOCK) void ppo_sample_logprob_kernel(
    const float* __restrict__ mu, const float* __restrict__ var, const float* __restrict__ eps,
    float* __restrict__ act_out, float* __restrict__ logp_out, long n)
{
    __shared__ float s_mu[SL_BLOCK * SL_PAD];
    __shared__ float s_eps[SL_BLOCK * SL_PAD];
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * SL_BLOCK;
    const long rows = (n - row0) < SL_BLOCK ? (n - row0) : SL_BLOCK;
    const long base = row0 * NA;
    const int count = (int)rows * NA;
    for (int i = tid; i < count; i += SL_BLOCK) {
        int rr = i / NA, cc = i - rr * NA;
        s_mu[rr * SL_PAD + cc] = mu[base + i];
        s_eps[rr * SL_PAD + cc] = eps[base + i];
    }
    __syncthreads();
    // scale_tril = cholesky(diag(var)) = diag(sqrt(var)); half_log_det = sum log L_jj (ppo.py:215-217)
    float L[NA];
    float half_log_det = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; ++j) { L[j] = sqrtf(var[j]); half_log_det = __fadd_rn(half_log_det, logf(L[j])); }
    const float klog2pi = GAUSS_DIM_LOG_2PI;    // 18 * log(2*pi)
    if (tid < rows) {
        float M = 0.0f;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            float m = s_mu[tid * SL_PAD + j];
            float a = __fadd_rn(m, __fmul_rn(L[j], s_eps[tid * SL_PAD + j]));   // rsample
            float x = __fsub_rn(a, m) / L[j];                                    // mahalanobis
            M = __fadd_rn(M, __fmul_rn(x, x));
            s_mu[tid * SL_PAD + j] = fminf(fmaxf(a, -1.0f), 1.0f);               // ppo.py:220
        }
        logp_out[row0 + tid] = __fsub_rn(__fmul_rn(-0.5f, __fadd_rn(klog2pi, M)), half_log_det);
    }
    __syncthreads();
    for (int i = tid; i < count; i += SL_BLOCK) {
        int rr = i / NA, cc = i - rr * NA;
        act_out[base + i] = s_mu[rr * SL_PAD + cc];
    }
}

// The reference's row (ppo.py:157-171), written once for the four kernels below.  `a_next` is the advantage carried from t + 1;
// returns the advantage of this row and its target in `tg`.  VNORM: v / v_next are mapped to reward units under the
// value-normalisation table first (value_norm.h); otherwise the ops and their order are the same.  All separately rounded.
template <int MODE, bool VNORM>
__device__ __forceinline__ float td_gae_row(float r, float v, float v_next, float d, float tm, float ts, float gamma, float gl,
                                            float a_next, float& tg)
{
    const float vv = VNORM ? value_denorm(v, tm, ts) : v;
    const float vn = VNORM ? value_denorm(v_next, tm, ts) : v_next;
    tg = __fadd_rn(r, __fmul_rn(__fmul_rn(gamma, vn), d));                            // ppo.py:160
    const float delta = __fsub_rn(tg, vv);                                            // ppo.py:161
    const float carry = (MODE & PPO_GAE_MASK_RECURRENCE) ? __fmul_rn(a_next, d) : a_next;
    return __fadd_rn(__fmul_rn(gl, carry), delta);                                    // ppo.py:167
}

// the kernels' inputs: the rollout tensors [T][N], `done` per env or per step (MODE), the table's m | s (read under VNORM only)
#define TD_GAE_INPUTS                                                                                                         \
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,                         \
        const float* __restrict__ done, float tm, float ts, float gamma, float gl, long N

// Env e's rows t_hi - 1 .. t_lo, backwards from the carried advantage `a`; returns the advantage of row t_lo.  sink(i, tg, a)
// sees every row: the loads of step t - 1.. do not depend on the carried advantage, so an unrolled body keeps several time
// steps of loads in flight.  UNROLL is the loop's unroll count: 8 with lane = env (a wave walks all T rows), 1 in the scan, whose
// lanes walk short chunks twice.
template <int MODE, bool VNORM, int UNROLL, class Sink>
__device__ __forceinline__ float td_gae_walk(TD_GAE_INPUTS, long e, long t_lo, long t_hi, float a, Sink sink)
{
    const float d_row = (MODE & PPO_GAE_DONE_PER_STEP) ? 0.0f : done[e];
#pragma unroll UNROLL
    for (long t = t_hi - 1; t >= t_lo; --t) {
        const long i = t * N + e;
        const float d = (MODE & PPO_GAE_DONE_PER_STEP) ? done[i] : d_row;
        float tg;
        a = td_gae_row<MODE, VNORM>(reward[i], v[i], v_next[i], d, tm, ts, gamma, gl, a, tg);
        sink(i, tg, a);
    }
    return a;
}

// GAE as a wavefront scan, for the shapes where "lane = env" has nothing to run on: few envs, very long rollouts (the
// reference's own 16-env configuration has T = 40 960, ppo.py:118-122).  One wave per env; the 64 lanes own 64 consecutive
// chunks of the time axis, lane 0 the LAST one (time_scan.h).
//   pass 1  every lane runs the recurrence over its chunk from a zero carry (its chunk's own contribution S_l) and forms the
//           chunk's multiplier gl^len -- 64 chunks in parallel instead of one 40 960-long chain;
//   carry   the carry into chunk l is A_l = S_{l+1} + c^{len(l+1)} A_{l+1}: affine_carry;
//   pass 2  every lane reruns its chunk from the true carry, and sink(i, tg, a) sees every row exactly once.
// Inside a chunk the arithmetic is the reference's (separately rounded mul/add); only the 63 carries are re-associated, so the
// result agrees with the sequential loop to fp32 rounding (tested at 1e-5), not bit for bit: the host picks this form only when
// N is small (PPO_GAE_SCAN).  The masked recurrence (PPO_GAE_MASK_RECURRENCE) has no scan form: MODE is 0 or 1.
template <int MODE, bool VNORM, class Sink>
__device__ __forceinline__ void td_gae_scan_env(TD_GAE_INPUTS, long e, const TimeChunk& c, int lane, Sink sink)
{
    static_assert((MODE & PPO_GAE_MASK_RECURRENCE) == 0, "the scan form does not mask the recurrence");
    float m = 1.0f;
    const float S = td_gae_walk<MODE, VNORM, 1>(reward, v, v_next, done, tm, ts, gamma, gl, N, e, c.t_lo, c.t_hi, 0.0f,
                                                [&](long, float, float) { m *= gl; });
    td_gae_walk<MODE, VNORM, 1>(reward, v, v_next, done, tm, ts, gamma, gl, N, e, c.t_lo, c.t_hi, affine_carry(m, S, lane), sink);
}

// The four kernels: a grid mapping around the walk or the scan each.  Plain: one env (block) per lane (workgroup), as many
// workgroups as that takes.  Value-normalising (--normalize_value): always VALUE_NORM_SETS workgroups
// that stride over the env blocks / envs -- one block for N <= 16384 -- and every lane keeps Welford moments of the targets it
// wrote (not raw sums: targets of mean 1e3 / std 1e-2 keep their digits), one set per workgroup for value_norm_merge_kernel.
constexpr int GAE_BLOCK = 64;               // one wave per workgroup: envs spread over the CUs

template <int MODE>
__global__ __launch_bounds__(256) void ppo_td_gae_kernel(
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,
    const float* __restrict__ done, float gamma, float gl, long T, long N,
    float* __restrict__ target_out, float* __restrict__ adv_out)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    td_gae_walk<MODE, false, 8>(reward, v, v_next, done, 0.0f, 1.0f, gamma, gl, N, e, 0, T, 0.0f, [&](long i, float tg, float a) {
        target_out[i] = tg;
        adv_out[i] = a;
    });
}

template <int MODE>
__global__ __launch_bounds__(GAE_BLOCK) void ppo_td_gae_scan_kernel(
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,
    const float* __restrict__ done, float gamma, float gl, long T, long N,
    float* __restrict__ target_out, float* __restrict__ adv_out)
{
    const int lane = threadIdx.x;
    td_gae_scan_env<MODE, false>(reward, v, v_next, done, 0.0f, 1.0f, gamma, gl, N, blockIdx.x, reverse_chunk(T, lane), lane,
                                 [&](long i, float tg, float a) {
        target_out[i] = tg;
        adv_out[i] = a;
    });
}

template <int MODE>
__global__ __launch_bounds__(GAE_BLOCK) void ppo_td_gae_vnorm_kernel(
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,
    const float* __restrict__ done, const float* __restrict__ table, float gamma, float gl, long T, long N,
    float* __restrict__ target_out, float* __restrict__ adv_out, double* __restrict__ sets)
{
    const float tm = table[0], ts = table[1];
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long e = (long)blockIdx.x * GAE_BLOCK + threadIdx.x; e < N; e += (long)gridDim.x * GAE_BLOCK)
        td_gae_walk<MODE, true, 8>(reward, v, v_next, done, tm, ts, gamma, gl, N, e, 0, T, 0.0f, [&](long i, float tg, float a) {
            target_out[i] = tg;
            adv_out[i] = a;
            value_moments_add(cn, cm, cq, tg);
        });
    value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

template <int MODE>
__global__ __launch_bounds__(GAE_BLOCK) void ppo_td_gae_vnorm_scan_kernel(
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,
    const float* __restrict__ done, const float* __restrict__ table, float gamma, float gl, long T, long N,
    float* __restrict__ target_out, float* __restrict__ adv_out, double* __restrict__ sets)
{
    const float tm = table[0], ts = table[1];
    const int lane = threadIdx.x;
    const TimeChunk c = reverse_chunk(T, lane);
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long e = blockIdx.x; e < N; e += gridDim.x)
        td_gae_scan_env<MODE, true>(reward, v, v_next, done, tm, ts, gamma, gl, N, e, c, lane, [&](long i, float tg, float a) {
            target_out[i] = tg;
            adv_out[i] = a;
            value_moments_add(cn, cm, cq, tg);
        });
    value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

// Advantage normalisation (named by BASELINE's north_star; the reference does NOT normalise,
// ppo.py:171, so this is opt-in): (x - mean) / (std + eps) with the unbiased std torch uses.  The statistics are CENTRED
// second moments in float64 -- raw sums of x and x^2 in fp32 lose the variance to cancellation once |mean| is a few dozen
// std.  Every thread keeps Welford moments (count, mean, M2) of its grid-stride elements, a fixed
// shuffle / LDS tree merges them per workgroup (Chan et al.'s update, value_norm.h) and one workgroup merges the
// ADV_BLOCKS sets in index order: deterministic.  stats[0..1] return sum = count * mean and M2 = sum (x - mean)^2, each
// rounded once to fp32; stats + 2 is the scratch of the per-workgroup sets (f64 mean | M2; a workgroup's count follows
// from n).  Data-parallel callers combine the ranks' (sum, M2) pairs (ppo.py: combine_adv_stats).
constexpr int ADV_BLOCKS = 128;         // 128 sets x 2 doubles = the 512 floats behind stats[0..1]

__device__ __forceinline__ long adv_block_count(long n, int b)
{
    const long round = (long)ADV_BLOCKS * 256;
    const long rem = n % round - (long)b * 256;
    return n / round * 256 + (rem < 0 ? 0 : rem > 256 ? 256 : rem);
}

__global__ __launch_bounds__(256) void ppo_adv_stats_kernel(const float* __restrict__ adv, long n,
                                                            double* __restrict__ part)
{
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        value_moments_add(cn, cm, cq, adv[i]);
    value_moments_to_thread0(cn, cm, cq);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = cm;
        part[2 * blockIdx.x + 1] = cq;
    }
}

__global__ __launch_bounds__(256) void ppo_adv_apply_kernel(float* __restrict__ adv, long n, const float* __restrict__ totals,
                                                            float count, float eps)
{
    const double mean = (double)totals[0] / (double)count;
    const double var = fmax((double)totals[1] / ((double)count - 1.0), 0.0);
    const double inv = 1.0 / (sqrt(var) + (double)eps);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        adv[i] = (float)(((double)adv[i] - mean) * inv);
}

__global__ __launch_bounds__(64) void ppo_adv_totals_kernel(const double* __restrict__ part, long n, float* __restrict__ totals)
{
    if (threadIdx.x != 0) return;
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (int b = 0; b < ADV_BLOCKS; ++b)
        value_moments_merge(cn, cm, cq, (double)adv_block_count(n, b), part[2 * b], part[2 * b + 1]);
    totals[0] = (float)(cn * cm);
    totals[1] = (float)(cq > 0.0 ? cq : 0.0);
}

// One row's score term, mean(row) * score_scale (ppo.py:233), by a workgroup of 1024 threads; thread 0 returns it, the others
// 0.  16-byte loads where the row allows it, all of a thread's loads in flight at once (n = 8192 -> two float4 per thread), then
// the wave tree and the 16 waves' sums in wave order: one fixed reduction order, so the term does not depend on who asks.
__device__ __forceinline__ float score_row_term(const float* __restrict__ row, long n, float score_scale)
{
    __shared__ float red[16];
    const int tid = threadIdx.x;
    float s = 0.0f;
    const long n4 = n >> 2;
    const float4* r4 = reinterpret_cast<const float4*>(row);
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    if (aligned) {
        for (long i = tid; i < n4; i += 1024) { const float4 v = r4[i]; s += (v.x + v.y) + (v.z + v.w); }
        for (long i = 4 * n4 + tid; i < n; i += 1024) s += row[i];
    } else {
        for (long i = tid; i < n; i += 1024) s += row[i];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid != 0) return 0.0f;
    float t = 0.0f;
    for (int w = 0; w < 16; ++w) t += red[w];
    return t / (float)n * score_scale;
}

// ppo.py:233 + :237 in one tiny launch: score += mean(reward)/num_eval_freq (kept on the device:
// the reference's per-step .item() host sync is gone) and action_var = max(var_min, var - decay).
// One workgroup, fixed reduction order: deterministic.
__global__ __launch_bounds__(1024) void ppo_bookkeeping_kernel(const float* __restrict__ reward, long n,
                                                               float* __restrict__ score_acc, float score_scale,
                                                               float* __restrict__ action_var, int nvar,
                                                               float var_decay, float var_min)
{
    const int tid = threadIdx.x;
    const float term = score_row_term(reward, n, score_scale);
    if (tid == 0) *score_acc += term;
    if (tid < nvar && var_decay > 0.0f) action_var[tid] = fmaxf(var_min, action_var[tid] - var_decay);
}

// The same bookkeeping for `rows` consecutive env steps at once (reward [rows][n]), bit for bit what
// `rows` calls of the kernel above leave: one workgroup per row computes that row's score term by
// the same function, a second single-wave launch adds the terms in row order and applies the
// variance decay `rows` times.  The rollout calls this when the score is printed and before an
// update instead of paying a latency-bound single-workgroup launch on every env step.
__global__ __launch_bounds__(1024) void ppo_row_terms_kernel(const float* __restrict__ reward, long n, float score_scale,
                                                             float* __restrict__ terms)
{
    const float term = score_row_term(reward + (long)blockIdx.x * n, n, score_scale);
    if (threadIdx.x == 0) terms[blockIdx.x] = term;
}

__global__ __launch_bounds__(64) void ppo_rows_apply_kernel(const float* __restrict__ terms, long rows,
                                                            float* __restrict__ score_acc, float* __restrict__ action_var,
                                                            int nvar, float var_decay, float var_min, int* __restrict__ rows_applied)
{
    const int tid = threadIdx.x;
    if (tid == 63) {
        float acc = *score_acc;
        for (long r = 0; r < rows; ++r) acc += terms[r];
        *score_acc = acc;
        if (rows_applied) *rows_applied += (int)rows;       // the policy launches subtract this from their row index
    }
    if (tid < nvar && var_decay > 0.0f) {
        float v = action_var[tid];
        for (long r = 0; r < rows; ++r) v = fmaxf(var_min, v - var_decay);
        action_var[tid] = v;
    }
}

}  // namespace

extern "C" hipError_t flyhip_launch_rollout_bookkeeping(const float* reward, int64_t rows, int64_t n, float* terms,
                                                        float* score_acc, float score_scale, float* action_var, int nvar,
                                                        float var_decay, float var_min, int* rows_applied, void* stream)
{
    hipError_t e = launch_kernel<ppo_row_terms_kernel>((unsigned)rows, 1024, 0, stream, reward, (long)n, score_scale, terms);
    if (e != hipSuccess) return e;
    return launch_kernel<ppo_rows_apply_kernel>(1, 64, 0, stream, terms, (long)rows, score_acc, action_var, nvar, var_decay, var_min,
                                                rows_applied);
}

extern "C" hipError_t flyhip_launch_bookkeeping(const float* reward, int64_t n, float* score_acc, float score_scale,
                                                float* action_var, int nvar, float var_decay, float var_min,
                                                void* stream)
{
    return launch_kernel<ppo_bookkeeping_kernel>(1, 1024, 0, stream, reward, (long)n, score_acc, score_scale, action_var, nvar,
                                                 var_decay, var_min);
}

extern "C" hipError_t flyhip_launch_sample_logprob(const float* mu, const float* var, const float* eps,
                                                   float* act_out, float* logp_out, int64_t n, void* stream)
{
    int grid = (int)((n + SL_BLOCK - 1) / SL_BLOCK);
    return launch_kernel<ppo_sample_logprob_kernel>(grid, SL_BLOCK, 0, stream, mu, var, eps, act_out, logp_out, (long)n);
}

extern "C" hipError_t flyhip_launch_td_gae(const float* reward, const float* v, const float* v_next,
                                           const float* done, float gamma, float lambda, int64_t T, int64_t N,
                                           float* target_out, float* adv_out, int mode, void* stream)
{
    const float gl = (float)((double)gamma * (double)lambda);   // python double product, ppo.py:167
    if (mode & PPO_GAE_SCAN)
        return with_int<0, 1>(mode & PPO_GAE_DONE_PER_STEP ? 1 : 0, [&](auto m) {
            return launch_kernel<ppo_td_gae_scan_kernel<m.value>>(dim3((unsigned)N), GAE_BLOCK, 0, stream, reward, v, v_next, done, gamma,
                                                                  gl, (long)T, (long)N, target_out, adv_out);
        });
    int grid = (int)((N + GAE_BLOCK - 1) / GAE_BLOCK);
    return with_int<0, 1, 2, 3>(mode & 3, [&](auto m) {
        return launch_kernel<ppo_td_gae_kernel<m.value>>(grid, GAE_BLOCK, 0, stream, reward, v, v_next, done, gamma, gl, (long)T, (long)N,
                                                         target_out, adv_out);
    });
}

extern "C" hipError_t flyhip_launch_td_gae_vnorm(const float* reward, const float* v, const float* v_next, const float* done,
                                                 const float* table, float gamma, float lambda, int64_t T, int64_t N,
                                                 float* target_out, float* adv_out, double* sets, int mode, void* stream)
{
    const float gl = (float)((double)gamma * (double)lambda);   // python double product, ppo.py:167
    // always FLY_VALUE_NORM_SETS workgroups: one set each, and those with no env write an empty set
    if (mode & PPO_GAE_SCAN)
        return with_int<0, 1>(mode & PPO_GAE_DONE_PER_STEP ? 1 : 0, [&](auto m) {
            return launch_kernel<ppo_td_gae_vnorm_scan_kernel<m.value>>(VALUE_NORM_SETS, GAE_BLOCK, 0, stream, reward, v, v_next, done,
                                                                        table, gamma, gl, (long)T, (long)N, target_out, adv_out, sets);
        });
    return with_int<0, 1, 2, 3>(mode & 3, [&](auto m) {
        return launch_kernel<ppo_td_gae_vnorm_kernel<m.value>>(VALUE_NORM_SETS, GAE_BLOCK, 0, stream, reward, v, v_next, done, table,
                                                               gamma, gl, (long)T, (long)N, target_out, adv_out, sets);
    });
}

extern "C" hipError_t flyhip_launch_adv_stats(const float* adv, int64_t n, float* stats, void* stream)
{
    double* part = reinterpret_cast<double*>(stats + 2);         // the ABI checks that stats is 8-byte aligned
    hipError_t e = launch_kernel<ppo_adv_stats_kernel>(ADV_BLOCKS, 256, 0, stream, adv, (long)n, part);
    if (e != hipSuccess) return e;
    return launch_kernel<ppo_adv_totals_kernel>(1, 64, 0, stream, part, (long)n, stats);
}

extern "C" hipError_t flyhip_launch_adv_apply(float* adv, int64_t n, const float* totals, float count, float eps, void* stream)
{
    return launch_kernel<ppo_adv_apply_kernel>(512, 256, 0, stream, adv, (long)n, totals, count, eps);
}
