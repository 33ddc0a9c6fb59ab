// gae_episodic.hip — the episode-aware advantage estimate (PPO --gae episodic).
//
//   gae_episodic_kernel        lane = env, t walks backwards: ppo_td_gae_kernel's loop on the rollout's own int64 flag rows
//   gae_episodic_scan_kernel   one wave per env, time on lanes (PPO_GAE_SCAN): the scan of ppo_td_gae_scan_kernel with a per-step
//                              multiplier gl * cont_t in {0, gl}, so a chunk that holds an episode end passes no carry at all
//
// Both exist plain and with value normalisation (template argument VNORM: v / v_next denormalised under the table, the float64
// moments of the targets into one set per workgroup); the row itself is written once, episodic_row.
//
// Per row i = (t, e), from the flags the env step left (fly_body.inc: rs = 1 when the fly fell or progress >= max_episode_length
// - 1, set AFTER the observation of step t was packed, so the ring's row t + 1 is the old episode's true next observation):
//   ended   = reset[t][e] != 0
//   timeout = ended && progress[t][e] >= max_episode_length - 1      a fall in the limit's own step counts as a time-out
//                                                                   (IsaacGymEnvs' convention, and all the two rows can tell)
//   stale   = (t > 0 ? reset[t-1][e] : ended_prev[e]) != 0          the step that performed the reset: its reward and next
//                                                                   value say nothing about the action taken
//   boot = (ended && !timeout) ? 0 : 1,  cont = ended ? 0 : 1
//   not stale:  tg = r + (gamma v') boot;  delta = tg - v;  a = gl (a_next cont) + delta     ppo_td_gae mode 1|2, op for op
//   stale:      tg = v;  a = 0              (the row before it has cont = 0: nothing reads its carry; stale wins over ended)
// All separately rounded fp32 ops (no fma), so a float32 numpy restatement reproduces the lane = env form bit for bit.
// Deterministic: fixed combination order, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "time_scan.h"
#include "launch.h"

namespace {

constexpr int GAE_BLOCK = 64;               // one wave per workgroup, as ppo_td_gae: envs spread over the CUs
constexpr long SCAN_GRID_MAX = 65536;       // plain scan form: one wave per env up to here, then envs are strided

// The row.  `a_next` is the advantage carried from t + 1; returns the advantage of this row and its target in `tg`.
template <bool VNORM>
__device__ __forceinline__ float episodic_row(float r, float v, float v_next, bool ended, bool timeout, bool stale, float tm,
                                              float ts, float gamma, float gl, float a_next, float& tg)
{
    const float vv = VNORM ? value_denorm(v, tm, ts) : v;
    const float vn = VNORM ? value_denorm(v_next, tm, ts) : v_next;
    const float boot = (ended && !timeout) ? 0.0f : 1.0f;
    const float cont = ended ? 0.0f : 1.0f;
    const float t_live = __fadd_rn(r, __fmul_rn(__fmul_rn(gamma, vn), boot));
    const float delta = __fsub_rn(t_live, vv);
    const float a_live = __fadd_rn(__fmul_rn(gl, __fmul_rn(a_next, cont)), delta);
    tg = stale ? vv : t_live;
    return stale ? 0.0f : a_live;
}

// the flag that makes step t stale: the end flag of step t - 1, or the one the env carried into the rollout
// (loaded once per step: it is `stale` of step t and `ended` of step t - 1)
__device__ __forceinline__ bool ended_before(const int64_t* __restrict__ reset, const int64_t* __restrict__ ended_prev, long t,
                                             long e, long N)
{
    const int64_t* p = t > 0 ? reset + (t - 1) * N + e : ended_prev + e;
    return *p != 0;
}

// the kernels' inputs: the rollout tensors [T][N], the flag rows as the rollout wrote them, limit = max_episode_length - 1
#define EPISODIC_INPUTS                                                                                                       \
    const float* __restrict__ reward, const float* __restrict__ v, const float* __restrict__ v_next,                         \
        const int64_t* __restrict__ reset, const int64_t* __restrict__ progress, const int64_t* __restrict__ ended_prev,     \
        long limit, const float* __restrict__ table, float gamma, float gl, long T, long N

// lane = env; workgroup g takes the env blocks g, g + gridDim.x, ...  The loads of step t - 1.. do not depend on the carried
// advantage, so the unrolled body keeps several steps of loads in flight.
template <bool VNORM>
__global__ __launch_bounds__(GAE_BLOCK) void gae_episodic_kernel(EPISODIC_INPUTS, float* __restrict__ target_out,
                                                                 float* __restrict__ adv_out, double* __restrict__ sets)
{
    float tm = 0.0f, ts = 1.0f;
    if (VNORM) { tm = table[0]; ts = table[1]; }
    double cn = 0.0, cm = 0.0, cq = 0.0;
    // VNORM: a fixed number of workgroups strides over the env blocks; plain: one block each, and said so -- a loop the compiler
    // must assume to repeat keeps it from hoisting the unrolled steps' loads over the stores
    for (long e = (long)blockIdx.x * GAE_BLOCK + threadIdx.x; e < N; e = VNORM ? e + (long)gridDim.x * GAE_BLOCK : N) {
        float a = 0.0f;
        bool ended = reset[(T - 1) * N + e] != 0;
        auto step = [&](long i, bool stale) {
            const bool timeout = ended & (progress[i] >= limit);      // the load is unconditional
            float tg;
            a = episodic_row<VNORM>(reward[i], v[i], v_next[i], ended, timeout, stale, tm, ts, gamma, gl, a, tg);
            target_out[i] = tg;
            adv_out[i] = a;
            if (VNORM) value_moments_add(cn, cm, cq, tg);
            ended = stale;                                            // loaded once: `stale` of step t is `ended` of step t - 1
        };
#pragma unroll 8
        for (long t = T - 1; t > 0; --t) step(t * N + e, reset[(t - 1) * N + e] != 0);
        step(e, ended_prev[e] != 0);                                  // t = 0: the flag the env carried into the rollout
    }
    if (VNORM) value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

// One wave per env; the 64 lanes own 64 consecutive chunks of ceil(T / 64) steps, lane 0 the LAST one (ppo_kernels.hip describes
// the scan).  A step's recurrence is a = mult_t a_next + delta_t with mult_t = gl cont_t, and 0 on a stale row: still linear, so
//   pass 1  every lane runs its chunk from a zero carry (S) and multiplies its steps' multipliers (m): 0 as soon as the chunk
//           holds an end or a stale row, gl^len otherwise -- the product ppo_td_gae_scan_kernel forms, in the same order;
//   carry   the same Kogge-Stone scan of (m, S) pairs.  m = 0 is exact, and 0 x (a finite carry) + S = S: a chunk with an end
//           hands on what lies on its own side of the end and nothing from beyond it;
//   pass 2  every lane reruns its chunk from the true carry.
// Lanes whose chunk lies before t = 0 (T < 64, or a ragged T) run no step and contribute (1, 0).
template <bool VNORM>
__global__ __launch_bounds__(GAE_BLOCK) void gae_episodic_scan_kernel(EPISODIC_INPUTS, float* __restrict__ target_out,
                                                                      float* __restrict__ adv_out, double* __restrict__ sets)
{
    float tm = 0.0f, ts = 1.0f;
    if (VNORM) { tm = table[0]; ts = table[1]; }
    const int lane = threadIdx.x;
    const TimeChunk c = reverse_chunk(T, lane);
    const long t_lo = c.t_lo, t_hi = c.t_hi;
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long e = blockIdx.x; e < N; e += gridDim.x) {
        const bool ended_hi = t_hi > 0 ? reset[(t_hi - 1) * N + e] != 0 : false;
        // pass 1: chunk contribution and multiplier
        float S = 0.0f, m = 1.0f;
        bool ended = ended_hi;
        for (long t = t_hi - 1; t >= t_lo && t_hi > 0; --t) {
            const long i = t * N + e;
            const bool stale = ended_before(reset, ended_prev, t, e, N);
            const bool timeout = ended & (progress[i] >= limit);      // the load is unconditional
            float tg;
            S = episodic_row<VNORM>(reward[i], v[i], v_next[i], ended, timeout, stale, tm, ts, gamma, gl, S, tg);
            m = (ended || stale) ? 0.0f : m * gl;
            ended = stale;
        }
        if (t_hi <= 0) { S = 0.0f; m = 1.0f; }
        // pass 2: the real recurrence from the true carry, the advantage entering this chunk
        float a = affine_carry(m, S, lane);
        ended = ended_hi;
        for (long t = t_hi - 1; t >= t_lo && t_hi > 0; --t) {
            const long i = t * N + e;
            const bool stale = ended_before(reset, ended_prev, t, e, N);
            const bool timeout = ended & (progress[i] >= limit);      // the load is unconditional
            float tg;
            a = episodic_row<VNORM>(reward[i], v[i], v_next[i], ended, timeout, stale, tm, ts, gamma, gl, a, tg);
            target_out[i] = tg;
            adv_out[i] = a;
            if (VNORM) value_moments_add(cn, cm, cq, tg);
            ended = stale;
        }
    }
    if (VNORM) value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

// table == NULL: the plain kernels (no sets); else the value-normalising ones, always VALUE_NORM_SETS workgroups: one set each,
// and those with no env write an empty set.
hipError_t launch_episodic(const float* reward, const float* v, const float* v_next, const int64_t* reset, const int64_t* progress,
                           const int64_t* ended_prev, int64_t max_episode_length, const float* table, float gamma, float lambda,
                           int64_t T, int64_t N, float* target_out, float* adv_out, double* sets, int mode, void* stream)
{
    const float gl = (float)((double)gamma * (double)lambda);   // python double product, ppo.py:167
    const long limit = (long)max_episode_length - 1;
    const bool vnorm = table != nullptr;
    if (mode & PPO_GAE_SCAN)
        return with_bools([&](auto vn) {
            const long grid = vn.value ? VALUE_NORM_SETS : (N < SCAN_GRID_MAX ? (long)N : SCAN_GRID_MAX);
            return launch_kernel<gae_episodic_scan_kernel<vn.value>>(dim3((unsigned)grid), GAE_BLOCK, 0, stream, reward, v, v_next, reset, progress,
                                                                     ended_prev, limit, table, gamma, gl, (long)T, (long)N, target_out, adv_out,
                                                                     sets);
        }, vnorm);
    return with_bools([&](auto vn) {
        const long grid = vn.value ? VALUE_NORM_SETS : (N + GAE_BLOCK - 1) / GAE_BLOCK;
        return launch_kernel<gae_episodic_kernel<vn.value>>(dim3((unsigned)grid), GAE_BLOCK, 0, stream, reward, v, v_next, reset, progress, ended_prev,
                                                            limit, table, gamma, gl, (long)T, (long)N, target_out, adv_out, sets);
    }, vnorm);
}

}  // namespace

extern "C" hipError_t flyhip_launch_td_gae_episodic(const float* reward, const float* v, const float* v_next, const int64_t* reset,
                                                    const int64_t* progress, const int64_t* ended_prev,
                                                    int64_t max_episode_length, float gamma, float lambda, int64_t T, int64_t N,
                                                    float* target_out, float* adv_out, int mode, void* stream)
{
    return launch_episodic(reward, v, v_next, reset, progress, ended_prev, max_episode_length, nullptr, gamma, lambda, T, N,
                           target_out, adv_out, nullptr, mode, stream);
}

extern "C" hipError_t flyhip_launch_td_gae_episodic_vnorm(const float* reward, const float* v, const float* v_next,
                                                          const int64_t* reset, const int64_t* progress, const int64_t* ended_prev,
                                                          int64_t max_episode_length, const float* table, float gamma, float lambda,
                                                          int64_t T, int64_t N, float* target_out, float* adv_out, double* sets,
                                                          int mode, void* stream)
{
    return launch_episodic(reward, v, v_next, reset, progress, ended_prev, max_episode_length, table, gamma, lambda, T, N,
                           target_out, adv_out, sets, mode, stream);
}
