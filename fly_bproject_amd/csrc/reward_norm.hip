// reward_norm.hip — running reward scaling (PPO --normalize_reward).
//
//   reward_returns_kernel        lane = env, t walks forward with the env's discounted return G in a register
//   reward_returns_scan_kernel   one wave per env, time on lanes (PPO_GAE_SCAN): a scan of the chunks' affine maps
//   reward_scale_kernel          out = clamp(reward * r, -clip, +clip), elementwise
//
// Per env e and step t = 0 .. T-1, from the rollout's reward row and the int64 reset-flag row the env step left:
//   G = fl(fl(g * G) + (double)reward[t][e])      g = (double)gamma; two separately rounded float64 ops, no fma
//   the moments take G                            every (t, e) counts, the step that performs a reset too
//   reset[t][e] != 0:  G = 0                      episode_stats.hip's end rule
// The moments are value_norm.h's sets (count | mean | M2, one per workgroup), so ppo_value_norm_merge folds them into the
// running statistics S_r and writes the table whose r scales the rewards.  Deterministic: fixed order, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "float4_map.h"
#include "launch.h"

namespace {

constexpr int RETURNS_BLOCK = 64;           // one wave per workgroup, as episode_stats_kernel: envs spread over the CUs

// one step of the return: the definition's two rounded ops
__device__ __forceinline__ double return_step(double g, double G, float r)
{
    return __dadd_rn(__dmul_rn(g, G), (double)r);
}

// lane = env; workgroup b takes the env blocks b, b + gridDim.x, ...  No load depends on the carry, so the unrolled body keeps
// several steps of loads in flight.  A lane reads carry_in[e] before it writes carry_out[e]: the two may be one buffer.
__global__ __launch_bounds__(RETURNS_BLOCK) void reward_returns_kernel(const float* __restrict__ reward,
                                                                       const int64_t* __restrict__ reset, double g, long T,
                                                                       long N, const double* carry_in, double* carry_out,
                                                                       double* __restrict__ sets)
{
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long e = (long)blockIdx.x * RETURNS_BLOCK + threadIdx.x; e < N; e += (long)gridDim.x * RETURNS_BLOCK) {
        double G = carry_in[e];
#pragma unroll 8
        for (long t = 0; t < T; ++t) {
            const long i = t * N + e;
            const float r = reward[i];
            const bool ended = reset[i] != 0;
            G = return_step(g, G, r);
            value_moments_add(cn, cm, cq, G);
            G = ended ? 0.0 : G;
        }
        carry_out[e] = G;
    }
    value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

// One wave per env; the 64 lanes own 64 consecutive chunks of L = ceil(T / 64) steps, lane 0 the EARLIEST one.  Over a chunk
// the return is an affine map of the return that enters it, G_out = a * G_in + b: a = g^len without an end in the chunk, a = 0
// and b the return behind the last end otherwise.  Pass 1 walks the chunk from (1, 0); maps compose as
// (a1, b1) then (a2, b2) = (a1 * a2, a2 * b1 + b2), associative, so a Kogge-Stone inclusive scan by __shfl_up gives every lane
// the map from the rollout's start to its chunk's end; moved up one lane and applied to carry_in[e] it is the chunk's G_in, and
// pass 2 walks the chunk again from there with the sequential rule and takes the moments.  a == 0 passes on exactly nothing
// (not 0 * b1: a NaN or an infinity stays behind the end that closed it).  Lanes whose chunk starts at or beyond T contribute
// the identity (1, 0) and no moments, so lane 63's inclusive map applied to carry_in[e] is the carry-out.
__global__ __launch_bounds__(RETURNS_BLOCK) void reward_returns_scan_kernel(const float* __restrict__ reward,
                                                                            const int64_t* __restrict__ reset, double g,
                                                                            long T, long N, const double* carry_in,
                                                                            double* carry_out, double* __restrict__ sets)
{
    const int lane = threadIdx.x;
    const long L = (T + 63) / 64;
    const long t_lo = (long)lane * L < T ? (long)lane * L : T;
    const long t_hi = t_lo + L < T ? t_lo + L : T;          // exclusive; t_lo == t_hi: nothing to walk
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (long e = blockIdx.x; e < N; e += gridDim.x) {
        const double cin = carry_in[e];                     // wave-uniform
        // pass 1: the same L trips in every lane, so the unrolled loads are in flight together; a step beyond the lane's chunk
        // (the ragged last chunk, the empty lanes) reads row 0 and is ignored
        double a = 1.0, b = 0.0;
#pragma unroll 4
        for (long k = 0; k < L; ++k) {
            const bool live = t_lo + k < t_hi;
            const long i = (live ? t_lo + k : 0) * N + e;
            const float r = reward[i];
            const bool ended = live & (reset[i] != 0);
            const double nb = return_step(g, b, r), na = __dmul_rn(a, g);
            b = live ? nb : b;
            a = live ? na : a;
            if (ended) { a = 0.0; b = 0.0; }
        }
        // inclusive scan over lanes: (pa, pb) is the earlier map
        double xa = a, xb = b;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double pa = __shfl_up(xa, o, 64), pb = __shfl_up(xb, o, 64);
            if (lane >= o && xa != 0.0) { xb = __dadd_rn(__dmul_rn(xa, pb), xb); xa = __dmul_rn(pa, xa); }
        }
        // the return that enters this chunk
        double ia = __shfl_up(xa, 1, 64), ib = __shfl_up(xb, 1, 64);
        if (lane == 0) { ia = 1.0; ib = 0.0; }
        double G = ia != 0.0 ? __dadd_rn(__dmul_rn(ia, cin), ib) : ib;
        // pass 2
#pragma unroll 4
        for (long k = 0; k < L; ++k) {
            const bool live = t_lo + k < t_hi;
            const long i = (live ? t_lo + k : 0) * N + e;
            const float r = reward[i];
            const bool ended = live & (reset[i] != 0);
            if (live) {
                G = return_step(g, G, r);
                value_moments_add(cn, cm, cq, G);
            }
            G = ended ? 0.0 : G;
        }
        if (lane == 63) carry_out[e] = xa != 0.0 ? __dadd_rn(__dmul_rn(xa, cin), xb) : xb;
    }
    value_write_set(cn, cm, cq, sets + (long)blockIdx.x * VALUE_NORM_SET);
}

// one rounded multiply, then the clamp by comparisons: NaN fails both and passes through
__device__ __forceinline__ float reward_scale(float x, float r, float clip)
{
    float y = __fmul_rn(x, r);
    y = y > clip ? clip : y;
    return y < -clip ? -clip : y;
}

// out[i] = clamp(reward[i] * r, -clip, clip), elementwise (float4_map.h).  Every element is read before it is written by the
// same thread, so out may be the reward buffer itself: the two pointers are not __restrict__.
__global__ __launch_bounds__(FLOAT4_MAP_THREADS) void reward_scale_kernel(const float* reward, long n,
                                                                          const float* __restrict__ table, float clip, float* out)
{
    const float r = table[2];
    float4_map(reward, n, out, [=](float x) { return reward_scale(x, r, clip); });
}

}  // namespace

// always VALUE_NORM_SETS workgroups: one set each, and those with no env write the empty set
extern "C" hipError_t flyhip_launch_reward_returns(const float* reward, const int64_t* reset, float gamma, int64_t T, int64_t N,
                                                   const double* carry_in, double* carry_out, double* sets, int mode,
                                                   void* stream)
{
    const double g = (double)gamma;
    if (mode & PPO_GAE_SCAN)
        return launch_kernel<reward_returns_scan_kernel>(VALUE_NORM_SETS, RETURNS_BLOCK, 0, stream, reward, reset, g, (long)T,
                                                         (long)N, carry_in, carry_out, sets);
    return launch_kernel<reward_returns_kernel>(VALUE_NORM_SETS, RETURNS_BLOCK, 0, stream, reward, reset, g, (long)T, (long)N,
                                                carry_in, carry_out, sets);
}

extern "C" hipError_t flyhip_launch_reward_scale(const float* reward, int64_t n, const float* table, float clip, float* out,
                                                 void* stream)
{
    return launch_kernel<reward_scale_kernel>(float4_map_grid(n), FLOAT4_MAP_THREADS, 0, stream, reward, (long)n, table, clip, out);
}
