// episode_stats.hip — return and length of finished episodes (PPO --episode_stats).
//
//   episode_stats_kernel         lane = env, t walks forward with the env's carry (return so far, steps so far)
//   episode_stats_scan_kernel    one wave per env, time on lanes (PPO_GAE_SCAN): a segmented scan of the chunk sums
//   episode_stats_merge_kernel   one workgroup: the launch's sets, in index order, into the persistent `window` and `total`
//
// Per env e and step t = 0 .. T-1, from the rollout's reward row and the int64 flag rows the env step left:
//   carry_ret += (double)reward[t][e];  carry_len += 1                       every step counts, the one that performs a reset too
//   reset[t][e] != 0:  an episode closes with return carry_ret, length carry_len and
//                      timeout = progress[t][e] >= max_episode_length - 1    (gae_episodic.hip's rule);  carry_ret = carry_len = 0
// A set is EPISODE_SET doubles:  n | ret_mean | ret_M2 | ret_min | ret_max | len_sum | len_min | len_max | timeouts | rows
// (integers held exactly; rows = the (t, e) rows the workgroup walked).  Returns are folded one by one with value_norm.h's
// value_moments_merge (a one-element set: the float64 Welford update), lanes by its shuffle tree.  Deterministic: fixed
// order, no atomics.  A NaN reward makes its episode's return NaN; the integer fields and the other envs' carries do not see it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "launch.h"

#define EPISODE_SET FLY_EPISODE_SET
#define EPISODE_SETS FLY_EPISODE_SETS

namespace {

constexpr int EPISODE_BLOCK = 64;           // one wave per workgroup, as gae_episodic_kernel: envs spread over the CUs

struct EpisodeSet {
    double n, mean, m2, rmin, rmax, lsum, lmin, lmax, timeouts, rows;
};

__device__ __forceinline__ EpisodeSet episode_set_empty()
{
    return {0.0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY, 0.0, (double)INFINITY, 0.0, 0.0, 0.0};
}

// one closed episode into the set
__device__ __forceinline__ void episode_close(EpisodeSet& s, double ret, long len, bool timeout)
{
    value_moments_merge(s.n, s.mean, s.m2, 1.0, ret, 0.0);
    s.rmin = ret < s.rmin ? ret : s.rmin;
    s.rmax = ret > s.rmax ? ret : s.rmax;
    const double l = (double)len;
    s.lsum += l;
    s.lmin = l < s.lmin ? l : s.lmin;
    s.lmax = l > s.lmax ? l : s.lmax;
    s.timeouts += timeout ? 1.0 : 0.0;
}

// a <- a + b; an empty side leaves the other's episode fields as they are
__device__ __forceinline__ void episode_set_merge(EpisodeSet& a, const EpisodeSet& b)
{
    value_moments_merge(a.n, a.mean, a.m2, b.n, b.mean, b.m2);
    a.rmin = b.rmin < a.rmin ? b.rmin : a.rmin;
    a.rmax = b.rmax > a.rmax ? b.rmax : a.rmax;
    a.lsum += b.lsum;
    a.lmin = b.lmin < a.lmin ? b.lmin : a.lmin;
    a.lmax = b.lmax > a.lmax ? b.lmax : a.lmax;
    a.timeouts += b.timeouts;
    a.rows += b.rows;
}

__device__ __forceinline__ EpisodeSet episode_set_load(const double* __restrict__ p)
{
    return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]};
}

__device__ __forceinline__ void episode_set_store(const EpisodeSet& s, double* __restrict__ p)
{
    p[0] = s.n; p[1] = s.mean; p[2] = s.m2; p[3] = s.rmin; p[4] = s.rmax;
    p[5] = s.lsum; p[6] = s.lmin; p[7] = s.lmax; p[8] = s.timeouts; p[9] = s.rows;
}

// The wave's 64 per-lane sets -> lane 0 by value_write_set's shuffle tree; lane 0 writes the workgroup's set.
__device__ __forceinline__ void episode_write_set(EpisodeSet s, double* __restrict__ set)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        EpisodeSet b;
        b.n = __shfl_down(s.n, o, 64); b.mean = __shfl_down(s.mean, o, 64); b.m2 = __shfl_down(s.m2, o, 64);
        b.rmin = __shfl_down(s.rmin, o, 64); b.rmax = __shfl_down(s.rmax, o, 64); b.lsum = __shfl_down(s.lsum, o, 64);
        b.lmin = __shfl_down(s.lmin, o, 64); b.lmax = __shfl_down(s.lmax, o, 64);
        b.timeouts = __shfl_down(s.timeouts, o, 64); b.rows = __shfl_down(s.rows, o, 64);
        episode_set_merge(s, b);
    }
    if (threadIdx.x == 0) episode_set_store(s, set);
}

// lane = env; workgroup g takes the env blocks g, g + gridDim.x, ...  No load depends on the carry, so the unrolled body keeps
// several steps of loads in flight; the three loads of a step are unconditional.
__global__ __launch_bounds__(EPISODE_BLOCK) void episode_stats_kernel(const float* __restrict__ reward,
                                                                      const int64_t* __restrict__ reset,
                                                                      const int64_t* __restrict__ progress, long limit, long T,
                                                                      long N, double* __restrict__ carry_ret,
                                                                      int64_t* __restrict__ carry_len, double* __restrict__ sets)
{
    EpisodeSet s = episode_set_empty();
    for (long e = (long)blockIdx.x * EPISODE_BLOCK + threadIdx.x; e < N; e += (long)gridDim.x * EPISODE_BLOCK) {
        double cr = carry_ret[e];
        long cl = carry_len[e];
#pragma unroll 8
        for (long t = 0; t < T; ++t) {
            const long i = t * N + e;
            const float r = reward[i];
            const bool ended = reset[i] != 0;
            const bool timeout = progress[i] >= limit;
            cr += (double)r;
            cl += 1;
            if (ended) {
                episode_close(s, cr, cl, timeout);
                cr = 0.0;
                cl = 0;
            }
        }
        s.rows += (double)T;
        carry_ret[e] = cr;
        carry_len[e] = cl;
    }
    episode_write_set(s, sets + (long)blockIdx.x * EPISODE_SET);
}

// One wave per env; the 64 lanes own 64 consecutive chunks of L = ceil(T / 64) steps, lane 0 the EARLIEST one.  A lane walks its
// chunk once from a zero carry and keeps
//   head  (sum, len) up to and including its first end, and that end's timeout      -- closed after the scan, with what comes in
//   tail  (sum, len) behind its last end; without an end, of the whole chunk        -- what the chunk hands on
// and folds the episodes that begin and end inside the chunk into its set at once.  The chunks' (has_end, sum, len) triples
// combine as  a . b = b if b.has_end else (a.has_end, a.sum + b.sum, a.len + b.len)  (a the earlier one): associative, so a
// Kogge-Stone inclusive scan by __shfl_up gives every lane the open episode at its chunk's end; moved up one lane it is the one
// at the chunk's start, and where no lane before has an end the env's carry-in is added in front.  Lanes whose chunk starts at
// or beyond T walk nothing and contribute the neutral (false, 0, 0), so lane 63 holds the env's carry-out.
__global__ __launch_bounds__(EPISODE_BLOCK) void episode_stats_scan_kernel(const float* __restrict__ reward,
                                                                           const int64_t* __restrict__ reset,
                                                                           const int64_t* __restrict__ progress, long limit,
                                                                           long T, long N, double* __restrict__ carry_ret,
                                                                           int64_t* __restrict__ carry_len,
                                                                           double* __restrict__ sets)
{
    const int lane = threadIdx.x;
    const long L = (T + 63) / 64;
    const long t_lo = (long)lane * L < T ? (long)lane * L : T;
    const long t_hi = t_lo + L < T ? t_lo + L : T;          // exclusive; t_lo == t_hi: nothing to walk
    EpisodeSet s = episode_set_empty();
    for (long e = blockIdx.x; e < N; e += gridDim.x) {
        const double in_ret = carry_ret[e];                 // wave-uniform
        const long long in_len = carry_len[e];
        double sum = 0.0, head_sum = 0.0;
        long long len = 0, head_len = 0;
        bool has_end = false, head_timeout = false;
        // the same L trips in every lane, so the unrolled loads are in flight together; a step beyond the lane's chunk (the
        // ragged last chunk, the empty lanes) reads row 0 and is ignored
#pragma unroll 4
        for (long k = 0; k < L; ++k) {
            const bool live = t_lo + k < t_hi;
            const long i = (live ? t_lo + k : 0) * N + e;
            const float r = reward[i];
            const bool ended = live & (reset[i] != 0);
            const bool timeout = progress[i] >= limit;
            sum += live ? (double)r : 0.0;
            len += live ? 1 : 0;
            if (ended) {
                if (has_end) {
                    episode_close(s, sum, len, timeout);
                } else {
                    head_sum = sum; head_len = len; head_timeout = timeout;
                    has_end = true;
                }
                sum = 0.0;
                len = 0;
            }
        }
        s.rows += (double)(t_hi - t_lo);
        // inclusive scan over lanes
        int xe = has_end ? 1 : 0;
        double xs = sum;
        long long xl = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int pe = __shfl_up(xe, o, 64);
            const double ps = __shfl_up(xs, o, 64);
            const long long pl = __shfl_up(xl, o, 64);
            if (lane >= o && !xe) { xe = pe; xs = ps + xs; xl = pl + xl; }
        }
        // the open episode at this chunk's start
        int ie = __shfl_up(xe, 1, 64);
        double is = __shfl_up(xs, 1, 64);
        long long il = __shfl_up(xl, 1, 64);
        if (lane == 0) { ie = 0; is = 0.0; il = 0; }
        if (!ie) { is = in_ret + is; il = in_len + il; }
        if (has_end) episode_close(s, is + head_sum, (long)(il + head_len), head_timeout);
        if (lane == 63) {
            carry_ret[e] = xe ? xs : in_ret + xs;
            carry_len[e] = xe ? xl : in_len + xl;
        }
    }
    episode_write_set(s, sets + (long)blockIdx.x * EPISODE_SET);
}

// One workgroup.  The nsets sets go through LDS 64 at a time; thread 0 folds them in index order into one set of this launch
// and that into `window` and into `total`.
__global__ __launch_bounds__(EPISODE_BLOCK) void episode_stats_merge_kernel(const double* __restrict__ sets, long nsets,
                                                                            double* __restrict__ window,
                                                                            double* __restrict__ total)
{
    __shared__ double buf[EPISODE_BLOCK][EPISODE_SET + 1];
    EpisodeSet b = episode_set_empty();
    for (long base = 0; base < nsets; base += EPISODE_BLOCK) {
        const long mine = base + threadIdx.x;
        if (mine < nsets) {
#pragma unroll
            for (int k = 0; k < EPISODE_SET; ++k) buf[threadIdx.x][k] = sets[mine * EPISODE_SET + k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long count = nsets - base < EPISODE_BLOCK ? nsets - base : EPISODE_BLOCK;
            for (long j = 0; j < count; ++j) episode_set_merge(b, episode_set_load(buf[j]));
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    EpisodeSet w = episode_set_load(window), a = episode_set_load(total);
    episode_set_merge(w, b);
    episode_set_merge(a, b);
    episode_set_store(w, window);
    episode_set_store(a, total);
}

}  // namespace

// always EPISODE_SETS workgroups: one set each, and those with no env write the empty set
extern "C" hipError_t flyhip_launch_episode_stats(const float* reward, const int64_t* reset, const int64_t* progress,
                                                  int64_t max_episode_length, int64_t T, int64_t N, double* carry_ret,
                                                  int64_t* carry_len, double* sets, int mode, void* stream)
{
    const long limit = (long)max_episode_length - 1;
    if (mode & PPO_GAE_SCAN)
        return launch_kernel<episode_stats_scan_kernel>(EPISODE_SETS, EPISODE_BLOCK, 0, stream, reward, reset, progress, limit,
                                                        (long)T, (long)N, carry_ret, carry_len, sets);
    return launch_kernel<episode_stats_kernel>(EPISODE_SETS, EPISODE_BLOCK, 0, stream, reward, reset, progress, limit, (long)T,
                                               (long)N, carry_ret, carry_len, sets);
}

extern "C" hipError_t flyhip_launch_episode_stats_merge(const double* sets, int64_t nsets, double* window, double* total,
                                                        void* stream)
{
    return launch_kernel<episode_stats_merge_kernel>(1, EPISODE_BLOCK, 0, stream, sets, (long)nsets, window, total);
}
