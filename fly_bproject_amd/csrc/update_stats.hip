// update_stats.hip — diagnostics of a finished PPO update (PPO --update_stats).
//
//   update_stats_kernel          256 workgroups, grid-stride over tiles of 256 rows: one set per workgroup
//   update_stats_merge_kernel    one workgroup: the sets, in index order, into `last`, and that into `window` and `total`
//
// A probe BEHIND the update: the rows' mu and v come from one mlp_forward of the updated network, and this file reduces them
// with the rollout's action / old log-prob / advantage / target rows.  Per row, in fp32 with separately rounded ops:
//   L_d = sqrtf(var_d), hld = sum_d logf(L_d) (d order), inv_var_d = 1.0f / var_d           once per launch, as ppo_sample_logprob
//   M     = sum_d ((a_d - mu_d)^2 * inv_var_d)                                              d order 0..17, from 0
//   logp  = gauss_logp(M, hld);  lr = logp - old_logp;  ratio = expf(lr)
//   pol, hub = ppo_row_loss<false>(M, hld, old_logp, A, v, target, 1.0f, clip)              loss_head.inc's lines themselves
//   clipped  = !(ratio >= 1 - clip && ratio <= 1 + clip)                                    the loss head's closed interval
// A row is NON-FINITE when any of lr, ratio, A, v, target is NaN or +-inf: it counts in rows and nonfinite and in nothing else.
// A set is UPDATE_SET float64 (flyhip_update_stats.h has the table); finite rows accumulate in float64, moments by value_norm.h
// (Welford per lane, Chan merge), everything by one fixed tree: shuffle tree per wave, waves 1..3 into wave 0 in wave order.
// No atomics: two launches give the same bits.
//
// Memory form: a row is 72 bytes in mu and in action, so lane = row would issue 18 dword loads at a 72-byte lane stride per
// array.  Instead a tile's mu and action are read as FLAT arrays (16-byte loads when both bases allow it; a tile starts at a
// multiple of 256 * 72 bytes), e = (a - mu)^2 * inv_var[flat index mod 18] is formed at load time and written to LDS rows
// padded to 19 floats (a stride of 18 dwords is a 2-way conflict across a wave, 19 is conflict-free), and after a barrier
// lane = row sums its 18 terms in d order.  The next tile's loads are issued before this tile's row phase.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "value_norm.h"
#include "launch.h"

#define UPDATE_SET FLY_UPDATE_STATS_SET
#define UPDATE_SETS FLY_UPDATE_STATS_SETS

namespace {

#include "loss_head.inc"

constexpr int US_BLOCK = 256;               // threads = rows of a tile
constexpr int US_NA = 18;                   // action dimensions
constexpr int US_PAD = 19;                  // LDS row stride in floats
constexpr int US_TILE_FLOATS = US_BLOCK * US_NA;                    // 4608 floats of mu (and of action) per tile
constexpr int US_VEC_TRIPS = (US_TILE_FLOATS / 4 + US_BLOCK - 1) / US_BLOCK;     // 5 float4 per thread (the fifth: half the threads)
static_assert(UPDATE_SET == 17, "the set layout below");

struct UpdateSet {
    double rows, k1, k3, clipped, rmin, rmax, pol, hub, tn, tmean, tm2, en, emean, em2, nonfinite, amax, tmax;
};

__device__ __forceinline__ UpdateSet update_set_empty()
{
    return {0.0, 0.0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
}

// a <- a + b: sums and counts add, extremes combine, moments by Chan's merge; an empty b (no rows) leaves a as it is
__device__ __forceinline__ void update_set_merge(UpdateSet& a, const UpdateSet& b)
{
    if (!(b.rows > 0.0)) return;
    a.rows += b.rows;
    a.k1 += b.k1;
    a.k3 += b.k3;
    a.clipped += b.clipped;
    a.rmin = b.rmin < a.rmin ? b.rmin : a.rmin;
    a.rmax = b.rmax > a.rmax ? b.rmax : a.rmax;
    a.pol += b.pol;
    a.hub += b.hub;
    value_moments_merge(a.tn, a.tmean, a.tm2, b.tn, b.tmean, b.tm2);
    value_moments_merge(a.en, a.emean, a.em2, b.en, b.emean, b.em2);
    a.nonfinite += b.nonfinite;
    a.amax = b.amax > a.amax ? b.amax : a.amax;
    a.tmax = b.tmax > a.tmax ? b.tmax : a.tmax;
}

__device__ __forceinline__ UpdateSet update_set_load(const double* p)
{
    return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], p[15], p[16]};
}

__device__ __forceinline__ void update_set_store(const UpdateSet& s, double* p)
{
    p[0] = s.rows; p[1] = s.k1; p[2] = s.k3; p[3] = s.clipped; p[4] = s.rmin; p[5] = s.rmax; p[6] = s.pol; p[7] = s.hub;
    p[8] = s.tn; p[9] = s.tmean; p[10] = s.tm2; p[11] = s.en; p[12] = s.emean; p[13] = s.em2; p[14] = s.nonfinite;
    p[15] = s.amax; p[16] = s.tmax;
}

__device__ __forceinline__ UpdateSet update_set_shfl_down(const UpdateSet& s, int o)
{
    UpdateSet b;
    b.rows = __shfl_down(s.rows, o, 64); b.k1 = __shfl_down(s.k1, o, 64); b.k3 = __shfl_down(s.k3, o, 64);
    b.clipped = __shfl_down(s.clipped, o, 64); b.rmin = __shfl_down(s.rmin, o, 64); b.rmax = __shfl_down(s.rmax, o, 64);
    b.pol = __shfl_down(s.pol, o, 64); b.hub = __shfl_down(s.hub, o, 64);
    b.tn = __shfl_down(s.tn, o, 64); b.tmean = __shfl_down(s.tmean, o, 64); b.tm2 = __shfl_down(s.tm2, o, 64);
    b.en = __shfl_down(s.en, o, 64); b.emean = __shfl_down(s.emean, o, 64); b.em2 = __shfl_down(s.em2, o, 64);
    b.nonfinite = __shfl_down(s.nonfinite, o, 64); b.amax = __shfl_down(s.amax, o, 64); b.tmax = __shfl_down(s.tmax, o, 64);
    return b;
}

// one row into the lane's set
__device__ __forceinline__ void update_set_row(UpdateSet& s, float M, float hld, float old_logp, float A, float v, float target,
                                               float clip)
{
    const float logp = gauss_logp(M, hld);
    const float lr = logp - old_logp;
    const float ratio = expf(lr);
    const PpoRowLoss r = ppo_row_loss<false>(M, hld, old_logp, A, v, target, 1.0f, clip);
    s.rows += 1.0;
    if (!(isfinite(lr) && isfinite(ratio) && isfinite(A) && isfinite(v) && isfinite(target))) {
        s.nonfinite += 1.0;
        return;
    }
    const double dr = (double)ratio, dl = (double)lr;
    s.k1 += -dl;
    s.k3 += dr - 1.0 - dl;
    s.clipped += (ratio >= 1.0f - clip && ratio <= 1.0f + clip) ? 0.0 : 1.0;
    s.rmin = dr < s.rmin ? dr : s.rmin;
    s.rmax = dr > s.rmax ? dr : s.rmax;
    s.pol += (double)r.pol;
    s.hub += (double)r.hub;
    value_moments_add(s.tn, s.tmean, s.tm2, target);
    value_moments_add(s.en, s.emean, s.em2, (double)target - (double)v);
    const double aa = (double)fabsf(A), at = (double)fabsf(target);
    s.amax = aa > s.amax ? aa : s.amax;
    s.tmax = at > s.tmax ? at : s.tmax;
}

// What a thread holds of a tile between its loads and its LDS stores: the e terms of its flat elements and its row's scalars.
template <bool VEC>
struct UpdateTile {
    float e[VEC ? US_VEC_TRIPS * 4 : US_NA];
    float old_logp, adv, v, target;
};

__device__ __forceinline__ float update_e(float a, float mu, float inv_var)
{
    const float d = __fsub_rn(a, mu);
    return __fmul_rn(__fmul_rn(d, d), inv_var);
}

// The loads of the tile that starts at row r0 (nr = its rows, 1..256).  No element at or beyond flat index nr * 18 is read.
template <bool VEC>
__device__ __forceinline__ void update_tile_load(UpdateTile<VEC>& t, const float* __restrict__ mu, const float* __restrict__ action,
                                                 const float* __restrict__ old_logp, const float* __restrict__ adv,
                                                 const float* __restrict__ v, const float* __restrict__ target,
                                                 const float* inv_var, long r0, int nr)
{
    const int tid = threadIdx.x;
    const int nfl = nr * US_NA;
    const float* m = mu + r0 * US_NA;
    const float* a = action + r0 * US_NA;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < US_VEC_TRIPS; ++k) {
            const int f = 4 * (tid + k * US_BLOCK);
            float mm[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aa[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (f + 4 <= nfl) {
                const float4 m4 = *reinterpret_cast<const float4*>(m + f), a4 = *reinterpret_cast<const float4*>(a + f);
                mm[0] = m4.x; mm[1] = m4.y; mm[2] = m4.z; mm[3] = m4.w;
                aa[0] = a4.x; aa[1] = a4.y; aa[2] = a4.z; aa[3] = a4.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (f + j < nfl) { mm[j] = m[f + j]; aa[j] = a[f + j]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = (f + j) % US_NA;                    // f + j < 5120: the table read stays inside inv_var[18]
                t.e[4 * k + j] = update_e(aa[j], mm[j], inv_var[col]);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < US_NA; ++k) {
            const int f = tid + k * US_BLOCK;
            float mm = 0.0f, aa = 0.0f;
            if (f < nfl) { mm = m[f]; aa = a[f]; }
            t.e[k] = update_e(aa, mm, inv_var[f % US_NA]);
        }
    }
    t.old_logp = t.adv = t.v = t.target = 0.0f;
    if (tid < nr) {
        const long r = r0 + tid;
        t.old_logp = old_logp[r]; t.adv = adv[r]; t.v = v[r]; t.target = target[r];
    }
}

// The tile's e terms into the padded LDS rows: flat element f is row f / 18, column f % 18, at f + f / 18.
template <bool VEC>
__device__ __forceinline__ void update_tile_to_lds(const UpdateTile<VEC>& t, float* es)
{
    const int tid = threadIdx.x;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < US_VEC_TRIPS; ++k) {
            const int f = 4 * (tid + k * US_BLOCK);
            if (f < US_TILE_FLOATS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) es[f + j + (f + j) / US_NA] = t.e[4 * k + j];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < US_NA; ++k) {
            const int f = tid + k * US_BLOCK;
            es[f + f / US_NA] = t.e[k];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(US_BLOCK) void update_stats_kernel(const float* __restrict__ mu, const float* __restrict__ action,
                                                                const float* __restrict__ old_logp,
                                                                const float* __restrict__ adv, const float* __restrict__ v,
                                                                const float* __restrict__ target, const float* __restrict__ var,
                                                                float clip, long R, double* __restrict__ sets)
{
    __shared__ float es[US_BLOCK * US_PAD];
    __shared__ float inv_var[US_NA];
    __shared__ float hld_s;
    __shared__ double part[3][UPDATE_SET];
    const int tid = threadIdx.x;
    if (tid < US_NA) inv_var[tid] = 1.0f / var[tid];
    if (tid == 0) {
        float h = 0.0f;
        for (int d = 0; d < US_NA; ++d) h = __fadd_rn(h, logf(sqrtf(var[d])));
        hld_s = h;
    }
    __syncthreads();
    const float hld = hld_s;
    UpdateSet s = update_set_empty();
    const long ntiles = (R + US_BLOCK - 1) / US_BLOCK;
    long tile = blockIdx.x;
    UpdateTile<VEC> t;
    if (tile < ntiles) {
        const long r0 = tile * US_BLOCK;
        update_tile_load<VEC>(t, mu, action, old_logp, adv, v, target, inv_var, r0, (int)(R - r0 < US_BLOCK ? R - r0 : US_BLOCK));
    }
    while (tile < ntiles) {
        const long r0 = tile * US_BLOCK;
        const int nr = (int)(R - r0 < US_BLOCK ? R - r0 : US_BLOCK);
        update_tile_to_lds<VEC>(t, es);
        const float old_lp = t.old_logp, A = t.adv, vv = t.v, tg = t.target;
        __syncthreads();
        tile += gridDim.x;
        if (tile < ntiles) {                                        // the next tile's loads, in flight under this tile's row phase
            const long n0 = tile * US_BLOCK;
            update_tile_load<VEC>(t, mu, action, old_logp, adv, v, target, inv_var, n0, (int)(R - n0 < US_BLOCK ? R - n0 : US_BLOCK));
        }
        if (tid < nr) {
            float M = 0.0f;
#pragma unroll
            for (int d = 0; d < US_NA; ++d) M = __fadd_rn(M, es[tid * US_PAD + d]);
            update_set_row(s, M, hld, old_lp, A, vv, tg, clip);
        }
        __syncthreads();                                            // every row is summed before the next tile overwrites es
    }
    // the fixed tree: 64 lanes -> lane 0 of each wave, waves 1..3 -> thread 0 in wave order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const UpdateSet b = update_set_shfl_down(s, o);
        update_set_merge(s, b);
    }
    const int wave = tid >> 6;
    if ((tid & 63) == 0 && wave > 0) update_set_store(s, part[wave - 1]);
    __syncthreads();
    if (tid != 0) return;
    for (int w = 0; w < 3; ++w) update_set_merge(s, update_set_load(part[w]));
    s.tm2 = s.tm2 > 0.0 ? s.tm2 : 0.0;
    s.em2 = s.em2 > 0.0 ? s.em2 : 0.0;
    update_set_store(s, sets + (long)blockIdx.x * UPDATE_SET);
}

// One workgroup.  The nsets sets go through LDS 64 at a time; thread 0 folds them in index order into one set, writes it to
// `last` and folds it into `window` and into `total`.
__global__ __launch_bounds__(64) void update_stats_merge_kernel(const double* __restrict__ sets, long nsets, double* last,
                                                                double* window, double* total)
{
    __shared__ double buf[64][UPDATE_SET + 1];
    UpdateSet b = update_set_empty();
    for (long base = 0; base < nsets; base += 64) {
        const long mine = base + threadIdx.x;
        if (mine < nsets) {
#pragma unroll
            for (int k = 0; k < UPDATE_SET; ++k) buf[threadIdx.x][k] = sets[mine * UPDATE_SET + k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long count = nsets - base < 64 ? nsets - base : 64;
            for (long j = 0; j < count; ++j) update_set_merge(b, update_set_load(buf[j]));
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    UpdateSet w = update_set_load(window), a = update_set_load(total);
    update_set_merge(w, b);
    update_set_merge(a, b);
    update_set_store(b, last);
    update_set_store(w, window);
    update_set_store(a, total);
}

}  // namespace

// always UPDATE_SETS workgroups: one set each, and those with no tile write the empty set
extern "C" hipError_t flyhip_launch_update_stats(const float* mu, const float* action, const float* old_logp, const float* adv,
                                                 const float* v, const float* target, const float* var, float clip, int64_t R,
                                                 double* sets, void* stream)
{
    const bool vec = ((reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(action)) & 15) == 0;
    if (vec)
        return launch_kernel<update_stats_kernel<true>>(UPDATE_SETS, US_BLOCK, 0, stream, mu, action, old_logp, adv, v, target, var,
                                                        clip, (long)R, sets);
    return launch_kernel<update_stats_kernel<false>>(UPDATE_SETS, US_BLOCK, 0, stream, mu, action, old_logp, adv, v, target, var,
                                                     clip, (long)R, sets);
}

extern "C" hipError_t flyhip_launch_update_stats_merge(const double* sets, int64_t nsets, double* last, double* window,
                                                       double* total, void* stream)
{
    return launch_kernel<update_stats_merge_kernel>(1, 64, 0, stream, sets, (long)nsets, last, window, total);
}
