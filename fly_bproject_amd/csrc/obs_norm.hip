// obs_norm.hip — running observation normalisation for PPO (--normalize_obs).
//
//   obs_norm_pass_kernel    one pass over the raw observation ring: the normalised copy under the current table, and the
//                           batch moments (count, mean, M2) of the counted rows in float64, one set per workgroup
//   obs_norm_merge_kernel   one workgroup: the sets combined in order (Chan et al.'s parallel update), folded into the running
//                           statistics S, and the fp32 table rewritten in place -- no host sync, the table never moves
//
// Both are deterministic: every sum runs in a fixed order, so two runs on the same data are bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "obs_norm.h"
#include "launch.h"

namespace {

constexpr int NC = OBS_NORM_COLS;
constexpr int SUBS = 12;                    // rows a workgroup reads at once: 12 x 73 consecutive floats, one per thread
constexpr int PASS_THREADS = 896;           // 14 waves; threads 876 .. 895 only take part in the barrier
constexpr int UNROLL = 4;                   // loads in flight per thread
static_assert(SUBS * NC <= PASS_THREADS, "one thread per (row, column) of a row group");

// Workgroup g walks flat rows [rows * g / G, rows * (g + 1) / G) of ring [rows][73].  Thread (sub, col) reads rows sub, sub + 12,
// ... of that range (so each step of the workgroup reads 876 consecutive floats), writes their normalised values and, for rows
// >= count_from, sums d = x - x0 and d^2 in float64.  The shift x0 is the range's first counted value of the column: close to the
// column's values whatever their mean, so the sums do not cancel (a column of mean 1e3 and std 1e-2 keeps its digits).
__global__ __launch_bounds__(PASS_THREADS) void obs_norm_pass_kernel(const float* __restrict__ ring, long rows, long count_from,
                                                                      const float* __restrict__ table, float* __restrict__ out,
                                                                      double* __restrict__ sets)
{
    __shared__ double red[2][SUBS][NC];
    const int tid = threadIdx.x;
    const int sub = tid / NC, col = tid - sub * NC;
    const bool act = tid < SUBS * NC;
    const long r0 = rows * blockIdx.x / gridDim.x, r1 = rows * (blockIdx.x + 1) / gridDim.x;
    const long rf = r0 > count_from ? r0 : count_from;         // first counted row of the range
    double s1 = 0.0, s2 = 0.0;
    if (act) {
        const float m = table[col], rs = table[NC + col], clip = table[2 * NC];
        const double x0 = rf < r1 ? (double)ring[rf * NC + col] : 0.0;
        long r = r0 + sub;
        for (; r + (UNROLL - 1) * SUBS < r1; r += UNROLL * SUBS) {
            float v[UNROLL];
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) v[k] = ring[(r + k * SUBS) * NC + col];
#pragma unroll
            for (int k = 0; k < UNROLL; ++k) {
                out[(r + k * SUBS) * NC + col] = obs_norm_apply(v[k], m, rs, clip);
                if (r + k * SUBS >= count_from) {
                    const double d = (double)v[k] - x0;
                    s1 += d;
                    s2 += d * d;
                }
            }
        }
        for (; r < r1; r += SUBS) {
            const float v = ring[r * NC + col];
            out[r * NC + col] = obs_norm_apply(v, m, rs, clip);
            if (r >= count_from) {
                const double d = (double)v - x0;
                s1 += d;
                s2 += d * d;
            }
        }
        red[0][sub][col] = s1;
        red[1][sub][col] = s2;
    }
    __syncthreads();
    if (tid < NC) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int s = 0; s < SUBS; ++s) { t1 += red[0][s][tid]; t2 += red[1][s][tid]; }
        const long cnt = rf < r1 ? r1 - rf : 0;
        double* set = sets + (long)blockIdx.x * OBS_NORM_SET;
        if (cnt > 0) {
            const double nd = (double)cnt;
            const double m2 = t2 - t1 * (t1 / nd);
            set[1 + tid] = (rf < r1 ? (double)ring[rf * NC + tid] : 0.0) + t1 / nd;
            set[1 + NC + tid] = m2 > 0.0 ? m2 : 0.0;
        } else {
            set[1 + tid] = 0.0;
            set[1 + NC + tid] = 0.0;
        }
        if (tid == 0) set[0] = (double)cnt;
    }
}

// One workgroup, thread j = column j.  The k sets are combined in index order, (count, mean, M2) by Chan's update
//     n = na + nb,  d = mb - ma,  m = ma + d (nb / n),  M2 = M2a + M2b + d^2 (na nb / n),
// skipping empty sets; the result is folded into S the same way (S's M2 = var * count), and m / r of the table are rewritten.
// From the initial S (count 0, mean 0, var 1) the first merge leaves exactly the batch's mean and variance.
__global__ __launch_bounds__(128) void obs_norm_merge_kernel(double* __restrict__ stats, float* __restrict__ table,
                                                             const double* __restrict__ sets, long k, float clip)
{
    const int j = threadIdx.x;
    const double c = stats[0];
    __syncthreads();                        // every thread has read the count before thread 0 rewrites it
    if (j >= NC) return;
    double na = 0.0, ma = 0.0, qa = 0.0;
    for (long s = 0; s < k; ++s) {
        const double* set = sets + s * OBS_NORM_SET;
        const double nb = set[0];
        if (!(nb > 0.0)) continue;
        const double n = na + nb, d = set[1 + j] - ma;
        ma += d * (nb / n);
        qa += set[1 + NC + j] + d * d * (na * nb / n);
        na = n;
    }
    if (na > 0.0) {
        const double n = c + na, mu = stats[1 + j], d = ma - mu;
        const double q = stats[1 + NC + j] * c + qa + d * d * (c * na / n);
        const double mean = mu + d * (na / n), var = q / n;
        stats[1 + j] = mean;
        stats[1 + NC + j] = var;
        if (j == 0) stats[0] = n;
        table[j] = (float)mean;
        table[NC + j] = (float)(1.0 / sqrt(var + 1e-5));
    }
    if (j == 0) table[2 * NC] = clip;
}

}  // namespace

extern "C" hipError_t flyhip_launch_obs_norm_pass(const float* ring, int64_t rows, int64_t count_from, const float* table,
                                                  float* out, double* sets, void* stream)
{
    return launch_kernel<obs_norm_pass_kernel>(FLY_OBS_NORM_SETS, PASS_THREADS, 0, stream, ring, (long)rows, (long)count_from, table,
                                               out, sets);
}

extern "C" hipError_t flyhip_launch_obs_norm_merge(double* stats, float* table, const double* sets, int64_t k, float clip,
                                                   void* stream)
{
    return launch_kernel<obs_norm_merge_kernel>(1, 128, 0, stream, stats, table, sets, (long)k, clip);
}
