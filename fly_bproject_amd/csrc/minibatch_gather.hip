// minibatch_gather.hip — shuffled PPO minibatches (PPO --minibatch shuffled): a keyed permutation of the
// rollout's rows, evaluated in the kernel, and the gather of the chosen rows into a contiguous staging minibatch for the
// optimizer-step kernels, which want contiguous [rows][73] inputs and are left as they are.
//
//   pi(i), a bijection of [0, R): a balanced 6-round Feistel network on [0, 2^b), b = max(2, bit_length(R - 1)) rounded up to
//   even, h = b / 2, with cycle walking (include/flyhip.h states it; tests/minibatch_ref.py restates it in numpy).  A pure
//   function of (seed, epoch_key, i): no index tensor in memory, and a redone optimizer step sees its minibatch again bit for bit.
//
//   minibatch_gather_kernel    one wave (= one workgroup) owns 32 output rows.  Lane l < 32 evaluates pi once, for row k0 + l,
//                              carries that row's three scalars and leaves the index in LDS.  The wave then walks its rows'
//                              32 x 73 observation floats and 32 x 18 action floats as FLAT ranges, 16 bytes per lane: the output
//                              offset of a wave's first row is a multiple of 32 x 292 B and 32 x 72 B, both multiples of 16, so
//                              every store is an aligned global_store_dwordx4 and the wave's stores cover its range without a
//                              gap.  Source rows are only 4-byte aligned: observation words are loaded as dwords (16-byte loads
//                              of the covering aligned span, realigned through LDS, were slower: DESIGN.md 8b).
//                              Every load of the wave -- scalars, observation words, action words -- is issued before its
//                              first store (addresses of elements past a ragged end are clamped, not branched around), so a
//                              wave pays one memory round trip after the index is known, not one per range or per 16 bytes.
//
// Words are moved as uint32: a bitwise copy, NaN payloads, infinities and -0 included.  Deterministic: no atomics, every output
// word has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "domain_rand.h"
#include "launch.h"

namespace {

constexpr int ROWS = 32;                    // rows a wave owns (measured against 64: DESIGN.md 3.3e)
constexpr int OBS = 73, ACT = 18;           // floats of an observation / action row
constexpr int OBS_IT = (ROWS * OBS / 4 + 63) / 64;      // 16-byte pieces of a wave's observation range, per lane: 10
constexpr int ACT_IT = (ROWS * ACT / 4 + 63) / 64;      // 3
static_assert(ROWS <= 64 && ROWS * OBS % 4 == 0 && ROWS * ACT % 4 == 0, "a full wave's ranges are whole 16-byte pieces");

__device__ __forceinline__ uint32_t perm_index(uint32_t i, uint32_t R, uint32_t key, int h)
{
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = i;
    do {                                    // cycle walking: the cycle through i < R returns below R
        uint32_t L = x >> h, Q = x & mask;
#pragma unroll
        for (uint32_t r = 0; r < 6; ++r) {
            const uint32_t f = dr_lowbias32(Q + key + 0x9E3779B9u * (r + 1u)) & mask;
            const uint32_t t = L ^ f;
            L = Q;
            Q = t;
        }
        x = (L << h) | Q;
    } while (x >= R);
    return x;
}

__global__ __launch_bounds__(64) void minibatch_gather_kernel(const uint32_t* __restrict__ obs, const uint32_t* __restrict__ act,
                                                              const uint32_t* __restrict__ logp, const uint32_t* __restrict__ adv,
                                                              const uint32_t* __restrict__ target, uint32_t R, uint32_t seed,
                                                              uint32_t epoch_key, int h, long first, long n,
                                                              uint32_t* __restrict__ obs_out, uint32_t* __restrict__ act_out,
                                                              uint32_t* __restrict__ logp_out, uint32_t* __restrict__ adv_out,
                                                              uint32_t* __restrict__ target_out, int32_t* __restrict__ index_out,
                                                              int act_al8)
{
    __shared__ uint32_t s_src[64];
    const int lane = threadIdx.x;
    const long k0 = (long)blockIdx.x * ROWS;
    const int m = n - k0 < ROWS ? (int)(n - k0) : ROWS;     // rows of this wave: 1..ROWS
    uint32_t src = 0;
    if (lane < m) {                                         // a lane without a row must not walk: its cycle may never come below R
        const uint32_t key = dr_lowbias32(seed ^ dr_lowbias32(epoch_key));
        src = perm_index((uint32_t)(first + k0 + lane), R, key, h);
    }
    s_src[lane] = src;
    __syncthreads();

    // ---- loads.  The scalars: one lane per row (lanes without a row read row 0 of the source and store nothing)
    const uint32_t s_logp = logp[src], s_adv = adv[src], s_target = target[src];
    // observations: the wave's m x 73 words as a flat range
    const int total = m * OBS;
    uint32_t v[OBS_IT][4];
#pragma unroll
    for (int it = 0; it < OBS_IT; ++it) {
        const int f = 4 * (lane + 64 * it);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int fe = f + e < total ? f + e : total - 1;       // past the end: a valid address, the value is not stored
            const int row = fe / OBS, col = fe - OBS * row;
            v[it][e] = obs[(size_t)s_src[row] * OBS + col];
        }
    }
    // actions: m x 18 words, in pairs (a pair never crosses a row: 18 is even)
    const int pairs = m * (ACT / 2);
    uint2 va[ACT_IT][2];
#pragma unroll
    for (int it = 0; it < ACT_IT; ++it) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int p = 2 * (lane + 64 * it) + e;
            const int pe = p < pairs ? p : pairs - 1;
            const int row = pe / (ACT / 2), col = 2 * (pe - (ACT / 2) * row);
            const uint32_t* s = act + (size_t)s_src[row] * ACT + col;
            if (act_al8) {
                va[it][e] = *reinterpret_cast<const uint2*>(s);
            } else {
                va[it][e].x = s[0];
                va[it][e].y = s[1];
            }
        }
    }

    // ---- stores
    uint32_t* oo = obs_out + k0 * OBS;
#pragma unroll
    for (int it = 0; it < OBS_IT; ++it) {
        const int f = 4 * (lane + 64 * it);
        if (f + 3 < total) {
            *reinterpret_cast<uint4*>(oo + f) = make_uint4(v[it][0], v[it][1], v[it][2], v[it][3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (f + e < total) oo[f + e] = v[it][e];
        }
    }
    uint32_t* ao = act_out + k0 * ACT;
#pragma unroll
    for (int it = 0; it < ACT_IT; ++it) {
        const int p = 2 * (lane + 64 * it);
        if (p + 1 < pairs)
            *reinterpret_cast<uint4*>(ao + 2 * p) = make_uint4(va[it][0].x, va[it][0].y, va[it][1].x, va[it][1].y);
        else if (p < pairs)
            *reinterpret_cast<uint2*>(ao + 2 * p) = va[it][0];
    }
    if (lane < m) {
        logp_out[k0 + lane] = s_logp;
        adv_out[k0 + lane] = s_adv;
        target_out[k0 + lane] = s_target;
        if (index_out) index_out[k0 + lane] = (int32_t)src;
    }
}

}  // namespace

// The arguments have been checked (flyhip_abi.hip): 1 <= R < 2^31, 0 <= first, 1 <= n, first + n <= R, obs_out and act_out
// 16-byte aligned.
extern "C" hipError_t flyhip_launch_minibatch_gather(const float* obs, const float* act, const float* logp, const float* adv,
                                                     const float* target, int64_t R, uint32_t seed, uint32_t epoch_key,
                                                     int64_t first, int64_t n, float* obs_out, float* act_out, float* logp_out,
                                                     float* adv_out, float* target_out, int32_t* index_out, void* stream)
{
    int b = 0;
    for (uint64_t x = (uint64_t)R - 1; x; x >>= 1) ++b;     // bit_length(R - 1)
    if (b < 2) b = 2;
    b += b & 1;
    auto w = [](const float* p) { return reinterpret_cast<const uint32_t*>(p); };
    auto o = [](float* p) { return reinterpret_cast<uint32_t*>(p); };
    const long grid = (long)((n + ROWS - 1) / ROWS);
    return launch_kernel<minibatch_gather_kernel>(
        dim3((unsigned)grid), 64, 0, stream, w(obs), w(act), w(logp), w(adv), w(target), (uint32_t)R, seed, epoch_key, b / 2,
        (long)first, (long)n, o(obs_out), o(act_out), o(logp_out), o(adv_out), o(target_out), index_out,
        (int)((reinterpret_cast<uintptr_t>(act) & 7) == 0));
}
