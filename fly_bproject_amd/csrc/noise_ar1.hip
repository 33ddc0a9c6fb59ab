// noise_ar1.hip — temporally correlated exploration noise (PPO --action_noise ar1): an AR(1) filter with
// unit stationary variance along the time axis of the rollout's noise buffer, launched right behind the white draw and in front
// of the unchanged rollout kernels, which read the buffer by pointer.
//
//   per column c of eps [T][C] (C = 18 N), in place, include/flyhip.h states it and tests/noise_ar1_ref.py restates it in numpy:
//     y[-1] = carry[c];   y[t] = fadd(fmul(rho, y[t-1]), fmul(s, x[t]));   carry[c] = y[T-1]
//   with s = (float) sqrt(1 - rho^2) formed in double by the launcher.  Separately rounded fp32 ops (no fma).
//
//   noise_ar1_kernel<W, U>     lane = W adjacent columns (W floats = one 16-, 8- or 4-byte access), t walks forward, the carried
//                              value lives in registers.  A step's load does not depend on the carried value: the kernel is a
//                              pure HBM stream, so the loads of the NEXT block of U steps are requested before the current
//                              block is filtered and stored (two register buffers used in turn), and a wave always has a block
//                              of loads in flight while it waits.  One wave per workgroup, so the columns spread over the CUs.
//                              The launcher takes the widest W the shape and the two base addresses allow; every W computes
//                              the same bits, and at 8192 envs all three run at the same rate (measured: DESIGN.md 3.2b).
//
// Deterministic: no atomics, every word of eps and carry has one writer, and a lane reads only the words it writes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "launch.h"

namespace {

constexpr int AR1_BLOCK = 64;               // one wave per workgroup, as the GAE kernels
constexpr int AR1_U = 8;                    // steps per block of loads (two blocks live: 2 x 8 x W registers)

// a lane's W columns as one native vector: one load / store instruction of 4 W bytes each
typedef float ar1_f2 __attribute__((ext_vector_type(2)));
typedef float ar1_f4 __attribute__((ext_vector_type(4)));
template <int W> struct ar1_vec;
template <> struct ar1_vec<1> { using type = float; };
template <> struct ar1_vec<2> { using type = ar1_f2; };
template <> struct ar1_vec<4> { using type = ar1_f4; };

// one step of the recurrence, per lane width: whole vectors in and out, so a 16-byte lane stores 16 bytes at once
__device__ __forceinline__ float ar1_step(float y, float x, float rho, float s)
{
    return __fadd_rn(__fmul_rn(rho, y), __fmul_rn(s, x));
}
__device__ __forceinline__ ar1_f2 ar1_step(ar1_f2 y, ar1_f2 x, float rho, float s)
{
    return ar1_f2{ar1_step(y.x, x.x, rho, s), ar1_step(y.y, x.y, rho, s)};
}
__device__ __forceinline__ ar1_f4 ar1_step(ar1_f4 y, ar1_f4 x, float rho, float s)
{
    return ar1_f4{ar1_step(y.x, x.x, rho, s), ar1_step(y.y, x.y, rho, s), ar1_step(y.z, x.z, rho, s), ar1_step(y.w, x.w, rho, s)};
}

// eps and carry are not __restrict__: eps is filtered in place.  C is a multiple of W and both bases are W-float aligned.
template <int W, int U>
__global__ __launch_bounds__(AR1_BLOCK) void noise_ar1_kernel(float* eps, float* carry, long T, long C, float rho, float s)
{
    using V = typename ar1_vec<W>::type;
    const long c = ((long)blockIdx.x * AR1_BLOCK + threadIdx.x) * W;
    if (c >= C) return;
    V* col = reinterpret_cast<V*>(eps + c);                 // row t of this lane: col[t * pitch]
    const long pitch = C / W;
    V y = *reinterpret_cast<const V*>(carry + c);
    const long blocks = T / U;
    V a[U], b[U];                                   // two blocks of steps, filled and drained in turn (no copies)
    auto load = [&](V (&buf)[U], long blk) {
#pragma unroll
        for (int u = 0; u < U; ++u) buf[u] = col[(blk * U + u) * pitch];
    };
    auto filter = [&](const V (&buf)[U], long blk) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            y = ar1_step(y, buf[u], rho, s);
            col[(blk * U + u) * pitch] = y;
        }
    };
    if (blocks > 0) load(a, 0);
    long blk = 0;
    for (; blk + 2 <= blocks; blk += 2) {                   // each block's loads are requested before the previous block's stores
        load(b, blk + 1);
        filter(a, blk);
        if (blk + 2 < blocks) load(a, blk + 2);
        filter(b, blk + 1);
    }
    if (blk < blocks) filter(a, blk);                       // an odd count: the last block is already in `a`
    for (long t = blocks * U; t < T; ++t) {             // the ragged end: fewer than U steps
        y = ar1_step(y, col[t * pitch], rho, s);
        col[t * pitch] = y;
    }
    *reinterpret_cast<V*>(carry + c) = y;
}

template <int W>
hipError_t launch_ar1(float* eps, float* carry, int64_t T, int64_t C, float rho, float s, void* stream)
{
    const long lanes = (long)(C / W);
    const long grid = (lanes + AR1_BLOCK - 1) / AR1_BLOCK;
    return launch_kernel<noise_ar1_kernel<W, AR1_U>>(dim3((unsigned)grid), AR1_BLOCK, 0, stream, eps, carry, (long)T, (long)C, rho, s);
}

}  // namespace

// The arguments have been checked (flyhip_abi.hip): eps and carry not null, T, C >= 1, 0 < rho < 1.
extern "C" hipError_t flyhip_launch_noise_ar1(float* eps, float* carry, int64_t T, int64_t C, float rho, void* stream)
{
    const float s = (float)sqrt(1.0 - (double)rho * (double)rho);
    // a row starts C floats after the previous one: 16-byte lanes need C % 4 == 0 besides the two bases, 8-byte lanes C % 2 == 0
    const uintptr_t al = reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(carry);
    if (C % 4 == 0 && (al & 15) == 0) return launch_ar1<4>(eps, carry, T, C, rho, s, stream);
    if (C % 2 == 0 && (al & 7) == 0) return launch_ar1<2>(eps, carry, T, C, rho, s, stream);
    return launch_ar1<1>(eps, carry, T, C, rho, s, stream);
}
