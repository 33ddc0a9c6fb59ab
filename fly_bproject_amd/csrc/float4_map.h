// float4_map.h — out[i] = f(in[i]) over n floats, for the elementwise kernels (value_norm_apply_kernel, reward_scale_kernel).
//
// Grid-stride over FLOAT4_MAP_THREADS-thread workgroups: 16-byte accesses where both buffers allow it, a scalar tail; element by
// element the same call of f either way.  Every element is read before it is written, by the same thread, so `out` may be `in`
// -- which is why the pointers here are not __restrict__; a kernel whose buffers never overlap says so on its own parameters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int FLOAT4_MAP_THREADS = 256;

template <class F>
__device__ __forceinline__ void float4_map(const float* in, long n, float* out, F f)
{
    const long stride = (long)gridDim.x * FLOAT4_MAP_THREADS, first = (long)blockIdx.x * FLOAT4_MAP_THREADS + threadIdx.x;
    const bool aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long n4 = aligned ? n >> 2 : 0;
    const float4* in4 = reinterpret_cast<const float4*>(in);
    float4* out4 = reinterpret_cast<float4*>(out);
    for (long i = first; i < n4; i += stride) {
        const float4 x = in4[i];
        out4[i] = make_float4(f(x.x), f(x.y), f(x.z), f(x.w));
    }
    for (long i = 4 * n4 + first; i < n; i += stride) out[i] = f(in[i]);
}

// the grid of such a kernel: one float4 per thread, at most 1024 workgroups
inline unsigned float4_map_grid(int64_t n)
{
    const long per = 4L * FLOAT4_MAP_THREADS;
    const long grid = (n + per - 1) / per;
    return (unsigned)(grid > 1024 ? 1024 : grid);
}
