// domain_rand.hip — the registration draw of per-env physics domain randomisation (fly_set_randomization): one thread per env
// draws the env's next row from its current count (domain_rand.h) and stores it with the count advanced.  The redraws at resets
// run inside the env body (fly_body.inc, DR instantiations).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flyhip.h"
#include "domain_rand.h"
#include "launch.h"

namespace {

constexpr int DR_THREADS = 256;

__global__ __launch_bounds__(DR_THREADS) void dr_register_kernel(const FlyConfig* __restrict__ c, int n)
{
    const long e = (long)blockIdx.x * DR_THREADS + threadIdx.x;
    if (e >= n) return;
    const float* row = dr_slot(c)->table + e * FLY_DR_ROW;
    const uint32_t k = __builtin_bit_cast(uint32_t, row[6]);
    float m[FLY_DR_PARAMS];
    dr_draw(c, (uint32_t)e, k, m);
    dr_store_row(c, e, m, k + 1u);
}

}  // namespace

extern "C" hipError_t flyhip_launch_dr_register(const FlyConfig* dcfg, int n, void* stream)
{
    hipLaunchKernelGGL(dr_register_kernel, dim3((unsigned)((n + DR_THREADS - 1) / DR_THREADS)), dim3(DR_THREADS), 0,
                       (hipStream_t)stream, dcfg, n);
    return hipGetLastError();
}
