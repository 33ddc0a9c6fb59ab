// mlp_fused_h2.hip — translation unit of the fused optimizer-step gradient in the fp16x2 arithmetic (mlp_fused_h2.inc): the
// persistent kernel, its slab reduction with the scale bookkeeping, and their launcher.  The bf16x3 kernel it stands beside lives
// in mlp_mfma.hip (mlp_fused_step.inc), whose layout constants, slab addressing and LDS swizzle this unit shares.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include "flyhip.h"
#include "mlp_layout.h"
#include "h2_warm.h"
#include "obs_norm.h"
#include "launch.h"

namespace {

#include "loss_head.inc"
#include "mlp_gemm.inc"
#include "fs_stamp.inc"
#include "mlp_fused_step.inc"       // constants and helpers only: mlp_fused_step_kernel is instantiated in mlp_mfma.hip
#include "mlp_fused_h2.inc"

}  // namespace

static int64_t h2_slab_floats() { return fs_pad256(FS_STRIDE1) + fs_pad256(FS_STRIDE2) + fs_pad256(FS_STRIDE3) + fs_pad256(FS_STRIDE4); }

// one partial slab per workgroup (chunked layout) + eight class maxima per workgroup behind them
// (+ 8 floats: the launch's unscale factors, left by workgroup 0 for the reduction)
extern "C" int64_t flyhip_mlp_fused_h2_workspace_floats(void) { return (int64_t)device_cus() * (h2_slab_floats() + H2_NACT_CLASSES) + 8; }

extern "C" hipError_t flyhip_launch_mlp_fused_grad_h2(const float* P, const uint16_t* PH, const uint16_t* PTH, float* fsc, int* ovf,
                                                      int freeze, const float* x, int64_t n, const float* action,
                                                      const float* old_logp, const float* adv, const float* target, const float* var,
                                                      float inv_batch, float clip, float* workspace, float* grad_out,
                                                      const float* norm_mask, float* norm_ws, int* norm_step, float* loss_part,
                                                      float* const* dump, void* stream)
{
    const int cus = device_cus();
    const long tiles = (n + BM - 1) / BM;
    if (tiles + 4096 >= (1L << 31)) return hipErrorInvalidValue;        // the kernel counts tiles in 32 bits
    const int grid = fused_grid(n, BM);
    FusedDump d;
    float* wsmax = workspace + (int64_t)cus * h2_slab_floats();
    hipError_t e = with_int<0, 1, 2>(decode_dump(dump, d), [&](auto mode) {
        return launch_kernel<mlp_fused_step_h2_kernel<mode.value>>(grid, THREADS, H2_LDS_BYTES, stream, P, PH, PTH, (const float*)fsc, x,
                                                                   (long)n, action, old_logp, adv, target, var, inv_batch, clip, workspace,
                                                                   wsmax, loss_part, d);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mlp_grad_reduce_h2_kernel, dim3(H2_RED_BLOCKS), dim3(64 * H2_RED_WAVES), 0, (hipStream_t)stream,
                       (const float*)workspace, grid, grad_out, norm_mask, norm_ws, norm_step, (const float*)wsmax, fsc, ovf, freeze);
    return hipGetLastError();
}
