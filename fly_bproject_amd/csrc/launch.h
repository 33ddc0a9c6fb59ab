// launch.h — the host side shared by the launchers: private to csrc/ (not installed, not part of include/flyhip.h).
//
//   1. the ONE declaration of every internal entry point flyhip_abi.hip calls in another translation unit.  flyhip_abi.hip and
//      every file that defines one of them include this header, so a definition that drifts from its declaration is a compile
//      error ("conflicting types for ..."), not a call that links and passes garbage.
//   2. with_bools / with_int: runtime flags -> template arguments, and launch_kernel: the one place a kernel is launched with
//      dynamic LDS (hipFuncSetAttribute lives here and nowhere else).  A new variant flag is one more argument of a with_bools call.
//   3. the helpers the launchers shared by copy: the cached CU count, the fused kernels' grid, the decoding of debug_dump, the
//      slab table of the fixed-order reductions.
// Host code only: nothing here is device code, and the kernels' types (GradWTable, FusedDump: per translation unit, in anonymous
// namespaces) reach the helpers as template parameters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "flyhip.h"

// the phase bits of the env step (fly_body.inc's template argument PH; flyhip_abi.hip's buffer checks)
enum : int { PH_SCALE = 1, PH_RESET = 2, PH_INTEGRATE = 4, PH_OBS = 8, PH_REWARD = 16, PH_PROGRESS = 32 };

extern "C" {

// fly_env.hip, domain_rand.hip, fly_render.hip
hipError_t flyhip_launch_env(int phases, const FlyConfig* dcfg, int n, const float* actions, const FlyBuffers* b, void* stream,
                             int dr);
hipError_t flyhip_launch_dr_register(const FlyConfig* dcfg, int n, void* stream);
hipError_t flyhip_launch_render(const FlyConfig* dcfg, const float* poses, int frames, const FlyRenderConfig* rc,
                                uint32_t* rgba_out, uint8_t* id_out, void* stream);

// ppo_kernels.hip
hipError_t flyhip_launch_sample_logprob(const float* mu, const float* var, const float* eps, float* act_out, float* logp_out,
                                        int64_t n, void* stream);
hipError_t flyhip_launch_td_gae(const float* reward, const float* v, const float* v_next, const float* done, float gamma,
                                float lambda, int64_t T, int64_t N, float* target_out, float* adv_out, int mode, void* stream);
hipError_t flyhip_launch_bookkeeping(const float* reward, int64_t n, float* score_acc, float score_scale, float* action_var,
                                     int nvar, float var_decay, float var_min, void* stream);
hipError_t flyhip_launch_rollout_bookkeeping(const float* reward, int64_t rows, int64_t n, float* terms, float* score_acc,
                                             float score_scale, float* action_var, int nvar, float var_decay, float var_min,
                                             int* rows_applied, void* stream);
hipError_t flyhip_launch_adv_stats(const float* adv, int64_t n, float* stats, void* stream);
hipError_t flyhip_launch_adv_apply(float* adv, int64_t n, const float* totals, float count, float eps, void* stream);

// obs_norm.hip, value_norm.hip
hipError_t flyhip_launch_obs_norm_pass(const float* ring, int64_t rows, int64_t count_from, const float* table, float* out,
                                       double* sets, void* stream);
hipError_t flyhip_launch_obs_norm_merge(double* stats, float* table, const double* sets, int64_t k, float clip, void* stream);
hipError_t flyhip_launch_td_gae_vnorm(const float* reward, const float* v, const float* v_next, const float* done,
                                      const float* table, float gamma, float lambda, int64_t T, int64_t N, float* target_out,
                                      float* adv_out, double* sets, int mode, void* stream);
hipError_t flyhip_launch_value_norm_merge(const double* stats_in, const double* sets, int64_t k, double* stats_out,
                                          float* table_out, void* stream);
hipError_t flyhip_launch_value_norm_apply(const float* target, int64_t n, const float* table, float* out, void* stream);

// value_target.hip
hipError_t flyhip_launch_lambda_targets(const float* adv, const float* v, const float* table, int64_t n, float* target_out,
                                        double* sets, void* stream);

// gae_episodic.hip
hipError_t flyhip_launch_td_gae_episodic(const float* reward, const float* v, const float* v_next, const int64_t* reset,
                                         const int64_t* progress, const int64_t* ended_prev, int64_t max_episode_length,
                                         float gamma, float lambda, int64_t T, int64_t N, float* target_out, float* adv_out,
                                         int mode, void* stream);
hipError_t flyhip_launch_td_gae_episodic_vnorm(const float* reward, const float* v, const float* v_next, const int64_t* reset,
                                               const int64_t* progress, const int64_t* ended_prev, int64_t max_episode_length,
                                               const float* table, float gamma, float lambda, int64_t T, int64_t N,
                                               float* target_out, float* adv_out, double* sets, int mode, void* stream);

// episode_stats.hip
hipError_t flyhip_launch_episode_stats(const float* reward, const int64_t* reset, const int64_t* progress,
                                       int64_t max_episode_length, int64_t T, int64_t N, double* carry_ret, int64_t* carry_len,
                                       double* sets, int mode, void* stream);
hipError_t flyhip_launch_episode_stats_merge(const double* sets, int64_t nsets, double* window, double* total, void* stream);

// reward_norm.hip
hipError_t flyhip_launch_reward_returns(const float* reward, const int64_t* reset, float gamma, int64_t T, int64_t N,
                                        const double* carry_in, double* carry_out, double* sets, int mode, void* stream);
hipError_t flyhip_launch_reward_scale(const float* reward, int64_t n, const float* table, float clip, float* out, void* stream);

// update_stats.hip
hipError_t flyhip_launch_update_stats(const float* mu, const float* action, const float* old_logp, const float* adv,
                                      const float* v, const float* target, const float* var, float clip, int64_t R, double* sets,
                                      void* stream);
hipError_t flyhip_launch_update_stats_merge(const double* sets, int64_t nsets, double* last, double* window, double* total,
                                            void* stream);

// minibatch_gather.hip
hipError_t flyhip_launch_minibatch_gather(const float* obs, const float* act, const float* logp, const float* adv,
                                          const float* target, int64_t R, uint32_t seed, uint32_t epoch_key, int64_t first,
                                          int64_t n, float* obs_out, float* act_out, float* logp_out, float* adv_out,
                                          float* target_out, int32_t* index_out, void* stream);

// noise_ar1.hip
hipError_t flyhip_launch_noise_ar1(float* eps, float* carry, int64_t T, int64_t C, float rho, void* stream);

// mlp_mfma.hip
hipError_t flyhip_launch_mlp_forward(const float* P, const float* PF, const float* x, int64_t n, float* mu_out, float* v_out,
                                     float* out_save, float* h1_save, float* h2_save, float* h3_save, const uint16_t* PB,
                                     void* stream);
hipError_t flyhip_launch_mlp_forward_sample(const float* P, const float* PF, const float* x, int64_t n, const float* eps,
                                            const float* var, int var_steps, float var_decay, float var_min, float* act_out,
                                            float* logp_out, float* mu_out, float* v_out, const uint16_t* PB, const int* var_base,
                                            void* stream);
hipError_t flyhip_launch_mlp_backward_dx(const float* PT, const float* out_saved, const float* h1, const float* h2,
                                         const float* h3, const float* action, const float* old_logp, const float* adv,
                                         const float* target, const float* var, int64_t n, float inv_batch, float clip, float* dz4,
                                         float* dz3, float* dz2, float* dz1, float* loss_part, const uint16_t* PTB, void* stream);
hipError_t flyhip_launch_mlp_fwd_bwd(const float* P, const float* PF, const float* PT, const float* x, int64_t n, float* out_save,
                                     float* h1_save, float* h2_save, float* h3_save, const float* action, const float* old_logp,
                                     const float* adv, const float* target, const float* var, float inv_batch, float clip,
                                     float* dz4, float* dz3, float* dz2, float* dz1, float* loss_part, int* flags, int epoch,
                                     int* err, const uint16_t* PB, const uint16_t* PTB, int coherent, void* stream);
hipError_t flyhip_launch_rollout_step(const FlyConfig* dcfg, const FlyBuffers* b, const float* P, const float* PF, const float* x,
                                      int64_t n, const float* eps, const float* var, int var_steps, float var_decay, float var_min,
                                      float* act, float* logp, float* v_out, const uint16_t* PB, const int* var_base, void* stream,
                                      int norm, int dr);
hipError_t flyhip_launch_rollout_all(const FlyConfig* dcfg, const FlyBuffers* b, const float* P, const float* PF, float* obs_ring,
                                     int64_t n, const float* eps_all, const float* var, float var_decay, float var_min,
                                     float* act_all, float* logp_all, float* v_ring, float* reward_all, int T,
                                     const int* rows_applied, const uint16_t* PB, int64_t* reset_rows, int64_t* progress_rows,
                                     void* stream, unsigned long long* stamps, float* poses, int norm, int dr);
int64_t flyhip_mlp_grad_workspace_floats(void);
hipError_t flyhip_launch_mlp_grad_w(const float* x, const float* h1, const float* h2, const float* h3, const float* dz1,
                                    const float* dz2, const float* dz3, const float* dz4, int64_t n, float* workspace,
                                    float* grad_out, const float* norm_mask, float* norm_ws, int* norm_step, const int* err,
                                    int gemm_b3, void* stream);
int flyhip_mlp_reduce_blocks(void);
int flyhip_debug_get_fused_grid(void);      // the test hook that shrinks the grid of both fused kernels (flyhip_debug_set_fused_grid)
int64_t flyhip_mlp_fused_workspace_floats(void);
hipError_t flyhip_launch_mlp_fused_grad(const float* P, const uint16_t* PB, const uint16_t* PTB, const float* x, int64_t n,
                                        const float* action, const float* old_logp, const float* adv, const float* target,
                                        const float* var, float inv_batch, float clip, float* workspace, float* grad_out,
                                        const float* norm_mask, float* norm_ws, int* norm_step, float* loss_part,
                                        float* const* dump, void* stream);
hipError_t flyhip_launch_mlp_adam(float* P, float* PF, float* PT, const int* idx_f, const int* idx_t, const float* G,
                                  const float* mask, float* m, float* v, int* step, float lr, float beta1, float beta2, float eps,
                                  float max_norm, float grad_scale, float* norm_ws, int norm_ready, uint16_t* PB, uint16_t* PTB,
                                  const int* idx_fb, const int* idx_tb, int* step_out, const int* grad_invalid, uint16_t* PH,
                                  uint16_t* PTH, float* h2_scales, int h2_period, void* stream);
hipError_t flyhip_launch_mlp_h2_rescale(const float* P, const int* idx_fb, const int* idx_tb, uint16_t* PH, uint16_t* PTH,
                                        float* h2_scales, void* stream);

// mlp_fused_h2.hip
int64_t flyhip_mlp_fused_h2_workspace_floats(void);
hipError_t flyhip_launch_mlp_fused_grad_h2(const float* P, const uint16_t* PH, const uint16_t* PTH, float* fsc, int* ovf, int freeze,
                                           const float* x, int64_t n, const float* action, const float* old_logp, const float* adv,
                                           const float* target, const float* var, float inv_batch, float clip, float* workspace,
                                           float* grad_out, const float* norm_mask, float* norm_ws, int* norm_step,
                                           float* loss_part, float* const* dump, void* stream);

// dqn_kernels.hip, dqn_mfma.hip
hipError_t flyhip_launch_dqn_eps_greedy(const float* q, const float* coin_u, const float* rand_u, float epsilon, int A,
                                        float* act_out, int64_t n, void* stream);
hipError_t flyhip_launch_dqn_huber_td(const float* q_table, const float* act, const float* reward, const float* q_next,
                                      const float* done, float discount, int A, int64_t B, float* dq, float* loss_part,
                                      void* stream);
hipError_t flyhip_launch_dqn_forward(const float* P, const float* PF, const float* x, int64_t n, float* q_out, void* stream);
hipError_t flyhip_launch_dqn_act(const float* P, const float* PF, const float* x, int64_t n, const float* coin_u,
                                 const float* rand_u, float epsilon, float* act_out, float* q_out, void* stream);
hipError_t flyhip_launch_dqn_td(const float* P, const float* PF, const float* PT, const float* P_tgt, const float* PF_tgt,
                                const float* obs, const float* next_obs, const float* act, const float* reward, const float* done,
                                int64_t n, float discount, float inv_B, float* h1, float* h2, float* dz3, float* dz2, float* dz1,
                                float* loss_part, void* stream);
int64_t flyhip_dqn_grad_workspace_floats(void);
hipError_t flyhip_launch_dqn_grad_w(const float* x, const float* h1, const float* h2, const float* dz1, const float* dz2,
                                    const float* dz3, int64_t n, float* workspace, float* grad, int accumulate, void* stream);
hipError_t flyhip_launch_dqn_adam(float* P, float* PF, float* PT, float* P_tgt, float* PF_tgt, const int* idx_f, const int* idx_t,
                                  const float* G, const float* mask, float* m, float* v, int* step, float lr, float beta1,
                                  float beta2, float eps, float tau, uint16_t* QB, uint16_t* QTB, uint16_t* QB_tgt,
                                  const int* idx_fb, const int* idx_tb, const int* grad_invalid, void* stream);
int64_t flyhip_dqn_fused_workspace_floats(void);
int64_t flyhip_dqn_fused_image_halves(int64_t rows);
hipError_t flyhip_launch_dqn_fused_update(const float* P, const uint16_t* QB, const uint16_t* QTB, const float* P_tgt,
                                          const uint16_t* QB_tgt, const void* chunks, int S, int64_t n, float discount, float inv_B,
                                          uint16_t* images, float* workspace, float* grad, float* loss_part, int rows_aligned16,
                                          void* stream);
int64_t flyhip_dqn_fused_h2_workspace_floats(void);
int64_t flyhip_dqn_fused_h2_image_halves(int64_t rows);
hipError_t flyhip_launch_dqn_fused_update_h2(const float* P, uint16_t* QH, uint16_t* QTH, const float* P_tgt, uint16_t* QH_tgt,
                                             const int* idx_fb, const int* idx_tb, float* fsc, int* ovf, const void* chunks, int S,
                                             int64_t n, float discount, float inv_B, uint16_t* images, float* workspace,
                                             float* grad, float* loss_part, int rows_aligned16, int flags, void* stream);

// dp_p2p.hip
hipError_t flyhip_p2p_alloc(int64_t n_floats, void** out);
hipError_t flyhip_launch_p2p_allreduce(float* G, int64_t n, void* const* bases, int rank, int world, uint32_t epoch, int* err,
                                       int64_t fail_slot, void* stream);

}  // extern "C"

// ---- runtime flags -> template arguments ------------------------------------------------------------------------------------
// with_bools(f, b0, b1, ...) calls the generic lambda f with one std::true_type / std::false_type per flag, in order: inside f,
// `flag.value` is a constant expression and goes straight into a kernel's template argument list.  Only the instantiations f names
// are emitted: a form that exists for some flag combinations only (the stamped kernels) is a branch of its own around the call.
template <class F>
hipError_t with_bools(F&& f) { return f(); }
template <class F, class... R>
hipError_t with_bools(F&& f, bool b, R... r)
{
    return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, r...)
             : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, r...);
}
// with_int<I0, I1, ...>(v, f): f(std::integral_constant<int, v>{}) when v is one of the listed values, hipErrorInvalidValue otherwise
template <int I>
using int_c = std::integral_constant<int, I>;
template <int... Is, class F>
hipError_t with_int(int v, F&& f)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Is ? (e = f(int_c<Is>{}), true) : false) || ...);
    return e;
}

// Launches kernel K.  A launch that asks for dynamic LDS first raises the kernel's limit to what it asks for -- on every launch,
// not cached: the attribute belongs to the CURRENT device, and a process may drive more than one.
template <auto K, class... A>
hipError_t launch_kernel(dim3 grid, dim3 block, size_t lds_bytes, void* stream, A... a)
{
    if (lds_bytes) {
        hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(K, grid, block, lds_bytes, (hipStream_t)stream, a...);
    return hipGetLastError();
}

// ---- shared helpers ----------------------------------------------------------------------------------------------------------
// CU count of the current device, read once per DEVICE (a process may drive more than one); 256 where it cannot be read.
// (inline: one cache for the library; hidden: it is not an export)
__attribute__((visibility("hidden"))) inline int device_cus()
{
    static int cus[16] = {0};
    int dev = 0;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    if (!cus[dev]) cus[dev] = hipGetDeviceProperties(&pr, dev) == hipSuccess ? pr.multiProcessorCount : 256;
    return cus[dev];
}

// grid of the persistent fused-gradient kernels (bf16x3 and fp16x2): one workgroup per CU, fewer under the test hook or when
// there are fewer tiles of `tile_rows` rows
__attribute__((visibility("hidden"))) inline int fused_grid(int64_t n, int tile_rows)
{
    int g = device_cus();
    const int ovr = flyhip_debug_get_fused_grid();
    if (ovr > 0 && ovr < g) g = ovr;
    const long tiles = (n + tile_rows - 1) / tile_rows;
    return (int)(tiles < g ? tiles : g);
}

// debug_dump of the fused-gradient entry points -> the kernel's DUMP mode and its FusedDump: NULL = 0 (none); 8 pointers = 1, the
// chain dump (tests); ONE pointer followed by NULL = 2, a stamp buffer (tools/stamp_fused.py)
template <class Dump>
int decode_dump(float* const* dump, Dump& d)
{
    d = {};
    const int mode = dump == nullptr ? 0 : (dump[1] == nullptr ? 2 : 1);
    if (mode == 1) { d.out = dump[0]; d.h1 = dump[1]; d.h2 = dump[2]; d.h3 = dump[3]; d.dz4 = dump[4]; d.dz3 = dump[5]; d.dz2 = dump[6]; d.dz1 = dump[7]; }
    if (mode == 2) d.out = dump[0];
    return mode;
}

// The GradWTable of a fused kernel's slabs for the fixed-order reduction: layer l has `grid` slabs (one per workgroup) of
// N[l] * KP[l] + N[l] floats at part[l]; chunked: padded to whole 1 KiB chunks and interleaved chunk by chunk (fs_slab).
template <class Table, int L>
void fill_slab_table(Table& T, const int (&N)[L], const int (&KP)[L], float* const (&part)[L], int grid, int chunked)
{
    for (int l = 0; l < L; ++l) {
        T.l[l].dz = nullptr; T.l[l].a = nullptr; T.l[l].partial = part[l];
        T.l[l].N = N[l]; T.l[l].Ka = KP[l]; T.l[l].KP = KP[l]; T.l[l].wgs = grid; T.l[l].first_block = 0; T.l[l].accumulate = 0;
        T.l[l].chunked = chunked;
    }
    for (int l = L; l < 4; ++l) T.l[l] = T.l[L - 1];
}
