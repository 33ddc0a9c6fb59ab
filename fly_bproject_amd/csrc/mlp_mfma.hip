// mlp_mfma.hip — the actor-critic MLP (reference ppo.py:10-102) on the gfx950 matrix cores:
// translation unit of the MLP kernels (the pieces live in the .inc files it includes) and their
// launchers.
//
//   mlp_gemm.inc      tile GEMMs: straight-line runs of v_mfma_f32_32x32x2_f32 (fp32 in, fp32
//                     accumulate: the reference's fp32 numerics on the matrix pipe) over a ring of
//                     named operand fragments, and the bf16x3 variant on v_mfma_f32_32x32x16_bf16;
//                     bias + ELU epilogues working on accumulator fragments
//   mlp_forward.inc   all four layers of a 32-row tile in one workgroup: activations stay in LDS
//                     between layers, weights stream from L2 in fragment order (mlp_layout.h),
//                     layers 1/2 in two halves of 128 hidden columns, layer 4 split-K over the waves,
//                     optional fused action sampling; written once over ArithF32 / ArithB3 (there too)
//   mlp_backward.inc  PPO loss gradient + dX chain of a tile (once, over the same two), and the ONE-launch forward+backward
//                     kernel whose backward workgroups wait on per-tile flags of the forward ones
//   mlp_grad_w.inc    dW = dZ^T A over row slabs (one partial per workgroup) + fixed-order reduction
//   mlp_fused_step.inc  ONE persistent launch per minibatch: forward, loss, dX chain and dW of every tile in the workgroup
//                     that owns it (bf16x3; activations never leave the CU, dW accumulated in registers)
//   mlp_adam.inc      clip_grad_norm_ + Adam on the packed parameters
//   launch.h          host side of every launcher in this directory: the declarations of the flyhip_launch_* entry points,
//                     with_bools / with_int (runtime flags -> template arguments; a new variant flag is one more argument there)
//                     and launch_kernel
//
// The operand roles are fixed throughout: weights are the MFMA "A" operand, activations the "B"
// operand, so a lane of a 32x32 result tile owns one batch row and groups of four consecutive
// output columns.  DESIGN.md section 3.4 has the measurements this structure follows from.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include "flyhip.h"
#include "mlp_layout.h"
#include "obs_norm.h"
#include "domain_rand.h"
#include "launch.h"

namespace {

#include "loss_head.inc"
#include "mlp_gemm.inc"
#include "fs_stamp.inc"
#include "mlp_forward.inc"
#include "mlp_backward.inc"
#include "mlp_grad_w.inc"
#include "mlp_fused_step.inc"
#include "mlp_adam.inc"
#include "fly_body.inc"

// One launch per env step of the rollout (ppo.py:213-230): workgroup b runs the policy forward +
// sampling for the 32 envs of tile b (writing their action / log-prob / value rows) and then the
// fused env step of exactly those envs (fly.py:624-681) -- the env body has the same 256-thread,
// 32-env shape.  The actions go through HBM rows the workgroup itself just wrote (it waits for its
// stores and re-reads them: same CU, and nothing has read those lines since the kernel began).
// Bit for bit what mlp_forward_sample followed by fly_step leave.
template <class Arith>       // the policy's arena, or the env step's observation block where that is larger
constexpr int RS_LDS_FLOATS = Arith::FWD_FLOATS > ENVS_PER_BLOCK * FLY_NUM_OBS ? Arith::FWD_FLOATS : ENVS_PER_BLOCK * FLY_NUM_OBS;
static_assert(ENVS_PER_BLOCK == BM && BLOCK == THREADS, "one forward tile = one env block");
constexpr int NORM_LDS_FLOATS = OBS_NORM_TABLE + 1;     // the NORM instantiations' copy of the normalisation table (obs_norm.h)
static_assert(MLP_IN == OBS_NORM_COLS && OBS_NORM_TABLE <= THREADS, "one table entry per thread");

// B3: the policy body on the bf16 matrix pipe (three-term splits; PF then points at the term planes)
// NORM: the policy input is normalised under the table registered with the handle (fly_set_obs_norm, read through `c`)
// DR: the env step runs on each env's randomised constants and redraws them at its resets (fly_set_randomization, through `c`)
template <bool B3, bool NORM = false, bool DR = false>
__global__ __launch_bounds__(THREADS, B3 ? 1 : 2) void rollout_step_kernel(
    const FlyConfig* __restrict__ c, FlyBuffers b, const float* __restrict__ P, const void* __restrict__ PF,
    const float* __restrict__ x, long n, const float* __restrict__ eps, const float* __restrict__ var, int var_steps,
    float var_decay, float var_min, float* __restrict__ act, float* __restrict__ logp, float* __restrict__ v_out,
    const int* __restrict__ var_base)
{
    typedef ArithOf<B3> Arith;
    constexpr int ARENA = RS_LDS_FLOATS<Arith>;
    __shared__ __attribute__((aligned(16))) float lds[ARENA + (NORM ? NORM_LDS_FLOATS : 0)];
    float* const norm_tab = NORM ? lds + ARENA : nullptr;
    if (NORM) obs_norm_load(norm_tab, c);
    var_steps -= var_base ? *var_base : 0;                  // pending decays: frozen row index minus what is already applied
    constexpr int PH_ALL = PH_SCALE | PH_RESET | PH_INTEGRATE | PH_OBS | PH_PROGRESS | PH_REWARD;
    FlyRegs st;
    fly_load<PH_ALL, DR>(st, c, b, blockIdx.x);             // the env state's HBM round trip hides under the forward
    if (NORM) __syncthreads();                              // publishes the table
    forward_body<Arith, false, false, NORM>(lds, blockIdx.x, 1L << 40, P, PF, x, n, nullptr, v_out, nullptr, nullptr, nullptr, nullptr, eps,
                                            var, act, logp, nullptr, var_steps, var_decay, var_min, norm_tab);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);          // this thread's action stores are acknowledged by L2
    __syncthreads();
    fly_body<PH_ALL, DR>(c, FlyRead{c}, act, b, lds, blockIdx.x, st);
}

// Pose record (fly_set_pose_record): env 0's pose after step t -- root position, quaternion xyzw, the 18 joint angles in DoF
// order (FLY_POSE_FLOATS) -- out of the state `nx` the env step just left, i.e. exactly what root / dof_state hold after that
// step.  Called by workgroup 0's first tile only: its lanes 0..7 are env 0, the leg lanes store their three angles and the lane
// that stores the root in fly_body stores position and quaternion.
__device__ __forceinline__ void store_pose(float* __restrict__ poses, int t, const FlyRegs& nx)
{
    const int sub = threadIdx.x;
    if (sub >= LANES_PER_ENV) return;
    float* p = poses + (long)t * FLY_POSE_FLOATS;
    if (sub < FLY_NUM_LEGS) {
#pragma unroll
        for (int i = 0; i < 3; ++i) p[7 + 3 * sub + i] = nx.jq[i];
    }
    if (sub == LANES_PER_ENV - 1) {
        p[0] = nx.r.px; p[1] = nx.r.py; p[2] = nx.r.pz; p[3] = nx.r.qx; p[4] = nx.r.qy; p[5] = nx.r.qz; p[6] = nx.r.qw;
    }
}

// One launch per ROLLOUT (ppo.py:204-237 for T consecutive env steps): the envs of a 32-env tile depend on no other
// tile and the policy does not change inside a rollout, so workgroup b simply loops over the T steps of ITS tile --
// policy forward + sampling on observation row t, env step, observation row t + 1 -- with the env state carried in
// registers.  What a launch per step pays T times (the launch boundary, the prologue, the state's round trip) is paid
// once.  Row t's buffers are row t of the rollout tensors (fixed strides); the deferred bookkeeping is exact because
// row t decays the variance t - *rows_applied times and no flush can run while the launch does.  Between steps the
// workgroup waits for its own observation-row stores (vmcnt(0) + barrier): row t + 1 is read only by the workgroup
// that wrote it, at addresses this CU has not read before.  Bit for bit what T launches of rollout_step_kernel leave.
// WPS = waves per SIMD the registers are budgeted for: 1 when the launch has at most one workgroup per CU (<= 8192
// envs: the step body plus the carried env state want ~300 registers and spill at 256), 2 beyond that.
// REC: store env 0's pose of every step to poses [T][FLY_POSE_FLOATS] (store_pose); the other instantiations ignore `poses`.
// NORM: the policy input of every step is normalised (rollout_step_kernel's NORM); the observation ring stays raw.
// DR: rollout_step_kernel's DR; the env's multipliers and draw count ride in FlyRegs from step to step (read once, stored at draws).
template <bool B3, int WPS, bool REC, bool NORM = false, bool DR = false>
__global__ __launch_bounds__(THREADS, WPS) void rollout_all_kernel(
    const FlyConfig* __restrict__ c, FlyBuffers b, const float* __restrict__ P, const void* __restrict__ PF,
    float* __restrict__ obs_ring, long n, const float* __restrict__ eps_all, const float* __restrict__ var, float var_decay,
    float var_min, float* __restrict__ act_all, float* __restrict__ logp_all, float* __restrict__ v_ring,
    float* __restrict__ reward_all, int T, const int* __restrict__ rows_applied, int64_t* __restrict__ reset_rows,
    int64_t* __restrict__ progress_rows, float* __restrict__ poses)
{
    typedef ArithOf<B3> Arith;
    constexpr int ARENA = RS_LDS_FLOATS<Arith>;
    __shared__ __attribute__((aligned(16))) float lds[ARENA + 32 + BM * MLP_NACT + (NORM ? NORM_LDS_FLOATS : 0)];
    float* const norm_tab = NORM ? lds + ARENA + 32 + BM * MLP_NACT : nullptr;
    if (NORM) obs_norm_load(norm_tab, c);                        // published by the barrier below
    constexpr int PH_ALL = PH_SCALE | PH_RESET | PH_INTEGRATE | PH_OBS | PH_PROGRESS | PH_REWARD;
    // the variance of the CURRENT row lives in LDS and is decayed once per step (ppo.py:236-237): the same sequence of
    // fp32 operations as the per-step form, O(1) per step however long the rollout (T = 40 960 at 16 envs)
    float* varcur = lds + ARENA;
    // bf16x3 body: the two hand-offs between the policy and the env step of a tile stay in LDS -- the sampled actions go to
    // `acts` as well as to their HBM row, and the observation row the env step stages in the arena IS the next step's
    // policy input -- so neither waits for its stores to be acknowledged nor reads its own row back through L2
    // (the HBM rows are still written: the update reads them).  Same values, same bits.
    float* acts = B3 ? lds + ARENA + 32 : nullptr;
    // the launch is the FIRST device work of its rollout: *rows_applied was zeroed just before it and no bookkeeping
    // flush can run until it has finished, so `var` is exactly the variance of row 0
    if (threadIdx.x < MLP_NACT) varcur[threadIdx.x] = var[threadIdx.x];
    FlyRegs st;
    fly_load<PH_ALL, DR>(st, c, b, blockIdx.x);
    FlyCarry cy;                                                 // the episode accumulators and what the state stores need: stored after step T - 1
    fly_load_carry(cy, c, b, blockIdx.x);
    __syncthreads();
    const bool whole = (long)(blockIdx.x + 1) * BM <= n;         // a ragged last tile keeps the HBM hand-offs (its LDS rows are partly stale)
    for (int t = 0; t < T; ++t) {
        const float* x = obs_ring + (long)t * n * FLY_NUM_OBS;
        float* act = act_all + (long)t * n * MLP_NACT;
        b.obs = obs_ring + (long)(t + 1) * n * FLY_NUM_OBS;
        b.reward = reward_all + (long)t * n;
        if (reset_rows) { b.reset = reset_rows + (long)t * n; b.progress = progress_rows + (long)t * n; }   // fly.py:175-177, per step
        const bool in_lds = B3 && whole;
        forward_body<Arith, false, false, NORM>(lds, blockIdx.x, 1L << 40, P, PF, x, n, nullptr, v_ring + (long)t * n, nullptr, nullptr,
                                                nullptr, nullptr, eps_all + (long)t * n * MLP_NACT, varcur, act, logp_all + (long)t * n,
                                                nullptr, 0, var_decay, var_min, norm_tab, in_lds && t > 0 ? lds : nullptr,
                                                in_lds ? acts : nullptr, B3 && t > 0);
        if (!in_lds) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);      // this thread's action stores are acknowledged by L2
        }
        __syncthreads();
        // FlyConfig is still read step by step here: this kernel's registers are full (fetching it once spills)
        FlyRegs nx;
        fly_body<PH_ALL, DR>(c, FlyRead{c}, act, b, lds, blockIdx.x, st, &nx, in_lds ? acts : nullptr, &cy);
        if (REC && blockIdx.x == 0) store_pose(poses, t, nx);
        st = nx;
        if (threadIdx.x < MLP_NACT && var_decay > 0.0f) varcur[threadIdx.x] = fmaxf(var_min, varcur[threadIdx.x] - var_decay);
        if (!in_lds) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // observation row t + 1 is in L2 before any wave of this workgroup reads it
        __syncthreads();
    }
    // the env's state tensors and episode accumulators: nothing reads them before the launch ends, so they are stored once, here
    if (T > 0) fly_store_carried<PH_ALL>(b, blockIdx.x, (int)n, st, cy);
}

// The same loop with the policy in the fused step's style (policy_tile_fs, mlp_fused_step.inc): swizzled plane images, the chain
// GEMMs' asm MFMA streams, 135 KB of LDS -- one workgroup per CU, whole tiles only (the launcher checks both).  The env step
// stages its observation block in H2's region of that image, which is where the next step's policy converts it from.
// STAMP (diagnostic instantiation, bench.py / tools/ab_rollout.py): thread 0 of every workgroup stores s_memtime into stamps
// u64 [tile][T + 1][8]: slot 0 the top of step t, 1 .. 5 inside the policy (x converted, layer 1, 2, 3, 4 done), 7 between the
// policy and env halves (+ the 100 MHz real-time counter once, at [T][1]).
// MULTI: more tiles than workgroups (> 8192 envs on 256 CUs): the outer loop really loops; the single-tile instantiation keeps
// the register allocation of a kernel without it.
// REC: the pose record of rollout_all_kernel (store_pose, workgroup 0's first tile), poses [T][FLY_POSE_FLOATS] in `aux`.
// NORM: the observation block is normalised before its conversion (policy_tile_fs); the table sits behind the FR_LDS_BYTES of
// the image (the launch asks for NORM_LDS_FLOATS more).
// DR: rollout_all_kernel's DR (each tile's rows are read by its fly_load, then carried in FlyRegs).
template <bool STAMP, bool MULTI, bool REC, bool NORM = false, bool DR = false>
__global__ __launch_bounds__(THREADS, 1) void rollout_all_fs_kernel(
    const FlyConfig* __restrict__ c, FlyBuffers b, const float* __restrict__ P, const u16* __restrict__ PB,
    float* __restrict__ obs_ring, long n, const float* __restrict__ eps_all, const float* __restrict__ var, float var_decay,
    float var_min, float* __restrict__ act_all, float* __restrict__ logp_all, float* __restrict__ v_ring,
    float* __restrict__ reward_all, int T, int64_t* __restrict__ reset_rows, int64_t* __restrict__ progress_rows,
    void* __restrict__ aux)
{
    // aux: the stamps (STAMP) or the pose record (REC) -- one slot, so that the kernel arguments, and with them the offsets of the
    // implicit ones (gridDim), stay those of the kernel without recording
    static_assert(!(STAMP && REC) && !(STAMP && NORM) && !(STAMP && DR), "the stamped diagnostic form neither records, normalises nor randomises");
    unsigned long long* const stamps = static_cast<unsigned long long*>(aux);
    float* const poses = static_cast<float*>(aux);
    extern __shared__ __attribute__((aligned(16))) u16 fr_lds[];
    const FrLds L(fr_lds);
    constexpr int PH_ALL = PH_SCALE | PH_RESET | PH_INTEGRATE | PH_OBS | PH_PROGRESS | PH_REWARD;
    policy_tile_fs_setup(L, P);
    float* const norm_tab = NORM ? reinterpret_cast<float*>(fr_lds) + FR_LDS_BYTES / 4 : nullptr;
    if (NORM) obs_norm_load(norm_tab, c);                     // published, like the biases, by the barrier before step 0
    int64_t* const reset0 = b.reset;                          // the CURRENT flags: read once per tile, before the tile's step 0
    int64_t* const progress0 = b.progress;
    const long ntiles = n / BM;                               // whole tiles only (the launcher checks)
    const FlyConsts k(c);                                   // once per launch, in front of the tile loop: no step reads FlyConfig
    // persistent over tiles: workgroup g runs the T steps of tiles g, g + grid, ... one after the other (one tile per workgroup at
    // <= 8192 envs on 256 CUs; two at 16384).  Tiles are independent, so the order is free and every row equals the per-step launches'.
    long tile = blockIdx.x;
    do {
        unsigned long long* st_tile = STAMP ? stamps + tile * (T + 1) * 8 : nullptr;
        if (threadIdx.x < 32) L.varcur[threadIdx.x] = threadIdx.x < MLP_NACT ? var[threadIdx.x] : 1.0f;   // the variance of row 0 (see rollout_all_kernel)
        b.reset = reset0; b.progress = progress0;
        FlyRegs st;
        fly_load<PH_ALL, DR>(st, c, b, (int)tile);
        FlyCarry cy;                                          // the episode accumulators and what the state stores need: stored after step T - 1
        fly_load_carry(cy, c, b, (int)tile);
        WeightHeadT<2> w1;
        policy_tile_fs_head(w1, PB);
        __syncthreads();
        if (STAMP && threadIdx.x == 0) st_tile[6] = realtime_cu();      // (with [T][1]: the shader clock the stamps tick at)
        for (int t = 0; t < T; ++t) {
            stamp<STAMP>(st_tile, 8 * t);
            float* act = act_all + (long)t * n * MLP_NACT;
            b.obs = obs_ring + (long)(t + 1) * n * FLY_NUM_OBS;
            b.reward = reward_all + (long)t * n;
            if (reset_rows) { b.reset = reset_rows + (long)t * n; b.progress = progress_rows + (long)t * n; }   // fly.py:175-177, per step
            policy_tile_fs<STAMP, NORM>(L, tile, PB, t == 0 ? obs_ring : nullptr, n, v_ring + (long)t * n, eps_all + (long)t * n * MLP_NACT,
                                        act, logp_all + (long)t * n, w1, STAMP ? st_tile + 8 * t : nullptr, norm_tab);
            stamp<STAMP>(st_tile, 8 * t + 7);
            policy_tile_fs_head(w1, PB);     // the NEXT step's first weights: their round trip hides under the physics (A/B: requested
                                             // after the env step; not kept)
            FlyRegs nx;
            fly_body<PH_ALL, DR>(c, k, act, b, L.obs, (int)tile, st, &nx, L.acts, &cy);
            if (REC && tile == 0) store_pose(poses, t, nx);
            st = nx;
            if (threadIdx.x < MLP_NACT && var_decay > 0.0f) L.varcur[threadIdx.x] = fmaxf(var_min, L.varcur[threadIdx.x] - var_decay);
            __syncthreads();
        }
        // the tile's state tensors and episode accumulators: nothing reads them before the launch ends, so they are stored once, here
        if (T > 0) fly_store_carried<PH_ALL>(b, (int)tile, (int)n, st, cy);
        stamp<STAMP>(st_tile, 8 * T);
        if (STAMP && threadIdx.x == 0) st_tile[8 * T + 1] = realtime_cu();
        tile += gridDim.x;
    } while (MULTI && tile < ntiles);
}

}  // namespace

// poses (optional, device [T][FLY_POSE_FLOATS]): launch the REC instantiation of whichever kernel the shape selects -- recording
// never changes the launch form.  The stamped diagnostic instantiation does not record.  norm: the NORM instantiation of the same
// kernel (the table registered in dcfg's slot, fly_set_obs_norm); dr: its DR instantiation (fly_set_randomization); neither with
// stamps.
extern "C" hipError_t flyhip_launch_rollout_all(const FlyConfig* dcfg, const FlyBuffers* b, const float* P, const float* PF,
                                                float* obs_ring, int64_t n, const float* eps_all, const float* var,
                                                float var_decay, float var_min, float* act_all, float* logp_all, float* v_ring,
                                                float* reward_all, int T, const int* rows_applied, const uint16_t* PB,
                                                int64_t* reset_rows, int64_t* progress_rows, void* stream,
                                                unsigned long long* stamps, float* poses, int norm, int dr)
{
    const dim3 grid((unsigned)((n + BM - 1) / BM));
    const int cus = device_cus();
    const bool one_per_cu = (int)grid.x <= cus;
    const char* fs_env = getenv("FLY_ROLLOUT_FS");               // read per launch: the tests flip it inside one process
    const bool fs_off = fs_env != nullptr && fs_env[0] == '0';
    if (stamps && (poses || norm || dr)) return hipErrorInvalidValue;
    const bool rec = poses != nullptr;
    if (PB && n % BM == 0 && !fs_off) {       // the policy body in the fused step's style (A/B: FLY_ROLLOUT_FS=0); persistent over tiles
        const dim3 grid_fs(one_per_cu ? grid.x : (unsigned)cus);     // the fused-style kernel walks its tiles itself
        static_assert(FR_LDS_BYTES % 4 == 0, "the table follows the image");
        // aux: the stamps or the pose record; the table and the randomisation slot are read through dcfg
        auto fs = [&](void* aux, auto S, auto M, auto R, auto N, auto D) {
            return launch_kernel<rollout_all_fs_kernel<S.value, M.value, R.value, N.value, D.value>>(
                grid_fs, THREADS, FR_LDS_BYTES + (N.value ? NORM_LDS_FLOATS * 4 : 0), stream, dcfg, *b, P, PB, obs_ring, (long)n, eps_all,
                var, var_decay, var_min, act_all, logp_all, v_ring, reward_all, T, reset_rows, progress_rows, aux);
        };
        constexpr std::false_type no{};
        const bool multi = !one_per_cu;
        if (stamps) return with_bools([&](auto M) { return fs(stamps, std::true_type{}, M, no, no, no); }, multi);   // records, normalises, randomises nothing
        return with_bools([&](auto M, auto R, auto N, auto D) { return fs(poses, no, M, R, N, D); }, multi, rec, norm != 0, dr != 0);
    }
    if (stamps) return hipErrorInvalidValue;        // only the fused-style kernel has a stamped instantiation
    auto ra = [&](auto B3, auto WPS, const void* pf) {
        return with_bools([&](auto R, auto N, auto D) {
            return launch_kernel<rollout_all_kernel<B3.value, WPS.value, R.value, N.value, D.value>>(
                grid, THREADS, 0, stream, dcfg, *b, P, pf, obs_ring, (long)n, eps_all, var, var_decay, var_min, act_all, logp_all, v_ring,
                reward_all, T, rows_applied, reset_rows, progress_rows, poses);
        }, rec, norm != 0, dr != 0);
    };
    if (PB) return ra(std::true_type{}, int_c<1>{}, PB);        // the bf16x3 body needs one wave per SIMD anyway
    return one_per_cu ? ra(std::false_type{}, int_c<1>{}, PF) : ra(std::false_type{}, int_c<2>{}, PF);
}

extern "C" hipError_t flyhip_launch_mlp_forward(const float* P, const float* PF, const float* x, int64_t n, float* mu_out,
                                                float* v_out, float* out_save, float* h1_save, float* h2_save,
                                                float* h3_save, const uint16_t* PB, void* stream)
{
    if (PB) {       // bf16x3 GEMMs
        const long tiles = (n + BM - 1) / BM;
        const int grid = (int)tiles;
        hipLaunchKernelGGL(mlp_forward_b3_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, P, PB, x, (long)n, mu_out,
                           v_out, out_save, h1_save, h2_save, h3_save, (const float*)nullptr, (const float*)nullptr,
                           (float*)nullptr, (float*)nullptr, 0, 0.0f, 0.0f, (const int*)nullptr);
        return hipGetLastError();
    }
    // Large inputs (the critic pass over the whole rollout) run persistent workgroups, 3 per CU, each
    // walking many tiles with the next tile's rows prefetched.  Up to a few tiles per slot the
    // hardware's dynamic workgroup dispatch balances better than a fixed walk (1280 tiles over 768
    // slots would leave part of the chip idle for the second half), so those launch one tile each.
    const long tiles = (n + BM - 1) / BM;
    const int grid = (int)(tiles <= 4 * PERSIST_GRID ? tiles : PERSIST_GRID);
    hipLaunchKernelGGL(mlp_forward_kernel<false>, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, P, PF, x, (long)n,
                       mu_out, v_out, out_save, h1_save, h2_save, h3_save, (const float*)nullptr, (const float*)nullptr,
                       (float*)nullptr, (float*)nullptr, (unsigned long long*)nullptr, 0, 0.0f, 0.0f, (const int*)nullptr);
    return hipGetLastError();
}

extern "C" hipError_t flyhip_launch_mlp_forward_sample(const float* P, const float* PF, const float* x, int64_t n,
                                                       const float* eps, const float* var, int var_steps,
                                                       float var_decay, float var_min, float* act_out,
                                                       float* logp_out, float* mu_out, float* v_out, const uint16_t* PB,
                                                       const int* var_base, void* stream)
{
    if (PB) {
        const long tiles = (n + BM - 1) / BM;
        const int grid = (int)tiles;
        hipLaunchKernelGGL(mlp_forward_b3_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, P, PB, x, (long)n, mu_out,
                           v_out, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, eps, var, act_out,
                           logp_out, var_steps, var_decay, var_min, var_base);
        return hipGetLastError();
    }
    const long tiles = (n + BM - 1) / BM;
    const int grid = (int)(tiles <= 4 * PERSIST_GRID ? tiles : PERSIST_GRID);
    hipLaunchKernelGGL(mlp_forward_kernel<false>, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, P, PF, x, (long)n,
                       mu_out, v_out, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, eps,
                       var, act_out, logp_out, (unsigned long long*)nullptr, var_steps, var_decay, var_min, var_base);
    return hipGetLastError();
}

// diagnostic build of the same kernel with phase stamps (tools/stamp_forward.py); not part of the ABI header
extern "C" int flyhip_debug_mlp_forward_stamped(const float* P, const float* PF, const float* x, int64_t n,
                                                float* out_save, float* h1_save, float* h2_save, float* h3_save,
                                                unsigned long long* stamps, void* stream, int grid_override)
{
    const long tiles = (n + BM - 1) / BM;
    const int grid = grid_override > 0 ? grid_override : (int)(tiles <= 4 * PERSIST_GRID ? tiles : PERSIST_GRID);
    hipLaunchKernelGGL(mlp_forward_kernel<true>, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, P, PF, x, (long)n,
                       (float*)nullptr, (float*)nullptr, out_save, h1_save, h2_save, h3_save, (const float*)nullptr,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr, stamps, 0, 0.0f, 0.0f, (const int*)nullptr);
    return (int)hipGetLastError();
}

extern "C" hipError_t flyhip_launch_mlp_backward_dx(const float* PT, const float* out_saved, const float* h1,
                                                    const float* h2, const float* h3, const float* action,
                                                    const float* old_logp, const float* adv, const float* target,
                                                    const float* var, int64_t n, float inv_batch, float clip,
                                                    float* dz4, float* dz3, float* dz2, float* dz1, float* loss_part,
                                                    const uint16_t* PTB, void* stream)
{
    if (PTB) {
        hipLaunchKernelGGL(mlp_backward_dx_b3_kernel, dim3((unsigned)((n + BM - 1) / BM)), dim3(THREADS), 0, (hipStream_t)stream,
                           PTB, out_saved, h1, h2, h3, action, old_logp, adv, target, var, (long)n, inv_batch, clip, dz4, dz3,
                           dz2, dz1, loss_part);
        return hipGetLastError();
    }
    const int grid = (int)((n + BM - 1) / BM);
    hipLaunchKernelGGL(mlp_backward_dx_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, PT, out_saved,
                       h1, h2, h3, action, old_logp, adv, target, var, (long)n, inv_batch, clip, dz4, dz3, dz2, dz1,
                       loss_part);
    return hipGetLastError();
}

// workgroups per layer, proportional to the layer's share of the dW FLOPs (256 in total)
// slabs are whole 32-row tiles; a chunk costs its MFMAs plus a fixed staging/barrier overhead, so the thin layers
// (3 and 4) get more workgroups than their FLOP share: measured best of a dozen splits at 1280 tiles
static int kGradWgs[4] = {80, 100, 52, 24};
// the bf16x3 kernel (grad_w_b3.inc) pays a fixed staging + barrier cost per 16-row chunk, so its thin layers get
// the kernel streams: a CU pulls ~22 GB/s, so the split follows each layer's BYTES (54 / 63 / 42 / 26 MB), not its FLOPs
static int kGradWgsB3[4] = {72, 88, 64, 32};
static bool gw_env_read = false;
static void gw_read_env()
{   // tuning aid: FLYHIP_GW_SPLIT="a,b,c,d" overrides the split (sum <= 256)
    if (gw_env_read) return;
    gw_env_read = true;
    const char* e = getenv("FLYHIP_GW_SPLIT");
    int v[4];
    if (e && sscanf(e, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) == 4 && v[0] > 0 && v[1] > 0 && v[2] > 0 && v[3] > 0 &&
        v[0] + v[1] + v[2] + v[3] <= 1024)
        for (int i = 0; i < 4; ++i) kGradWgs[i] = kGradWgsB3[i] = v[i];
}

static int g_fb_consumer_shift = 0;     // test hook: moves the consumer range off its producers' XCDs (forces err = 2 in xcd mode)
extern "C" void flyhip_debug_set_fwd_bwd_consumer_shift(int shift) { g_fb_consumer_shift = shift; }

extern "C" hipError_t flyhip_launch_mlp_fwd_bwd(const float* P, const float* PF, const float* PT, const float* x, int64_t n,
                                                float* out_save, float* h1_save, float* h2_save, float* h3_save,
                                                const float* action, const float* old_logp, const float* adv,
                                                const float* target, const float* var, float inv_batch, float clip,
                                                float* dz4, float* dz3, float* dz2, float* dz1, float* loss_part,
                                                int* flags, int epoch, int* err, const uint16_t* PB, const uint16_t* PTB,
                                                int coherent, void* stream)
{
    const long tiles = (n + BM - 1) / BM;
    const int shift = g_fb_consumer_shift;
    const long pad_tiles = ((tiles + 7) & ~7L) + shift;
    const dim3 grid((unsigned)(pad_tiles + tiles));
    const bool b3 = PB && PTB;
    const void* pf = b3 ? (const void*)PB : (const void*)PF;
    const void* pt = b3 ? (const void*)PTB : (const void*)PT;
    return with_bools([&](auto B3, auto COH) {
        return launch_kernel<mlp_fwd_bwd_kernel<false, B3.value, COH.value>>(
            grid, THREADS, 0, stream, P, pf, pt, x, (long)n, out_save, h1_save, h2_save, h3_save, action, old_logp, adv, target, var,
            inv_batch, clip, dz4, dz3, dz2, dz1, loss_part, flags, epoch, err, (unsigned long long*)nullptr, shift);
    }, b3, coherent != 0);
}

// diagnostic build with per-workgroup start/end stamps (tools/stamp_fwd_bwd.py); not part of the ABI header
extern "C" int flyhip_debug_mlp_fwd_bwd_stamped(const float* P, const float* PF, const float* PT, const float* x, int64_t n,
                                                float* out_save, float* h1_save, float* h2_save, float* h3_save,
                                                const float* action, const float* old_logp, const float* adv,
                                                const float* target, const float* var, float inv_batch, float clip,
                                                float* dz4, float* dz3, float* dz2, float* dz1, float* loss_part,
                                                int* flags, int epoch, int* err, unsigned long long* stamps, void* stream)
{
    const long tiles = (n + BM - 1) / BM;
    const long pad_tiles = (tiles + 7) & ~7L;
    hipLaunchKernelGGL((mlp_fwd_bwd_kernel<true, false, true>), dim3((unsigned)(pad_tiles + tiles)), dim3(THREADS), 0, (hipStream_t)stream, P,
                       (const void*)PF, (const void*)PT, x, (long)n, out_save, h1_save, h2_save, h3_save, action, old_logp, adv, target, var, inv_batch,
                       clip, dz4, dz3, dz2, dz1, loss_part, flags, epoch, err, stamps, 0);
    return (int)hipGetLastError();
}

extern "C" hipError_t flyhip_launch_rollout_step(const FlyConfig* dcfg, const FlyBuffers* b, const float* P, const float* PF,
                                                 const float* x, int64_t n, const float* eps, const float* var, int var_steps,
                                                 float var_decay, float var_min, float* act, float* logp, float* v_out,
                                                 const uint16_t* PB, const int* var_base, void* stream, int norm, int dr)
{
    const dim3 grid((unsigned)((n + BM - 1) / BM));
    return with_bools([&](auto B3, auto N, auto D) {
        return launch_kernel<rollout_step_kernel<B3.value, N.value, D.value>>(
            grid, THREADS, 0, stream, dcfg, *b, P, B3.value ? (const void*)PB : (const void*)PF, x, (long)n, eps, var, var_steps, var_decay,
            var_min, act, logp, v_out, var_base);
    }, PB != nullptr, norm != 0, dr != 0);
}

extern "C" int64_t flyhip_mlp_grad_workspace_floats(void)
{
    gw_read_env();
    int64_t need = 0;
    for (const int* w : {kGradWgs, kGradWgsB3}) {
        const int64_t f = (int64_t)w[0] * MLP_H1 * (MLP_IN_PAD + 1) + (int64_t)w[1] * MLP_H2 * (MLP_H1 + 1) +
                          (int64_t)w[2] * MLP_H3 * (MLP_H2 + 1) + (int64_t)w[3] * MLP_OUT * (MLP_H3 + 1);   // N*KP + N per slab
        need = f > need ? f : need;
    }
    return need;
}

extern "C" hipError_t flyhip_launch_mlp_grad_w(const float* x, const float* h1, const float* h2, const float* h3,
                                               const float* dz1, const float* dz2, const float* dz3, const float* dz4,
                                               int64_t n, float* workspace, float* grad_out, const float* norm_mask,
                                               float* norm_ws, int* norm_step, const int* err, int gemm_b3, void* stream)
{
    gw_read_env();
    GradWTable T;
    const float* dz[4] = {dz1, dz2, dz3, dz4};
    const float* a[4] = {x, h1, h2, h3};
    const int N[4] = {MLP_H1, MLP_H2, MLP_H3, MLP_OUT};
    const int Ka[4] = {MLP_IN, MLP_H1, MLP_H2, MLP_H3};
    const int KP[4] = {MLP_IN_PAD, MLP_H1, MLP_H2, MLP_H3};
    float* ws = workspace;
    int first = 0;
    const int* wgs = gemm_b3 ? kGradWgsB3 : kGradWgs;
    for (int l = 0; l < 4; ++l) {
        T.l[l].dz = dz[l]; T.l[l].a = a[l]; T.l[l].partial = ws;
        T.l[l].N = N[l]; T.l[l].Ka = Ka[l]; T.l[l].KP = KP[l]; T.l[l].wgs = wgs[l]; T.l[l].first_block = first;
        T.l[l].accumulate = 0; T.l[l].chunked = 0;
        ws += (long)wgs[l] * ((long)N[l] * KP[l] + N[l]);
        first += wgs[l];
    }
    // dynamic LDS: two buffers of the largest layer's chunk (padded pitches): 2 x 32 x (136 + 264) floats = 100 KiB
    const size_t lds_bytes = sizeof(float) * 2 * GW_ROWS * (MLP_H2 + GW_PAD + MLP_H1 + GW_PAD);
    static_assert(MLP_H1 + GW_PAD + 96 <= MLP_H2 + GW_PAD + MLP_H1 + GW_PAD, "layer 1 chunk fits");
    // two buffers of three bf16 term planes of a chunk: layers 1 / 2 stage 16 rows x (288 + 160) columns (84 KiB),
    // layer 3 32 rows x (160 + 160) (120 KiB, the largest), layer 4 32 rows x (32 + 160) (72 KiB)
    const size_t b3_bytes = 2 * 3 * GB_ROWS_L3 * 2 * gb_pitch<MLP_H3>() * sizeof(u16);
    static_assert(16 * (gb_pitch<MLP_H1>() + gb_pitch<MLP_H2>()) <= GB_ROWS_L3 * 2 * gb_pitch<MLP_H3>() &&
                  GB_ROWS_L4 * (gb_pitch<MLP_OUT>() + gb_pitch<MLP_H3>()) <= GB_ROWS_L3 * 2 * gb_pitch<MLP_H3>(), "layer 3's chunk is the largest");
    hipError_t e = gemm_b3 ? launch_kernel<mlp_grad_w_b3_kernel>(first, GW_THREADS, b3_bytes, stream, T, (long)n)
                           : launch_kernel<mlp_grad_w_kernel>(first, GW_THREADS, lds_bytes, stream, T, (long)n);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mlp_grad_reduce_kernel<4>, dim3(RED_BLOCKS), dim3(64 * RED_WAVES), 0,
                       (hipStream_t)stream, T, grad_out, norm_mask, norm_ws, norm_step, err);
    return hipGetLastError();
}

extern "C" int flyhip_mlp_reduce_blocks(void) { return RED_BLOCKS; }

// ---- the fused optimizer-step gradient: mlp_fused_step_kernel + the fixed-order reduction of its per-workgroup slabs ------
static int g_fused_grid_override = 0;    // test / tuning hook: fewer workgroups than CUs (each then walks more tiles)
extern "C" void flyhip_debug_set_fused_grid(int grid) { g_fused_grid_override = grid; }
extern "C" int flyhip_debug_get_fused_grid(void) { return g_fused_grid_override; }

extern "C" int64_t flyhip_mlp_fused_workspace_floats(void)
{
    // one partial slab per workgroup; chunked layout: every layer's block padded to whole 1 KiB chunks
    return (int64_t)device_cus() * (fs_pad256(FS_STRIDE1) + fs_pad256(FS_STRIDE2) + fs_pad256(FS_STRIDE3) + fs_pad256(FS_STRIDE4));
}

extern "C" hipError_t flyhip_launch_mlp_fused_grad(const float* P, const uint16_t* PB, const uint16_t* PTB, const float* x,
                                                   int64_t n, const float* action, const float* old_logp, const float* adv,
                                                   const float* target, const float* var, float inv_batch, float clip,
                                                   float* workspace, float* grad_out, const float* norm_mask, float* norm_ws,
                                                   int* norm_step, float* loss_part, float* const* dump, void* stream)
{
    const int grid = fused_grid(n, BM);
    FusedDump d;
    hipError_t e = with_int<0, 1, 2>(decode_dump(dump, d), [&](auto mode) {
        return launch_kernel<mlp_fused_step_kernel<mode.value>>(grid, THREADS, FS_LDS_BYTES, stream, P, PB, PTB, x, (long)n, action, old_logp,
                                                                adv, target, var, inv_batch, clip, workspace, loss_part, d);
    });
    if (e != hipSuccess) return e;
    // the slabs have the layout the reduction already sums: per layer `grid` blocks of N*KP + N floats, padded to whole 1 KiB chunks
    // and interleaved chunk by chunk (fs_slab)
    GradWTable T;
    const int N[4] = {MLP_H1, MLP_H2, MLP_H3, MLP_OUT};
    const int KP[4] = {MLP_IN_PAD, MLP_H1, MLP_H2, MLP_H3};
    float* part[4];
    float* w = workspace;
    for (int l = 0; l < 4; ++l) { part[l] = w; w += (long)grid * fs_pad256((long)N[l] * KP[l] + N[l]); }
    fill_slab_table(T, N, KP, part, grid, 1);
    // (loads in flight per wave: 4 -> 15.8 us for the 256 slabs, 8 -> 17.2, 16 -> 58 (the 1024-thread block's register budget))
    hipLaunchKernelGGL(mlp_grad_reduce_kernel<4>, dim3(RED_BLOCKS), dim3(64 * RED_WAVES), 0, (hipStream_t)stream, T, grad_out,
                       norm_mask, norm_ws, norm_step, (const int*)nullptr);
    return hipGetLastError();
}

// mlp_adam_apply_kernel requests everything it reads at entry, in one round trip (mlp_adam.inc).  What that rests on, held here at
// compile time: every launch form hands each thread AT MOST ONE norm partial (73 of its own norm kernel, 291 of the slab reductions),
// so the partial is one of those requests and not a loop behind them; and the words the kernel reads in place of a scale table that
// is not passed (norm_ws[8 .. 11], norm_ws[H2_SINCE], norm_ws[H2_SINCE + 1]: read and dropped) and every partial lie inside the
// 1280 floats include/flyhip.h asks of norm_ws.
constexpr int MLP_NORM_WS_FLOATS = 1280;
static_assert(ADAM_BLOCKS <= ADAM_THREADS && RED_BLOCKS <= ADAM_THREADS,
              "one norm partial per thread of mlp_adam_apply_kernel");
static_assert(1 + ADAM_BLOCKS <= MLP_NORM_WS_FLOATS && 1 + RED_BLOCKS <= MLP_NORM_WS_FLOATS && H2_SINCE + 1 < MLP_NORM_WS_FLOATS &&
              8 + 3 < MLP_NORM_WS_FLOATS, "mlp_adam_apply_kernel reads norm_ws inside its documented size");
static_assert(MLP_PACKED_FLOATS / 4 >= ADAM_THREADS && MLP_ERR_SLOT < MLP_PACKED_FLOATS,
              "the first trip of the self_norm gradient sum and the error mark are inside G");

extern "C" hipError_t flyhip_launch_mlp_adam(float* P, float* PF, float* PT, const int* idx_f, const int* idx_t,
                                             const float* G, const float* mask, float* m,
                                             float* v, int* step, float lr, float beta1, float beta2, float eps,
                                             float max_norm, float grad_scale, float* norm_ws, int norm_ready,
                                             uint16_t* PB, uint16_t* PTB, const int* idx_fb, const int* idx_tb,
                                             int* step_out, const int* grad_invalid, uint16_t* PH, uint16_t* PTH,
                                             float* h2_scales, int h2_period, void* stream)
{
    int nparts = ADAM_BLOCKS;
    float part_scale = 1.0f;
    if (step_out) {                 // one launch: the kernel sums the gradient itself and ping-pongs the step counter
        part_scale = 1.0f;          // its sum is of the SCALED gradient
    } else if (norm_ready) {               // mlp_grad_w already left per-block sums of squares (unscaled) and advanced the step
        nparts = RED_BLOCKS;
        part_scale = grad_scale * grad_scale;
    } else {
        hipLaunchKernelGGL(mlp_adam_norm_kernel, dim3(ADAM_BLOCKS), dim3(ADAM_THREADS), 0, (hipStream_t)stream, G, mask,
                           grad_scale, norm_ws, step, grad_invalid);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mlp_adam_apply_kernel, dim3(ADAM_BLOCKS), dim3(ADAM_THREADS), 0, (hipStream_t)stream, P, PF, PT,
                       idx_f, idx_t, G, mask, m, v, step, lr, beta1, beta2, eps, max_norm, grad_scale, norm_ws, nparts,
                       part_scale, PB, PTB, idx_fb, idx_tb, step_out, grad_invalid, PH, PTH, h2_scales, h2_period);
    return hipGetLastError();
}

extern "C" hipError_t flyhip_launch_mlp_h2_rescale(const float* P, const int* idx_fb, const int* idx_tb, uint16_t* PH, uint16_t* PTH,
                                                   float* h2_scales, void* stream)
{
    hipLaunchKernelGGL(mlp_h2_rescale_kernel, dim3(1), dim3(H2_RESCALE_THREADS), 0, (hipStream_t)stream, P, idx_fb, idx_tb, PH, PTH, h2_scales);
    return hipGetLastError();
}
