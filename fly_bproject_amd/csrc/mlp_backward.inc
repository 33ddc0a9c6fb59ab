// mlp_backward.inc — loss gradient + dX chain body (both arithmetics), its kernels, and the one-launch
// forward+backward kernel with per-tile flags.
// ---------------------------------------------------------------------------------------------
// Backward, part 1: PPO loss gradient at the network outputs + the dX chain (ppo.py:184-197).
// One 32-row tile per workgroup.  The loss (ppo.py:191-194) is
//     mean_i( -min(ratio_i A_i, clamp(ratio_i, 1-c, 1+c) A_i) ) + mean_i huber(v_i - target_i)
// with ratio_i = exp(logp_i - old_logp_i) and logp the diagonal-Gaussian log-density of the
// stored action under the CURRENT variance.  The row's loss terms and their gradient, torch's
// subgradient choices included, are ppo_row_loss in loss_head.inc, shared with the fused kernels.
//   dz4 [n][32]: cols 0..17 d/d(pre-ELU mean), col 18 d/d(value), rest 0
//   dz3 [n][128], dz2 [n][128], dz1 [n][256]: gradients at the pre-activations of layers 3,2,1
//   loss_part [grid][2]: per-workgroup sums of the policy term and of the Huber term
// dZ = dA * ELU'(H) with H read from the saved activations (hfrag_load / epilogue_dact, mlp_gemm.inc).
// Loss gradient at the outputs of one tile, one thread per (row, output column), for both arithmetics: the 32 lanes of a
// row reduce the Mahalanobis term and log-determinant with a fixed xor butterfly, every lane then holds the row's loss
// terms (ppo_row_loss, loss_head.inc) and writes its own column of dZ4 -- to HBM and, through `store_z4(row, col, d)`,
// to the LDS operand of the next GEMM in that arithmetic's form.  Ends with the workgroup's barrier and the tile's loss
// partials.
template <bool COH, class StoreZ4>
__device__ __forceinline__ void ppo_loss_phase(
    const long tile, const float* __restrict__ out_saved, const float* __restrict__ action,
    const float* __restrict__ old_logp, const float* __restrict__ adv, const float* __restrict__ target,
    const float* __restrict__ var, int nvalid, float inv_batch, float clip, float* __restrict__ dz4, float* rowloss,
    float* __restrict__ loss_part, StoreZ4 store_z4)
{
    const int tid = threadIdx.x;
    const long row0 = tile * BM;
    const float* out_t = out_saved + row0 * MLP_OUT;       // wave-uniform tile bases, 32-bit lane offsets
    const float* act_t = action + row0 * MLP_NACT;
    const float* olp_t = old_logp + row0;
    const float* adv_t = adv + row0;
    const float* tgt_t = target + row0;
    float* dz4_t = dz4 + row0 * MLP_OUT;
    const int col = tid & 31;
    const bool act = col < MLP_NACT;
    const float L = act ? sqrtf(var[col]) : 1.0f;
    const float inv_L = 1.0f / L, inv_var = act ? 1.0f / var[col] : 0.0f;       // one division each per thread, not per element
    float half_log_det = act ? logf(L) : 0.0f;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) half_log_det += __shfl_xor(half_log_det, o, 32);
#pragma unroll
    for (int k = 0; k < BM * MLP_OUT / THREADS; ++k) {
        const int row = (tid >> 5) + k * (THREADS / 32);
        const bool in = row < nvalid;
        const float y = in ? gload1<COH>(out_t, frag_off(row, col)) : 0.0f;                   // mean (cols 0..17), value (col 18)
        const float a = (in && act) ? act_t[row * MLP_NACT + col] : 0.0f;
        const float xj = act ? (a - y) * inv_L : 0.0f;
        float M = xj * xj;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) M += __shfl_xor(M, o, 32);
        float d = 0.0f, pol = 0.0f, hub = 0.0f;
        if (in) {
            const PpoRowLoss r = ppo_row_loss<false>(M, half_log_det, olp_t[row], adv_t[row], __shfl(y, MLP_NACT, 32), tgt_t[row],
                                                     inv_batch, clip);
            pol = r.pol;
            hub = r.hub;
            if (act) d = ppo_mean_dz4(r.c, a, y, inv_var);
            else if (col == MLP_NACT) d = r.dv;
            dz4_t[frag_off(row, col)] = d;
        }
        store_z4(row, col, d);
        if (col == 0) { rowloss[2 * row] = pol; rowloss[2 * row + 1] = hub; }
    }
    __syncthreads();
    if (tid < 32 && loss_part) tile_loss_sum<2>(rowloss, tid, loss_part + 2 * tile);
}

// The dX chain of one tile, written once over the arithmetic (ArithF32 / ArithB3, mlp_forward.inc) on the caller's LDS arena
// (Arith::BW_FLOATS): dZ2 | dZ3 operand tiles, dZ4 and the per-row loss terms where Arith puts them.
// `weights_t`: the packed transposed weights in Arith's form (PT fragments / PTB term planes).
template <class Arith, bool COH = false>
__device__ __forceinline__ void backward_body(
    float* lds, const long tile,
    const void* __restrict__ weights_t, const float* __restrict__ out_saved, const float* __restrict__ h1_saved,
    const float* __restrict__ h2_saved, const float* __restrict__ h3_saved,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, long n, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part)
{
    typedef typename Arith::E E;
    const typename Arith::W* const PT = static_cast<const typename Arith::W*>(weights_t);
    E* ldsZ2 = reinterpret_cast<E*>(lds);
    E* ldsZ3 = reinterpret_cast<E*>(lds + Arith::TILE);
    E* ldsZ4 = reinterpret_cast<E*>(lds + Arith::BW_Z4);
    float* rowloss = lds + Arith::BW_ROWLOSS;              // [32][2]: policy term, Huber term of each row
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR: weight bases become scalar
    const long row0 = tile * BM;
    const int nvalid = (int)(n - row0 < BM ? n - row0 : BM);                // rows of this tile that exist

    typename Arith::Head wt4, wt3;
    Arith::template prefetch<MLP_OUT>(wt4, PT + Arith::T4, wave, lane);
    HFrag<1> hf3;
    hfrag_load<MLP_H3, 1, COH>(hf3, h3_saved + row0 * MLP_H3, nvalid, wave * 32, lane);     // in flight during the loss phase

    // loss gradient at the outputs: dZ4 to HBM and to the LDS operand, the tile's loss partials (ends behind its barrier)
    ppo_loss_phase<COH>(tile, out_saved, action, old_logp, adv, target, var, nvalid, inv_batch, clip, dz4, rowloss, loss_part,
                        [&](int row, int col, float d) { Arith::template stage<MLP_OUT>(ldsZ4, row, col, d); });
    HFrag<1> hf2;
    {   // dA3 = dZ4 . W4  ->  dZ3
        typename Arith::Acc acc;
        Arith::template gemm<MLP_OUT>(wt4, PT + Arith::T4, wave, ldsZ4, acc, lane);
        Arith::template prefetch<MLP_H3>(wt3, PT + Arith::T3, wave, lane);    // both land during the epilogue + barrier
        hfrag_load<MLP_H2, 1, COH>(hf2, h2_saved + row0 * MLP_H2, nvalid, wave * 32, lane);
        Arith::template epilogue_dact<MLP_H3>(acc, hf3, wave * 32, ldsZ3, dz3 + row0 * MLP_H3, nvalid, lane);
    }
    __syncthreads();
    typename Arith::Head2 wt2;
    {   // dA2 = dZ3 . W3  ->  dZ2
        typename Arith::Acc acc;
        Arith::template gemm<MLP_H3>(wt3, PT + Arith::T3, wave, ldsZ3, acc, lane);
        Arith::dz1_prefetch(wt2, PT, wave * 2, lane);
        Arith::template epilogue_dact<MLP_H2>(acc, hf2, wave * 32, ldsZ2, dz2 + row0 * MLP_H2, nvalid, lane);
    }
    __syncthreads();
    // dA1 = dZ2 . W2  ->  dZ1 (no later GEMM reads it: HBM only)
    Arith::template dz1_stage<COH>(wt2, PT, ldsZ2, h1_saved, dz1, row0, nvalid, wave * 2, wave * 64, lane);
}

__global__ __launch_bounds__(THREADS, WGS_PER_CU) void mlp_backward_dx_kernel(
    const float* __restrict__ PT, const float* __restrict__ out_saved, const float* __restrict__ h1_saved,
    const float* __restrict__ h2_saved, const float* __restrict__ h3_saved,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, long n, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part)
{
    __shared__ __attribute__((aligned(16))) float lds[ArithF32::BW_FLOATS];
    backward_body<ArithF32>(lds, blockIdx.x, PT, out_saved, h1_saved, h2_saved, h3_saved, action, old_logp, adv, target, var, n,
                            inv_batch, clip, dz4, dz3, dz2, dz1, loss_part);
}

__global__ __launch_bounds__(THREADS, 2) void mlp_backward_dx_b3_kernel(
    const u16* __restrict__ PTB, const float* __restrict__ out_saved, const float* __restrict__ h1_saved,
    const float* __restrict__ h2_saved, const float* __restrict__ h3_saved,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, long n, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part)
{
    __shared__ __attribute__((aligned(16))) float lds[ArithB3::BW_FLOATS];
    backward_body<ArithB3>(lds, blockIdx.x, PTB, out_saved, h1_saved, h2_saved, h3_saved, action, old_logp, adv, target, var, n,
                           inv_batch, clip, dz4, dz3, dz2, dz1, loss_part);
}

// Forward and backward of one minibatch in ONE launch of 2 * tiles workgroups.  Both are row-local:
// workgroup b < tiles runs the forward of tile b and publishes flag[b]; workgroup tiles + b waits
// for that flag and runs the backward of tile b.  A launch of `tiles` workgroups at 3 per CU ends
// in a ragged tail (5 tiles per CU at 40 960 rows: the last third of its time runs one or two
// workgroups per CU); here the backward workgroups of the tiles that finished first fill the
// slots the forward frees, so only ONE tail is left per minibatch instead of two.
//
// LIVENESS rests on an assumption HIP does not promise: workgroups are dispatched in blockIdx order, so
// every forward workgroup is resident or finished before its consumer starts to poll.  If that ever
// fails the poll budget (~1 s) turns it into *err = 1 instead of a hang.
//
// VISIBILITY of the handed-off tensors (out / h1 / h2 / h3 of the tile) comes in two forms:
//  * COH = true (the default): inside the memory model as the microarchitecture guide measures it.
//    Every store of the handed-off bytes is an sc1 (write-through) store; every storing wave waits for
//    vmcnt(0); the workgroup's barrier; ONE lane's sc1 flag store.  The consumer polls the flag with sc1
//    loads from one lane, joins a workgroup barrier, and reads the tile ONLY with sc1 loads (they bypass
//    the reading CU's L1; L2 has no private copy to go stale because write-through stores do not leave one
//    on another XCD).  No placement assumption: producer and consumer may sit on any two CUs.
//  * COH = false (`FLY_FWD_BWD_HANDOFF=xcd`): plain stores and loads, no cache maintenance at all --
//    producer and consumer must then share an L2, i.e. an XCD.  Workgroups go round-robin over the 8
//    XCDs and the consumer range starts at a multiple of 8, so b and pad_tiles + b land together; the
//    producer publishes its XCC id with the flag and the consumer raises *err = 2 on a mismatch.  This
//    leans on dispatch placement and on the consumer CU's L1 not holding the lines (it is invalidated at
//    kernel start and nothing on the CU has read this tile's rows since): speed-only properties the
//    guide says must never carry correctness, so it is kept as an A/B measurement, not as the default.
// In both forms a consumer that gives up writes nothing: *err stays set, the optimizer kernels
// (mlp_grad_reduce / mlp_adam) turn into no-ops while it is set, and the host redoes the step with two
// launches (PPO._update_hip) -- weights and moments never see a stale gradient.
// B3: the bf16x3 arithmetic (PF/PT then point at the 16-bit term planes PB/PTB)
template <bool STAMP, bool B3, bool COH>
__global__ __launch_bounds__(THREADS, B3 ? 3 : WGS_PER_CU) void mlp_fwd_bwd_kernel(
    const float* __restrict__ P, const void* __restrict__ PF, const void* __restrict__ PT,
    const float* __restrict__ x, long n, float* __restrict__ out_save, float* __restrict__ h1_save,
    float* __restrict__ h2_save, float* __restrict__ h3_save,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part, int* __restrict__ flags, int epoch, int* __restrict__ err,
    unsigned long long* __restrict__ stamps, int consumer_shift)
{
    typedef ArithOf<B3> Arith;
    constexpr int FB_LDS_FLOATS = Arith::FWD_FLOATS > Arith::BW_FLOATS ? Arith::FWD_FLOATS : Arith::BW_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds[FB_LDS_FLOATS];
    // bf16x3: the consumer's wait result lives in the arena's last word, past everything the backward
    // body uses (a separate word would push the allocation over a third of the CU's LDS)
    static_assert(!B3 || FB_LDS_FLOATS > Arith::BW_FLOATS, "room for the flag word");
    __shared__ int ok_word;
    int& ok = B3 ? *reinterpret_cast<int*>(lds + FB_LDS_FLOATS - 1) : ok_word;
    if (STAMP && threadIdx.x == 0) stamps[4L * blockIdx.x] = realtime_cu();
    const long tiles = (n + BM - 1) / BM;
    // consumers start at a multiple of 8: same XCD as their producer (`consumer_shift` is 0 outside the
    // test that forces a mismatch)
    const long pad_tiles = ((tiles + 7) & ~7L) + consumer_shift;
    if ((long)blockIdx.x < pad_tiles) {
        const long tile = blockIdx.x;
        if (tile >= tiles) return;
        forward_body<Arith, false, COH>(lds, tile, tiles, P, PF, x, n, nullptr, nullptr, out_save, h1_save, h2_save, h3_save, nullptr,
                                        nullptr, nullptr, nullptr, nullptr);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave: its stores are acknowledged (inline asm: the
        __syncthreads();                                  // compiler cannot drop it as "scoreboard provably empty")
        if (threadIdx.x == 0) {
            const int xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf;
            __hip_atomic_store(flags + tile, (epoch << 4) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (STAMP) stamps[4L * blockIdx.x + 1] = realtime_cu();
        }
    } else {
        const long tile = (long)blockIdx.x - pad_tiles;
        if (tile >= tiles) return;
        if (threadIdx.x == 0) {
            int state = 1;                                 // 0 ok, 1 flag never came, 2 producer on another XCD
            for (int poll = 0; poll < (1 << 21); ++poll) {
                const int f = __hip_atomic_load(flags + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((f >> 4) == epoch) {
                    state = (COH || (f & 0xf) == (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf)) ? 0 : 2;
                    break;
                }
                __builtin_amdgcn_s_sleep(16);
            }
            ok = state;
            if (state) atomicMax(err, state);
        }
        __syncthreads();
        if (ok) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");     // ordering only: no cache maintenance (see above)
        if (STAMP && threadIdx.x == 0) stamps[4L * blockIdx.x + 2] = realtime_cu();
        backward_body<Arith, COH>(lds, tile, PT, out_save, h1_save, h2_save, h3_save, action, old_logp, adv, target, var, n, inv_batch,
                                  clip, dz4, dz3, dz2, dz1, loss_part);
        if (STAMP && threadIdx.x == 0) {
            __builtin_amdgcn_s_waitcnt(0);
            stamps[4L * blockIdx.x + 1] = realtime_cu();
        }
    }
}
