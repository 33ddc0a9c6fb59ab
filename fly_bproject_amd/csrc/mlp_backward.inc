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
// dZ = dA * ELU'(H).  H is read from the saved activations in exactly the accumulator layout (a
// lane owns row lane&31 and four consecutive columns per register group): one 16-byte load per
// group, requested before the GEMM whose epilogue consumes it.  The four loads of a column tile
// touch one 128-byte line per row, so L1 serves three of them.
template <int NT>
struct HFrag { float4 v[NT][4]; };

template <int N, int NT, bool COH = false>
__device__ __forceinline__ void hfrag_load(HFrag<NT>& hf, const float* __restrict__ htile, int nvalid, int col0, int lane)
{
    // the saved activations are in tile-fragment order (see below): this wave's four loads of a
    // column tile are four contiguous KiB.  Rows past the end of the batch read whatever the
    // (allocated) rest of the last tile holds: their results are never stored and a row of an
    // MFMA only feeds the same row.
    const int go = (col0 / 32) * 1024 + lane * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) hf.v[t][g] = gload4<COH>(htile, go + t * 1024 + g * 256);
}

// writes dZ to the gradient rows in HBM and (lds_out != nullptr) to the LDS tile the next GEMM reads
template <int N, int NT>
__device__ __forceinline__ void epilogue_dact(const f32x16 (&acc)[NT], const HFrag<NT>& hf, int col0, float* lds_out,
                                              float* __restrict__ gtile, int nvalid, int lane)
{
    const int r = lane & 31;
    float4 z[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int nb = col0 + 32 * t + acc_n(g, lane);
            const float4 hv = hf.v[t][g];
            z[t][g].x = dact(acc[t][4 * g + 0], hv.x);
            z[t][g].y = dact(acc[t][4 * g + 1], hv.y);
            z[t][g].z = dact(acc[t][4 * g + 2], hv.z);
            z[t][g].w = dact(acc[t][4 * g + 3], hv.w);
            if (lds_out) *reinterpret_cast<float4*>(lds_out + r * (N + 4) + nb) = z[t][g];
        }
    }
    if (r < nvalid) {
        float* gl = gtile + (col0 / 32) * 1024 + lane * 4;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) GSTORE4(gl + t * 1024 + g * 256, z[t][g]);
    }
}

constexpr int BW_Z2 = 0;                                   // [32][132]
constexpr int BW_Z3 = BW_Z2 + BM * (MLP_H2 + 4);           // [32][132]
constexpr int BW_Z4 = BW_Z3 + BM * (MLP_H3 + 4);           // [32][36]
constexpr int BW_TAIL = BW_Z4 + BM * (MLP_OUT + 4);        // [32][2] per-row loss terms
constexpr int BW_FLOATS = BW_TAIL + 2 * BM;                // 38.9 KB

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

template <bool COH = false>
__device__ __forceinline__ void backward_body(
    float* lds, const long tile,
    const float* __restrict__ PT, const float* __restrict__ out_saved, const float* __restrict__ h1_saved,
    const float* __restrict__ h2_saved, const float* __restrict__ h3_saved,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, long n, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part)
{
    float* ldsZ2 = lds + BW_Z2;
    float* ldsZ3 = lds + BW_Z3;
    float* ldsZ4 = lds + BW_Z4;
    float* rowloss = lds + BW_TAIL;                        // [32][2]: policy term, Huber term of each row
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR: weight bases become scalar
    const long row0 = tile * BM;
    const int nvalid = (int)(n - row0 < BM ? n - row0 : BM);                // rows of this tile that exist

    WeightHead<1> wt4, wt3;
    gemm_prefetch<MLP_OUT, 1>(wt4, PT + MLP_OFF_TF4, wave, lane);
    HFrag<1> hf3;
    hfrag_load<MLP_H3, 1, COH>(hf3, h3_saved + row0 * MLP_H3, nvalid, wave * 32, lane);     // in flight during the loss phase

    // loss gradient at the outputs: dZ4 to HBM and to the LDS operand, the tile's loss partials (ends behind its barrier)
    ppo_loss_phase<COH>(tile, out_saved, action, old_logp, adv, target, var, nvalid, inv_batch, clip, dz4, rowloss, loss_part,
                        [&](int row, int col, float d) { ldsZ4[row * (MLP_OUT + 4) + col] = d; });
    HFrag<1> hf2;
    {   // dA3 = dZ4 . W4  ->  dZ3
        f32x16 acc[1];
        tile_gemm<MLP_OUT, 1>(wt4, PT + MLP_OFF_TF4, wave, ldsZ4, acc, lane);
        gemm_prefetch<MLP_H3, 1>(wt3, PT + MLP_OFF_TF3, wave, lane);          // both land during the epilogue + barrier
        hfrag_load<MLP_H2, 1, COH>(hf2, h2_saved + row0 * MLP_H2, nvalid, wave * 32, lane);
        epilogue_dact<MLP_H3, 1>(acc, hf3, wave * 32, ldsZ3, dz3 + row0 * MLP_H3, nvalid, lane);
    }
    __syncthreads();
    WeightHead<2> wt2;
    HFrag<2> hf1;
    {   // dA2 = dZ3 . W3  ->  dZ2
        f32x16 acc[1];
        tile_gemm<MLP_H3, 1>(wt3, PT + MLP_OFF_TF3, wave, ldsZ3, acc, lane);
        gemm_prefetch<MLP_H2, 2>(wt2, PT + MLP_OFF_TF2, wave * 2, lane);
        epilogue_dact<MLP_H2, 1>(acc, hf2, wave * 32, ldsZ2, dz2 + row0 * MLP_H2, nvalid, lane);
    }
    __syncthreads();
    {   // dA1 = dZ2 . W2  ->  dZ1 (no later GEMM reads it: HBM only)
        hfrag_load<MLP_H1, 2, COH>(hf1, h1_saved + row0 * MLP_H1, nvalid, wave * 64, lane);       // lands during the MFMAs
        f32x16 acc[2];
        tile_gemm<MLP_H2, 2>(wt2, PT + MLP_OFF_TF2, wave * 2, ldsZ2, acc, lane);
        epilogue_dact<MLP_H1, 2>(acc, hf1, wave * 64, nullptr, dz1 + row0 * MLP_H1, nvalid, lane);
    }
}

// dZ = (hi + lo) * ELU'(H) of the bf16x3 path: fp32 rows to HBM, three bf16 terms to the next GEMM's LDS tile
template <int N>
__device__ __forceinline__ void epilogue_dact_b3(const f32x16& hi, const f32x16& lo, const HFrag<1>& hf, int col0,
                                                 u16* lds_plane0, float* __restrict__ gtile, int nvalid, int lane)
{
    const int r = lane & 31;
    float4 z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 hv = hf.v[0][g];
        z[g].x = dact(hi[4 * g + 0] + lo[4 * g + 0], hv.x);
        z[g].y = dact(hi[4 * g + 1] + lo[4 * g + 1], hv.y);
        z[g].z = dact(hi[4 * g + 2] + lo[4 * g + 2], hv.z);
        z[g].w = dact(hi[4 * g + 3] + lo[4 * g + 3], hv.w);
        if (lds_plane0) store_split4<N>(lds_plane0, r, col0 + acc_n(g, lane), z[g]);
    }
    if (r < nvalid) {
        float* gl = gtile + (col0 / 32) * 1024 + lane * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) GSTORE4(gl + g * 256, z[g]);
    }
}

constexpr int BW_B3_LDS_FLOATS = 2 * B3_TILE_FLOATS + 2 * BM;

template <bool COH = false>
__device__ __forceinline__ void backward_body_b3(
    float* lds, const long tile,
    const u16* __restrict__ PTB, const float* __restrict__ out_saved, const float* __restrict__ h1_saved,
    const float* __restrict__ h2_saved, const float* __restrict__ h3_saved,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, long n, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part)
{
    u16* ldsZ2 = reinterpret_cast<u16*>(lds);                     // dZ2: three [32][136] term planes
    u16* ldsZ3 = reinterpret_cast<u16*>(lds + B3_TILE_FLOATS);    // dZ3: three [32][136] term planes
    u16* ldsZ4 = ldsZ2;                                           // dZ4 ([32][40] planes) is dead before dZ2 is written
    float* rowloss = lds + 2 * B3_TILE_FLOATS;                        // [32][2]: policy term, Huber term of each row
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR: weight bases become scalar
    const long row0 = tile * BM;
    const int nvalid = (int)(n - row0 < BM ? n - row0 : BM);                // rows of this tile that exist

    WeightHead3 wt4, wt3;
    gemm_prefetch_b3<MLP_OUT>(wt4, PTB + MLP_OFF_PTB4, wave, lane);
    HFrag<1> hf3;
    hfrag_load<MLP_H3, 1, COH>(hf3, h3_saved + row0 * MLP_H3, nvalid, wave * 32, lane);     // in flight during the loss phase

    // loss gradient at the outputs: dZ4 to HBM and to the LDS operand, the tile's loss partials (ends behind its barrier)
    ppo_loss_phase<COH>(tile, out_saved, action, old_logp, adv, target, var, nvalid, inv_batch, clip, dz4, rowloss, loss_part,
                        [&](int row, int col, float d) {
                            u16 sa, sb, sc;
                            split3(d, sa, sb, sc);
                            u16* q = ldsZ4 + row * (MLP_OUT + B3_PAD) + col;
                            q[0] = sa; q[b3_plane<MLP_OUT>()] = sb; q[2 * b3_plane<MLP_OUT>()] = sc;
                        });
    HFrag<1> hf2;
    {   // dA3 = dZ4 . W4  ->  dZ3
        f32x16 hi, lo;
        tile_gemm_b3<MLP_OUT>(wt4, PTB + MLP_OFF_PTB4, wave, ldsZ4, hi, lo, lane);
        gemm_prefetch_b3<MLP_H3>(wt3, PTB + MLP_OFF_PTB3, wave, lane);        // both land during the epilogue + barrier
        hfrag_load<MLP_H2, 1, COH>(hf2, h2_saved + row0 * MLP_H2, nvalid, wave * 32, lane);
        epilogue_dact_b3<MLP_H3>(hi, lo, hf3, wave * 32, ldsZ3, dz3 + row0 * MLP_H3, nvalid, lane);
    }
    __syncthreads();
    WeightHead3 wt2;
    HFrag<1> hf1;
    {   // dA2 = dZ3 . W3  ->  dZ2
        f32x16 hi, lo;
        tile_gemm_b3<MLP_H3>(wt3, PTB + MLP_OFF_PTB3, wave, ldsZ3, hi, lo, lane);
        gemm_prefetch_b3<MLP_H2>(wt2, PTB + MLP_OFF_PTB2, wave * 2, lane);
        epilogue_dact_b3<MLP_H2>(hi, lo, hf2, wave * 32, ldsZ2, dz2 + row0 * MLP_H2, nvalid, lane);
    }
    __syncthreads();
    {   // dA1 = dZ2 . W2  ->  dZ1 (no later GEMM reads it: HBM only): this wave's two column tiles in turn
        WeightHead3 wt2b;
        HFrag<1> hf1b;
        hfrag_load<MLP_H1, 1, COH>(hf1, h1_saved + row0 * MLP_H1, nvalid, wave * 64, lane);              // lands during the MFMAs
        f32x16 hi, lo;
        tile_gemm_b3<MLP_H2>(wt2, PTB + MLP_OFF_PTB2, wave * 2, ldsZ2, hi, lo, lane);
        gemm_prefetch_b3<MLP_H2>(wt2b, PTB + MLP_OFF_PTB2, wave * 2 + 1, lane);
        hfrag_load<MLP_H1, 1, COH>(hf1b, h1_saved + row0 * MLP_H1, nvalid, wave * 64 + 32, lane);
        epilogue_dact_b3<MLP_H1>(hi, lo, hf1, wave * 64, nullptr, dz1 + row0 * MLP_H1, nvalid, lane);
        tile_gemm_b3<MLP_H2>(wt2b, PTB + MLP_OFF_PTB2, wave * 2 + 1, ldsZ2, hi, lo, lane);
        epilogue_dact_b3<MLP_H1>(hi, lo, hf1b, wave * 64 + 32, nullptr, dz1 + row0 * MLP_H1, nvalid, lane);
    }
}

__global__ __launch_bounds__(THREADS, WGS_PER_CU) void mlp_backward_dx_kernel(
    const float* __restrict__ PT, const float* __restrict__ out_saved, const float* __restrict__ h1_saved,
    const float* __restrict__ h2_saved, const float* __restrict__ h3_saved,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, long n, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part)
{
    __shared__ __attribute__((aligned(16))) float lds[BW_FLOATS];
    backward_body<false>(lds, blockIdx.x, PT, out_saved, h1_saved, h2_saved, h3_saved, action,
                  old_logp, adv, target, var, n, inv_batch, clip, dz4, dz3, dz2, dz1, loss_part);
}

__global__ __launch_bounds__(THREADS, 2) void mlp_backward_dx_b3_kernel(
    const u16* __restrict__ PTB, const float* __restrict__ out_saved, const float* __restrict__ h1_saved,
    const float* __restrict__ h2_saved, const float* __restrict__ h3_saved,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, long n, float inv_batch, float clip,
    float* __restrict__ dz4, float* __restrict__ dz3, float* __restrict__ dz2, float* __restrict__ dz1,
    float* __restrict__ loss_part)
{
    __shared__ __attribute__((aligned(16))) float lds[BW_B3_LDS_FLOATS];
    backward_body_b3<false>(lds, blockIdx.x, PTB, out_saved, h1_saved, h2_saved, h3_saved, action, old_logp, adv, target, var, n,
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
constexpr int FB_LDS_FLOATS = FWD_LDS_FLOATS > BW_FLOATS ? FWD_LDS_FLOATS : BW_FLOATS;

constexpr int FB_B3_LDS_FLOATS = FWD_B3_LDS_FLOATS > BW_B3_LDS_FLOATS ? FWD_B3_LDS_FLOATS : BW_B3_LDS_FLOATS;

// B3: the bf16x3 GEMM bodies (PF/PT then point at the 16-bit term planes PB/PTB)
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
    __shared__ __attribute__((aligned(16))) float lds[B3 ? FB_B3_LDS_FLOATS : FB_LDS_FLOATS];
    // bf16x3: the consumer's wait result lives in the arena's last word, past everything the backward
    // body uses (a separate word would push the allocation over a third of the CU's LDS)
    static_assert(FB_B3_LDS_FLOATS > BW_B3_LDS_FLOATS, "room for the flag word");
    __shared__ int ok_word;
    int& ok = B3 ? *reinterpret_cast<int*>(lds + FB_B3_LDS_FLOATS - 1) : ok_word;
    if (STAMP && threadIdx.x == 0) stamps[4L * blockIdx.x] = realtime_cu();
    const long tiles = (n + BM - 1) / BM;
    // consumers start at a multiple of 8: same XCD as their producer (`consumer_shift` is 0 outside the
    // test that forces a mismatch)
    const long pad_tiles = ((tiles + 7) & ~7L) + consumer_shift;
    if ((long)blockIdx.x < pad_tiles) {
        const long tile = blockIdx.x;
        if (tile >= tiles) return;
        if (B3)
            forward_body_b3<false, COH>(lds, tile, tiles, P, static_cast<const u16*>(PF), x, n, nullptr, nullptr, out_save, h1_save,
                                        h2_save, h3_save, nullptr, nullptr, nullptr, nullptr, nullptr);
        else
            forward_body<false, COH>(lds, tile, tiles, P, static_cast<const float*>(PF), x, n, nullptr, nullptr, out_save, h1_save,
                                     h2_save, h3_save, nullptr, nullptr, nullptr, nullptr, nullptr);
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
        if (B3)
            backward_body_b3<COH>(lds, tile, static_cast<const u16*>(PT), out_save, h1_save, h2_save, h3_save, action, old_logp, adv,
                             target, var, n, inv_batch, clip, dz4, dz3, dz2, dz1, loss_part);
        else
            backward_body<COH>(lds, tile, static_cast<const float*>(PT), out_save, h1_save, h2_save, h3_save, action, old_logp, adv,
                          target, var, n, inv_batch, clip, dz4, dz3, dz2, dz1, loss_part);
        if (STAMP && threadIdx.x == 0) {
            __builtin_amdgcn_s_waitcnt(0);
            stamps[4L * blockIdx.x + 1] = realtime_cu();
        }
    }
}
