// mlp_forward.inc — the two MFMA arithmetics (fp32 MFMA, bf16x3) as compile-time descriptions, the fused four-layer forward
// body written once over them, and its kernels.
// The fp32 tile kernel fits four workgroups per CU (<= 40 KB of LDS and <= 128 VGPRs each), the bf16x3 one three.
constexpr int WGS_PER_CU = 4;
constexpr int PERSIST_GRID = 256 * WGS_PER_CU;       // persistent launches: every slot of the chip
constexpr int LB1 = 0, LB2 = MLP_H1, LB3 = LB2 + MLP_H2, LB4 = LB3 + MLP_H3, LSD = LB4 + MLP_OUT, LLG = LSD + 32;
constexpr int XV = (BM * MLP_IN / 4 + THREADS - 1) / THREADS;       // float4 per thread for one x tile (584 / 256 -> 3)

// What an arithmetic is to forward_body and backward_body (mlp_backward.inc): types, constants and forwarding members only,
// everything resolved at compile time.  They live here and not beside the GEMMs they wrap because mlp_gemm.inc is shared with
// translation units that do not know the policy's packed layout (mlp_layout.h).
//   W / E / Head / Acc    packed weight element, LDS operand element, the prefetched head of a GEMM's weights, its accumulator(s)
//   TILE                  floats of one LDS operand tile: the forward arena is tile A | tile B | BIAS floats of biases
//   F1..F4, F2B, T2..T4   the layers' offsets in the packed forward / transposed weights (F2B: the second K half of W2, from F2)
//   prefetch / gemm / epilogue_elu / epilogue_dact   the helpers of mlp_gemm.inc
//   stage<K>              one fp32 element into a [32][K] LDS operand tile (the staged input, dZ4)
//   W4 / NW4              this wave's layer-4 weight fragments (the split-K block itself is in forward_body)
//   Head2 / dz1_prefetch / dz1_stage   the backward's last stage (dA1 = dZ2 . W2 -> dZ1), where the two really differ
// The accumulators and fragments are bare arrays and the members only forward: a struct around an accumulator, or the layer-4
// block as a member, changes how the compiler splits these arrays into registers and with it the kernels' code.
struct ArithF32 {
    typedef float W;
    typedef float E;                                     // [32][K + 4] floats
    typedef WeightHead<1> Head;
    typedef WeightHead<2> Head2;
    typedef f32x16 Acc[1];
    typedef float4 W4;                                   // layer-4 weights of this wave's k range: four k-quads
    static constexpr int NW4 = 4;
    static constexpr bool BF16X3 = false;
    static constexpr bool LDS_HANDOFF = false;           // x_tile_lds / act_tile_lds / biases_resident: not supported
    static constexpr int TILE = BM * (MLP_H2 + 4);       // one 128-column half of H1 / H3; X0, H2, the split-K partials
    static constexpr int BIAS = LLG + 32;                // biases + sampling constants (2.4 KB)
    static constexpr int FWD_FLOATS = 2 * TILE + BIAS;
    static constexpr int BW_Z4 = 2 * TILE;               // dZ2 [32][132] | dZ3 [32][132] | dZ4 [32][36] | per-row loss terms [32][2]
    static constexpr int BW_ROWLOSS = BW_Z4 + BM * (MLP_OUT + 4);
    static constexpr int BW_FLOATS = BW_ROWLOSS + 2 * BM;     // 38.9 KB
    static constexpr int F1 = MLP_OFF_F1, F2 = MLP_OFF_F2, F2B = MLP_H2 * (MLP_H1 / 2), F3 = MLP_OFF_F3, F4 = MLP_OFF_F4;
    static constexpr int T2 = MLP_OFF_TF2, T3 = MLP_OFF_TF3, T4 = MLP_OFF_TF4;

    template <int K>
    static __device__ __forceinline__ void prefetch(Head& w, const W* Wf, int tile0, int lane) { gemm_prefetch<K, 1>(w, Wf, tile0, lane); }
    template <int K, bool ZERO = true>
    static __device__ __forceinline__ void gemm(const Head& w, const W* Wf, int tile0, const E* lds_in, Acc& acc, int lane)
    {
        tile_gemm<K, 1, ZERO>(w, Wf, tile0, lds_in, acc, lane);
    }
    template <int N, int NG, bool COH>
    static __device__ __forceinline__ void epilogue_elu(const Acc& acc, const float* bias, int col0, E* lds_out, int lane, float* gtile, int nvalid)
    {
        ::epilogue_elu<N, 1, NG, COH>(acc, bias, col0, lds_out, lane, gtile, nvalid);
    }
    template <int N>
    static __device__ __forceinline__ void epilogue_dact(const Acc& acc, const HFrag<1>& hf, int col0, E* lds_out, float* gtile, int nvalid, int lane)
    {
        ::epilogue_dact<N, 1>(acc, hf, col0, lds_out, gtile, nvalid, lane);
    }
    template <int K>
    static __device__ __forceinline__ void stage(E* tile, int row, int col, float v) { tile[row * (K + 4) + col] = v; }

    static __device__ __forceinline__ void dz1_prefetch(Head2& w, const W* PT, int tile0, int lane) { gemm_prefetch<MLP_H2, 2>(w, PT + T2, tile0, lane); }
    // both column tiles of this wave in one NT = 2 GEMM
    template <bool COH>
    static __device__ __forceinline__ void dz1_stage(const Head2& wt2, const W* PT, const E* ldsZ2, const float* h1_saved, float* dz1,
                                                     long row0, int nvalid, int tile0, int col0, int lane)
    {
        HFrag<2> hf1;
        hfrag_load<MLP_H1, 2, COH>(hf1, h1_saved + row0 * MLP_H1, nvalid, col0, lane);       // lands during the MFMAs
        f32x16 acc[2];
        tile_gemm<MLP_H2, 2>(wt2, PT + T2, tile0, ldsZ2, acc, lane);
        ::epilogue_dact<MLP_H1, 2>(acc, hf1, col0, nullptr, dz1 + row0 * MLP_H1, nvalid, lane);
    }
};

// bf16x3: activations live in LDS as three bf16 term planes ([32][K + 8] each)
constexpr int B3_TILE_FLOATS = 3 * b3_plane<MLP_H2>() / 2;        // a [32][128] tile as three planes, in floats
struct ArithB3 {
    typedef u16 W;
    typedef u16 E;
    typedef WeightHead3 Head;
    typedef WeightHead3 Head2;
    typedef f32x16 Acc[2];                               // hi (the large term w0 x0), lo (the five small ones)
    typedef Frag3 W4;                                    // layer-4 weights of this wave's two k blocks
    static constexpr int NW4 = 2;
    static constexpr bool BF16X3 = true;
    static constexpr bool LDS_HANDOFF = true;
    static constexpr int TILE = B3_TILE_FLOATS;          // H1 half / H3; X ([32][88] planes), H2, the fp32 split-K partials
    static constexpr int BIAS = LB4;                     // b1 | b2 | b3 only: 54 272 B in all, three workgroups per CU
    static constexpr int FWD_FLOATS = 2 * TILE + BIAS;
    static constexpr int BW_Z4 = 0;                      // dZ2 | dZ3 | per-row loss terms; dZ4 ([32][40] planes) is dead before dZ2 is written
    static constexpr int BW_ROWLOSS = 2 * TILE;
    static constexpr int BW_FLOATS = BW_ROWLOSS + 2 * BM;
    static constexpr int F1 = MLP_OFF_PB1, F2 = MLP_OFF_PB2, F2B = 3 * MLP_H2 * (MLP_H1 / 2), F3 = MLP_OFF_PB3, F4 = MLP_OFF_PB4;
    static constexpr int T2 = MLP_OFF_PTB2, T3 = MLP_OFF_PTB3, T4 = MLP_OFF_PTB4;

    template <int K>
    static __device__ __forceinline__ void prefetch(Head& w, const W* Wb, int tile0, int lane) { gemm_prefetch_b3<K>(w, Wb, tile0, lane); }
    template <int K, bool ZERO = true>
    static __device__ __forceinline__ void gemm(const Head& w, const W* Wb, int tile0, const E* lds_in, Acc& acc, int lane)
    {
        tile_gemm_b3<K, ZERO>(w, Wb, tile0, lds_in, acc[0], acc[1], lane);
    }
    template <int N, int NG, bool COH>
    static __device__ __forceinline__ void epilogue_elu(const Acc& acc, const float* bias, int col0, E* lds_out, int lane, float* gtile, int nvalid)
    {
        epilogue_elu_b3<N, NG, COH>(acc[0], acc[1], bias, col0, lds_out, lane, gtile, nvalid);
    }
    template <int N>
    static __device__ __forceinline__ void epilogue_dact(const Acc& acc, const HFrag<1>& hf, int col0, E* lds_out, float* gtile, int nvalid, int lane)
    {
        epilogue_dact_b3<N>(acc[0], acc[1], hf, col0, lds_out, gtile, nvalid, lane);
    }
    template <int K>
    static __device__ __forceinline__ void stage(E* tile, int row, int col, float v)
    {
        u16 sa, sb, sc;
        split3(v, sa, sb, sc);
        u16* q = tile + row * (K + B3_PAD) + col;
        q[0] = sa; q[b3_plane<K>()] = sb; q[2 * b3_plane<K>()] = sc;
    }

    static __device__ __forceinline__ void dz1_prefetch(Head2& w, const W* PTB, int tile0, int lane) { gemm_prefetch_b3<MLP_H2>(w, PTB + T2, tile0, lane); }
    // this wave's two column tiles in turn, the second head prefetched under the first GEMM
    template <bool COH>
    static __device__ __forceinline__ void dz1_stage(const Head2& wt2, const W* PTB, const E* ldsZ2, const float* h1_saved, float* dz1,
                                                     long row0, int nvalid, int tile0, int col0, int lane)
    {
        WeightHead3 wt2b;
        HFrag<1> hf1, hf1b;
        hfrag_load<MLP_H1, 1, COH>(hf1, h1_saved + row0 * MLP_H1, nvalid, col0, lane);              // lands during the MFMAs
        f32x16 hi, lo;
        tile_gemm_b3<MLP_H2>(wt2, PTB + T2, tile0, ldsZ2, hi, lo, lane);
        gemm_prefetch_b3<MLP_H2>(wt2b, PTB + T2, tile0 + 1, lane);
        hfrag_load<MLP_H1, 1, COH>(hf1b, h1_saved + row0 * MLP_H1, nvalid, col0 + 32, lane);
        epilogue_dact_b3<MLP_H1>(hi, lo, hf1, col0, nullptr, dz1 + row0 * MLP_H1, nvalid, lane);
        tile_gemm_b3<MLP_H2>(wt2b, PTB + T2, tile0 + 1, ldsZ2, hi, lo, lane);
        epilogue_dact_b3<MLP_H1>(hi, lo, hf1b, col0 + 32, nullptr, dz1 + row0 * MLP_H1, nvalid, lane);
    }
};
template <bool B3> using ArithOf = std::conditional_t<B3, ArithB3, ArithF32>;

// x [n][73] -> out [n][32] (cols 0..17 = mean after ELU, col 18 = value, rest 0).
// mu_out [n][18] / v_out [n] / h*_save are optional.
// The body walks tiles first_tile, first_tile + tile_stride, ... (< ntiles) on the caller's LDS arena (Arith::FWD_FLOATS).  A
// persistent caller (the fp32 kernel: at most WGS_PER_CU workgroups per CU) passes blockIdx.x / gridDim.x: the NEXT tile's input
// rows are fetched into registers (16-byte loads: a 32x73 tile is one contiguous, 16-byte aligned block) while the current tile
// computes, so the ~5 us HBM round trip that used to open every workgroup is hidden.  A one-tile caller passes a stride no tile
// index reaches.
// `weights`: the packed forward weights in Arith's form (PF fragments / PB term planes).
// NORM: the input rows are normalised (obs_norm_apply) under the table norm_tab (LDS, published by a barrier before the call)
// on their way into LDS; the rows in HBM stay raw.
// Arith::LDS_HANDOFF only (the one-launch rollout; compiled out otherwise):
//   biases_resident: an earlier call on the same arena has left b1 | b2 | b3 in `ldsBias` and nothing has touched them since
//   x_tile_lds: the FIRST tile's rows lie in LDS as fp32 [32][73] (the env step of the same workgroup left them there, at the
//     start of the arena: read before anything of this body overwrites it) -- no round trip through L2
//   act_tile_lds: the sampled, clipped actions of a tile are ALSO left in LDS as [32][18] for the env step that follows
template <class Arith, bool STAMP, bool COH = false, bool NORM = false>
__device__ __forceinline__ void forward_body(
    float* lds, const long first_tile, const long tile_stride,
    const float* __restrict__ P, const void* __restrict__ weights, const float* __restrict__ x, long n,
    float* __restrict__ mu_out, float* __restrict__ v_out, float* __restrict__ out_save,
    float* __restrict__ h1_save, float* __restrict__ h2_save, float* __restrict__ h3_save,
    const float* __restrict__ smp_eps, const float* __restrict__ smp_var, float* __restrict__ smp_act,
    float* __restrict__ smp_logp, unsigned long long* __restrict__ stamps_base,
    const int smp_var_steps = 0, const float smp_var_decay = 0.0f, const float smp_var_min = 0.0f,
    const float* norm_tab = nullptr,
    const float* x_tile_lds = nullptr, float* act_tile_lds = nullptr, const bool biases_resident = false)
{
    typedef typename Arith::E E;
    typedef typename Arith::Acc Acc;
    const typename Arith::W* const PF = static_cast<const typename Arith::W*>(weights);
    unsigned long long* stamps = stamps_base;
    E* ldsA = reinterpret_cast<E*>(lds);
    float* ldsBf = lds + Arith::TILE;                      // tile B as the fp32 split-K partials
    E* ldsB = reinterpret_cast<E*>(ldsBf);
    float* ldsBias = lds + 2 * Arith::TILE;   // b1 | b2 | b3 (| b4 | sqrt(var) | log sqrt(var)): read by every epilogue
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR: weight bases become scalar
    const long ntiles = (n + BM - 1) / BM;
    const long total = n * MLP_IN;

    float4 xr[XV];
    auto x_load = [&](long tile) {
        if (Arith::LDS_HANDOFF && x_tile_lds != nullptr && tile == first_tile) {       // (wave-uniform)
#pragma unroll
            for (int u = 0; u < XV; ++u)
                xr[u] = tid + u * THREADS < BM * MLP_IN / 4 ? reinterpret_cast<const float4*>(x_tile_lds)[tid + u * THREADS]
                                                            : make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
        const long base = tile * (BM * MLP_IN);
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const long f = base + 4L * (tid + u * THREADS);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tid + u * THREADS < BM * MLP_IN / 4) {
                if (f + 3 < total) v = *reinterpret_cast<const float4*>(x + f);
                else {
                    if (f < total) v.x = x[f];
                    if (f + 1 < total) v.y = x[f + 1];
                    if (f + 2 < total) v.z = x[f + 2];
                }
            }
            xr[u] = v;
        }
    };
    auto x_store = [&](int tid) {   // registers -> ldsB as a [32][80] operand tile; pad columns 73..79 zeroed
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int i4 = tid + u * THREADS;
            if (i4 < BM * MLP_IN / 4) {
                const float e[4] = {xr[u].x, xr[u].y, xr[u].z, xr[u].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 4 * i4 + j;
                    const int rr = f / MLP_IN, cc = f - rr * MLP_IN;
                    Arith::template stage<MLP_IN_PAD>(
                        ldsB, rr, cc, NORM ? obs_norm_apply(e[j], norm_tab[cc], norm_tab[MLP_IN + cc], norm_tab[2 * MLP_IN]) : e[j]);
                }
            }
        }
        if (tid < BM * (MLP_IN_PAD - MLP_IN)) {
            const int rr = tid / (MLP_IN_PAD - MLP_IN), cc = MLP_IN + tid - rr * (MLP_IN_PAD - MLP_IN);
            Arith::template stage<MLP_IN_PAD>(ldsB, rr, cc, 0.0f);
        }
    };

    long tile = first_tile;
    if (tile < ntiles) x_load(tile);
    if (!(Arith::LDS_HANDOFF && biases_resident)) {   // biases -> LDS once per workgroup; the first tile's barrier publishes them
        ldsBias[LB1 + tid] = P[MLP_OFF_B1 + tid];
        if (tid < MLP_H2) ldsBias[LB2 + tid] = P[MLP_OFF_B2 + tid];
        else ldsBias[LB3 + tid - MLP_H2] = P[MLP_OFF_B3 + tid - MLP_H2];
    }
    // the last phase's per-column constants b4, sqrt(var), log sqrt(var).  fp32: in the LDS bias block, published with the
    // biases.  bf16x3: this thread's output column is the same in every tile, so they stay in registers (the LDS budget of
    // that path is exactly three workgroups per CU)
    float b4v = 0.0f, smpL = 1.0f, smpLog = 0.0f;
    if constexpr (!Arith::BF16X3) {
        if (tid < MLP_OUT) ldsBias[LB4 + tid] = P[MLP_OFF_B4 + tid];
        if (smp_var && tid >= 64 && tid < 64 + MLP_NACT) {
            float v = smp_var[tid - 64];
            for (int i = 0; i < smp_var_steps; ++i) v = fmaxf(smp_var_min, v - smp_var_decay);   // ppo.py:236-237, not yet applied to the tensor
            const float L = sqrtf(v);
            ldsBias[LSD + tid - 64] = L;
            ldsBias[LLG + tid - 64] = logf(L);
        }
    } else {
        b4v = P[MLP_OFF_B4 + (tid & 31)];
        if (smp_var && (tid & 31) < MLP_NACT) {
            float v = smp_var[tid & 31];
            for (int i = 0; i < smp_var_steps; ++i) v = fmaxf(smp_var_min, v - smp_var_decay);   // ppo.py:236-237, not yet applied to the tensor
            smpL = sqrtf(v);
            smpLog = logf(smpL);
        }
    }
    for (; tile < ntiles; tile += tile_stride) {
        const long row0 = tile * BM;
        const int nvalid = (int)(n - row0 < BM ? n - row0 : BM);            // rows of this tile that exist
        float* h1_tile = h1_save ? h1_save + row0 * MLP_H1 : nullptr;       // wave-uniform tile bases
        float* h2_tile = h2_save ? h2_save + row0 * MLP_H2 : nullptr;
        float* h3_tile = h3_save ? h3_save + row0 * MLP_H3 : nullptr;
        // opaque per-iteration copy of the thread index: keeps the dozens of tile-invariant LDS/global
        // offsets from being hoisted out of the tile loop (they would all be live across it and spill)
        int tl = tid;
        asm volatile("" : "+v"(tl));
        // the sampling noise of this tile's (row, column) slots of the last phase, requested now: one
        // wave per SIMD (8192 rollout rows = one tile per CU) has nobody to hide a late HBM load behind
        float eps_pre[BM * MLP_OUT / THREADS];
        if (smp_eps) {
#pragma unroll
            for (int k = 0; k < BM * MLP_OUT / THREADS; ++k) {
                const int i = tl + k * THREADS, row = i >> 5, col = i & 31;
                eps_pre[k] = (col < MLP_NACT && row < nvalid) ? (smp_eps + row0 * MLP_NACT)[row * MLP_NACT + col] : 0.0f;
            }
        }
        if (STAMP) stamps = stamps_base + tile * 16;         // one 16-slot record per tile
        stamp<STAMP>(stamps, 0);
        if (STAMP && threadIdx.x == 0) stamps[14] = realtime_cu();       // (which CU this workgroup landed on)
        // Layers 1 and 2 run in two halves of 128 hidden-1 columns so that only a [32][128] slice of
        // H1 is ever in LDS (fp32: 36 KB per workgroup -> four workgroups per CU): L1 produces columns
        // [0,128), L2 accumulates their k range, L1 produces [128,256), L2 accumulates the rest.
        typename Arith::Head w1a, w1b, w2a, w2b, w3;
        Arith::template prefetch<MLP_IN_PAD>(w1a, PF + Arith::F1, wave, lane);       // lands during the x staging
        x_store(tl);
        __syncthreads();
        if (tile + tile_stride < ntiles) x_load(tile + tile_stride);     // lands during this tile's MFMAs
        stamp<STAMP>(stamps, 1);
        Acc acc2;
        {   // L1, columns [0,128): wave owns 32 of them
            Acc acc;
            Arith::template gemm<MLP_IN_PAD>(w1a, PF + Arith::F1, wave, ldsB, acc, lane);
            stamp<STAMP>(stamps, 2);
            Arith::template prefetch<MLP_H2>(w2a, PF + Arith::F2, wave, lane);           // both land during the epilogue
            Arith::template prefetch<MLP_IN_PAD>(w1b, PF + Arith::F1, 4 + wave, lane);
            Arith::template epilogue_elu<MLP_H2, MLP_H1, COH>(acc, ldsBias + LB1, wave * 32, ldsA, lane, h1_tile, nvalid);
        }
        stamp<STAMP>(stamps, 3);
        __syncthreads();
        stamp<STAMP>(stamps, 4);
        {   // L2 over k in [0,128), then L1 columns [128,256) -- one uninterrupted run of MFMAs
            Acc acc;
            Arith::template gemm<MLP_H2>(w2a, PF + Arith::F2, wave, ldsA, acc2, lane);
            Arith::template gemm<MLP_IN_PAD>(w1b, PF + Arith::F1, 4 + wave, ldsB, acc, lane);
            stamp<STAMP>(stamps, 5);
            Arith::template prefetch<MLP_H2>(w2b, PF + Arith::F2 + Arith::F2B, wave, lane);
            __syncthreads();                                   // every wave has finished reading the first half of H1
            Arith::template epilogue_elu<MLP_H2, MLP_H1, COH>(acc, ldsBias + LB1 + MLP_H1 / 2, wave * 32, ldsA, lane,
                                                              h1_tile ? h1_tile + 4 * 1024 : nullptr, nvalid);
        }
        stamp<STAMP>(stamps, 6);
        __syncthreads();
        stamp<STAMP>(stamps, 7);
        {   // L2 over k in [128,256): 256 -> 128 complete, wave owns 32 columns
            Arith::template gemm<MLP_H2, false>(w2b, PF + Arith::F2 + Arith::F2B, wave, ldsA, acc2, lane);
            stamp<STAMP>(stamps, 8);
            Arith::template prefetch<MLP_H2>(w3, PF + Arith::F3, wave, lane);
            Arith::template epilogue_elu<MLP_H2, MLP_H2, COH>(acc2, ldsBias + LB2, wave * 32, ldsB, lane, h2_tile, nvalid);   // x is dead: every wave passed the barrier above
        }
        __syncthreads();
        typename Arith::W4 w4[Arith::NW4];
        {   // L3: 128 -> 128 (actor | critic heads stacked)
            Acc acc;
            stamp<STAMP>(stamps, 9);
            Arith::template gemm<MLP_H2>(w3, PF + Arith::F3, wave, ldsB, acc, lane);
            stamp<STAMP>(stamps, 10);
            if constexpr (!Arith::BF16X3) {
                const float* bp = PF + Arith::F4 + (wave * 4) * 256 + lane * 4;    // [wave][kq][lane][4]
#pragma unroll
                for (int kq = 0; kq < 4; ++kq) w4[kq] = *reinterpret_cast<const float4*>(bp + 256 * kq);
            } else {
                const u16* bp = PF + Arith::F4 + (wave * 2) * 1536 + lane * 8;    // [k block][term][lane][8]
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) w4[kk].p[pl] = *reinterpret_cast<const float4*>(bp + kk * 1536 + pl * 512);
            }
            Arith::template epilogue_elu<MLP_H3, MLP_H3, COH>(acc, ldsBias + LB3, wave * 32, ldsA, lane, h3_tile, nvalid);
        }
        stamp<STAMP>(stamps, 11);
        __syncthreads();
        stamp<STAMP>(stamps, 12);
        // L4: 128 -> 32, split-K over the four waves (32 k each), partials reduced through LDS.  Every wave must be done
        // reading H2 (tile B, layer 3) before the partials overwrite it: they are -- the barrier after the layer-3 epilogue
        // is behind all of them
        if constexpr (!Arith::BF16X3) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            const int r = lane & 31, h = lane >> 5;
            const float* ap = ldsA + r * (MLP_H3 + 4) + wave * 32 + h * 16;
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
                const float4 a = *reinterpret_cast<const float4*>(ap + 4 * kq);
                const float4 b = w4[kq];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, a.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, a.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, a.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, a.w, acc, 0, 0, 0);
            }
            float* part = ldsBf + wave * (BM * MLP_OUT);                         // [row][32]
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(part + r * MLP_OUT + 4 * ((acc_n(g, lane) >> 2) ^ ((r >> 1) & 7))) =
                    make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        } else {
            f32x16 hi, lo;
#pragma unroll
            for (int i = 0; i < 16; ++i) { hi[i] = 0.0f; lo[i] = 0.0f; }
            const int r = lane & 31, h = lane >> 5;
            const u16* ap = ldsA + r * (MLP_H3 + B3_PAD) + wave * 32 + 8 * h;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 xq[3], wq[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    xq[pl] = as_bf16x8(*reinterpret_cast<const float4*>(ap + pl * b3_plane<MLP_H3>() + 16 * kk));
                    wq[pl] = as_bf16x8(w4[kk].p[pl]);
                }
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[0], xq[2], lo, 0, 0, 0);
                hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[0], xq[0], hi, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[2], xq[0], lo, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[1], xq[1], lo, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[0], xq[1], lo, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[1], xq[0], lo, 0, 0, 0);
            }
            float* part = ldsBf + wave * (BM * MLP_OUT);                         // [row][32]
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(part + r * MLP_OUT + 4 * ((acc_n(g, lane) >> 2) ^ ((r >> 1) & 7))) =
                    make_float4(hi[4 * g] + lo[4 * g], hi[4 * g + 1] + lo[4 * g + 1], hi[4 * g + 2] + lo[4 * g + 2],
                                hi[4 * g + 3] + lo[4 * g + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BM * MLP_OUT / THREADS; ++k) {
            const int i = tl + k * THREADS;
            const int row = i >> 5, col = i & 31;
            const int is = (i & ~31) + 4 * (((i & 31) >> 2) ^ ((row >> 1) & 7)) + (i & 3);      // where the writer put this element (chunk rotation)
            float z = ((ldsBf[is] + ldsBf[BM * MLP_OUT + is]) + ldsBf[2 * BM * MLP_OUT + is]) + ldsBf[3 * BM * MLP_OUT + is];
            z += Arith::BF16X3 ? b4v : ldsBias[LB4 + col];
            float y = (col < MLP_NACT) ? elu(z) : ((col == MLP_NACT) ? z : 0.0f);   // ELU on the mean (ppo.py:30), none on v
            const bool in = row < nvalid;
            if (in) {
                if (out_save) gstore1<COH>(out_save + row0 * MLP_OUT, frag_off(row, col), y);
                if (mu_out && col < MLP_NACT) (mu_out + row0 * MLP_NACT)[row * MLP_NACT + col] = y;
                if (v_out && col == MLP_NACT) (v_out + row0)[row] = y;
            }
            if (smp_eps) {
                // ppo.py:215-220 fused: the 32 lanes that hold one output row sample its action
                // (a = mu + sqrt(var) eps), reduce the Mahalanobis term and sum log L with a fixed
                // xor-butterfly over the half-wave, and write the clipped action and the log-prob.
                float x2 = 0.0f, lg = 0.0f, a = 0.0f;
                const bool on = (col < MLP_NACT) && in;
                if (on) {
                    const float L = Arith::BF16X3 ? smpL : ldsBias[LSD + col];
                    a = y + L * eps_pre[k];
                    const float xj = (a - y) / L;
                    x2 = xj * xj;
                    lg = Arith::BF16X3 ? smpLog : ldsBias[LLG + col];
                }
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) { x2 += __shfl_xor(x2, o, 32); lg += __shfl_xor(lg, o, 32); }
                if (on) {
                    const float ac = fminf(fmaxf(a, -1.0f), 1.0f);
                    (smp_act + row0 * MLP_NACT)[row * MLP_NACT + col] = ac;
                    if (Arith::LDS_HANDOFF && act_tile_lds) act_tile_lds[row * MLP_NACT + col] = ac;
                }
                if (col == 0 && in) (smp_logp + row0)[row] = gauss_logp(x2, lg);
            }
        }
        stamp<STAMP>(stamps, 13);
        if (STAMP && threadIdx.x == 0) {
            unsigned long long t;
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
            stamps[15] = t;
        }
        __syncthreads();            // tile B (partials) is the next tile's input buffer
    }
}

template <bool STAMP>
__global__ __launch_bounds__(THREADS, 2) void mlp_forward_kernel(
    const float* __restrict__ P, const float* __restrict__ PF, const float* __restrict__ x, long n,
    float* __restrict__ mu_out, float* __restrict__ v_out, float* __restrict__ out_save,
    float* __restrict__ h1_save, float* __restrict__ h2_save, float* __restrict__ h3_save,
    const float* __restrict__ smp_eps, const float* __restrict__ smp_var, float* __restrict__ smp_act,
    float* __restrict__ smp_logp, unsigned long long* __restrict__ stamps_base, int smp_var_steps, float smp_var_decay,
    float smp_var_min, const int* __restrict__ smp_var_base)
{
    __shared__ __attribute__((aligned(16))) float lds[ArithF32::FWD_FLOATS];
    // pending decays = smp_var_steps - *smp_var_base: the launch argument can be frozen in a captured graph (the row
    // index of the rollout) while the device word follows what ppo_rollout_bookkeeping has already applied
    const int steps = smp_var_steps - (smp_var_base ? *smp_var_base : 0);
    forward_body<ArithF32, STAMP>(lds, blockIdx.x, gridDim.x, P, PF, x, n, mu_out, v_out, out_save, h1_save, h2_save, h3_save,
                                  smp_eps, smp_var, smp_act, smp_logp, stamps_base, steps, smp_var_decay, smp_var_min);
}

__global__ __launch_bounds__(THREADS, 1) void mlp_forward_b3_kernel(
    const float* __restrict__ P, const u16* __restrict__ PB, const float* __restrict__ x, long n,
    float* __restrict__ mu_out, float* __restrict__ v_out, float* __restrict__ out_save,
    float* __restrict__ h1_save, float* __restrict__ h2_save, float* __restrict__ h3_save,
    const float* __restrict__ smp_eps, const float* __restrict__ smp_var, float* __restrict__ smp_act,
    float* __restrict__ smp_logp, int smp_var_steps, float smp_var_decay, float smp_var_min,
    const int* __restrict__ smp_var_base)
{
    __shared__ __attribute__((aligned(16))) float lds[ArithB3::FWD_FLOATS];
    const int steps = smp_var_steps - (smp_var_base ? *smp_var_base : 0);
    // one tile per workgroup: this body's straight-line GEMMs leave no registers for the next-tile prefetch of the
    // persistent fp32 variant
    forward_body<ArithB3, false>(lds, blockIdx.x, 1L << 40, P, PB, x, n, mu_out, v_out, out_save, h1_save, h2_save, h3_save,
                                 smp_eps, smp_var, smp_act, smp_logp, nullptr, steps, smp_var_decay, smp_var_min);
}
