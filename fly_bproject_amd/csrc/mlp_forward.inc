// mlp_forward.inc — the fused four-layer forward body (fp32-MFMA and bf16x3 arithmetic) and its kernels.
// Both tile kernels fit four workgroups per CU: <= 40 KB of LDS and <= 128 VGPRs each.
constexpr int WGS_PER_CU = 4;
constexpr int PERSIST_GRID = 256 * WGS_PER_CU;       // persistent launches: every slot of the chip
constexpr int LDS_A_FLOATS = BM * (MLP_H2 + 4);      // one 128-column half of H1 at a time, later H3
constexpr int LDS_B_FLOATS = BM * (MLP_H2 + 4);      // X0, later H2, later the split-K partials
constexpr int LB1 = 0, LB2 = MLP_H1, LB3 = LB2 + MLP_H2, LB4 = LB3 + MLP_H3, LSD = LB4 + MLP_OUT, LLG = LSD + 32;
constexpr int LDS_C_FLOATS = LLG + 32;               // biases + sampling constants (2.4 KB)

// x [n][73] -> out [n][32] (cols 0..17 = mean after ELU, col 18 = value, rest 0).
// mu_out [n][18] / v_out [n] / h*_save are optional.
// Persistent workgroups: the grid is at most 3 workgroups per CU and each walks tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...; the NEXT tile's input rows are fetched into registers
// (16-byte loads: a 32x73 tile is one contiguous, 16-byte aligned block) while the current tile
// computes, so the ~5 us HBM round trip that used to open every workgroup is hidden.
constexpr int XV = (BM * MLP_IN / 4 + THREADS - 1) / THREADS;       // float4 per thread for one x tile (584 / 256 -> 3)

constexpr int FWD_LDS_FLOATS = LDS_A_FLOATS + LDS_B_FLOATS + LDS_C_FLOATS;

// The body walks tiles first_tile, first_tile + tile_stride, ... (< ntiles) on the caller's LDS
// arena.
// NORM: the input rows are normalised (obs_norm_apply) under the table norm_tab (LDS, published by a barrier before the call)
// on their way into LDS; the rows in HBM stay raw.
template <bool STAMP, bool COH = false, bool NORM = false>
__device__ __forceinline__ void forward_body(
    float* lds, const long first_tile, const long tile_stride,
    const float* __restrict__ P, const float* __restrict__ PF, const float* __restrict__ x, long n,
    float* __restrict__ mu_out, float* __restrict__ v_out, float* __restrict__ out_save,
    float* __restrict__ h1_save, float* __restrict__ h2_save, float* __restrict__ h3_save,
    const float* __restrict__ smp_eps, const float* __restrict__ smp_var, float* __restrict__ smp_act,
    float* __restrict__ smp_logp, unsigned long long* __restrict__ stamps_base,
    const int smp_var_steps = 0, const float smp_var_decay = 0.0f, const float smp_var_min = 0.0f,
    const float* norm_tab = nullptr)
{
    unsigned long long* stamps = stamps_base;
    float* ldsA = lds;
    float* ldsB = lds + LDS_A_FLOATS;
    float* ldsBias = ldsB + LDS_B_FLOATS;   // b1 | b2 | b3 | b4 | sqrt(var) | log sqrt(var): read by every epilogue
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR: weight bases become scalar
    const long ntiles = (n + BM - 1) / BM;
    const long total = n * MLP_IN;

    float4 xr[XV];
    auto x_load = [&](long tile) {
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
    auto x_store = [&](int tid) {   // registers -> ldsB as [32][80+4]; pad columns 73..79 zeroed
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int i4 = tid + u * THREADS;
            if (i4 < BM * MLP_IN / 4) {
                const float e[4] = {xr[u].x, xr[u].y, xr[u].z, xr[u].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 4 * i4 + j;
                    const int rr = f / MLP_IN, cc = f - rr * MLP_IN;
                    ldsB[rr * (MLP_IN_PAD + 4) + cc] =
                        NORM ? obs_norm_apply(e[j], norm_tab[cc], norm_tab[MLP_IN + cc], norm_tab[2 * MLP_IN]) : e[j];
                }
            }
        }
        if (tid < BM * (MLP_IN_PAD - MLP_IN)) {
            const int rr = tid / (MLP_IN_PAD - MLP_IN), cc = MLP_IN + tid - rr * (MLP_IN_PAD - MLP_IN);
            ldsB[rr * (MLP_IN_PAD + 4) + cc] = 0.0f;
        }
    };

    long tile = first_tile;
    if (tile < ntiles) x_load(tile);
    {   // biases (and the sampling constants) -> LDS once per workgroup; the first tile's barrier publishes them
        ldsBias[LB1 + tid] = P[MLP_OFF_B1 + tid];
        if (tid < MLP_H2) ldsBias[LB2 + tid] = P[MLP_OFF_B2 + tid];
        else ldsBias[LB3 + tid - MLP_H2] = P[MLP_OFF_B3 + tid - MLP_H2];
        if (tid < MLP_OUT) ldsBias[LB4 + tid] = P[MLP_OFF_B4 + tid];
        if (smp_var && tid >= 64 && tid < 64 + MLP_NACT) {
            float v = smp_var[tid - 64];
            for (int i = 0; i < smp_var_steps; ++i) v = fmaxf(smp_var_min, v - smp_var_decay);   // ppo.py:236-237, not yet applied to the tensor
            const float L = sqrtf(v);
            ldsBias[LSD + tid - 64] = L;
            ldsBias[LLG + tid - 64] = logf(L);
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
        if (STAMP && threadIdx.x == 0) {
            unsigned long long t;
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
            // top 16 bits: which CU this workgroup landed on (HW_ID cu/sh/se bits 8..15, XCC_ID)
            const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
            t = (t & 0xffffffffffffull) | ((unsigned long long)(((hw >> 8) & 0xff) | ((xcc & 0xf) << 8)) << 48);
            stamps[14] = t;
        }
        // Layers 1 and 2 run in two halves of 128 hidden-1 columns so that only a [32][132] slice of
        // H1 is ever in LDS (36 KB per workgroup -> four workgroups per CU): L1 produces columns
        // [0,128), L2 accumulates their k range, L1 produces [128,256), L2 accumulates the rest.
        WeightHead<1> w1a, w1b, w2a, w2b, w3;
        gemm_prefetch<MLP_IN_PAD, 1>(w1a, PF + MLP_OFF_F1, wave, lane);       // lands during the x staging
        x_store(tl);
        __syncthreads();
        if (tile + tile_stride < ntiles) x_load(tile + tile_stride);     // lands during this tile's MFMAs
        stamp<STAMP>(stamps, 1);
        f32x16 acc2[1];
        {   // L1, columns [0,128): wave owns 32 of them
            f32x16 acc[1];
            tile_gemm<MLP_IN_PAD, 1>(w1a, PF + MLP_OFF_F1, wave, ldsB, acc, lane);
            stamp<STAMP>(stamps, 2);
            gemm_prefetch<MLP_H2, 1>(w2a, PF + MLP_OFF_F2, wave, lane);           // both land during the epilogue
            gemm_prefetch<MLP_IN_PAD, 1>(w1b, PF + MLP_OFF_F1, 4 + wave, lane);
            epilogue_elu<MLP_H2, 1, MLP_H1, COH>(acc, ldsBias + LB1, wave * 32, ldsA, lane, h1_tile, nvalid);
        }
        stamp<STAMP>(stamps, 3);
        __syncthreads();
        stamp<STAMP>(stamps, 4);
        {   // L2 over k in [0,128), then L1 columns [128,256) -- one uninterrupted run of MFMAs
            f32x16 acc[1];
            tile_gemm<MLP_H2, 1>(w2a, PF + MLP_OFF_F2, wave, ldsA, acc2, lane);
            tile_gemm<MLP_IN_PAD, 1>(w1b, PF + MLP_OFF_F1, 4 + wave, ldsB, acc, lane);
            stamp<STAMP>(stamps, 5);
            gemm_prefetch<MLP_H2, 1>(w2b, PF + MLP_OFF_F2 + MLP_H2 * (MLP_H1 / 2), wave, lane);
            __syncthreads();                                   // every wave has finished reading the first half of H1
            epilogue_elu<MLP_H2, 1, MLP_H1, COH>(acc, ldsBias + LB1 + MLP_H1 / 2, wave * 32, ldsA, lane, h1_tile ? h1_tile + 4 * 1024 : nullptr, nvalid);
        }
        stamp<STAMP>(stamps, 6);
        __syncthreads();
        stamp<STAMP>(stamps, 7);
        {   // L2 over k in [128,256): 256 -> 128 complete, wave owns 32 columns
            tile_gemm<MLP_H2, 1, false>(w2b, PF + MLP_OFF_F2 + MLP_H2 * (MLP_H1 / 2), wave, ldsA, acc2, lane);
            stamp<STAMP>(stamps, 8);
            gemm_prefetch<MLP_H2, 1>(w3, PF + MLP_OFF_F3, wave, lane);
            epilogue_elu<MLP_H2, 1, MLP_H2, COH>(acc2, ldsBias + LB2, wave * 32, ldsB, lane, h2_tile, nvalid);   // x is dead: every wave passed the barrier above
        }
        __syncthreads();
        float4 w4[4];                                                            // layer-4 weights of this wave's k range
        {   // L3: 128 -> 128 (actor | critic heads stacked)
            f32x16 acc[1];
            stamp<STAMP>(stamps, 9);
            tile_gemm<MLP_H2, 1>(w3, PF + MLP_OFF_F3, wave, ldsB, acc, lane);
            stamp<STAMP>(stamps, 10);
            const float* bp = PF + MLP_OFF_F4 + (wave * 4) * 256 + lane * 4;    // [wave][kq][lane][4]
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) w4[kq] = *reinterpret_cast<const float4*>(bp + 256 * kq);
            epilogue_elu<MLP_H3, 1, MLP_H3, COH>(acc, ldsBias + LB3, wave * 32, ldsA, lane, h3_tile, nvalid);
        }
        stamp<STAMP>(stamps, 11);
        __syncthreads();
        stamp<STAMP>(stamps, 12);
        {   // L4: 128 -> 32, split-K over the four waves (32 k each), partials reduced through LDS
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
            float* part = ldsB + wave * (BM * MLP_OUT);                          // [row][32]
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(part + r * MLP_OUT + 4 * ((acc_n(g, lane) >> 2) ^ ((r >> 1) & 7))) =
                    make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BM * MLP_OUT / THREADS; ++k) {
            const int i = tl + k * THREADS;
            const int row = i >> 5, col = i & 31;
            const int is = (i & ~31) + 4 * (((i & 31) >> 2) ^ ((row >> 1) & 7)) + (i & 3);      // where the writer put this element (chunk rotation)
            float z = ((ldsB[is] + ldsB[BM * MLP_OUT + is]) + ldsB[2 * BM * MLP_OUT + is]) + ldsB[3 * BM * MLP_OUT + is];
            z += ldsBias[LB4 + col];
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
                    const float L = ldsBias[LSD + col];
                    a = y + L * eps_pre[k];
                    const float xj = (a - y) / L;
                    x2 = xj * xj;
                    lg = ldsBias[LLG + col];
                }
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) { x2 += __shfl_xor(x2, o, 32); lg += __shfl_xor(lg, o, 32); }
                if (on) (smp_act + row0 * MLP_NACT)[row * MLP_NACT + col] = fminf(fmaxf(a, -1.0f), 1.0f);
                if (col == 0 && in) (smp_logp + row0)[row] = gauss_logp(x2, lg);
            }
        }
        stamp<STAMP>(stamps, 13);
        if (STAMP && threadIdx.x == 0) {
            unsigned long long t;
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
            stamps[15] = t;
        }
        __syncthreads();            // ldsB (partials) is the next tile's input buffer
    }
}

// bf16x3 variant of the forward body: same tile flow, activations live in LDS as three bf16 term planes
constexpr int B3_TILE_FLOATS = 3 * b3_plane<MLP_H2>() / 2;        // a [32][128] tile as three planes, in floats
constexpr int FWD_B3_LDS_FLOATS = 2 * B3_TILE_FLOATS + LB4;      // two tiles + b1 | b2 | b3: 54 272 B, three workgroups per CU

// The body walks tiles first_tile, first_tile + tile_stride, ... (< ntiles) on the caller's LDS
// arena.
// NORM / norm_tab: as forward_body's.
template <bool STAMP, bool COH = false, bool NORM = false>
__device__ __forceinline__ void forward_body_b3(
    float* lds, const long first_tile, const long tile_stride,
    const float* __restrict__ P, const u16* __restrict__ PB, const float* __restrict__ x, long n,
    float* __restrict__ mu_out, float* __restrict__ v_out, float* __restrict__ out_save,
    float* __restrict__ h1_save, float* __restrict__ h2_save, float* __restrict__ h3_save,
    const float* __restrict__ smp_eps, const float* __restrict__ smp_var, float* __restrict__ smp_act,
    float* __restrict__ smp_logp, unsigned long long* __restrict__ stamps_base,
    const int smp_var_steps = 0, const float smp_var_decay = 0.0f, const float smp_var_min = 0.0f,
    const float* x_tile_lds = nullptr, float* act_tile_lds = nullptr, const bool biases_resident = false,
    const float* norm_tab = nullptr)
{
    // biases_resident: an earlier call on the same arena has left b1 | b2 | b3 in `ldsBias` and nothing has touched them since
    // x_tile_lds (one-launch rollout): the FIRST tile's rows lie in LDS as fp32 [32][73] (the env step of the same workgroup left
    // them there, at the start of the arena: read before anything of this body overwrites it) -- no round trip through L2.
    // act_tile_lds: the sampled, clipped actions of a tile are ALSO left in LDS as [32][18] for the env step that follows.
    unsigned long long* stamps = stamps_base;
    u16* ldsA = reinterpret_cast<u16*>(lds);                                   // H1 half / H3: three [32][136] planes
    u16* ldsB = reinterpret_cast<u16*>(lds + B3_TILE_FLOATS);                  // X ([32][88] planes) / H2 / fp32 split-K partials
    float* ldsBf = lds + B3_TILE_FLOATS;
    float* ldsBias = lds + 2 * B3_TILE_FLOATS;   // b1 | b2 | b3 | b4 | sqrt(var) | log sqrt(var): read by every epilogue
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index in an SGPR: weight bases become scalar
    const long ntiles = (n + BM - 1) / BM;
    const long total = n * MLP_IN;

    float4 xr[XV];
    auto x_load = [&](long tile) {
        if (x_tile_lds != nullptr && tile == first_tile) {       // (wave-uniform)
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
    auto x_store = [&](int tid) {   // registers -> ldsB as three [32][80+8] bf16 term planes; pad columns 73..79 zeroed
#pragma unroll
        for (int u = 0; u < XV; ++u) {
            const int i4 = tid + u * THREADS;
            if (i4 < BM * MLP_IN / 4) {
                const float e[4] = {xr[u].x, xr[u].y, xr[u].z, xr[u].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 4 * i4 + j;
                    const int rr = f / MLP_IN, cc = f - rr * MLP_IN;
                    u16 sa, sb, sc;
                    split3(NORM ? obs_norm_apply(e[j], norm_tab[cc], norm_tab[MLP_IN + cc], norm_tab[2 * MLP_IN]) : e[j], sa, sb, sc);
                    u16* q = ldsB + rr * (MLP_IN_PAD + B3_PAD) + cc;
                    q[0] = sa; q[b3_plane<MLP_IN_PAD>()] = sb; q[2 * b3_plane<MLP_IN_PAD>()] = sc;
                }
            }
        }
        if (tid < BM * (MLP_IN_PAD - MLP_IN)) {
            const int rr = tid / (MLP_IN_PAD - MLP_IN), cc = MLP_IN + tid - rr * (MLP_IN_PAD - MLP_IN);
            u16* q = ldsB + rr * (MLP_IN_PAD + B3_PAD) + cc;
            q[0] = 0; q[b3_plane<MLP_IN_PAD>()] = 0; q[2 * b3_plane<MLP_IN_PAD>()] = 0;
        }
    };

    long tile = first_tile;
    if (tile < ntiles) x_load(tile);
    if (!biases_resident) {   // biases (and the sampling constants) -> LDS once per workgroup; the first tile's barrier publishes them
        ldsBias[LB1 + tid] = P[MLP_OFF_B1 + tid];
        if (tid < MLP_H2) ldsBias[LB2 + tid] = P[MLP_OFF_B2 + tid];
        else ldsBias[LB3 + tid - MLP_H2] = P[MLP_OFF_B3 + tid - MLP_H2];
    }
    // this thread's output column is the same in every tile: its layer-4 bias and sampling constants
    // stay in registers (the LDS budget of this path is exactly three workgroups per CU)
    const float b4v = P[MLP_OFF_B4 + (tid & 31)];
    float smpL = 1.0f, smpLog = 0.0f;
    if (smp_var && (tid & 31) < MLP_NACT) {
        float v = smp_var[tid & 31];
        for (int i = 0; i < smp_var_steps; ++i) v = fmaxf(smp_var_min, v - smp_var_decay);   // ppo.py:236-237, not yet applied to the tensor
        smpL = sqrtf(v);
        smpLog = logf(smpL);
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
        if (STAMP && threadIdx.x == 0) {
            unsigned long long t;
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
            // top 16 bits: which CU this workgroup landed on (HW_ID cu/sh/se bits 8..15, XCC_ID)
            const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
            t = (t & 0xffffffffffffull) | ((unsigned long long)(((hw >> 8) & 0xff) | ((xcc & 0xf) << 8)) << 48);
            stamps[14] = t;
        }
        // Layers 1 and 2 run in two halves of 128 hidden-1 columns so that only a [32][128] slice of
        // H1 is ever in LDS: L1 produces columns
        // [0,128), L2 accumulates their k range, L1 produces [128,256), L2 accumulates the rest.
        WeightHead3 w1a, w1b, w2a, w2b, w3;
        gemm_prefetch_b3<MLP_IN_PAD>(w1a, PB + MLP_OFF_PB1, wave, lane);       // lands during the x staging
        x_store(tl);
        __syncthreads();
        if (tile + tile_stride < ntiles) x_load(tile + tile_stride);     // lands during this tile's MFMAs
        stamp<STAMP>(stamps, 1);
        f32x16 hi2, lo2;
        {   // L1, columns [0,128): wave owns 32 of them
            f32x16 hi, lo;
            tile_gemm_b3<MLP_IN_PAD>(w1a, PB + MLP_OFF_PB1, wave, ldsB, hi, lo, lane);
            stamp<STAMP>(stamps, 2);
            gemm_prefetch_b3<MLP_H2>(w2a, PB + MLP_OFF_PB2, wave, lane);              // both land during the epilogue
            gemm_prefetch_b3<MLP_IN_PAD>(w1b, PB + MLP_OFF_PB1, 4 + wave, lane);
            epilogue_elu_b3<MLP_H2, MLP_H1, COH>(hi, lo, ldsBias + LB1, wave * 32, ldsA, lane, h1_tile, nvalid);
        }
        stamp<STAMP>(stamps, 3);
        __syncthreads();
        stamp<STAMP>(stamps, 4);
        {   // L2 over k in [0,128), then L1 columns [128,256) -- one uninterrupted run of MFMAs
            f32x16 hi, lo;
            tile_gemm_b3<MLP_H2>(w2a, PB + MLP_OFF_PB2, wave, ldsA, hi2, lo2, lane);
            tile_gemm_b3<MLP_IN_PAD>(w1b, PB + MLP_OFF_PB1, 4 + wave, ldsB, hi, lo, lane);
            stamp<STAMP>(stamps, 5);
            gemm_prefetch_b3<MLP_H2>(w2b, PB + MLP_OFF_PB2 + 3 * MLP_H2 * (MLP_H1 / 2), wave, lane);
            __syncthreads();                                   // every wave has finished reading the first half of H1
            epilogue_elu_b3<MLP_H2, MLP_H1, COH>(hi, lo, ldsBias + LB1 + MLP_H1 / 2, wave * 32, ldsA, lane, h1_tile ? h1_tile + 4 * 1024 : nullptr, nvalid);
        }
        stamp<STAMP>(stamps, 6);
        __syncthreads();
        stamp<STAMP>(stamps, 7);
        {   // L2 over k in [128,256): 256 -> 128 complete, wave owns 32 columns
            tile_gemm_b3<MLP_H2, false>(w2b, PB + MLP_OFF_PB2 + 3 * MLP_H2 * (MLP_H1 / 2), wave, ldsA, hi2, lo2, lane);
            stamp<STAMP>(stamps, 8);
            gemm_prefetch_b3<MLP_H2>(w3, PB + MLP_OFF_PB3, wave, lane);
            epilogue_elu_b3<MLP_H2, MLP_H2, COH>(hi2, lo2, ldsBias + LB2, wave * 32, ldsB, lane, h2_tile, nvalid);   // x is dead: every wave passed the barrier above
        }
        __syncthreads();
        Frag3 w4[2];                                                             // layer-4 weights of this wave's two k blocks
        {   // L3: 128 -> 128 (actor | critic heads stacked)
            f32x16 hi, lo;
            stamp<STAMP>(stamps, 9);
            tile_gemm_b3<MLP_H2>(w3, PB + MLP_OFF_PB3, wave, ldsB, hi, lo, lane);
            stamp<STAMP>(stamps, 10);
            const u16* bp = PB + MLP_OFF_PB4 + (wave * 2) * 1536 + lane * 8;    // [k block][term][lane][8]
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) w4[kk].p[pl] = *reinterpret_cast<const float4*>(bp + kk * 1536 + pl * 512);
            epilogue_elu_b3<MLP_H3, MLP_H3, COH>(hi, lo, ldsBias + LB3, wave * 32, ldsA, lane, h3_tile, nvalid);
        }
        stamp<STAMP>(stamps, 11);
        __syncthreads();
        stamp<STAMP>(stamps, 12);
        {   // L4: 128 -> 32, split-K over the four waves (32 k each), partials reduced through LDS
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
            // every wave must be done reading H2 (ldsB, layer 3) before the partials overwrite it:
            // they are -- the barrier after the layer-3 epilogue is behind all of them
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
            z += b4v;
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
                    const float L = smpL;
                    a = y + L * eps_pre[k];
                    const float xj = (a - y) / L;
                    x2 = xj * xj;
                    lg = smpLog;
                }
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) { x2 += __shfl_xor(x2, o, 32); lg += __shfl_xor(lg, o, 32); }
                if (on) {
                    const float ac = fminf(fmaxf(a, -1.0f), 1.0f);
                    (smp_act + row0 * MLP_NACT)[row * MLP_NACT + col] = ac;
                    if (act_tile_lds) act_tile_lds[row * MLP_NACT + col] = ac;
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
        __syncthreads();            // ldsB (partials) is the next tile's input buffer
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
    __shared__ __attribute__((aligned(16))) float lds[FWD_LDS_FLOATS];
    // pending decays = smp_var_steps - *smp_var_base: the launch argument can be frozen in a captured graph (the row
    // index of the rollout) while the device word follows what ppo_rollout_bookkeeping has already applied
    const int steps = smp_var_steps - (smp_var_base ? *smp_var_base : 0);
    forward_body<STAMP>(lds, blockIdx.x, gridDim.x, P, PF, x, n, mu_out, v_out, out_save, h1_save,
                        h2_save, h3_save, smp_eps, smp_var, smp_act, smp_logp, stamps_base, steps, smp_var_decay,
                        smp_var_min);
}

__global__ __launch_bounds__(THREADS, 1) void mlp_forward_b3_kernel(
    const float* __restrict__ P, const u16* __restrict__ PB, const float* __restrict__ x, long n,
    float* __restrict__ mu_out, float* __restrict__ v_out, float* __restrict__ out_save,
    float* __restrict__ h1_save, float* __restrict__ h2_save, float* __restrict__ h3_save,
    const float* __restrict__ smp_eps, const float* __restrict__ smp_var, float* __restrict__ smp_act,
    float* __restrict__ smp_logp, int smp_var_steps, float smp_var_decay, float smp_var_min,
    const int* __restrict__ smp_var_base)
{
    __shared__ __attribute__((aligned(16))) float lds[FWD_B3_LDS_FLOATS];
    const int steps = smp_var_steps - (smp_var_base ? *smp_var_base : 0);
    // one tile per workgroup (a constant stride no tile index reaches): this body's straight-line GEMMs
    // leave no registers for the next-tile prefetch of the persistent fp32 variant
    forward_body_b3<false>(lds, blockIdx.x, 1L << 40, P, PB, x, n, mu_out, v_out, out_save, h1_save, h2_save, h3_save,
                           smp_eps, smp_var, smp_act, smp_logp, nullptr, steps, smp_var_decay, smp_var_min);
}
