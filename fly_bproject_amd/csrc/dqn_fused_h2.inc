// dqn_fused_h2.inc — the fused DQN update (dqn_fused.inc: reference UselessFiles/dqn.py:64-85 in two persistent launches) in the fp16x2
// arithmetic of mlp_fused_h2.inc: every GEMM operand is TWO fp16 terms of its scaled value (x s = h0 + h1, s a power of two per tensor
// class), a 16-wide k block is THREE v_mfma_f32_32x32x16_f16 (h0 h0 -> `hi`; h0 h1, h1 h0 -> `lo`) instead of six bf16 products, LDS
// plane images, weight planes and the saved H1 image have two planes instead of three.  Read dqn_fused.inc first: the phases,
// the k-step orders (H2GemmHost MODE 1 / 2), the guests in the MFMA gaps and the register-resident dW1 / dW3 are the same; this file
// restates them on two planes with scaled epilogues.
//
// SCALES (`fsc`, device, H2_FSC_FLOATS floats: s[c] at [c], 1 / s[c] at [16 + c], the last launch's maximum at [32 + c]):
//     0 X (obs and next_obs rows)   1 H1   2 H2 (both networks)   5 dZ2   6 dZ1        -- lagged: this update's class maxima of
//       |scaled value| set the NEXT update's scales (dqn_h2_scales_kernel, windows of fs_h2.inc: activations [2^7, 2^8), gradients
//       [2^2, 2^3)); a maximum of 65504 or more sets the device word *ovf: the host then forms this update's gradient again with the
//       bf16x3 launches (DQN.update) -- one update is one launch set, so nothing has been applied yet
//     4 dZ3 -- static: |d loss / d Q| <= inv_B (Huber, dqn.py:76), s = 2^(2 - ilogb(inv_B)) computed where it is used
//     8 .. 10 online W1 .. W3, 11 .. 13 target W1 .. W3 -- exact: dqn_h2_planes_kernel takes max |w| per layer in front of every
//       update and scales it into [2^11, 2^12)
// Products of powers of two are exact: every epilogue applies 1 / (s_a s_w) to hi + lo, the partial slabs leave unscaled.
constexpr int DHC_X = 0, DHC_H1 = 1, DHC_H2 = 2, DHC_Z3 = 4, DHC_Z2 = 5, DHC_Z1 = 6, DHC_W = 8, DHC_WT = 11;
constexpr int DH_NMAX = 5;                                               // running maxima: X, H1, H2, dZ2, dZ1 (slots 0 .. 4)
constexpr int DH_SLOT_X = 0, DH_SLOT_H1 = 1, DH_SLOT_H2 = 2, DH_SLOT_Z2 = 3, DH_SLOT_Z1 = 4;
__host__ __device__ constexpr int dh_slot_class(int s) { return s < 3 ? s : s + 2; }

// weight planes: the layout of QB / QTB (dqn_layout.h) with two terms per k block -- a block is 1024 16-bit words, not 1536
constexpr int DH_OFF_QH1 = 0, DH_OFF_QH2 = DH_OFF_QH1 + 2 * DQN_H * DQN_IN_PAD, DH_OFF_QH3 = DH_OFF_QH2 + 2 * DQN_H * DQN_H,
              DH_QH_HALVES = DH_OFF_QH3 + 2 * DQN_OUT * DQN_H;
constexpr int DH_OFF_QTH3 = 0, DH_OFF_QTH2 = DH_OFF_QTH3 + 2 * DQN_H * DQN_OUT, DH_QTH_HALVES = DH_OFF_QTH2 + 2 * DQN_H * DQN_H;
static_assert(DH_QH_HALVES * 3 == DQN_QB_HALVES * 2 && DH_QTH_HALVES * 3 == DQN_QTB_HALVES * 2, "two thirds of the bf16x3 planes");

// ---- LDS image ----------------------------------------------------------------------------------------------------------------------
constexpr int DH_OFF_X = 0;                                              // X planes [32][96] x 2 of the target pass (next_obs) ...
constexpr int DH_OFF_XO = DH_OFF_X + 2 * BM * FS_PX;                     // ... and of the online pass (obs): both are made in MFMA gaps
constexpr int DH_OFF_H1 = DH_OFF_XO + 2 * BM * FS_PX;                    // H1 planes [32][256] x 2
constexpr int DH_OFF_H2 = DH_OFF_H1 + 2 * BM * FS_P1;                    // H2 planes; dZ2 overwrites them in place
constexpr int DH_OFF_PART = DH_OFF_H2 + 2 * BM * FS_P1;                  // fp32 [4][32][32]: the last layer's split-K partials
constexpr int DH_OFF_Z3 = DH_OFF_PART + 4 * BM * DQN_OUT * 2;            // dZ3 planes [32][32] x 2
constexpr int DH_OFF_XS = DH_OFF_Z3 + 2 * BM * FS_P4;                    // staging blocks (dqn_fused.inc)
constexpr int DH_OFF_XS2 = DH_OFF_XS + DF_XS_HALVES;
constexpr int DH_OFF_F32 = DH_OFF_XS2 + DF_XS_HALVES;
// fp32 tail: online b1 s_h1 | b2 s_h2 | b3, the same of the target network, row loss, scale table (48), running maxima [5][256]
constexpr int DH_TAIL_FLOATS = 2 * DF_BIAS + BM + H2_FSC_FLOATS + DH_NMAX * THREADS;
constexpr int DH_LDS_BYTES = DH_OFF_F32 * 2 + DH_TAIL_FLOATS * 4;
constexpr int DH_IMAGE_HALVES = 2 * BM * FS_P1;                          // one image slot of a tile (H1's planes | dZ2's record): 16384 16-bit words
static_assert(DH_LDS_BYTES <= 160 * 1024 && (DH_OFF_XS * 2) % 16 == 0 && (DH_OFF_XS2 * 2) % 16 == 0 && (DH_OFF_F32 * 2) % 16 == 0,
              "fits one CU, 16-byte aligned regions");

// ---- epilogues as single-instruction ops of interleaved chains (dqn_fused.inc) --------------------------------------------------------
// LeakyReLU epilogue (lane = row): y s = max(t, slope t) with t = fma(hi + lo, k s, bias s) -- k = 1 / (s_a s_w), the bias was
// multiplied by s once per launch; powers of two commute with every rounding here -- then the two-term split and the running maximum
template <int PITCH>
struct DhLreluOps {
    static constexpr int HEAD_OPS = 8, CH = HEAD_OPS + H2_SPLIT_OPS;      // 13 ops per chain
    static constexpr int NG = 1 + 2 * CH + 2, TOTAL = 4 * NG;             // per group: bias load, two chains, two stores
    const f32x16 &hi, &lo;
    const float* bias;      // + col0 (scaled)
    u16* plane0;
    int col0, lane, r;
    float ks, am;
    float4 bv[2];
    H2Chain k[4];
    __device__ __forceinline__ DhLreluOps(const f32x16& hi_, const f32x16& lo_, const float* bias_, int col0_, u16* plane0_, int lane_, float ks_)
        : hi(hi_), lo(lo_), bias(bias_ + col0_), plane0(plane0_), col0(col0_), lane(lane_), r(lane_ & 31), ks(ks_), am(0.0f) {}
    __device__ __forceinline__ void chain_op(H2Chain& c, int g, int h, int i, const float4& b)
    {
        const int r0 = 4 * g + 2 * h;
        if (i == 0) { c.t0 = hi[r0] + lo[r0]; fs_pin(c.t0); }
        if (i == 1) { c.t1 = hi[r0 + 1] + lo[r0 + 1]; fs_pin(c.t1); }
        if (i == 2) { c.t0 = fmaf(c.t0, ks, h ? b.z : b.x); fs_pin(c.t0); }
        if (i == 3) { c.t1 = fmaf(c.t1, ks, h ? b.w : b.y); fs_pin(c.t1); }
        if (i == 4) { c.u0 = c.t0 * DF_SLOPE; fs_pin(c.u0); }
        if (i == 5) { c.u1 = c.t1 * DF_SLOPE; fs_pin(c.u1); }
        if (i == 6) { c.t0 = fmaxf(c.t0, c.u0); fs_pin(c.t0); }
        if (i == 7) { c.t1 = fmaxf(c.t1, c.u1); fs_pin(c.t1); }
        if (i >= HEAD_OPS) h2_split_op(c, am, i - HEAD_OPS);
    }
    __device__ __forceinline__ void op(int g, int o, int cb, int bs)
    {
        if (o == 0) bv[bs] = *reinterpret_cast<const float4*>(bias + acc_n(g, lane));
        else if (o <= 2 * CH) chain_op(k[cb + ((o - 1) & 1)], g, (o - 1) & 1, (o - 1) >> 1, bv[bs]);
        else {
            const int j = o - 2 * CH - 1;
            u16* q = plane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane)) + j * fs_plane<PITCH>();
            *reinterpret_cast<uint2*>(q) = j == 0 ? make_uint2(k[cb].a, k[cb + 1].a) : make_uint2(k[cb].b, k[cb + 1].b);
        }
    }
    // two groups at a time, FOUR chains interleaved (mlp_fused_h2.inc, H2EluOps): op t -> group 2 (t / 2 NG) + (t & 1), op (t % 2 NG) / 2 of it
    __device__ __forceinline__ void q(int t) { const int w = t & 1; op(2 * (t / (2 * NG)) + w, (t % (2 * NG)) >> 1, 2 * w, w); }
};

// dZ = dA LeakyReLU'(H) IN PLACE over H's planes (lane = row): dA = (hi + lo) / (s_z' s_w), what is split is dZ s_z: t = (hi + lo) qs
// with qs = s_z / (s_z' s_w), then the slope through the sign of H's LEADING fp16 term (df_dlrelu_op: a half's sign bit sits where a
// bf16's does).  Per group of four columns: the leading-term words of H (one 8-byte LDS read), two chains, two stores.
template <int PITCH>
struct DhDlreluOps {
    static constexpr int CH = 2 + DF_DLRELU_OPS + H2_SPLIT_OPS;            // 11 ops per chain
    static constexpr int NG = 1 + 2 * CH + 2 + 2, TOTAL = 4 * NG;          // ... + two ops that fold the group's LeakyReLU' flags into `negmask`
    const f32x16 &hi, &lo;
    u16* plane0;
    int col0, lane, r;
    float qs, am;
    unsigned negmask;       // bit 2 g + p (+ 16): column 8 g + 4 (lane >> 5) + 2 p (+ 1) of this lane's row has H <= 0 (the slope applies)
    uint2 hw[2];
    H2Chain k[4];
    __device__ __forceinline__ DhDlreluOps(const f32x16& hi_, const f32x16& lo_, int col0_, u16* plane0_, int lane_, float qs_)
        : hi(hi_), lo(lo_), plane0(plane0_), col0(col0_), lane(lane_), r(lane_ & 31), qs(qs_), am(0.0f), negmask(0u) {}
    // a packed pair of leading fp16 terms: the flag is set (the slope applies) exactly where df_dlrelu_op takes the slope for dA1,
    // i.e. where the term is <= 0 as a 16-bit integer -- +0.0 and -0.0 included.  Both zeros occur for nonzero pre-activations: the
    // leading term of h s_H2 flushes to +0.0 for 0 < z < 2^-25 / s_H2 and to -0.0 for 0 > z > -2^-25 / (0.01 s_H2) (LeakyReLU's
    // slope makes the negative window 100x wider).  x <= 0 <=> bit 15 of the SATURATING x - 1 is set (one v_pk_add_i16 ... clamp:
    // 0 -> -1, -0.0 = -32768 stays -32768; a wrapping subtraction would read -0.0 as 0x7fff, positive)
    __device__ __forceinline__ void fold(unsigned w, int kbit)
    {
        typedef short dh_s16x2 __attribute__((ext_vector_type(2)));
        dh_s16x2 x = __builtin_bit_cast(dh_s16x2, w);
        const dh_s16x2 one = {1, 1};
        x = __builtin_elementwise_sub_sat(x, one);
        negmask |= ((__builtin_bit_cast(unsigned, x) >> 15) & 0x00010001u) << kbit;
    }
    __device__ __forceinline__ void chain_op(H2Chain& c, int g, int h, int i, const uint2& w)
    {
        const int r0 = 4 * g + 2 * h;
        if (i == 0) { c.t0 = (hi[r0] + lo[r0]) * qs; fs_pin(c.t0); }
        if (i == 1) { c.t1 = (hi[r0 + 1] + lo[r0 + 1]) * qs; fs_pin(c.t1); }
        if (i >= 2 && i < 2 + DF_DLRELU_OPS) df_dlrelu_op(c.t0, c.t1, c.u0, c.u1, h ? w.y : w.x, i - 2);
        if (i >= 2 + DF_DLRELU_OPS) h2_split_op(c, am, i - 2 - DF_DLRELU_OPS);
    }
    __device__ __forceinline__ void op(int g, int o, int cb, int bs)
    {
        if (o == 0) hw[bs] = *reinterpret_cast<const uint2*>(plane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane)));
        else if (o <= 2 * CH) chain_op(k[cb + ((o - 1) & 1)], g, (o - 1) & 1, (o - 1) >> 1, hw[bs]);
        else if (o <= 2 * CH + 2) {
            const int j = o - 2 * CH - 1;
            u16* q = plane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane)) + j * fs_plane<PITCH>();
            *reinterpret_cast<uint2*>(q) = j == 0 ? make_uint2(k[cb].a, k[cb + 1].a) : make_uint2(k[cb].b, k[cb + 1].b);
        } else {
            const int p = o - 2 * CH - 3;
            fold(p ? hw[bs].y : hw[bs].x, 2 * g + p);
        }
    }
    // two groups at a time, FOUR chains interleaved (mlp_fused_h2.inc, H2EluOps): op t -> group 2 (t / 2 NG) + (t & 1), op (t % 2 NG) / 2 of it
    __device__ __forceinline__ void q(int t) { const int w = t & 1; op(2 * (t / (2 * NG)) + w, (t % (2 * NG)) >> 1, 2 * w, w); }
};

// dZ1 from the swapped-role dA1 GEMM (lane = column n, register reg = row acc_row(reg, lane)): register pair (8 ks + 2 m, + 1) and
// word m of the leading-term fragment of H1 (k-step ks) -> word m of the two dZ1^T fragments of k-step ks, which dW1 multiplies by as
// they are; the column sum db1 (still carrying s_z1) accumulates beside, one partial sum per interleaved chain.
struct DhDz1Ops {
    static constexpr int CH = 2 + DF_DLRELU_OPS + 2 + H2_SPLIT_OPS;        // 13 ops per chain
    static constexpr int TOTAL = 8 * CH;
    const f32x16 &hi, &lo;
    const df_u32x4 (&hw)[2];        // H1's leading-term fragments, k-steps 0 / 1
    df_u32x4 (&zw)[2][2];           // out: dZ1^T fragments [k-step][term]
    float qs, zs0, zs1, am;
    H2Chain k[2];
    __device__ __forceinline__ DhDz1Ops(const f32x16& hi_, const f32x16& lo_, const df_u32x4 (&hw_)[2], df_u32x4 (&zw_)[2][2], float qs_)
        : hi(hi_), lo(lo_), hw(hw_), zw(zw_), qs(qs_), zs0(0.0f), zs1(0.0f), am(0.0f) {}
    __device__ __forceinline__ void chain_op(int ch, int sl, int i)
    {
        const int ks = ch >> 2, m = ch & 3, reg = 8 * ks + 2 * m;
        H2Chain& c = k[sl];
        float& zs = sl ? zs1 : zs0;
        if (i == 0) { c.t0 = (hi[reg] + lo[reg]) * qs; fs_pin(c.t0); }
        if (i == 1) { c.t1 = (hi[reg + 1] + lo[reg + 1]) * qs; fs_pin(c.t1); }
        if (i >= 2 && i < 2 + DF_DLRELU_OPS) df_dlrelu_op(c.t0, c.t1, c.u0, c.u1, hw[ks][m], i - 2);
        if (i == 2 + DF_DLRELU_OPS) { zs += c.t0; fs_pin(zs); }
        if (i == 3 + DF_DLRELU_OPS) { zs += c.t1; fs_pin(zs); }
        if (i >= 4 + DF_DLRELU_OPS) {
            const int j = i - 4 - DF_DLRELU_OPS;
            h2_split_op(c, am, j);
            if (j == 0) zw[ks][0][m] = c.a;
            if (j == 4) zw[ks][1][m] = c.b;
        }
    }
    __device__ __forceinline__ void q(int t)
    {
        const int pp = t / (2 * CH), o = t % (2 * CH);
        chain_op(2 * pp + (o & 1), o & 1, o >> 1);
    }
    __device__ __forceinline__ float colsum() const { return zs0 + zs1; }
};

struct DhLds {
    u16 *Xt, *Xo, *H1, *H2, *Z3;
    float *part, *xs, *xs2, *bias, *bias_tgt, *rowloss, *sc, *amax;
    __device__ __forceinline__ explicit DhLds(u16* lds)
        : Xt(lds + DH_OFF_X), Xo(lds + DH_OFF_XO), H1(lds + DH_OFF_H1), H2(lds + DH_OFF_H2), Z3(lds + DH_OFF_Z3),
          part(reinterpret_cast<float*>(lds + DH_OFF_PART)), xs(reinterpret_cast<float*>(lds + DH_OFF_XS)),
          xs2(reinterpret_cast<float*>(lds + DH_OFF_XS2)),
          bias(reinterpret_cast<float*>(lds + DH_OFF_F32)), bias_tgt(bias + DF_BIAS), rowloss(bias_tgt + DF_BIAS), sc(rowloss + BM),
          amax(sc + H2_FSC_FLOATS) {}
};

// One 32 KB plane image LDS -> HBM: eight 16-byte reads per thread in flight, then eight stores (df_copy_image)
__device__ __forceinline__ void dh_copy_image(float4* __restrict__ dst, const float4* src, int tl)
{
    constexpr int PER = DH_IMAGE_HALVES / 8 / THREADS;          // 8
    static_assert(PER * THREADS * 8 == DH_IMAGE_HALVES && PER % 4 == 0, "whole float4 per thread");
    float4 v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) v[u] = src[tl + THREADS * u];
#pragma unroll
    for (int u = 0; u < PER; u += 4)
        asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w), "+v"(v[u + 1].x), "+v"(v[u + 1].y), "+v"(v[u + 1].z),
                          "+v"(v[u + 1].w), "+v"(v[u + 2].x), "+v"(v[u + 2].y), "+v"(v[u + 2].z), "+v"(v[u + 2].w), "+v"(v[u + 3].x),
                          "+v"(v[u + 3].y), "+v"(v[u + 3].z), "+v"(v[u + 3].w));
#pragma unroll
    for (int u = 0; u < PER; ++u) dst[tl + THREADS * u] = v[u];
}

// The Q-network forward of one 32-row tile on the two-plane images (df_forward).  `X` = the pass's input planes, `bias` = the network's
// b1 s_h1 | b2 s_h2 | b3 in LDS, `wc` = the class of its first weight matrix (DHC_W / DHC_WT).  am1 / am2: running maxima of
// |H1 s|, |H2 s| of this thread.  The input planes are made in MFMA gaps, never in the open (dqn_fused.inc converts them in front of each
// pass: 3.2k cycles per tile): XC (the target pass) makes the ONLINE pass's planes L.Xo from the staged rows L.xs2 in the second half of
// layer 2's first GEMM, whose guest is done at the half; the target pass's own planes were made a tile earlier, under dW1 (the caller).
// AHEAD: the target pass requests the online pass's first weights (w1n), the online pass dA2's two heads, in front of the last GEMM.
template <bool AHEAD, bool XC, int H1HEAD>
__device__ __forceinline__ void dh_forward(const DhLds& L, const u16* X, const u16* __restrict__ QHn, const float* bias, int wc,
                                           const WeightHeadH<H1HEAD>& w1, int tl, unsigned long long* sb, int slot0, WeightHead2& ahead0,
                                           WeightHead2& ahead1, const u16* __restrict__ ahead_w, WeightHeadH<4>& w1n,
                                           const u16* __restrict__ w1n_w, float& am1, float& am2, float& amx)
{
    const int wave = __builtin_amdgcn_readfirstlane(tl >> 6), lane = tl & 63, r = lane & 31;
    const float* sc = L.sc;
    const float k1 = sc[H2_FSC_INV + DHC_X] * sc[H2_FSC_INV + wc] * sc[DHC_H1];
    const float k2 = sc[H2_FSC_INV + DHC_H1] * sc[H2_FSC_INV + wc + 1] * sc[DHC_H2];
    WeightHeadH<4> w3;
    WeightHead2 w1b, w2a, w2b;
    df_stamp(sb, slot0);
    f32x16 hi, lo, hi0, lo0;
    h2_gemm_prefetch<DQN_IN_PAD>(w1b, QHn + DH_OFF_QH1, 2 * wave + 1, lane);
    h2_gemm<DQN_IN_PAD, FS_PX, false, true, H1HEAD>(w1, QHn + DH_OFF_QH1, 2 * wave, X, 0, hi0, lo0, lane);
    h2_gemm_prefetch<DQN_H>(w2a, QHn + DH_OFF_QH2, 2 * wave, lane);
    {
        DhLreluOps<FS_P1> e(hi0, lo0, bias, 64 * wave, L.H1, lane, k1);
        h2_gemm_host<DQN_IN_PAD, FS_PX, false>(w1b, QHn + DH_OFF_QH1, 2 * wave + 1, X, 0, hi, lo, lane, e);
        am1 = h2_nanmax(am1, e.am);
    }
    __syncthreads();                                                          // every wave's tile-a columns of H1 are stored
    df_stamp(sb, slot0 + 1);
    {
        DhLreluOps<FS_P1> e(hi, lo, bias, 64 * wave + 32, L.H1, lane, k1);     // layer 1, tile b
        if (XC) {
            H2XStoreOps xc(L.xs2, L.Xo, tl, sc[DHC_X]);                        // (the staged rows landed a tile ago: the caller drained)
            h2_gemm_host2<DQN_H, FS_P1, false, true, 2, 24, 1>(w2a, QHn + DH_OFF_QH2, 2 * wave, L.H1, 0, hi0, lo0, lane, e, xc);
            amx = h2_nanmax(amx, xc.am);
        } else {
            h2_gemm_host<DQN_H, FS_P1, false, true, 2, 24, 1>(w2a, QHn + DH_OFF_QH2, 2 * wave, L.H1, 0, hi0, lo0, lane, e);
        }
        am1 = h2_nanmax(am1, e.am);
    }
    h2_gemm_prefetch<DQN_H>(w2b, QHn + DH_OFF_QH2, 2 * wave + 1, lane);
    {
        DhLreluOps<FS_P1> e(hi0, lo0, bias + DQN_H, 64 * wave, L.H2, lane, k2);
        h2_gemm_host<DQN_H, FS_P1, false>(w2b, QHn + DH_OFF_QH2, 2 * wave + 1, L.H1, 0, hi, lo, lane, e);
        am2 = h2_nanmax(am2, e.am);
    }
    h2_gemm_prefetch<64, 4>(w3, QHn + DH_OFF_QH3 + (long)(4 * wave) * 1024, 0, lane);     // the last layer's k range of this wave
    if (AHEAD) {
        h2_gemm_prefetch<DQN_OUT>(ahead0, ahead_w, 2 * wave, lane);
        h2_gemm_prefetch<DQN_OUT>(ahead1, ahead_w, 2 * wave + 1, lane);
    } else {
        h2_gemm_prefetch<DQN_IN_PAD, 4>(w1n, w1n_w, 2 * wave, lane);
    }
    df_stamp(sb, slot0 + 2);
    // last layer: split-K over the four waves, the k range = this wave's OWN two tiles of H2 (MODE 2); the partials keep the factor
    // s_w3 s_h2 (dh_q_row removes it)
    {
        DhLreluOps<FS_P1> e(hi, lo, bias + DQN_H, 64 * wave + 32, L.H2, lane, k2);
        h2_gemm_host<64, FS_P1, false, true, 4, 6, 2>(w3, QHn + DH_OFF_QH3 + (long)(4 * wave) * 1024, 0, L.H2, 64 * wave, hi0, lo0, lane, e);
        am2 = h2_nanmax(am2, e.am);
    }
    float* pw = L.part + wave * (BM * DQN_OUT);
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(pw + r * DQN_OUT + 4 * ((acc_n(g, lane) >> 2) ^ ((r >> 1) & 7))) =
            make_float4(hi0[4 * g] + lo0[4 * g], hi0[4 * g + 1] + lo0[4 * g + 1], hi0[4 * g + 2] + lo0[4 * g + 2],
                        hi0[4 * g + 3] + lo0[4 * g + 3]);
    __syncthreads();
    df_stamp(sb, slot0 + 3);
}

// this thread's four Q values (df_q_row): the four partials summed in wave order, the scale factor removed, the bias added
__device__ __forceinline__ void dh_q_row(const DhLds& L, const float* bias3, float k3, int tl, float (&q)[4])
{
    const int lrow = tl >> 3, lq = tl & 7;
    const int cs = 4 * (lq ^ ((lrow >> 1) & 7));
    const float4 p0 = *reinterpret_cast<const float4*>(L.part + lrow * DQN_OUT + cs);
    const float4 p1 = *reinterpret_cast<const float4*>(L.part + BM * DQN_OUT + lrow * DQN_OUT + cs);
    const float4 p2 = *reinterpret_cast<const float4*>(L.part + 2 * BM * DQN_OUT + lrow * DQN_OUT + cs);
    const float4 p3 = *reinterpret_cast<const float4*>(L.part + 3 * BM * DQN_OUT + lrow * DQN_OUT + cs);
    const float4 b = *reinterpret_cast<const float4*>(bias3 + 4 * lq);
    q[0] = fmaf(((p0.x + p1.x) + p2.x) + p3.x, k3, b.x);
    q[1] = fmaf(((p0.y + p1.y) + p2.y) + p3.y, k3, b.y);
    q[2] = fmaf(((p0.z + p1.z) + p2.z) + p3.z, k3, b.z);
    q[3] = fmaf(((p0.w + p1.w) + p2.w) + p3.w, k3, b.w);
}

// the static scale of d loss / d Q: |dq| <= inv_B -> [2^2, 2^3)
__device__ __forceinline__ float dh_z3_scale(float inv_B) { return ldexpf(1.0f, H2_TARGET_EXP_GRAD - ilogbf(inv_B)); }

// chunks, tiles_per, images (u16 [S * tiles_per][2][DH_IMAGE_HALVES]), ws1 / ws2 / ws3, loss_part: dqn_chain_kernel's;
// fsc: the scale table (read only here); wsmax [gridDim.x][8]: this launch's class maxima of |scaled value| per workgroup (slots 0 .. 4)
__global__ __launch_bounds__(THREADS, 1) void dqn_chain_h2_kernel(
    const float* __restrict__ P, const u16* __restrict__ QH, const u16* __restrict__ QTH, const float* __restrict__ P_tgt,
    const u16* __restrict__ QH_tgt, const float* __restrict__ fsc, const DqnChunk* __restrict__ chunks, int S, long tiles_per,
    float discount, float inv_B, u16* __restrict__ images, float* __restrict__ ws1, float* __restrict__ ws2, float* __restrict__ ws3,
    float* __restrict__ wsmax, float* __restrict__ loss_part, unsigned long long* __restrict__ stamps, int dma)
{
    // dZ2's plane image does not leave (dqn_dw2r_h2_kernel rebuilds dZ2 from what a row of it IS: dq[r] W3[a_r, :] with LeakyReLU's
    // factor per column); in its place a 2304-byte record per tile in the second image slot -- float dq[r] s_z2 [32] | int a_r [32] |
    // the flags unsigned [8 column tiles][64 lanes of the dZ2 epilogue] (DhDlreluOps::negmask)
    extern __shared__ __attribute__((aligned(16))) u16 dh_lds[];
    const DhLds L(dh_lds);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the scale table, then the biases of both networks times the scale of the activation they are added to
    if (tid < H2_FSC_FLOATS) L.sc[tid] = fsc[tid];
#pragma unroll
    for (int c = 0; c < DH_NMAX; ++c) L.amax[c * THREADS + tid] = 0.0f;
    __syncthreads();
    {
        const float s1 = L.sc[DHC_H1], s2 = L.sc[DHC_H2];
        L.bias[tid] = P[DQN_OFF_B1 + tid] * s1;
        L.bias[DQN_H + tid] = P[DQN_OFF_B2 + tid] * s2;
        L.bias_tgt[tid] = P_tgt[DQN_OFF_B1 + tid] * s1;
        L.bias_tgt[DQN_H + tid] = P_tgt[DQN_OFF_B2 + tid] * s2;
        if (tid < DQN_OUT) { L.bias[2 * DQN_H + tid] = P[DQN_OFF_B3 + tid]; L.bias_tgt[2 * DQN_H + tid] = P_tgt[DQN_OFF_B3 + tid]; }
    }
    f32x16 aW1[2][3], aW3[2], aB3, aB2[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        aB3[i] = 0.0f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            aW3[a][i] = 0.0f; aB2[a][i] = 0.0f;
#pragma unroll
            for (int b = 0; b < 3; ++b) aW1[a][b][i] = 0.0f;
        }
    }
    float bs1[2] = {0.0f, 0.0f};
    float amx = 0.0f, am1 = 0.0f, am2 = 0.0f, amz2 = 0.0f, amz1 = 0.0f;
    __syncthreads();
    const float* sc = L.sc;
    const float sz3 = dh_z3_scale(inv_B), iz3 = 1.0f / sz3;
    const float k3 = sc[H2_FSC_INV + DHC_H2] * sc[H2_FSC_INV + DHC_W + 2], k3t = sc[H2_FSC_INV + DHC_H2] * sc[H2_FSC_INV + DHC_WT + 2];
    const float q2 = sc[DHC_Z2] * iz3 * sc[H2_FSC_INV + DHC_W + 2];                       // dZ2 s_z2 from the dA2 sums (s_z3 s_w3)
    const float q1 = sc[DHC_Z1] * sc[H2_FSC_INV + DHC_Z2] * sc[H2_FSC_INV + DHC_W + 1];   // dZ1 s_z1 from the dA1 sums (s_z2 s_w2)

    const unsigned ntiles = (unsigned)S * (unsigned)tiles_per, tper = (unsigned)tiles_per;
    if (blockIdx.x < ntiles) {
        const unsigned s0 = blockIdx.x / tper;
        const long off = (long)(blockIdx.x - s0 * tper) * BM * DQN_IN;
        df_rows_in(L.xs, chunks[s0].next_obs + off, tid, dma);
        df_rows_in(L.xs2, chunks[s0].obs + off, tid, dma);
    }
    float n_act = 0.0f, n_rew = 0.0f, n_done = 0.0f;
    WeightHead2 w1;                                       // the target pass's first weights: requested a phase ahead (here / under dW1; two
                                                          // k-steps: they live through dW1 and the tile boundary)
    if (blockIdx.x < ntiles) {
        const unsigned s0 = blockIdx.x / tper;
        const long r0 = (long)(blockIdx.x - s0 * tper) * BM + (tid >> 3);
        n_act = chunks[s0].act[r0]; n_rew = chunks[s0].reward[r0]; n_done = chunks[s0].done[r0];
        // the workgroup's FIRST tile: its target-pass planes are made here, in the open (every later tile's under the previous tile's dW1)
        h2_gemm_prefetch<DQN_IN_PAD>(w1, QH_tgt + DH_OFF_QH1, 2 * wave, tid & 63);
        fs_dma_drain();
        H2XStoreOps xc(L.xs, L.Xt, tid, sc[DHC_X]);
        xc.all();
        amx = h2_nanmax(amx, xc.am);
    }
    __syncthreads();
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tl = tid;
        asm volatile("" : "+v"(tl));                      // (keeps tile-invariant address arithmetic inside the loop)
        const int lane = tl & 63;
        const int lrow = tl >> 3, lq = tl & 7;
        const float r_act = n_act, r_rew = n_rew, r_done = n_done;
        unsigned long long* sb = (stamps != nullptr && tile == blockIdx.x + gridDim.x) ? stamps + 64L * blockIdx.x : nullptr;
        df_stamp(sb, 0);

        // ---- q_target(next_obs).max(1) (dqn.py:73-74) ----------------------------------------------------------------------
        const unsigned tile_n = tile + gridDim.x;
        const float *rows_n = nullptr, *rows_o = nullptr;
        const float *act_n = nullptr, *rew_n = nullptr, *done_n = nullptr;
        if (tile_n < ntiles) {
            const unsigned sn = tile_n / tper;
            const long rn = (long)(tile_n - sn * tper) * BM;
            const DqnChunk cn = chunks[sn];
            rows_n = cn.next_obs + rn * DQN_IN; rows_o = cn.obs + rn * DQN_IN;
            act_n = cn.act + rn + lrow; rew_n = cn.reward + rn + lrow; done_n = cn.done + rn + lrow;
        }
        WeightHead2 wt3a, wt3b;
        WeightHeadH<4> w1o;
        dh_forward<false, true, 2>(L, L.Xt, QH_tgt, L.bias_tgt, DHC_WT, w1, tl, sb, 1, wt3a, wt3b, nullptr, w1o, QH + DH_OFF_QH1, am1, am2, amx);
        float qn_max;
        {
            float q[4];
            dh_q_row(L, L.bias_tgt + 2 * DQN_H, k3t, tl, q);
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) m = (4 * lq + j < DQN_NACT) ? fmaxf(m, q[j]) : m;
            qn_max = df_max8(m);
        }
        __syncthreads();                                  // the partials are consumed, the online pass's X planes are whole; H1 / H2 free
        // ---- q(obs) (dqn.py:68) ----------------------------------------------------------------------------------------------
        df_stamp(sb, 5);
        dh_forward<true, false, 4>(L, L.Xo, QH, L.bias, DHC_W, w1o, tl, sb, 6, wt3a, wt3b, QTH + DH_OFF_QTH3, w1o, nullptr, am1, am2, amx);
        {   // everything that goes to or comes from HBM around the backward pass is issued HERE (dqn_fused.inc); the heads of dA2's two
            // GEMMs have landed and are pinned as whole 16-byte vectors
            typedef float df_f32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    float4 &u = wt3a.b[ks].p[pl], &v = wt3b.b[ks].p[pl];
                    df_f32x4 uu = {u.x, u.y, u.z, u.w}, vv = {v.x, v.y, v.z, v.w};
                    asm volatile("" : "+v"(uu), "+v"(vv));
                    u = make_float4(uu[0], uu[1], uu[2], uu[3]);
                    v = make_float4(vv[0], vv[1], vv[2], vv[3]);
                }
            if (act_n != nullptr) { n_act = *act_n; n_rew = *rew_n; n_done = *done_n; }
            if (rows_n != nullptr) {
                df_rows_in(L.xs, rows_n, tl, dma);
                df_rows_in(L.xs2, rows_o, tl, dma);
            }
        }
        {   // ---- TD target, Huber, d loss / d Q (dqn.py:69-79): eight lanes per row, four Q columns each -------------------------
            float q[4];
            dh_q_row(L, L.bias + 2 * DQN_H, k3, tl, q);
            const int idx = dqn_action_index(r_act, DQN_NACT);                 // (dqn.py:70)
            float sel = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) sel = (4 * lq + j == idx) ? q[j] : sel;
            const float q_val = fs_sum8(sel);                                  // one non-zero among the eight lanes: exact
            const DqnTdRow t = dqn_td_row(q_val, r_rew, discount, qn_max, r_done, inv_B);
            float unused = 0.0f;
            h2_store4<FS_P4>(L.Z3, lrow, 4 * lq, fs_dqn_dz3(lq, idx, t.dq * sz3), unused);
            if (lq == 0) {
                L.rowloss[lrow] = t.hub;
                float* rec = reinterpret_cast<float*>(images + tile * (2L * DH_IMAGE_HALVES) + DH_IMAGE_HALVES);
                rec[lrow] = t.dq * sc[DHC_Z2];
                reinterpret_cast<int*>(rec)[BM + lrow] = idx;
            }
        }
        __syncthreads();
        df_stamp(sb, 10);
        if (tl < 32) tile_loss_sum<1>(L.rowloss, tl, loss_part + tile);
        FsTr tr1, trx, tr4;
        fs_tr_init<FS_P1>(tr1, lane);
        fs_tr_init<FS_PX>(trx, lane);
        fs_tr_init<FS_P4>(tr4, lane);
        WeightHead2 wt2a, wt2b;
        h2_gemm_prefetch<DQN_H>(wt2a, QTH + DH_OFF_QTH2, 2 * wave, lane);          // dA1's first head: a phase ahead
        // H1's plane image (32 KB) leaves as it lies: the 256 x 256 layer's weight gradient is formed from it by dqn_dw2r_h2_kernel
        dh_copy_image(reinterpret_cast<float4*>(images + tile * (2L * DH_IMAGE_HALVES)), reinterpret_cast<const float4*>(L.H1), tl);
        f32x16 hi0, lo0, hi, lo;
        const f16x8 ones = h2_ones();
        {   // ---- dA2 = dZ3 . W3 -> dZ2 (in place over H2);  dW3 += dZ3^T H2;  db3 -----------------------------------------------
            // H2's fragments of THIS wave's two column tiles are read first and pinned: they must have landed before the first in-place store
            f16x8 af[2][2][2], zf[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) h2_trws<FS_P1>(af[t][ks], L.H2, tr1, 2 * wave + t, ks);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) h2_trns<FS_P4>(zf[ks], L.Z3, tr4, 0, ks);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) asm volatile("" : "+v"(af[t][ks][pl]));
            h2_gemm<DQN_OUT, FS_P4, false>(wt3a, QTH + DH_OFF_QTH3, 2 * wave, L.Z3, 0, hi0, lo0, lane);
            h2_gemm<DQN_OUT, FS_P4, false>(wt3b, QTH + DH_OFF_QTH3, 2 * wave + 1, L.Z3, 0, hi, lo, lane);
            {
                DhDlreluOps<FS_P1> e(hi0, lo0, 64 * wave, L.H2, lane, q2);
                h2_dw_host<0, 12>(aW3[0], zf[0], af[0][0], e);
                h2_dw_host<3, 12>(aW3[0], zf[1], af[0][1], e);
                h2_dw_host<6, 12>(aW3[1], zf[0], af[1][0], e);
                h2_dw_host<9, 12>(aW3[1], zf[1], af[1][1], e);
                amz2 = h2_nanmax(amz2, e.am);
                reinterpret_cast<unsigned*>(images + tile * (2L * DH_IMAGE_HALVES) + DH_IMAGE_HALVES)[2 * BM + (2 * wave) * 64 + lane] = e.negmask;
            }
            // db3 (wave 0) and db2 of this wave's first column tile: column sums through an all-ones operand (small term first)
            if (wave == 0) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int pl = 1; pl >= 0; --pl) aB3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, zf[ks][pl], aB3, 0, 0, 0);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                f16x8 z2[2];
                h2_trws<FS_P1>(z2, L.H2, tr1, 2 * wave, ks);
#pragma unroll
                for (int pl = 1; pl >= 0; --pl) aB2[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, z2[pl], aB2[0], 0, 0, 0);
            }
        }
        __syncthreads();                                  // every wave's tile-a columns of dZ2 are stored
        df_stamp(sb, 11);
        {   // ---- dA1 = dZ2 . W2 with the operand roles SWAPPED -> dZ1 as transposed fragments in registers;  dW1 += dZ1^T X ---------
            const int ct0 = 2 * wave, ct1 = 2 * wave + 1;
            h2_gemm_prefetch<DQN_H>(wt2b, QTH + DH_OFF_QTH2, ct1, lane);
            {
                DhDlreluOps<FS_P1> e(hi, lo, 64 * wave + 32, L.H2, lane, q2);
                h2_gemm_host<DQN_H, FS_P1, true, true, 2, 24, 1>(wt2a, QTH + DH_OFF_QTH2, ct0, L.H2, 0, hi0, lo0, lane, e);
                amz2 = h2_nanmax(amz2, e.am);
                reinterpret_cast<unsigned*>(images + tile * (2L * DH_IMAGE_HALVES) + DH_IMAGE_HALVES)[2 * BM + (2 * wave + 1) * 64 + lane] = e.negmask;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                f16x8 z2[2];
                h2_trws<FS_P1>(z2, L.H2, tr1, 2 * wave + 1, ks);
#pragma unroll
                for (int pl = 1; pl >= 0; --pl) aB2[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, z2[pl], aB2[1], 0, 0, 0);
            }
            df_u32x4 hw0[2], hw1[2], zw0[2][2], zw1[2][2];
            {
                f16x8 hf[2];
                h2_trws<FS_P1>(hf, L.H1, tr1, ct0, 0); hw0[0] = __builtin_bit_cast(df_u32x4, hf[0]);
                h2_trws<FS_P1>(hf, L.H1, tr1, ct0, 1); hw0[1] = __builtin_bit_cast(df_u32x4, hf[0]);
                h2_trws<FS_P1>(hf, L.H1, tr1, ct1, 0); hw1[0] = __builtin_bit_cast(df_u32x4, hf[0]);
                h2_trws<FS_P1>(hf, L.H1, tr1, ct1, 1); hw1[1] = __builtin_bit_cast(df_u32x4, hf[0]);
            }
            {
                DhDz1Ops e0(hi0, lo0, hw0, zw0, q1);
                h2_gemm_host<DQN_H, FS_P1, true>(wt2b, QTH + DH_OFF_QTH2, ct1, L.H2, 0, hi, lo, lane, e0);
                bs1[0] += e0.colsum();
                amz1 = h2_nanmax(amz1, e0.am);
            }
            // the next tile's rows (requested ~15k cycles ago) have landed: nothing younger than them is in flight HERE (the weight rings
            // were consumed, H1's image left at the top of the backward pass), so this wait is free
            fs_dma_drain();
            {
                DhDz1Ops e1(hi, lo, hw1, zw1, q1);
                const f16x8 z0[2] = {__builtin_bit_cast(f16x8, zw0[0][0]), __builtin_bit_cast(f16x8, zw0[0][1])};
                const f16x8 z1[2] = {__builtin_bit_cast(f16x8, zw0[1][0]), __builtin_bit_cast(f16x8, zw0[1][1])};
                f16x8 xf[2][2];
                h2_trns<FS_PX>(xf[0], L.Xo, trx, 0, 0); h2_trns<FS_PX>(xf[1], L.Xo, trx, 0, 1);
                h2_dw_host<0, 18>(aW1[0][0], z0, xf[0], e1); h2_dw_host<3, 18>(aW1[0][0], z1, xf[1], e1);
                h2_trns<FS_PX>(xf[0], L.Xo, trx, 1, 0); h2_trns<FS_PX>(xf[1], L.Xo, trx, 1, 1);
                h2_dw_host<6, 18>(aW1[0][1], z0, xf[0], e1); h2_dw_host<9, 18>(aW1[0][1], z1, xf[1], e1);
                h2_trns<FS_PX>(xf[0], L.Xo, trx, 2, 0); h2_trns<FS_PX>(xf[1], L.Xo, trx, 2, 1);
                h2_dw_host<12, 18>(aW1[0][2], z0, xf[0], e1); h2_dw_host<15, 18>(aW1[0][2], z1, xf[1], e1);
                bs1[1] += e1.colsum();
                amz1 = h2_nanmax(amz1, e1.am);
            }
            {   // the second column tile's dW1 (18 MFMAs) with the NEXT tile's target-pass planes (L.xs -> L.Xt: free since this tile's
                // target layer 1) in its gaps; its first weights requested in front
                const f16x8 z0[2] = {__builtin_bit_cast(f16x8, zw1[0][0]), __builtin_bit_cast(f16x8, zw1[0][1])};
                const f16x8 z1[2] = {__builtin_bit_cast(f16x8, zw1[1][0]), __builtin_bit_cast(f16x8, zw1[1][1])};
                if (rows_n != nullptr) {
                    h2_gemm_prefetch<DQN_IN_PAD>(w1, QH_tgt + DH_OFF_QH1, 2 * wave, lane);
                    H2XStoreOps xc(L.xs, L.Xt, tl, sc[DHC_X]);
                    f16x8 xf[2][2];
                    h2_trns<FS_PX>(xf[0], L.Xo, trx, 0, 0); h2_trns<FS_PX>(xf[1], L.Xo, trx, 0, 1);
                    h2_dw_host<0, 18>(aW1[1][0], z0, xf[0], xc); h2_dw_host<3, 18>(aW1[1][0], z1, xf[1], xc);
                    h2_trns<FS_PX>(xf[0], L.Xo, trx, 1, 0); h2_trns<FS_PX>(xf[1], L.Xo, trx, 1, 1);
                    h2_dw_host<6, 18>(aW1[1][1], z0, xf[0], xc); h2_dw_host<9, 18>(aW1[1][1], z1, xf[1], xc);
                    h2_trns<FS_PX>(xf[0], L.Xo, trx, 2, 0); h2_trns<FS_PX>(xf[1], L.Xo, trx, 2, 1);
                    h2_dw_host<12, 18>(aW1[1][2], z0, xf[0], xc); h2_dw_host<15, 18>(aW1[1][2], z1, xf[1], xc);
                    amx = h2_nanmax(amx, xc.am);
                } else {
#pragma unroll
                    for (int kt = 0; kt < 3; ++kt) {
                        f16x8 xf[2][2];
                        h2_trns<FS_PX>(xf[0], L.Xo, trx, kt, 0);
                        h2_trns<FS_PX>(xf[1], L.Xo, trx, kt, 1);
                        h2_dw(aW1[1][kt], z0, xf[0]);
                        h2_dw(aW1[1][kt], z1, xf[1]);
                    }
                }
            }
        }
        df_stamp(sb, 12);
        __syncthreads();            // every wave is done with X, H1 and dZ2 before the next tile's forward overwrites them
        df_stamp(sb, 13);
    }

    // ---- one partial slab per workgroup per UPDATE (dqn_chain_kernel's layout), the scale factors removed ---------------------------
    const int lane = tid & 63;
    const float u1 = sc[H2_FSC_INV + DHC_Z1] * sc[H2_FSC_INV + DHC_X], ub1 = sc[H2_FSC_INV + DHC_Z1];
    const float u3 = iz3 * sc[H2_FSC_INV + DHC_H2], ub2 = sc[H2_FSC_INV + DHC_Z2];
    float* o1 = ws1 + (long)blockIdx.x * DF_STRIDE1;
    float* o3 = ws3 + (long)blockIdx.x * DF_STRIDE3;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const int col = kt * 32 + (lane & 31);
            if (col < DQN_IN_PAD) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) o1[((2 * wave + t) * 32 + acc_row(reg, lane)) * DQN_IN_PAD + col] = aW1[t][kt][reg] * u1;
            }
        }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float v = bs1[t] + __shfl_xor(bs1[t], 32, 64);                    // db1 sits in the two lane halves of the swapped-role sums
        if (lane < 32) o1[DQN_H * DQN_IN_PAD + 32 * (2 * wave + t) + lane] = v * ub1;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) o3[acc_row(reg, lane) * DQN_H + (2 * wave + t) * 32 + (lane & 31)] = aW3[t][reg] * u3;
    }
    if (wave == 0 && lane < 32) o3[DQN_OUT * DQN_H + lane] = aB3[0] * iz3;
    if (lane < 32) {
#pragma unroll
        for (int t = 0; t < 2; ++t) ws2[(long)blockIdx.x * DF_STRIDE2 + DQN_H * DQN_H + 32 * (2 * wave + t) + lane] = aB2[t][0] * ub2;
    }
    // this workgroup's class maxima
    h2_amax_fold(L.amax, DH_SLOT_X, tid, amx);
    h2_amax_fold(L.amax, DH_SLOT_H1, tid, am1);
    h2_amax_fold(L.amax, DH_SLOT_H2, tid, am2);
    h2_amax_fold(L.amax, DH_SLOT_Z2, tid, amz2);
    h2_amax_fold(L.amax, DH_SLOT_Z1, tid, amz1);
    __syncthreads();
    for (int c = wave; c < DH_NMAX; c += NWAVE) {
        const float* a = L.amax + c * THREADS;
        float m = h2_nanmax(h2_nanmax(a[lane], a[lane + 64]), h2_nanmax(a[lane + 128], a[lane + 192]));     // (a NaN survives)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = h2_nanmax(m, __shfl_xor(m, o, 64));
        if (lane == 0) wsmax[(long)blockIdx.x * H2_NACT_CLASSES + c] = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dW2 = dZ2^T H1 over all tiles of the update (dqn_dw2_kernel) without dZ2's image: a row of dZ2 is dq[r] W3[a_r, :] with LeakyReLU'
// per column, so a k-step is H1's half image (16 KB by LDS-DMA) + the tile's 2304-byte record, and the kernel rebuilds its dZ2^T
// fragments in registers: per element one read of the W3 table (fp32 master rows, in LDS), a multiply by dq[r] s_z2, the flag's factor,
// then the two-term split -- in the fragment order of dw2h_frag (lane = column, elements 0 .. 3 = rows 4 hh .. + 3, 4 .. 7 = rows
// 8 + 4 hh .. + 3 of the 16-row k-step).  The slab leaves unscaled.
// The fragment of a 16-row half image of H1:
__device__ __forceinline__ void dw2h_frag(f16x8 (&f)[2], const u16* half0, const FsTr& t, int T)
{
    typedef __attribute__((address_space(3))) s16x4* lds_ptr;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const int xw = 32 * (T & 3);
    const u16* a = half0 + 32 * (T & ~3) + (t.lo ^ xw);
    const u16* b = half0 + 32 * (T & ~3) + (t.hi ^ xw);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + p * DW2_PLANE));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(b + p * DW2_PLANE));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        f[p] = __builtin_bit_cast(f16x8, v);
    }
}

constexpr int DW2R_REC_BYTES = 2 * BM * 4 + 8 * 64 * 4;                  // 2304
constexpr int DW2R_BUF_BYTES = 2 * DW2_PLANE * 2 + DW2R_REC_BYTES;        // 16384 + 2304
constexpr int DW2R_W3_FLOATS = DQN_NACT * DQN_H;
// A k-step's bytes arrive by LDS-DMA, five pieces per wave, four k-steps in LDS, counted waits.  (A/B: staged through registers instead,
// three k-steps in flight, 2.91 against 1.79 ms, DESIGN.md section 8b -- a DMA piece costs 0.1 - 0.2k cycles of issue beside MFMAs and a
// plain load + ds_write_b128 a quarter of that, but beside 256 accumulator registers and eight H1 fragments the 60-register staging
// ring spills (7 registers, 272 B of scratch per lane); not kept.)
constexpr int DW2R_NBUF = 4;
constexpr int DW2R_LDS_BYTES = DW2R_NBUF * DW2R_BUF_BYTES + DW2R_W3_FLOATS * 4 + 1024;   // (+ a dump slot: the fetch's fifth piece of wave 3)

__global__ __launch_bounds__(THREADS, 1) void dqn_dw2r_h2_kernel(const u16* __restrict__ images, long ntiles, const float* __restrict__ P,
                                                                   const float* __restrict__ fsc, float* __restrict__ ws2)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dwr_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // this wave's output tiles: n' tiles (dZ2 columns) 2 wave, 2 wave + 1 x ALL eight k tiles (H1 columns) -- not dqn_dw2_kernel's 4 x 4:
    // a dZ2^T fragment is rebuilt by exactly one wave (with 4 x 4 two waves would rebuild each), at the price of eight H1 fragments
    // per k-step instead of four (transposing LDS reads: nearly free beside MFMAs)
    const int nt0 = 2 * wave;
    float* w3 = reinterpret_cast<float*>(dwr_lds + DW2R_NBUF * DW2R_BUF_BYTES);
    for (int i = tid; i < DW2R_W3_FLOATS; i += THREADS) w3[i] = P[DQN_OFF_W3 + i];
    f32x16 acc[2][8];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b][i] = 0.0f;
    FsTr tr1;
    fs_tr_init<FS_P1>(tr1, lane);
    const long my_tiles = blockIdx.x < ntiles ? (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    const long steps = 2 * my_tiles;
    // this lane's place in a dZ2^T fragment: column jj of the tile, rows rho(e); where that column's flag sits in the record
    const int jj = lane & 31, hh = lane >> 5;
    const int fl_lane = ((jj >> 2) & 1) * 32;                              // the epilogue lane half that owned column jj
    const unsigned fl_bitmask = 1u << (2 * (jj >> 3) + ((jj >> 1) & 1) + 16 * (jj & 1));     // its bit of `negmask` (DhDlreluOps)
    // the products of k-step j from LDS buffer `buf` (H1's half image | the record)
    auto products = [&](long j, int buf) {
        const int half = (int)(j & 1);
        const unsigned char* bb = dwr_lds + buf * DW2R_BUF_BYTES;
        const u16* hb = reinterpret_cast<const u16*>(bb);                        // H1 half image
        const float* rec_dq = reinterpret_cast<const float*>(bb + 2 * DW2_PLANE * 2);
        const int* rec_act = reinterpret_cast<const int*>(rec_dq) + BM;
        const unsigned* rec_mask = reinterpret_cast<const unsigned*>(rec_dq) + 2 * BM;
        f16x8 af[8][2];
#pragma unroll
        for (int b = 0; b < 8; ++b) dw2h_frag(af[b], hb, tr1, b);
        // the eight rows of this lane's fragment elements: dq s_z2 (and its product with the slope) and the W3 row
        float dq[8], dqs[8];
        const float* wrow[8];
        const unsigned* mrow[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int row = 16 * half + (e < 4 ? 4 * hh + e : 8 + 4 * hh + (e - 4));
            dq[e] = rec_dq[row];
            dqs[e] = dq[e] * DF_SLOPE;
            wrow[e] = w3 + rec_act[row] * DQN_H + jj;
            mrow[e] = rec_mask + fl_lane + row;
        }
        auto rebuild = [&](f16x8 (&zf)[2], int T) {
            float t[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned m = mrow[e][T * 64];
                t[e] = wrow[e][32 * T] * ((m & fl_bitmask) ? dqs[e] : dq[e]);
            }
            unsigned za[4], zb[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) h2_split2(t[2 * p], t[2 * p + 1], za[p], zb[p]);
            const df_u32x4 qa = {za[0], za[1], za[2], za[3]}, qb = {zb[0], zb[1], zb[2], zb[3]};
            zf[0] = __builtin_bit_cast(f16x8, qa);
            zf[1] = __builtin_bit_cast(f16x8, qb);
        };
        f16x8 zf[2][2];
        rebuild(zf[0], nt0);
        rebuild(zf[1], nt0 + 1);                          // (independent of the first tile's products: the scheduler runs it beside them)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) h2_dw(acc[a][b], zf[a], af[b]);
    };
    typedef __attribute__((address_space(3))) void* lptr_t;
    const unsigned lds0 = (unsigned)(unsigned long)(lptr_t)dwr_lds;
    // one k-step: H1's half image = 2 planes x 8 pieces of 1 KB (16 wave-instructions, four per wave) + the record (144 16-byte pieces:
    // waves 0 .. 2; wave 3 issues a fifth instruction too -- the record's first KB once more, into a dump slot -- so that EVERY wave has
    // exactly five loads per k-step in flight and the counted waits below are the same immediate for all)
    auto fetch = [&](long j, int buf) {
        const long tile = blockIdx.x + (j >> 1) * gridDim.x;
        const u16* src = images + tile * (2L * DH_IMAGE_HALVES) + (j & 1) * DW2_PLANE;
        const unsigned base = lds0 + (unsigned)(buf * DW2R_BUF_BYTES);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = 4 * wave + i, p = piece >> 3, sub = piece & 7;
            const u16* g = src + (long)p * (2 * DW2_PLANE) + sub * 512 + lane * 8;
            const unsigned dst = base + 2u * (unsigned)(p * DW2_PLANE + sub * 512);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "s"(dst), "v"(g) : "memory", "scc");
        }
        if (wave == 3 || 64 * wave + lane < DW2R_REC_BYTES / 16) {
            const int rw = wave == 3 ? 0 : wave;
            const u16* g = images + tile * (2L * DH_IMAGE_HALVES) + DH_IMAGE_HALVES + (64 * rw + lane) * 8;
            const unsigned dst = wave == 3 ? lds0 + (unsigned)(DW2R_NBUF * DW2R_BUF_BYTES + DW2R_W3_FLOATS * 4)
                                           : base + (unsigned)(2 * DW2_PLANE * 2 + 1024 * wave);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "s"(dst), "v"(g) : "memory", "scc");
        }
    };
    for (int u = 0; u < DW2R_NBUF - 1; ++u)
        if (u < steps) fetch(u, u);
    for (long j = 0; j < steps; ++j) {
        const int buf = (int)(j % DW2R_NBUF);
        // this wave's five loads of k-step j have landed when at most the newer k-steps' (two, one or none near the end) are in flight:
        // loads return in order.  (An HBM round trip is ~4k cycles, a k-step's products ~1.7k: one k-step ahead is not enough.)
        const long newer = steps - 1 - j;
        if (newer >= 2) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (newer == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                  // ... and everybody's (the W3 table too, the first time); k-step j - 1 is read out
        if (j + DW2R_NBUF - 1 < steps) fetch(j + DW2R_NBUF - 1, (int)((j + DW2R_NBUF - 1) % DW2R_NBUF));
        products(j, buf);
    }
    const float u2 = fsc[H2_FSC_INV + DHC_Z2] * fsc[H2_FSC_INV + DHC_H1];
    float* o2 = ws2 + (long)blockIdx.x * DF_STRIDE2;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                o2[((nt0 + a) * 32 + acc_row(reg, lane)) * DQN_H + b * 32 + (lane & 31)] = acc[a][b][reg] * u2;
}

// ---- scale bookkeeping ------------------------------------------------------------------------------------------------------------
// After an update's gradient: the maximum over workgroups of every tracked class -> the NEXT update's scale (the launch's maximum
// would land in the class's window); a maximum that did not fit fp16 (or a NaN) sets *ovf.  One block, one wave per tracked class.
__global__ __launch_bounds__(64 * DH_NMAX) void dqn_h2_scales_kernel(const float* __restrict__ wsmax, int wgs, float* __restrict__ fsc,
                                                                       int* __restrict__ ovf, int freeze)
{
    const int lane = threadIdx.x & 63, slot = threadIdx.x >> 6, c = dh_slot_class(slot);
    float m = 0.0f;
    bool nan = false;
    for (int w = lane; w < wgs; w += 64) { const float v = wsmax[(long)w * H2_NACT_CLASSES + slot]; nan |= !(v == v); m = fmaxf(m, v); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    nan = __any(nan);
    if (lane == 0) {
        const float s_old = fsc[c];
        const bool over = nan || !(m < H2_F16_MAX);
        float s_new = s_old;
        if (nan || !(m < 3.0e38f)) s_new = s_old * 0.00390625f;
        else if (m > 0.0f) s_new = ldexpf(s_old, h2_target_exp(c) - ilogbf(m));
        s_new = fminf(fmaxf(s_new, 0x1p-100f), 0x1p100f);
        if (!freeze) { fsc[c] = s_new; fsc[H2_FSC_INV + c] = 1.0f / s_new; }
        fsc[32 + c] = m;
        if (over) *ovf = 1;
    }
}

// In front of every update: per-layer max |w| of both networks -> their scales (max(max |w|, 2^-4) into [2^11, 2^12)), then the
// two-term planes of every weight: online forward (QH) / transposed (QTH), target forward (QH_tgt).  idx_fb / idx_tb: the bf16x3 plane
// maps (term-0 position kf in a 1536-word block layout; here block kf / 1536 is 1024 words, term 1 follows 512 words later).
// Every block takes the six maxima itself (758 KB of L2 reads per block: nothing beside an update).
constexpr int DH_PL_THREADS = 1024, DH_PL_BLOCKS = (DQN_PACKED_FLOATS + DH_PL_THREADS - 1) / DH_PL_THREADS;
__global__ __launch_bounds__(DH_PL_THREADS) void dqn_h2_planes_kernel(const float* __restrict__ P, const float* __restrict__ P_tgt,
                                                                        const int* __restrict__ idx_fb, const int* __restrict__ idx_tb,
                                                                        u16* __restrict__ QH, u16* __restrict__ QTH, u16* __restrict__ QH_tgt,
                                                                        float* __restrict__ fsc)
{
    __shared__ float s_m[6][DH_PL_THREADS / 64], s_s[6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int lo[3] = {DQN_OFF_W1, DQN_OFF_W2, DQN_OFF_W3}, hi[3] = {DQN_OFF_B1, DQN_OFF_B2, DQN_OFF_B3};
#pragma unroll
    for (int l = 0; l < 3; ++l)
        for (int i = lo[l] + 4 * tid; i < hi[l]; i += 4 * DH_PL_THREADS) {
            const float4 a = *reinterpret_cast<const float4*>(P + i), b = *reinterpret_cast<const float4*>(P_tgt + i);
            m[l] = fmaxf(m[l], fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))));
            m[3 + l] = fmaxf(m[3 + l], fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
        }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m[c] = fmaxf(m[c], __shfl_xor(m[c], o, 64));
        if (lane == 0) s_m[c][wave] = m[c];
    }
    __syncthreads();
    if (tid < 6) {
        float v = 0.0f;
        for (int w = 0; w < DH_PL_THREADS / 64; ++w) v = fmaxf(v, s_m[tid][w]);
        const float s = ldexpf(1.0f, 11 - ilogbf(fmaxf(v, 0.0625f)));
        s_s[tid] = s;
        if (blockIdx.x == 0) { fsc[DHC_W + tid] = s; fsc[H2_FSC_INV + DHC_W + tid] = 1.0f / s; fsc[32 + DHC_W + tid] = v; }
    }
    __syncthreads();
    const int i = blockIdx.x * DH_PL_THREADS + tid;
    if (i >= DQN_PACKED_FLOATS) return;
    const int kf = idx_fb[i], kt = idx_tb[i];
    if (kf < 0 && kt < 0) return;
    const int l = i < DQN_OFF_W2 ? 0 : (i < DQN_OFF_W3 ? 1 : 2);
    unsigned a, b;
    h2_split2(P[i] * s_s[l], 0.0f, a, b);
    if (kf >= 0) { const int hf = (kf / 1536) * 1024 + kf % 1536; QH[hf] = (u16)a; QH[hf + 512] = (u16)b; }
    if (kt >= 0) { const int ht = (kt / 1536) * 1024 + kt % 1536; QTH[ht] = (u16)a; QTH[ht + 512] = (u16)b; }
    h2_split2(P_tgt[i] * s_s[3 + l], 0.0f, a, b);
    if (kf >= 0) { const int hf = (kf / 1536) * 1024 + kf % 1536; QH_tgt[hf] = (u16)a; QH_tgt[hf + 512] = (u16)b; }
}
