// dqn_fused.inc — one DQN update (reference UselessFiles/dqn.py:64-85; BASELINE configs[4]) in TWO persistent launches over ALL its
// sampled replay steps, bf16x3 arithmetic (three-term bf16 operand splits on v_mfma_f32_32x32x16_bf16, fp32 accumulate: mlp_layout.h):
//
//   dqn_chain_kernel   per 32-row tile, in the workgroup that owns it (one workgroup per CU, 4 waves, one per SIMD): target-network
//                      forward of next_obs -> max_a, online forward of obs, TD target, Huber loss and its gradient at the Q table,
//                      the dX chain down to dZ1, and dW1 / dW3 / db1 / db3 accumulated IN REGISTERS across the workgroup's tiles
//                      (the weights do not change inside an update, so the accumulators live through all sampled steps: one
//                      partial slab per workgroup per UPDATE).  Activations and gradients live in LDS as swizzled three-term
//                      plane images (fs_common.inc) and never go to HBM -- except the two images the 256 x 256 layer's weight
//                      gradient needs, H1 and dZ2, which are copied out AS THEY LIE IN LDS (96 KB per tile);
//   dqn_dw2_kernel     dW2 = dZ2^T H1 over all rows of the update: every workgroup holds the whole 256 x 256 product
//                      (64 tiles, 16 per wave, in the accumulator registers), LDS-DMAs the saved images back 16 rows at a time
//                      (double-buffered: no vector work at all, the split into terms happened where the values were made) and
//                      reads them through the transposing LDS reads; one partial slab per workgroup per update (db2 comes from the chain kernel).
//
// Why two launches: the 256 x 256 layer alone is 64 accumulator tiles, 96 with the other two layers = 24 per wave = 384 of the
// 512 registers a wave can have; the chain GEMMs and their epilogues do not fit beside that (DESIGN.md section 3.5).
// The three-launch fp32-MFMA path (dqn_td_kernel + dqn_grad_w_kernel per sampled step) stays as the A/B and for ragged row counts.
constexpr int DF_OFF_X = 0;                                              // X planes [32][96] x 3 (obs or next_obs of the tile)
constexpr int DF_OFF_H1 = DF_OFF_X + 3 * BM * FS_PX;                     // H1 planes [32][256] x 3
constexpr int DF_OFF_H2 = DF_OFF_H1 + 3 * BM * FS_P1;                    // H2 planes [32][256] x 3; dZ2 overwrites them in place
constexpr int DF_OFF_PART = DF_OFF_H2 + 3 * BM * FS_P1;                  // fp32 [4][32][32]: the last layer's split-K partials
constexpr int DF_OFF_Z3 = DF_OFF_PART + 4 * BM * DQN_OUT * 2;            // dZ3 planes [32][32] x 3
constexpr int DF_OFF_XS = DF_OFF_Z3 + 3 * BM * FS_P4;                    // fp32 [32][73]: a tile's rows as they lie in HBM
constexpr int DF_XS_HALVES = (BM * DQN_IN * 2 + 7) & ~7;
constexpr int DF_OFF_XS2 = DF_OFF_XS + DF_XS_HALVES;                     // the same for the tile's other row block (xs: next_obs, xs2: obs)
constexpr int DF_OFF_F32 = DF_OFF_XS2 + DF_XS_HALVES;                    // fp32 tail: online b1 | b2 | b3, target b1 | b2 | b3, row loss
constexpr int DF_BIAS = 2 * DQN_H + DQN_OUT;                             // 544
constexpr int DF_TAIL_FLOATS = 2 * DF_BIAS + BM;
constexpr int DF_LDS_BYTES = DF_OFF_F32 * 2 + DF_TAIL_FLOATS * 4;
constexpr int DF_IMAGE_HALVES = 3 * BM * FS_P1;                          // one saved image (H1 or dZ2) of a tile: 24576 16-bit words
static_assert(DF_LDS_BYTES <= 160 * 1024, "fits one CU");
static_assert(FS_IN == DQN_IN, "the x conversion slices are written for 73 input columns");
constexpr float DF_SLOPE = 0.01f;                                        // nn.LeakyReLU() default

// x > 0 ? x : slope x, as max(x, slope x): the same bits for every non-NaN x (slope in (0, 1)), one compare-select cheaper
__device__ __forceinline__ float df_lrelu(float x) { return fmaxf(x, x * DF_SLOPE); }
// dA * LeakyReLU'(pre-activation) through the saved OUTPUT h (same sign; h == 0 -> slope, as torch and as dqn_td_kernel)
__device__ __forceinline__ float df_dlrelu(float da, float h) { return h > 0.0f ? da : da * DF_SLOPE; }

// ---- epilogues as single-instruction ops -------------------------------------------------------------------------------------------
// One wave per SIMD pays ~8 cycles for a vector instruction that needs the result of the one before it and ~4.5 for an independent one
// (tools/mfma_fill_forms.hip); behind an MFMA about four independent instructions are free.  An epilogue written as a loop over output
// groups is one long dependent chain per pair of outputs (add, add, mul, max, then three rounds of convert / widen / subtract), and the
// compiler's schedule keeps most of that chain order: ~170 instructions cost 1.2 - 1.5k cycles, hosted in MFMA gaps or not (measured:
// four-to-six-instruction slices in the gaps of the next column tile's GEMM made that GEMM slower by exactly the epilogue's length).
// So the epilogue is written as OPS -- one instruction each, pinned where it is written -- of CHAINS (one pair of adjacent outputs
// each), and the order in which ops are issued interleaves chains: consecutive instructions never depend on each other.
//   hosted (q(t), fs_gemm_host): two chains interleaved, 1 - 2 ops per MFMA gap -> free where the GEMM has >= 84 gaps (layer 2)
//   exposed (all()): four chains interleaved
// The operations on every value and their order are ((hi + lo) + bias), max(y, slope y), split3x2: an unsliced loop's.
// dA * LeakyReLU'(z) for a PAIR, through the sign of the saved activation's LEADING bf16 term (`w` = the packed pair of leading terms:
// low half = first value).  h = LeakyReLU(z) has z's sign, and its leading term RNE_bf16(h) has h's sign -- or is zero, which it is for
// h == 0 (then the slope applies, as in torch and in dqn_td_kernel) and for 0 < |h| <= 2^-134 (a pre-activation in (0, 4.6e-41]: there,
// and only there, this takes the slope where the exact rule takes 1).  Saves recombining h from its three terms (10 instructions and
// two LDS reads per pair).  ops i = 0 .. 6 on (t0, t1) = dA.
__device__ __forceinline__ void df_dlrelu_op(float& t0, float& t1, float& u0, float& u1, unsigned w, int i)
{
    if (i == 0) { u0 = t0 * DF_SLOPE; fs_pin(u0); }
    if (i == 1) { u1 = t1 * DF_SLOPE; fs_pin(u1); }
    if (i == 2) { t0 = (int)(w << 16) > 0 ? t0 : u0; fs_pin(t0); }
    if (i == 3) { t1 = (int)w > 0xffff ? t1 : u1; fs_pin(t1); }
}
constexpr int DF_DLRELU_OPS = 4;

template <int PITCH>
struct DfLreluOps {
    static constexpr int HEAD_OPS = 8, CH = HEAD_OPS + FS_SPLIT_OPS;       // 19 ops per chain
    static constexpr int NG = 1 + 2 * CH + 3, TOTAL = 4 * NG;              // per group: bias load, two chains, three stores
    const f32x16 &hi, &lo;
    const float* bias;      // + col0
    u16* plane0;
    int col0, lane, r;
    float4 bv[2];
    FsChain k[4];
    __device__ __forceinline__ DfLreluOps(const f32x16& hi_, const f32x16& lo_, const float* bias_, int col0_, u16* plane0_, int lane_)
        : hi(hi_), lo(lo_), bias(bias_ + col0_), plane0(plane0_), col0(col0_), lane(lane_), r(lane_ & 31) {}
    __device__ __forceinline__ void chain_op(FsChain& c, int g, int h, int i, const float4& b)
    {
        const int r0 = 4 * g + 2 * h;
        if (i == 0) { c.t0 = hi[r0] + lo[r0]; fs_pin(c.t0); }
        if (i == 1) { c.t1 = hi[r0 + 1] + lo[r0 + 1]; fs_pin(c.t1); }
        if (i == 2) { c.t0 += h ? b.z : b.x; fs_pin(c.t0); }
        if (i == 3) { c.t1 += h ? b.w : b.y; fs_pin(c.t1); }
        if (i == 4) { c.u0 = c.t0 * DF_SLOPE; fs_pin(c.u0); }
        if (i == 5) { c.u1 = c.t1 * DF_SLOPE; fs_pin(c.u1); }
        if (i == 6) { c.t0 = fmaxf(c.t0, c.u0); fs_pin(c.t0); }
        if (i == 7) { c.t1 = fmaxf(c.t1, c.u1); fs_pin(c.t1); }
        if (i >= HEAD_OPS) fs_split_op(c, i - HEAD_OPS);
    }
    // op o of group g on chains k[cb], k[cb + 1] with bias register bv[bs]
    __device__ __forceinline__ void op(int g, int o, int cb, int bs)
    {
        if (o == 0) bv[bs] = *reinterpret_cast<const float4*>(bias + acc_n(g, lane));
        else if (o <= 2 * CH) chain_op(k[cb + ((o - 1) & 1)], g, (o - 1) & 1, (o - 1) >> 1, bv[bs]);
        else {
            u16* q = plane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane)) + (o - 2 * CH - 1) * fs_plane<PITCH>();
            const int j = o - 2 * CH - 1;
            *reinterpret_cast<uint2*>(q) = j == 0 ? make_uint2(k[cb].a, k[cb + 1].a) : j == 1 ? make_uint2(k[cb].b, k[cb + 1].b)
                                                                                              : make_uint2(k[cb].c, k[cb + 1].c);
        }
    }
    __device__ __forceinline__ void q(int t) { op(t / NG, t % NG, 0, 0); }
    // (template recursion, not loops: see FsGemmHost)
    template <int GP, int O>
    __device__ __forceinline__ void all_rec()
    {
        if constexpr (GP < 4) {
            op(GP, O, 0, 0);
            op(GP + 1, O, 2, 1);
            if constexpr (O + 1 < NG) all_rec<GP, O + 1>(); else all_rec<GP + 2, 0>();
        }
    }
    __device__ __forceinline__ void all()
    {
        all_rec<0, 0>();
        __builtin_amdgcn_sched_barrier(0);
    }
};

// dZ = dA * LeakyReLU'(H) IN PLACE over H's planes (lane = row), as ops: per group of four columns the leading-term words of H (one
// 8-byte LDS read), two chains, three stores
template <int PITCH>
struct DfDlreluOps {
    static constexpr int CH = 2 + DF_DLRELU_OPS + FS_SPLIT_OPS;            // 17 ops per chain
    static constexpr int NG = 1 + 2 * CH + 3, TOTAL = 4 * NG;
    const f32x16 &hi, &lo;
    u16* plane0;
    int col0, lane, r;
    uint2 hw[2];
    FsChain k[4];
    __device__ __forceinline__ DfDlreluOps(const f32x16& hi_, const f32x16& lo_, int col0_, u16* plane0_, int lane_)
        : hi(hi_), lo(lo_), plane0(plane0_), col0(col0_), lane(lane_), r(lane_ & 31) {}
    __device__ __forceinline__ void chain_op(FsChain& c, int g, int h, int i, const uint2& w)
    {
        const int r0 = 4 * g + 2 * h;
        if (i == 0) { c.t0 = hi[r0] + lo[r0]; fs_pin(c.t0); }
        if (i == 1) { c.t1 = hi[r0 + 1] + lo[r0 + 1]; fs_pin(c.t1); }
        if (i >= 2 && i < 2 + DF_DLRELU_OPS) df_dlrelu_op(c.t0, c.t1, c.u0, c.u1, h ? w.y : w.x, i - 2);
        if (i >= 2 + DF_DLRELU_OPS) fs_split_op(c, i - 2 - DF_DLRELU_OPS);
    }
    __device__ __forceinline__ void op(int g, int o, int cb, int bs)
    {
        if (o == 0) hw[bs] = *reinterpret_cast<const uint2*>(plane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane)));
        else if (o <= 2 * CH) chain_op(k[cb + ((o - 1) & 1)], g, (o - 1) & 1, (o - 1) >> 1, hw[bs]);
        else {
            const int j = o - 2 * CH - 1;
            u16* q = plane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane)) + j * fs_plane<PITCH>();
            *reinterpret_cast<uint2*>(q) = j == 0 ? make_uint2(k[cb].a, k[cb + 1].a) : j == 1 ? make_uint2(k[cb].b, k[cb + 1].b)
                                                                                              : make_uint2(k[cb].c, k[cb + 1].c);
        }
    }
    __device__ __forceinline__ void q(int t) { op(t / NG, t % NG, 0, 0); }
    template <int GP, int O>
    __device__ __forceinline__ void all_rec()
    {
        if constexpr (GP < 4) {
            op(GP, O, 0, 0);
            op(GP + 1, O, 2, 1);
            if constexpr (O + 1 < NG) all_rec<GP, O + 1>(); else all_rec<GP + 2, 0>();
        }
    }
    __device__ __forceinline__ void all()
    {
        all_rec<0, 0>();
        __builtin_amdgcn_sched_barrier(0);
    }
};

// dZ1 from the swapped-role dA1 GEMM (lane = column n, register reg = row acc_row(reg, lane)): register pair (8 ks + 2 m, + 1) and
// word m of the leading-term fragment of H1 (k-step ks) -> word m of the three dZ1^T fragments of k-step ks, which dW1 multiplies by
// as they are (no LDS round trip); the column sum db1 accumulates beside (two partial sums, one per interleaved chain: fixed order).
typedef unsigned df_u32x4 __attribute__((ext_vector_type(4)));
struct DfDz1Ops {
    static constexpr int CH = 2 + DF_DLRELU_OPS + 2 + FS_SPLIT_OPS;        // 19 ops per chain
    static constexpr int TOTAL = 8 * CH;
    const f32x16 &hi, &lo;
    const df_u32x4 (&hw)[2];        // H1's leading-term fragments, k-steps 0 / 1
    df_u32x4 (&zw)[2][3];           // out: dZ1^T fragments [k-step][term]
    float zs0, zs1;
    FsChain k[2];
    __device__ __forceinline__ DfDz1Ops(const f32x16& hi_, const f32x16& lo_, const df_u32x4 (&hw_)[2], df_u32x4 (&zw_)[2][3])
        : hi(hi_), lo(lo_), hw(hw_), zw(zw_), zs0(0.0f), zs1(0.0f) {}
    // op i of chain ch (= 4 ks + m) in state slot sl
    __device__ __forceinline__ void chain_op(int ch, int sl, int i)
    {
        const int ks = ch >> 2, m = ch & 3, reg = 8 * ks + 2 * m;
        FsChain& c = k[sl];
        float& zs = sl ? zs1 : zs0;
        if (i == 0) { c.t0 = hi[reg] + lo[reg]; fs_pin(c.t0); }
        if (i == 1) { c.t1 = hi[reg + 1] + lo[reg + 1]; fs_pin(c.t1); }
        if (i >= 2 && i < 2 + DF_DLRELU_OPS) df_dlrelu_op(c.t0, c.t1, c.u0, c.u1, hw[ks][m], i - 2);
        if (i == 2 + DF_DLRELU_OPS) { zs += c.t0; fs_pin(zs); }
        if (i == 3 + DF_DLRELU_OPS) { zs += c.t1; fs_pin(zs); }
        if (i >= 4 + DF_DLRELU_OPS) {
            const int j = i - 4 - DF_DLRELU_OPS;
            fs_split_op(c, j);
            if (j == 0) zw[ks][0][m] = c.a;
            if (j == 5) zw[ks][1][m] = c.b;
            if (j == 10) zw[ks][2][m] = c.c;
        }
    }
    // two chains interleaved: ops 2 CH pp .. 2 CH (pp + 1) - 1 belong to chains 2 pp, 2 pp + 1
    __device__ __forceinline__ void q(int t)
    {
        const int pp = t / (2 * CH), o = t % (2 * CH);
        chain_op(2 * pp + (o & 1), o & 1, o >> 1);
    }
    __device__ __forceinline__ float colsum() const { return zs0 + zs1; }
};

__device__ __forceinline__ void df_stamp(unsigned long long* buf, int slot)
{
    if (buf != nullptr && threadIdx.x == 0) {
        unsigned long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
        buf[slot] = t;
    }
}

__device__ __forceinline__ float df_max8(float x)      // max over 8 consecutive lanes (order-free), every lane gets it
{
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true)));
    return x;
}

struct DfLds {
    u16 *X, *H1, *H2, *Z3;
    float *part, *xs, *xs2, *bias, *bias_tgt, *rowloss;
    __device__ __forceinline__ explicit DfLds(u16* lds)
        : X(lds + DF_OFF_X), H1(lds + DF_OFF_H1), H2(lds + DF_OFF_H2), Z3(lds + DF_OFF_Z3),
          part(reinterpret_cast<float*>(lds + DF_OFF_PART)), xs(reinterpret_cast<float*>(lds + DF_OFF_XS)),
          xs2(reinterpret_cast<float*>(lds + DF_OFF_XS2)),
          bias(reinterpret_cast<float*>(lds + DF_OFF_F32)), bias_tgt(bias + DF_BIAS), rowloss(bias_tgt + DF_BIAS) {}
};

// A tile's 32 x 73 fp32 rows HBM -> a staging block (L.xs / L.xs2) by LDS-DMA (no registers, no waiting): wave w moves the 146 16-byte pieces of rows 8 w .. 8 w + 7,
// the rows its own threads convert, so its own vmcnt(0) (fs_dma_drain) is all the ordering the conversion needs.  `rows` must be
// 16-byte aligned (the caller checks once per launch).  M0 is reserved to the compiler: saved and put back.
__device__ __forceinline__ void df_fetch_rows(float* xs, const float* __restrict__ rows, int tl)
{
    typedef __attribute__((address_space(3))) void* lptr_t;
    constexpr int XW = BM * DQN_IN / 4 / NWAVE;                                // 146 pieces per wave
    const int w = __builtin_amdgcn_readfirstlane(tl >> 6), l = tl & 63;
    const unsigned dst = (unsigned)(unsigned long)(lptr_t)xs + 16u * (unsigned)(XW * w);
    const float* src = rows + 4L * (XW * w + l);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                 "s_add_u32 m0, %1, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(dst), "v"(src), "v"(src + 4 * 64) : "memory", "scc");
    if (l + 128 < XW)
        asm volatile("s_mov_b32 %0, m0\n\ts_add_u32 m0, %1, 0x800\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "s"(dst), "v"(src + 8 * 64) : "memory", "scc");
}

// One 48 KB plane image LDS -> HBM: twelve 16-byte reads per thread in flight, then twelve stores (a read-wait-store loop pays the LDS
// latency twelve times)
__device__ __forceinline__ void df_copy_image(float4* __restrict__ dst, const float4* src, int tl)
{
    constexpr int PER = DF_IMAGE_HALVES / 8 / THREADS;          // 12
    static_assert(PER * THREADS * 8 == DF_IMAGE_HALVES, "whole float4 per thread");
    float4 v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) v[u] = src[tl + THREADS * u];
    // (left alone the compiler reads, waits and stores one piece at a time through four registers)
#pragma unroll
    for (int u = 0; u < PER; u += 6)
        asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w), "+v"(v[u + 1].x), "+v"(v[u + 1].y), "+v"(v[u + 1].z),
                          "+v"(v[u + 1].w), "+v"(v[u + 2].x), "+v"(v[u + 2].y), "+v"(v[u + 2].z), "+v"(v[u + 2].w), "+v"(v[u + 3].x),
                          "+v"(v[u + 3].y), "+v"(v[u + 3].z), "+v"(v[u + 3].w), "+v"(v[u + 4].x), "+v"(v[u + 4].y), "+v"(v[u + 4].z),
                          "+v"(v[u + 4].w), "+v"(v[u + 5].x), "+v"(v[u + 5].y), "+v"(v[u + 5].z), "+v"(v[u + 5].w));
#pragma unroll
    for (int u = 0; u < PER; ++u) dst[tl + THREADS * u] = v[u];
}

// a tile's rows -> a staging block: by LDS-DMA (asynchronous: fs_dma_drain before the conversion), or -- tensors that are not 16-byte
// aligned -- through registers, finished when this returns.  Either way wave w moves the rows its own threads convert.
__device__ __forceinline__ void df_rows_in(float* xs, const float* __restrict__ rows, int tl, int dma)
{
    if (dma) { df_fetch_rows(xs, rows, tl); return; }
    constexpr int PER = BM * DQN_IN / NWAVE;                              // 584 floats
    const int wave = tl >> 6, lane = tl & 63;
    const float* src = rows + PER * wave;
    float* dst = xs + PER * wave;
    for (int i = lane; i < PER; i += 64) dst[i] = src[i];
}

// The Q-network forward of one 32-row tile on the plane images: rows (in the staging block `xs`, requested during the previous tile's
// backward pass) -> X planes -> H1 -> H2 -> split-K partials of the last layer in L.part (chunk-rotated).  `QBn` = the network's
// forward planes, `bias` = its b1 | b2 | b3 in LDS.  Ends with a barrier; the caller reads the partials (df_q_row) and must put a
// barrier before anything overwrites them.
// No epilogue stands exposed in front of a barrier: each wave owns two column tiles per layer; tile a's epilogue rides in the gaps of
// tile b's GEMM, tile b's in the first half of the NEXT layer's first GEMM, whose k-steps are ordered so that the half needs tile-a
// columns only (FsGemmHost MODE 1, one barrier between the halves); the last layer's k range is the wave's OWN two tiles (MODE 2).
// Every weight head is requested one GEMM ahead of the GEMM that uses it (a head requested right in front of its GEMM is an L2 round
// trip in front of that GEMM's first MFMA: 30 - 96 MFMAs do not amortise it).
// AHEAD: two more weight heads (the backward pass's first GEMMs: column tiles 2 wave, 2 wave + 1 of `ahead_w`, K = 32) are
// requested in front of the last layer's GEMM, so that the caller finds them landed.
// The pass's input: layer 1's first weights requested, the rows in the staging block `xs` (requested during the previous tile's backward
// pass: the drain waits for nothing) converted into the X planes.  The caller puts a barrier between this and df_forward.
__device__ __forceinline__ void df_input(const DfLds& L, const u16* __restrict__ QBn, const float* xs, int tl, WeightHeadT<4>& w1)
{
    const int wave = __builtin_amdgcn_readfirstlane(tl >> 6), lane = tl & 63;
    fs_dma_drain();
    gemm_prefetch_b3<DQN_IN_PAD, 4>(w1, QBn + DQN_OFF_QB1, 2 * wave, lane);
    FsXStoreSlices xc(xs, L.X, tl);
    xc.all();
}

template <bool AHEAD>
__device__ __forceinline__ void df_forward(const DfLds& L, const u16* __restrict__ QBn, const float* bias, const WeightHeadT<4>& w1, int tl,
                                           unsigned long long* sb, int slot0, WeightHeadT<2>& ahead0, WeightHeadT<2>& ahead1,
                                           const u16* __restrict__ ahead_w)
{
    const int wave = __builtin_amdgcn_readfirstlane(tl >> 6), lane = tl & 63, r = lane & 31;
    WeightHeadT<4> w3;
    WeightHead3 w1b, w2a, w2b;
    df_stamp(sb, slot0);
    f32x16 hi, lo, hi0, lo0;
    const int fine = slot0 == 1 ? 16 : 32;
    gemm_prefetch_b3<DQN_IN_PAD>(w1b, QBn + DQN_OFF_QB1, 2 * wave + 1, lane);
    fs_gemm<DQN_IN_PAD, FS_PX, false, true, 4>(w1, QBn + DQN_OFF_QB1, 2 * wave, L.X, 0, hi0, lo0, lane);
    df_stamp(sb, fine + 0);
    gemm_prefetch_b3<DQN_H>(w2a, QBn + DQN_OFF_QB2, 2 * wave, lane);
    {
        DfLreluOps<FS_P1> e(hi0, lo0, bias, 64 * wave, L.H1, lane);
        fs_gemm_host<DQN_IN_PAD, FS_PX, false>(w1b, QBn + DQN_OFF_QB1, 2 * wave + 1, L.X, 0, hi, lo, lane, e);
    }
    df_stamp(sb, fine + 1);
    __syncthreads();                                                          // every wave's tile-a columns of H1 are stored
    df_stamp(sb, slot0 + 1);
    {
        DfLreluOps<FS_P1> e(hi, lo, bias, 64 * wave + 32, L.H1, lane);         // layer 1, tile b
        fs_gemm_host<DQN_H, FS_P1, false, true, B3_HEAD, 48, 1>(w2a, QBn + DQN_OFF_QB2, 2 * wave, L.H1, 0, hi0, lo0, lane, e);
    }
    df_stamp(sb, fine + 3);
    gemm_prefetch_b3<DQN_H>(w2b, QBn + DQN_OFF_QB2, 2 * wave + 1, lane);
    {
        DfLreluOps<FS_P1> e(hi0, lo0, bias + DQN_H, 64 * wave, L.H2, lane);
        fs_gemm_host<DQN_H, FS_P1, false>(w2b, QBn + DQN_OFF_QB2, 2 * wave + 1, L.H1, 0, hi, lo, lane, e);
    }
    df_stamp(sb, fine + 4);
    gemm_prefetch_b3<64, 4>(w3, QBn + DQN_OFF_QB3 + (long)(4 * wave) * 1536, 0, lane);    // the last layer's k range of this wave
    if (AHEAD) {
        gemm_prefetch_b3<DQN_OUT>(ahead0, ahead_w, 2 * wave, lane);
        gemm_prefetch_b3<DQN_OUT>(ahead1, ahead_w, 2 * wave + 1, lane);
    }
    df_stamp(sb, slot0 + 2);
    // last layer: split-K over the four waves; wave w's k range is columns 64 w .. + 63 of H2 = its own two tiles: no barrier, and tile
    // b's epilogue rides in the k-steps over tile a.  Partials chunk-rotated (32 lanes writing one chunk column would meet in 8 banks).
    {
        DfLreluOps<FS_P1> e(hi, lo, bias + DQN_H, 64 * wave + 32, L.H2, lane);
        fs_gemm_host<64, FS_P1, false, true, 4, 12, 2>(w3, QBn + DQN_OFF_QB3 + (long)(4 * wave) * 1536, 0, L.H2, 64 * wave, hi0, lo0, lane, e);
    }
    df_stamp(sb, fine + 6);
    float* pw = L.part + wave * (BM * DQN_OUT);
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(pw + r * DQN_OUT + 4 * ((acc_n(g, lane) >> 2) ^ ((r >> 1) & 7))) =
            make_float4(hi0[4 * g] + lo0[4 * g], hi0[4 * g + 1] + lo0[4 * g + 1], hi0[4 * g + 2] + lo0[4 * g + 2],
                        hi0[4 * g + 3] + lo0[4 * g + 3]);
    __syncthreads();
    df_stamp(sb, slot0 + 3);
}

// this thread's four Q values: row tl >> 3, columns 4 (tl & 7) .. + 3 (columns >= 18 are padding)
__device__ __forceinline__ void df_q_row(const DfLds& L, const float* bias3, int tl, float (&q)[4])
{
    const int lrow = tl >> 3, lq = tl & 7;
    const int cs = 4 * (lq ^ ((lrow >> 1) & 7));
    const float4 p0 = *reinterpret_cast<const float4*>(L.part + lrow * DQN_OUT + cs);
    const float4 p1 = *reinterpret_cast<const float4*>(L.part + BM * DQN_OUT + lrow * DQN_OUT + cs);
    const float4 p2 = *reinterpret_cast<const float4*>(L.part + 2 * BM * DQN_OUT + lrow * DQN_OUT + cs);
    const float4 p3 = *reinterpret_cast<const float4*>(L.part + 3 * BM * DQN_OUT + lrow * DQN_OUT + cs);
    const float4 b = *reinterpret_cast<const float4*>(bias3 + 4 * lq);
    q[0] = (((p0.x + p1.x) + p2.x) + p3.x) + b.x;
    q[1] = (((p0.y + p1.y) + p2.y) + p3.y) + b.y;
    q[2] = (((p0.z + p1.z) + p2.z) + p3.z) + b.z;
    q[3] = (((p0.w + p1.w) + p2.w) + p3.w) + b.w;
}

// the lane's four columns of dZ3: `dq` in the taken action's column, 0 elsewhere
__device__ __forceinline__ float4 fs_dqn_dz3(int lq, int idx, float dq)
{
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * lq + 0 == idx) d.x = dq;
    if (4 * lq + 1 == idx) d.y = dq;
    if (4 * lq + 2 == idx) d.z = dq;
    if (4 * lq + 3 == idx) d.w = dq;
    return d;
}

struct DqnChunk { const float *obs, *next_obs, *act, *reward, *done; };      // one sampled replay step: n rows each (device pointers)

constexpr long DF_STRIDE1 = (long)DQN_H * DQN_IN_PAD + DQN_H, DF_STRIDE2 = (long)DQN_H * DQN_H + DQN_H,
               DF_STRIDE3 = (long)DQN_OUT * DQN_H + DQN_OUT;
static_assert(DF_STRIDE1 + DF_STRIDE2 + DF_STRIDE3 == DQN_PACKED_FLOATS, "the three layer blocks are one packed gradient");

// chunks: device array [S]; tiles_per = n / 32 (whole tiles: the launcher checks); images: u16 [S * tiles_per][2][DF_IMAGE_HALVES];
// ws1 / ws3: partial slabs [grid][DF_STRIDE1] / [grid][DF_STRIDE3]; loss_part f32 [S * tiles_per]
__global__ __launch_bounds__(THREADS, 1) void dqn_chain_kernel(
    const float* __restrict__ P, const u16* __restrict__ QB, const u16* __restrict__ QTB, const float* __restrict__ P_tgt,
    const u16* __restrict__ QB_tgt, const DqnChunk* __restrict__ chunks, int S, long tiles_per, float discount, float inv_B,
    u16* __restrict__ images, float* __restrict__ ws1, float* __restrict__ ws2, float* __restrict__ ws3, float* __restrict__ loss_part,
    unsigned long long* __restrict__ stamps, int dma)
{
    // `stamps` (diagnostics, normally null: tools/stamp_dqn.py): thread 0 stores s_memtime at the phase boundaries of the workgroup's
    // SECOND tile into stamps[blockIdx.x][64] (0 .. 13 phases; 16 + 16 pass + i: inside forward pass `pass`)
    extern __shared__ __attribute__((aligned(16))) u16 df_lds[];
    const DfLds L(df_lds);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // biases of both networks -> LDS, once per launch
    L.bias[tid] = P[DQN_OFF_B1 + tid];
    L.bias[DQN_H + tid] = P[DQN_OFF_B2 + tid];
    L.bias_tgt[tid] = P_tgt[DQN_OFF_B1 + tid];
    L.bias_tgt[DQN_H + tid] = P_tgt[DQN_OFF_B2 + tid];
    if (tid < DQN_OUT) { L.bias[2 * DQN_H + tid] = P[DQN_OFF_B3 + tid]; L.bias_tgt[2 * DQN_H + tid] = P_tgt[DQN_OFF_B3 + tid]; }
    // dW accumulators of this wave, alive across all its tiles: dW1[n tiles 2 wave, 2 wave + 1][3 k tiles], dW3[k tiles 2 wave, 2 wave + 1]
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
    __syncthreads();

    // (tile counts are 32-bit: the launcher refuses more than 2^31 tiles; a 64-bit division per tile costs ~1k cycles)
    const unsigned ntiles = (unsigned)S * (unsigned)tiles_per, tper = (unsigned)tiles_per;
    // rows by LDS-DMA when every chunk's row blocks are 16-byte aligned (the host launcher says so).  Both row blocks of a tile (next_obs
    // -> L.xs, obs -> L.xs2) are requested a tile ahead; the first tile's here.
    if (blockIdx.x < ntiles) {
        const unsigned s0 = blockIdx.x / tper;
        const long off = (long)(blockIdx.x - s0 * tper) * BM * DQN_IN;
        df_rows_in(L.xs, chunks[s0].next_obs + off, tid, dma);
        df_rows_in(L.xs2, chunks[s0].obs + off, tid, dma);
    }
    // the row's scalars (dqn.py:64-66) travel a tile ahead of their use (a load that misses to HBM holds every later load's wait)
    float n_act = 0.0f, n_rew = 0.0f, n_done = 0.0f;
    if (blockIdx.x < ntiles) {
        const unsigned s0 = blockIdx.x / tper;
        const long r0 = (long)(blockIdx.x - s0 * tper) * BM + (tid >> 3);
        n_act = chunks[s0].act[r0]; n_rew = chunks[s0].reward[r0]; n_done = chunks[s0].done[r0];
    }
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tl = tid;
        asm volatile("" : "+v"(tl));                      // (keeps tile-invariant address arithmetic inside the loop)
        const int lane = tl & 63;
        const int lrow = tl >> 3, lq = tl & 7;
        const float r_act = n_act, r_rew = n_rew, r_done = n_done;
        unsigned long long* sb = (stamps != nullptr && tile == blockIdx.x + gridDim.x) ? stamps + 64L * blockIdx.x : nullptr;
        df_stamp(sb, 0);

        // ---- q_target(next_obs).max(1) (dqn.py:73-74) ----------------------------------------------------------------------
        // the next tile of this workgroup: its rows and scalars are requested at the start of this tile's backward pass
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
        WeightHeadT<2> wt3a, wt3b;
        WeightHeadT<4> w1;
        df_input(L, QB_tgt, L.xs, tl, w1);
        __syncthreads();
        df_forward<false>(L, QB_tgt, L.bias_tgt, w1, tl, sb, 1, wt3a, wt3b, nullptr);
        // the online pass's input is made HERE, beside the target pass's max over its partials: X is free since the target pass's layer 1
        // (one barrier and one exposed phase less than converting at the top of the online pass)
        df_input(L, QB, L.xs2, tl, w1);
        float qn_max;
        {
            float q[4];
            df_q_row(L, L.bias_tgt + 2 * DQN_H, tl, q);
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) m = (4 * lq + j < DQN_NACT) ? fmaxf(m, q[j]) : m;
            qn_max = df_max8(m);
        }
        __syncthreads();                                  // the partials are consumed, the online pass's X planes are whole; H1 / H2 free
        // ---- q(obs) (dqn.py:68) ----------------------------------------------------------------------------------------------
        df_stamp(sb, 5);
        df_forward<true>(L, QB, L.bias, w1, tl, sb, 6, wt3a, wt3b, QTB + DQN_OFF_QTB3);
        {   // ---- everything that goes to or comes from HBM around the backward pass is issued HERE: the next memory-fed GEMM (dA1) is
            // ~7k cycles away, so none of it is waited for.  The heads of dA2's two GEMMs have landed (requested in front of the last
            // layer's GEMM) and are pinned: waiting for them later would wait for all of this too (vmcnt counts in order).
            // (pinned as whole 16-byte vectors: pinned component by component the allocator scatters a fragment's four registers and
            // reassembles the MFMA operand with v_mov right in front of the asm MFMA -- a vector write the compiler does not pad for
            // an opaque asm: the MFMA then reads the OLD register now and then.  tools/check_mfma_hazard.py looks for exactly that.)
            typedef float df_f32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    float4 &u = wt3a.b[ks].p[pl], &v = wt3b.b[ks].p[pl];
                    df_f32x4 uu = {u.x, u.y, u.z, u.w}, vv = {v.x, v.y, v.z, v.w};
                    asm volatile("" : "+v"(uu), "+v"(vv));
                    u = make_float4(uu[0], uu[1], uu[2], uu[3]);
                    v = make_float4(vv[0], vv[1], vv[2], vv[3]);
                }
            if (act_n != nullptr) { n_act = *act_n; n_rew = *rew_n; n_done = *done_n; }
            if (rows_n != nullptr) {                        // (both staging blocks are free: this tile's planes were made from them)
                df_rows_in(L.xs, rows_n, tl, dma);
                df_rows_in(L.xs2, rows_o, tl, dma);
            }
        }
        {   // ---- TD target, Huber, d loss / d Q (dqn.py:69-79): eight lanes per row, four Q columns each -------------------------
            float q[4];
            df_q_row(L, L.bias + 2 * DQN_H, tl, q);
            const int idx = dqn_action_index(r_act, DQN_NACT);                 // (dqn.py:70)
            float sel = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) sel = (4 * lq + j == idx) ? q[j] : sel;
            const float q_val = fs_sum8(sel);                                  // one non-zero among the eight lanes: exact
            const DqnTdRow t = dqn_td_row(q_val, r_rew, discount, qn_max, r_done, inv_B);
            fs_store4<FS_P4>(L.Z3, lrow, 4 * lq, fs_dqn_dz3(lq, idx, t.dq));
            if (lq == 0) L.rowloss[lrow] = t.hub;
        }
        __syncthreads();
        df_stamp(sb, 10);
        if (tl < 32) tile_loss_sum<1>(L.rowloss, tl, loss_part + tile);
        FsTr tr1, trx, tr4;
        fs_tr_init<FS_P1>(tr1, lane);
        fs_tr_init<FS_PX>(trx, lane);
        fs_tr_init<FS_P4>(tr4, lane);
        WeightHead3 wt2a, wt2b;
        gemm_prefetch_b3<DQN_H>(wt2a, QTB + DQN_OFF_QTB2, 2 * wave, lane);         // dA1's first head: a phase ahead
        // H1's plane image (48 KB) leaves as it lies: the 256 x 256 layer's weight gradient is formed from it by dqn_dw2_kernel
        df_copy_image(reinterpret_cast<float4*>(images + tile * (2L * DF_IMAGE_HALVES)), reinterpret_cast<const float4*>(L.H1), tl);
        df_stamp(sb, 52);
        f32x16 hi0, lo0, hi, lo;
            // ---- dA2 = dZ3 . W3 -> dZ2 (in place over H2);  dW3 += dZ3^T H2;  db3 -----------------------------------------------
            // H2's fragments of THIS wave's two column tiles (= dW3's k tiles, = the columns its dZ2 epilogues overwrite) are read
            // first and pinned: they must have landed before the first in-place store
            bf16x8 af[2][2][3], zf[2][3];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) fs_trws<FS_P1>(af[t][ks], L.H2, tr1, 2 * wave + t, ks);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) fs_trns<FS_P4>(zf[ks], L.Z3, tr4, 0, ks);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) asm volatile("" : "+v"(af[t][ks][pl]));
            // both GEMMs first (2 x 12 MFMAs on heads that are in registers), then dW3's 24 MFMAs with the first column tile's epilogue
            // in their gaps
            fs_gemm<DQN_OUT, FS_P4, false>(wt3a, QTB + DQN_OFF_QTB3, 2 * wave, L.Z3, 0, hi0, lo0, lane);
            fs_gemm<DQN_OUT, FS_P4, false>(wt3b, QTB + DQN_OFF_QTB3, 2 * wave + 1, L.Z3, 0, hi, lo, lane);
            {
                DfDlreluOps<FS_P1> e(hi0, lo0, 64 * wave, L.H2, lane);
                fs_dw_host<0, 24>(aW3[0], zf[0], af[0][0], e);
                fs_dw_host<6, 24>(aW3[0], zf[1], af[0][1], e);
                fs_dw_host<12, 24>(aW3[1], zf[0], af[1][0], e);
                fs_dw_host<18, 24>(aW3[1], zf[1], af[1][1], e);
            }
            // (the second column tile's epilogue rides in the first half of dA1's first GEMM, below)
            // db3 (wave 0) and db2 of this wave's first column tile: column sums through an all-ones operand (they land in every
            // register of lane n).  dZ2's columns 64 wave .. + 63 were written by THIS wave (lane = row), so its own transposing
            // reads of them need no barrier.
            const df_u32x4 o = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
            const bf16x8 ones = __builtin_bit_cast(bf16x8, o);
            if (wave == 0) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int pl = 2; pl >= 0; --pl) aB3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, zf[ks][pl], aB3, 0, 0, 0);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 z2[3];
                fs_trws<FS_P1>(z2, L.H2, tr1, 2 * wave, ks);
#pragma unroll
                for (int pl = 2; pl >= 0; --pl) aB2[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, z2[pl], aB2[0], 0, 0, 0);
            }
        __syncthreads();                                  // every wave's tile-a columns of dZ2 are stored
        df_stamp(sb, 11);
        {   // ---- dA1 = dZ2 . W2 with the operand roles SWAPPED -> dZ1 as transposed fragments in registers;  dW1 += dZ1^T X ---------
            // GEMM(tile 0): first the k-steps over every wave's tile-a columns of dZ2, with dZ2's tile-b epilogue in their gaps, a
            // barrier, the rest | db2 of tile b | GEMM(tile 1) with dZ1's tile-0 epilogue in its gaps | dZ2's image leaves |
            // dW1(tile 0) with dZ1's tile-1 epilogue in its gaps | dW1(tile 1)
            const int ct0 = 2 * wave, ct1 = 2 * wave + 1;
            gemm_prefetch_b3<DQN_H>(wt2b, QTB + DQN_OFF_QTB2, ct1, lane);
            {
                DfDlreluOps<FS_P1> e(hi, lo, 64 * wave + 32, L.H2, lane);
                fs_gemm_host<DQN_H, FS_P1, true, true, B3_HEAD, 48, 1>(wt2a, QTB + DQN_OFF_QTB2, ct0, L.H2, 0, hi0, lo0, lane, e);
            }
            {
                const df_u32x4 o = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
                const bf16x8 ones = __builtin_bit_cast(bf16x8, o);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 z2[3];
                    fs_trws<FS_P1>(z2, L.H2, tr1, 2 * wave + 1, ks);
#pragma unroll
                    for (int pl = 2; pl >= 0; --pl) aB2[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, z2[pl], aB2[1], 0, 0, 0);
                }
            }
            df_stamp(sb, 48);
            df_u32x4 hw0[2], hw1[2], zw0[2][3], zw1[2][3];
            {
                bf16x8 hf[3];
                fs_trws<FS_P1>(hf, L.H1, tr1, ct0, 0); hw0[0] = __builtin_bit_cast(df_u32x4, hf[0]);
                fs_trws<FS_P1>(hf, L.H1, tr1, ct0, 1); hw0[1] = __builtin_bit_cast(df_u32x4, hf[0]);
                fs_trws<FS_P1>(hf, L.H1, tr1, ct1, 0); hw1[0] = __builtin_bit_cast(df_u32x4, hf[0]);
                fs_trws<FS_P1>(hf, L.H1, tr1, ct1, 1); hw1[1] = __builtin_bit_cast(df_u32x4, hf[0]);
            }
            {
                DfDz1Ops e0(hi0, lo0, hw0, zw0);
                fs_gemm_host<DQN_H, FS_P1, true>(wt2b, QTB + DQN_OFF_QTB2, ct1, L.H2, 0, hi, lo, lane, e0);
                bs1[0] += e0.colsum();
            }
            df_stamp(sb, 49);
            {   // dZ2's plane image (the other 48 KB the 256 x 256 layer's weight gradient needs): the stores drain under dW1's 72 MFMAs
                df_copy_image(reinterpret_cast<float4*>(images + tile * (2L * DF_IMAGE_HALVES) + DF_IMAGE_HALVES),
                              reinterpret_cast<const float4*>(L.H2), tl);
            }
            df_stamp(sb, 50);
            {
                DfDz1Ops e1(hi, lo, hw1, zw1);
                const bf16x8 z0[3] = {__builtin_bit_cast(bf16x8, zw0[0][0]), __builtin_bit_cast(bf16x8, zw0[0][1]), __builtin_bit_cast(bf16x8, zw0[0][2])};
                const bf16x8 z1[3] = {__builtin_bit_cast(bf16x8, zw0[1][0]), __builtin_bit_cast(bf16x8, zw0[1][1]), __builtin_bit_cast(bf16x8, zw0[1][2])};
                bf16x8 xf[2][3];
                fs_trns<FS_PX>(xf[0], L.X, trx, 0, 0); fs_trns<FS_PX>(xf[1], L.X, trx, 0, 1);
                fs_dw_host<0, 36>(aW1[0][0], z0, xf[0], e1); fs_dw_host<6, 36>(aW1[0][0], z1, xf[1], e1);
                fs_trns<FS_PX>(xf[0], L.X, trx, 1, 0); fs_trns<FS_PX>(xf[1], L.X, trx, 1, 1);
                fs_dw_host<12, 36>(aW1[0][1], z0, xf[0], e1); fs_dw_host<18, 36>(aW1[0][1], z1, xf[1], e1);
                fs_trns<FS_PX>(xf[0], L.X, trx, 2, 0); fs_trns<FS_PX>(xf[1], L.X, trx, 2, 1);
                fs_dw_host<24, 36>(aW1[0][2], z0, xf[0], e1); fs_dw_host<30, 36>(aW1[0][2], z1, xf[1], e1);
                bs1[1] += e1.colsum();
            }
            df_stamp(sb, 51);
            {
                const bf16x8 z0[3] = {__builtin_bit_cast(bf16x8, zw1[0][0]), __builtin_bit_cast(bf16x8, zw1[0][1]), __builtin_bit_cast(bf16x8, zw1[0][2])};
                const bf16x8 z1[3] = {__builtin_bit_cast(bf16x8, zw1[1][0]), __builtin_bit_cast(bf16x8, zw1[1][1]), __builtin_bit_cast(bf16x8, zw1[1][2])};
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) {
                    bf16x8 xf[2][3];
                    fs_trns<FS_PX>(xf[0], L.X, trx, kt, 0);
                    fs_trns<FS_PX>(xf[1], L.X, trx, kt, 1);
                    fs_dw(aW1[1][kt], z0, xf[0]);
                    fs_dw(aW1[1][kt], z1, xf[1]);
                }
            }
        }
        df_stamp(sb, 12);
        __syncthreads();            // every wave is done with X, H1 and dZ2 before the next tile's forward overwrites them
        df_stamp(sb, 13);
    }

    // ---- one partial slab per workgroup per UPDATE: layer 1 block (weights [256][80], bias) and layer 3 block ([32][256], bias) ----
    const int lane = tid & 63;
    float* o1 = ws1 + (long)blockIdx.x * DF_STRIDE1;
    float* o3 = ws3 + (long)blockIdx.x * DF_STRIDE3;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const int col = kt * 32 + (lane & 31);
            if (col < DQN_IN_PAD) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) o1[((2 * wave + t) * 32 + acc_row(reg, lane)) * DQN_IN_PAD + col] = aW1[t][kt][reg];
            }
        }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float v = bs1[t] + __shfl_xor(bs1[t], 32, 64);                    // db1 sits in the two lane halves of the swapped-role sums
        if (lane < 32) o1[DQN_H * DQN_IN_PAD + 32 * (2 * wave + t) + lane] = v;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) o3[acc_row(reg, lane) * DQN_H + (2 * wave + t) * 32 + (lane & 31)] = aW3[t][reg];
    }
    if (wave == 0 && lane < 32) o3[DQN_OUT * DQN_H + lane] = aB3[0];
    // db2 goes to the bias part of this workgroup's layer-2 slab; its weight part is written by workgroup blockIdx.x of dqn_dw2_kernel
    if (lane < 32) {
#pragma unroll
        for (int t = 0; t < 2; ++t) ws2[(long)blockIdx.x * DF_STRIDE2 + DQN_H * DQN_H + 32 * (2 * wave + t) + lane] = aB2[t][0];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dW2 = dZ2^T H1, db2 = colsum(dZ2) over all tiles of the update, from the saved images.  LDS: two buffers of one 16-row k-step:
// [H1 | dZ2][3 planes][16 rows][256] = 48 KB each.  A 16-row half of an image keeps the image's swizzle (fs_key(r + 16) = fs_key(r)).
constexpr int DW2_PLANE = 16 * FS_P1;                                     // 16-bit words per plane of a half image
constexpr int DW2_BUF = 2 * 3 * DW2_PLANE;                                // 24576 words = 48 KB
constexpr int DW2_LDS_BYTES = 2 * DW2_BUF * 2;
// the fragment of fs_trq3 for a 16-row half image (plane stride DW2_PLANE)
__device__ __forceinline__ void dw2_frag(bf16x8 (&f)[3], const u16* half0, const FsTr& t, int T)
{
    typedef __attribute__((address_space(3))) s16x4* lds_ptr;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const int xw = 32 * (T & 3);
    const u16* a = half0 + 32 * (T & ~3) + (t.lo ^ xw);
    const u16* b = half0 + 32 * (T & ~3) + (t.hi ^ xw);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + p * DW2_PLANE));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(b + p * DW2_PLANE));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        f[p] = __builtin_bit_cast(bf16x8, v);
    }
}

__global__ __launch_bounds__(THREADS, 1) void dqn_dw2_kernel(const u16* __restrict__ images, long ntiles, float* __restrict__ ws2)
{
    extern __shared__ __attribute__((aligned(16))) u16 dw_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt0 = 4 * (wave >> 1), kt0 = 4 * (wave & 1);                  // this wave's 4 x 4 output tiles: n' tiles (dZ2), k tiles (H1)
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b][i] = 0.0f;
    FsTr tr1;
    fs_tr_init<FS_P1>(tr1, lane);
    typedef __attribute__((address_space(3))) void* lptr_t;
    const unsigned lds0 = (unsigned)(unsigned long)(lptr_t)dw_lds;
    // k-step j of this workgroup = half (j & 1) of its tile number (j >> 1): tile = blockIdx.x + (j >> 1) * gridDim.x
    const long my_tiles = blockIdx.x < ntiles ? (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    const long steps = 2 * my_tiles;
    // one k-step = 6 pieces of 8 KB (tensor T in {H1, dZ2}, plane p): 48 wave-instructions of 1 KB, twelve per wave
    auto fetch = [&](long j, int buf) {
        const long tile = blockIdx.x + (j >> 1) * gridDim.x;
        const u16* src = images + tile * (2L * DF_IMAGE_HALVES) + (j & 1) * DW2_PLANE;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int piece = 12 * wave + i, tp = piece >> 3, sub = piece & 7;     // tp = T * 3 + p
            const u16* g = src + (long)tp * (2 * DW2_PLANE) + sub * 512 + lane * 8;       // images keep 32 rows per plane: stride 2 halves
            const unsigned dst = lds0 + 2u * (unsigned)(buf * DW2_BUF + tp * DW2_PLANE + sub * 512);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "s"(dst), "v"(g) : "memory", "scc");
        }
    };
    if (steps > 0) fetch(0, 0);
    for (long j = 0; j < steps; ++j) {
        const int buf = (int)(j & 1);
        fs_dma_drain();                                   // this wave's pieces of k-step j have landed ...
        __syncthreads();                                  // ... and everybody's; everybody is done reading the other buffer (k-step j - 1)
        if (j + 1 < steps) fetch(j + 1, buf ^ 1);
        const u16* hb = dw_lds + buf * DW2_BUF;                                 // H1 half image
        const u16* zb = hb + 3 * DW2_PLANE;                                     // dZ2 half image
        bf16x8 zf[2][3], af[4][3];
#pragma unroll
        for (int b = 0; b < 4; ++b) dw2_frag(af[b], hb, tr1, kt0 + b);
        dw2_frag(zf[0], zb, tr1, nt0);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (a + 1 < 4) dw2_frag(zf[(a + 1) & 1], zb, tr1, nt0 + a + 1);
#pragma unroll
            for (int b = 0; b < 4; ++b) fs_dw(acc[a][b], zf[a & 1], af[b]);
        }
    }
    // one partial slab per workgroup: the weight part of the layer-2 block [256][256] (its bias part comes from dqn_chain_kernel)
    float* o2 = ws2 + (long)blockIdx.x * DF_STRIDE2;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                o2[((nt0 + a) * 32 + acc_row(reg, lane)) * DQN_H + (kt0 + b) * 32 + (lane & 31)] = acc[a][b][reg];
}
