// mlp_fused_h2.inc — the fused optimizer-step gradient (mlp_fused_step.inc: ppo.py:184-197 in ONE persistent launch) in the fp16x2
// arithmetic: every fp32 operand x of a GEMM is carried as TWO fp16 terms of its scaled value, x s = h0 + h1 (s a power of two per
// tensor class; |x s - h0 - h1| <= max(2^-24, 2^-23 |x s|): tools/f16_probe.hip), and a 16-wide k block is THREE
// v_mfma_f32_32x32x16_f16 (h0 h0 -> `hi`; h0 h1, h1 h0 -> `lo`; fp32 accumulate) instead of the six bf16 products of the
// three-term split: half the matrix time, two LDS planes and two weight planes instead of three, ~60 % of the split / recombine work.
// tools/bf16x3_gemm.hip holds the error of this scheme to fp64 (forward-like and gradient-like operands); tools/mfma_chain_interleave.hip
// `arith` the chain GEMM in isolation: 0.57 of the bf16x3 wall time.
//
// SCALES.  fp16 spans 6e-8 .. 65504, so every tensor class is multiplied by a power of two before it is split:
//     class 0 X, 1 H1, 2 H2, 3 H3, 4 dZ4, 5 dZ3, 6 dZ2, 7 dZ1 (activations / gradients), 8 .. 11 W1 .. W4 (weights)
// `fsc` (device, H2_FSC_FLOATS floats) holds s[c] at [c] and 1 / s[c] at [16 + c].  A dW accumulator lives across all of a workgroup's
// tiles and contracts over rows, so a class has ONE scale per launch.  Products of powers of two are exact: every epilogue applies
// 1 / (s_a s_w) to hi + lo, i.e. computes on the very fp32 values an unscaled kernel would see.
// Where the scales come from: every value that is split also folds |scaled value| into a running maximum (one v_maximum3_f32 per pair: a NaN survives into it);
// each workgroup leaves its eight class maxima behind its slab, the slab reduction (mlp_grad_reduce_h2_kernel) takes the maximum over
// workgroups and sets the NEXT launch's scales so that this launch's maximum would land in the class's window (h2_target_exp below:
// 2^8 of headroom under 65504 for activations, 2^13 for gradients).  A maximum of 65504 or more means some value of THIS launch did not fit: the reduction marks
// the gradient invalid (G[76], as the tile hand-off of mlp_forward_backward does) and sets a STICKY device word, so the optimizer
// kernels refuse this step and every later one of the update; the host redoes them on the bf16x3 kernel (PPO._update_hip) --
// bit for bit what an undisturbed bf16x3 step leaves.  Weight scales are set by the optimizer kernel's rescale steps from the per-layer
// max |w| with 16x of headroom (a step moves a weight by 3.2 lr at most: it cannot overflow before the next rescale; mlp_adam.inc).
//
// Structure, LDS swizzle, register placement, the phases P0 .. P8 and the guests riding in MFMA gaps are those of mlp_fused_step.inc
// (read that file first); this file restates the kernel on two planes, three products and scaled epilogues.  With two planes the
// LDS image is 128 KB: the staging block of the next tile's rows gets a region of its own.
#include "fs_h2.inc"

// weight planes (16-bit words): the layout of PB / PTB (mlp_layout.h) with two terms per k block -- a block is 1024 words, not 1536
constexpr int H2_OFF_PH1 = 0, H2_OFF_PH2 = H2_OFF_PH1 + 2 * MLP_H1 * MLP_IN_PAD, H2_OFF_PH3 = H2_OFF_PH2 + 2 * MLP_H2 * MLP_H1,
              H2_OFF_PH4 = H2_OFF_PH3 + 2 * MLP_H3 * MLP_H2, H2_PH_HALVES = H2_OFF_PH4 + 2 * MLP_OUT * MLP_H3;
constexpr int H2_OFF_PTH2 = 0, H2_OFF_PTH3 = H2_OFF_PTH2 + 2 * MLP_H1 * MLP_H2, H2_OFF_PTH4 = H2_OFF_PTH3 + 2 * MLP_H2 * MLP_H3,
              H2_PTH_HALVES = H2_OFF_PTH4 + 2 * MLP_H3 * MLP_OUT;
static_assert(H2_PH_HALVES * 3 == MLP_PB_HALVES * 2 && H2_PTH_HALVES * 3 == MLP_PTB_HALVES * 2, "two thirds of the bf16x3 planes");

// ---- LDS image ----------------------------------------------------------------------------------------------------------------------
constexpr int H2_X_HALVES = 2 * BM * FS_PX;                              // one X buffer (two planes)
constexpr int H2_OFF_X = 0;
constexpr int H2_OFF_H1 = H2_OFF_X + 2 * H2_X_HALVES;
constexpr int H2_OFF_H2 = H2_OFF_H1 + 2 * BM * FS_P1;
constexpr int H2_OFF_H3 = H2_OFF_H2 + 2 * BM * FS_P2;
constexpr int H2_OFF_R = H2_OFF_H3 + 2 * BM * FS_P2;                     // layer-4 split-K partials (fp32 [4][32][32]) | dZ4 behind them | dZ2
constexpr int H2_OFF_Z4 = H2_OFF_R + 4 * BM * MLP_OUT * 2;
constexpr int H2_R_HALVES = 4 * BM * MLP_OUT * 2 + 2 * BM * FS_P4;
static_assert(H2_R_HALVES >= 2 * BM * FS_P2, "dZ2's planes fit region R");
constexpr int H2_OFF_XS = H2_OFF_R + H2_R_HALVES;                        // staging: the raw fp32 rows of the NEXT tile (a region of its own)
constexpr int H2_OFF_F32 = H2_OFF_XS + BM * MLP_IN * 2;
// fp32 tail: b1 | b2 | b3 | b4 | rowloss[64] | 1/L[32] | 1/var[32] | half log det[4] | scales s[16] | 1/s[16] | class maxima [8][256]
constexpr int H2_TAIL_FLOATS = MLP_H1 + MLP_H2 + MLP_H3 + MLP_OUT + 2 * BM + 2 * MLP_OUT + 4 + 32 + H2_NACT_CLASSES * THREADS;
constexpr int H2_LDS_BYTES = H2_OFF_F32 * 2 + H2_TAIL_FLOATS * 4;
static_assert(H2_LDS_BYTES <= 160 * 1024 && (H2_OFF_XS * 2) % 16 == 0 && (H2_OFF_F32 * 2) % 16 == 0, "fits one CU, 16-byte aligned regions");

// bias + ELU epilogue (lane = row): y = ELU((hi + lo) k + bias) -- k = 1 / (s_w s_a) -- then y s -> the next GEMM's planes, as
// single-instruction ops of four interleaved chains (dqn_fused_h2.inc's DhLreluOps with two groups at a time), for the gaps of the NEXT
// GEMM: t = fma(hi + lo, k s, bias s) is s times the unscaled pre-activation (powers of two commute with every rounding), exp(x) as
// v_exp_f32 of x log2(e) with the 1 / s folded into the constant, (e - 1) s in one fma.  `bias_s` = the bias times s (made once per launch).
template <int PITCH, bool DUMP>
struct H2EluOps {
    static constexpr int HEAD_OPS = 12, CH = HEAD_OPS + H2_SPLIT_OPS;     // 17 ops per chain
    static constexpr int NG = 1 + 2 * CH + 2, TOTAL = 4 * NG;             // per group of four columns: bias load, two chains, two stores
    const f32x16 &hi, &lo;
    const float* bias;      // + col0 (scaled)
    u16* plane0;
    float* dump_tile;
    int col0, lane, r, nvalid;
    float ks, c1, s, is, am;
    float4 bv[2];
    H2Chain k[4];
    __device__ __forceinline__ H2EluOps(const f32x16& hi_, const f32x16& lo_, const float* bias_s, int col0_, u16* plane0_, int lane_,
                                        float* dump_tile_, int nvalid_, float k_, float s_, float is_)
        : hi(hi_), lo(lo_), bias(bias_s + col0_), plane0(plane0_), dump_tile(dump_tile_), col0(col0_), lane(lane_), r(lane_ & 31),
          nvalid(nvalid_), ks(k_ * s_), c1(1.4426950408889634f * is_), s(s_), is(is_), am(0.0f) {}
    __device__ __forceinline__ void chain_op(H2Chain& c, int g, int h, int i, const float4& b)
    {
        const int r0 = 4 * g + 2 * h;
        if (i == 0) { c.t0 = hi[r0] + lo[r0]; fs_pin(c.t0); }
        if (i == 1) { c.t1 = hi[r0 + 1] + lo[r0 + 1]; fs_pin(c.t1); }
        if (i == 2) { c.t0 = fmaf(c.t0, ks, h ? b.z : b.x); fs_pin(c.t0); }
        if (i == 3) { c.t1 = fmaf(c.t1, ks, h ? b.w : b.y); fs_pin(c.t1); }
        if (i == 4) { c.u0 = c.t0 * c1; fs_pin(c.u0); }
        if (i == 5) { c.u1 = c.t1 * c1; fs_pin(c.u1); }
        if (i == 6) { c.u0 = __builtin_amdgcn_exp2f(c.u0); fs_pin(c.u0); }
        if (i == 7) { c.u1 = __builtin_amdgcn_exp2f(c.u1); fs_pin(c.u1); }
        if (i == 8) { c.u0 = fmaf(c.u0, s, -s); fs_pin(c.u0); }
        if (i == 9) { c.u1 = fmaf(c.u1, s, -s); fs_pin(c.u1); }
        if (i == 10) { c.t0 = c.t0 > 0.0f ? c.t0 : c.u0; fs_pin(c.t0); }
        if (i == 11) { c.t1 = c.t1 > 0.0f ? c.t1 : c.u1; fs_pin(c.t1); }
        if (i >= HEAD_OPS) h2_split_op(c, am, i - HEAD_OPS);
    }
    // two groups at a time, FOUR chains interleaved (a dependent vector instruction costs ~8 cycles at one wave per SIMD: with two
    // chains every op would wait on the op two slots earlier): op t -> group 2 (t / 2 NG) + (t & 1), op (t % 2 NG) / 2 of it
    __device__ __forceinline__ void q(int t)
    {
        const int w = t & 1, g = 2 * (t / (2 * NG)) + w, o = (t % (2 * NG)) >> 1, cb = 2 * w;
        if (o == 0) bv[w] = *reinterpret_cast<const float4*>(bias + acc_n(g, lane));
        else if (o <= 2 * CH) chain_op(k[cb + ((o - 1) & 1)], g, (o - 1) & 1, (o - 1) >> 1, bv[w]);
        else {
            const int j = o - 2 * CH - 1;
            if (DUMP && j == 0 && dump_tile != nullptr && r < nvalid)
                GSTORE4(dump_tile + (col0 / 32) * 1024 + lane * 4 + g * 256,
                        make_float4(k[cb].t0 * is, k[cb].t1 * is, k[cb + 1].t0 * is, k[cb + 1].t1 * is));
            u16* p = plane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane)) + j * fs_plane<PITCH>();
            *reinterpret_cast<uint2*>(p) = j == 0 ? make_uint2(k[cb].a, k[cb + 1].a) : make_uint2(k[cb].b, k[cb + 1].b);
        }
    }
};

// The dZ epilogue (lane = row) as OPS for MFMA gaps: dZ = dA ELU'(H) with dA = (hi + lo) / (s_z' s_w) and H = (h0 + h1) / s_h; what
// is split is dZ s_z.  With q = s_z / (s_z' s_w) and ih = 1 / s_h (powers of two): t = (hi + lo) q, m = min(h0 + h1, 0) ih,
// dZ s_z = fma(t, m, t) -- the value the unscaled rule fma(dA, min(H, 0), dA) gives, times s_z, exactly.  4 column groups x 18 ops.
template <int PITCH, bool DUMP>
struct H2DactOps {
    static constexpr int NS = 18, TOTAL = 4 * NS;
    const f32x16& hi;
    const f32x16& lo;
    const u16* hplane0;
    u16* zplane0;
    float* dump_tile;
    int col0, lane, r, nvalid;
    float qs, ih, iz, am;
    uint2 ha[2], hb[2];                   // H's two term words of a group, requested a group ahead
    float m[4], t[4];
    unsigned a0, b0, a1, b1;
    __device__ __forceinline__ H2DactOps(const f32x16& hi_, const f32x16& lo_, const u16* hp, int col0_, u16* zp, int lane_,
                                         float* dump_tile_, int nvalid_, float q_, float ih_, float iz_)
        : hi(hi_), lo(lo_), hplane0(hp), zplane0(zp), dump_tile(dump_tile_), col0(col0_), lane(lane_), r(lane_ & 31), nvalid(nvalid_),
          qs(q_), ih(ih_), iz(iz_), am(0.0f) {}
    __device__ __forceinline__ void request(int g)
    {
        const u16* p = hplane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane));
        ha[g & 1] = *reinterpret_cast<const uint2*>(p);
        hb[g & 1] = *reinterpret_cast<const uint2*>(p + fs_plane<PITCH>());
    }
    __device__ __forceinline__ void op(int g, int k)
    {
        const uint2 a = ha[g & 1], b = hb[g & 1];
        if (k == 0) { m[0] = fminf(h2_sum_lo(a.x, b.x), 0.0f); fs_pin(m[0]); }
        if (k == 1) { m[1] = fminf(h2_sum_hi(a.x, b.x), 0.0f); fs_pin(m[1]); }
        if (k == 2) { m[2] = fminf(h2_sum_lo(a.y, b.y), 0.0f); fs_pin(m[2]); }
        if (k == 3) { m[3] = fminf(h2_sum_hi(a.y, b.y), 0.0f); fs_pin(m[3]); }
        if (k == 4) { if (g + 1 < 4) request(g + 1); t[0] = (hi[4 * g + 0] + lo[4 * g + 0]) * qs; fs_pin(t[0]); }   // (the request is not pinned)
        if (k == 5) { t[1] = (hi[4 * g + 1] + lo[4 * g + 1]) * qs; fs_pin(t[1]); }
        if (k == 6) { t[2] = (hi[4 * g + 2] + lo[4 * g + 2]) * qs; fs_pin(t[2]); }
        if (k == 7) { t[3] = (hi[4 * g + 3] + lo[4 * g + 3]) * qs; fs_pin(t[3]); }
        if (k == 8) { t[0] = fmaf(t[0], m[0] * ih, t[0]); fs_pin(t[0]); }
        if (k == 9) { t[1] = fmaf(t[1], m[1] * ih, t[1]); fs_pin(t[1]); }
        if (k == 10) { t[2] = fmaf(t[2], m[2] * ih, t[2]); fs_pin(t[2]); }
        if (k == 11) { t[3] = fmaf(t[3], m[3] * ih, t[3]); fs_pin(t[3]); }
        if (k == 12) {
            if (DUMP && dump_tile != nullptr && r < nvalid)
                GSTORE4(dump_tile + (col0 / 32) * 1024 + lane * 4 + g * 256, make_float4(t[0] * iz, t[1] * iz, t[2] * iz, t[3] * iz));
            am = h2_max3(am, t[0], t[1]); am = h2_max3(am, t[2], t[3]); fs_pin(am);
        }
        if (k == 13) { a0 = h2_cvt2(t[0], t[1]); fs_pin(a0); }
        if (k == 14) { a1 = h2_cvt2(t[2], t[3]); fs_pin(a1); }
        if (k == 15) { b0 = h2_cvt2(h2_resid_lo(a0, t[0]), h2_resid_hi(a0, t[1])); fs_pin(b0); }
        if (k == 16) { b1 = h2_cvt2(h2_resid_lo(a1, t[2]), h2_resid_hi(a1, t[3])); fs_pin(b1); }
        if (k == 17) {
            u16* p = zplane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane));
            *reinterpret_cast<uint2*>(p) = make_uint2(a0, a1);
            *reinterpret_cast<uint2*>(p + fs_plane<PITCH>()) = make_uint2(b0, b1);
        }
    }
    __device__ __forceinline__ void q(int t_) { op(t_ / NS, t_ % NS); }
};

// dZ1 from the swapped-role dA1 GEMM (lane = column n, register = row acc_row(reg, lane)) as ops of two interleaved chains for the gaps
// of the same column tile's dW2 product (FsDz1Ops): register pair (8 s + 2 m, + 1) and word m of H1's two term fragments of k-step s
// -> word m of the two dZ1^T fragments of k-step s, which dW1 multiplies by as they are.
struct H2Dz1St { float t0, t1, ha, hb, vs; unsigned a, b; };
template <bool DUMP>
struct H2Dz1Ops {
    static constexpr int CH = 15, TOTAL = 8 * CH;
    const f32x16 &hi, &lo;
    const fs_u32x4 (&hw)[2][2];         // H1's term fragments [k-step][term], as words
    unsigned (&zq)[2][2][4];            // out: the dZ1^T fragments being built [k-step][term][word]
    float* dt;
    int lane, nvalid;
    float qs, ih, iz, zsum, am;
    H2Dz1St k[2];
    __device__ __forceinline__ H2Dz1Ops(const f32x16& hi_, const f32x16& lo_, const fs_u32x4 (&hw_)[2][2], unsigned (&q_)[2][2][4], float* dt_,
                                        int lane_, int nvalid_, float qs_, float ih_, float iz_)
        : hi(hi_), lo(lo_), hw(hw_), zq(q_), dt(dt_), lane(lane_), nvalid(nvalid_), qs(qs_), ih(ih_), iz(iz_), zsum(0.0f), am(0.0f) {}
    __device__ __forceinline__ void chain_op(int c, int sl, int i)
    {
        const int s = c >> 2, mw = c & 3, reg = 8 * s + 2 * mw;
        H2Dz1St& e = k[sl];
        const unsigned u0 = hw[s][0][mw], u1 = hw[s][1][mw];
        if (i == 0) { e.ha = h2_sum_lo(u0, u1); fs_pin(e.ha); }
        if (i == 1) { e.hb = h2_sum_hi(u0, u1); fs_pin(e.hb); }
        if (i == 2) { e.t0 = hi[reg] + lo[reg]; fs_pin(e.t0); }
        if (i == 3) { e.t1 = hi[reg + 1] + lo[reg + 1]; fs_pin(e.t1); }
        if (i == 4) { e.ha = fminf(e.ha, 0.0f) * ih; fs_pin(e.ha); }
        if (i == 5) { e.hb = fminf(e.hb, 0.0f) * ih; fs_pin(e.hb); }
        if (i == 6) { e.t0 *= qs; fs_pin(e.t0); }
        if (i == 7) { e.t1 *= qs; fs_pin(e.t1); }
        if (i == 8) { e.t0 = fmaf(e.t0, e.ha, e.t0); fs_pin(e.t0); }
        if (i == 9) {
            e.t1 = fmaf(e.t1, e.hb, e.t1); fs_pin(e.t1);
            if (DUMP) {
                const int ra = acc_row(reg, lane), rb = acc_row(reg + 1, lane);
                if (ra < nvalid) dt[frag_off(ra, lane & 31)] = e.t0 * iz;
                if (rb < nvalid) dt[frag_off(rb, lane & 31)] = e.t1 * iz;
            }
        }
        if (i == 10) { e.vs = e.t0 + e.t1; fs_pin(e.vs); }
        if (i == 11) { e.a = h2_cvt2(e.t0, e.t1); fs_pin(e.a); zq[s][0][mw] = e.a; }
        if (i == 12) { am = h2_max3(am, e.t0, e.t1); fs_pin(am); }
        if (i == 13) { e.b = h2_cvt2(h2_resid_lo(e.a, e.t0), h2_resid_hi(e.a, e.t1)); fs_pin(e.b); zq[s][1][mw] = e.b; }
        if (i == 14) { zsum += e.vs; fs_pin(zsum); }
    }
    // pairs 2 pp, 2 pp + 1 interleaved: ops 2 CH pp .. 2 CH (pp + 1) - 1
    __device__ __forceinline__ void q(int t) { const int pp = t / (2 * CH), o = t % (2 * CH); chain_op(2 * pp + (o & 1), o & 1, o >> 1); }
};
// Where element p of a layer's block lives in the (chunked) partial slabs, as a BYTE offset from `ws`; GC = the grid size when it is
// known at compile time (256: one workgroup per CU on this chip -- the index then needs no multiplication), 0 = read gridDim.x
template <unsigned GC>
__device__ __forceinline__ unsigned h2_slab_bytes(unsigned lbase, unsigned G, unsigned wg, unsigned p)
{
    if (GC != 0) return (lbase + ((p >> 8) * GC << 8) + (wg << 8) + (p & 255u)) << 2;
    return (lbase + (((p >> 8) * G + wg) << 8) + (p & 255u)) << 2;
}
// partial slab: tile (nt, kt) of a layer's [N][KOUT] block, still carrying its scale factor (the reduction removes it: the sum of
// scaled values times a power of two IS the scaled sum); lane = column k, registers = rows n.  Buffer stores: one scalar
// descriptor + a 32-bit lane offset, no 64-bit address arithmetic per element.
template <unsigned GC>
__device__ __forceinline__ void h2_store_tile(__amdgpu_buffer_rsrc_t rs, unsigned lbase, unsigned G, unsigned wg, int KOUT, int nt, int kt,
                                              const f32x16& acc, int lane)
{
    const int col = kt * 32 + (lane & 31);
    if (col < KOUT) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float v = acc[reg];       // (a named value: __builtin_bit_cast of the vector ELEMENT expression stored element 0 sixteen times)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rs,
                                                  h2_slab_bytes<GC>(lbase, G, wg, (unsigned)((nt * 32 + acc_row(reg, lane)) * KOUT + col)), 0, 0);
        }
    }
}

// MODE 0: the product; 1: DUMP (tests: chain values to HBM, unscaled); 2: STAMP (tools/stamp_fused.py: the stamps of mlp_fused_step_kernel<2>)
// `fsc`: the scale table (read only here); `wsmax` [gridDim.x][8]: this launch's class maxima of |scaled value| per workgroup
template <int MODE>
__global__ __launch_bounds__(THREADS, 1) void mlp_fused_step_h2_kernel(
    const float* __restrict__ P, const u16* __restrict__ PH, const u16* __restrict__ PTH, const float* __restrict__ fsc,
    const float* __restrict__ x, long n, const float* __restrict__ action, const float* __restrict__ old_logp,
    const float* __restrict__ adv, const float* __restrict__ target, const float* __restrict__ var, float inv_batch, float clip,
    float* __restrict__ ws, float* __restrict__ wsmax, float* __restrict__ loss_part, FusedDump dump)
{
    constexpr bool DUMP = MODE == 1, STAMP = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char h2_lds_raw[];
    u16* lds = reinterpret_cast<u16*>(h2_lds_raw);
    unsigned long long* stamps = nullptr;
    int tslot = 0;
    (void)stamps; (void)tslot;
    if (STAMP) {
        stamps = reinterpret_cast<unsigned long long*>(dump.out) + ((long)blockIdx.x * 64 + 62) * FS_STAMP_SLOTS;
        stamp<STAMP>(stamps, 0);
        if (threadIdx.x == 0) stamps[1] = realtime_cu();
    }
    u16* X = lds + H2_OFF_X;
    u16* H1 = lds + H2_OFF_H1;
    u16* H2 = lds + H2_OFF_H2;
    u16* H3 = lds + H2_OFF_H3;
    u16* Z3 = H3;                                                 // dZ3 overwrites H3 in place
    u16* Z2 = lds + H2_OFF_R;
    float* part = reinterpret_cast<float*>(lds + H2_OFF_R);       // layer-4 split-K partials [wave][32][32]
    u16* Z4 = lds + H2_OFF_Z4;
    float* xs = reinterpret_cast<float*>(lds + H2_OFF_XS);        // [32][73] fp32: the next tile's rows as they lie in HBM
    float* tail = reinterpret_cast<float*>(lds + H2_OFF_F32);
    float* bias1 = tail, *bias2 = tail + MLP_H1, *bias3 = bias2 + MLP_H2, *bias4 = bias3 + MLP_H3, *rowloss = bias4 + MLP_OUT;
    float* c_invL = rowloss + 2 * BM, *c_invVar = c_invL + MLP_OUT, *c_hld = c_invVar + MLP_OUT;
    float* sc = c_hld + 4;                                        // s[0 .. 15] | 1 / s at [16 ..]
    float* amax = sc + 32;                                        // [8][256]: per-thread running maxima of |scaled value| per class

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long ntiles = (n + BM - 1) / BM;
    const long total = n * MLP_IN;

    // dW accumulators (mlp_fused_step.inc: REGISTER PLACEMENT): 16 tiles in the AGPRs, aW3[0][*] and aW4 in VGPRs
    f32x16 aW1[2][3], aW2[4][2], aW3[2][2], aW4;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        aW4[i] = 0.0f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) aW1[a][b][i] = 0.0f;
#pragma unroll
            for (int b = 0; b < 2; ++b) aW3[a][b][i] = 0.0f;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) aW2[a][b][i] = 0.0f;
    }
    float bs1[2] = {0.0f, 0.0f}, bs2 = 0.0f, bs3 = 0.0f, bs4 = 0.0f;

    typedef __attribute__((address_space(3))) void* lptr_t;
    const unsigned xs_lds = (unsigned)(unsigned long)(lptr_t)xs;
    constexpr int XW = BM * MLP_IN / 4 / NWAVE;                                // 16-byte pieces per wave: 146
    static_assert(XW * NWAVE * 4 == BM * MLP_IN && XW > 128 && XW <= 192, "x_fetch: three DMA instructions per wave, the third partial");
    const bool x_al16 = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    // The fetch runs once per tile in the middle of the backward pass (stamped: 0.46k cycles in its first form): tile numbers as 32-bit
    // values (the launcher refuses n >= 2^36 rows) -- 64-bit compares of uniform values run on the VECTOR unit, there is no s_cmp_lt_i64,
    // and come back through vcc --, and the addresses as ONE scalar base per wave + a 32-bit lane offset (the instruction's saddr form).
    const int ntiles32 = (int)ntiles, nfull32 = x_al16 ? (int)(n / BM) : 0;      // tiles that are whole and 16-byte aligned: DMA
    auto x_fetch = [&](int tile32, int tl) {     // mlp_fused_step.inc: the next tile's rows by LDS-DMA, wave w the rows its threads convert
        const long tile = tile32;
        const long base = tile * (BM * MLP_IN);
        const int w = __builtin_amdgcn_readfirstlane(tl >> 6), l = tl & 63;
        if (tile32 < nfull32) {
            const char* sbase = reinterpret_cast<const char*>(x) + base * 4 + (long)(16 * XW) * w;       // (uniform: scalar registers)
            const unsigned v0 = 16u * (unsigned)l, v1 = v0 + 1024u, v2 = v0 + 2048u;
            const unsigned dst = xs_lds + 16u * (unsigned)(XW * w);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %4\n\t"
                         "s_add_u32 m0, %1, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %4\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "s"(dst), "v"(v0), "v"(v1), "s"(sbase) : "memory", "scc");
            if (l + 128 < XW)
                asm volatile("s_mov_b32 %0, m0\n\ts_add_u32 m0, %1, 0x800\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "s"(dst), "v"(v2), "s"(sbase) : "memory", "scc");
        } else {
            for (int i = l; i < 4 * XW; i += 64) xs[4 * XW * w + i] = base + 4 * XW * w + i < total ? x[base + 4 * XW * w + i] : 0.0f;
        }
    };

    long tile = blockIdx.x;
    if (tile < ntiles) x_fetch((int)tile, tid);
    // THE HEAD: everything else the kernel reads before its first tile is requested HERE, behind the first x DMA and ahead of the one
    // wait below -- one round trip to memory instead of five in a row (var, the scale table, three groups of biases, each loaded,
    // waited for and stored before the next was requested) with layer 1's first weight fragments a sixth one behind the barriers.
    // No load stands under a condition (the compiler sinks such a load below its branch, behind the wait): a thread without a
    // column of its own reads a word of somebody else's.  The arithmetic on the loaded values is what it was.
    WeightHead2 w1;                                                       // the FIRST tile's layer-1 head; later tiles: the loop top
    h2_gemm_prefetch<MLP_IN_PAD>(w1, PH + H2_OFF_PH1, 2 * wave, tid & 63);
    float g_var = var[tid < MLP_NACT ? tid : 0], g_sc = fsc[tid & 31];
    float g_b1 = P[MLP_OFF_B1 + tid], g_b23 = P[tid < MLP_H2 ? MLP_OFF_B2 + tid : MLP_OFF_B3 + (tid - MLP_H2)];
    float g_b4 = P[MLP_OFF_B4 + (tid & (MLP_OUT - 1))];
    const float s_h1 = fsc[H2C_H1], s_h2 = fsc[H2C_H2], s_h3 = fsc[H2C_H3];      // (uniform: scalar loads)
    // L2 warm-up (h2_warm.h): one dword of every 128-byte line of this workgroup's share of the two weight planes, into registers
    // nobody reads.  asm, so that the compiler keeps them; the registers stay reserved up to the wait below, which is the only
    // wait these loads ever stand in front of.
    float warm0, warm1;
    {
        constexpr unsigned PHB = H2_PH_HALVES * 2, PTHB = H2_PTH_HALVES * 2;
        static_assert(h2_warm_loads(PHB, THREADS) == 1 && h2_warm_loads(PTHB, THREADS) == 1, "one load per plane and thread");
        const unsigned sh = h2_warm_share(blockIdx.x);
        const unsigned o0 = h2_warm_offset(PHB, sh, 0, (unsigned)tid, THREADS), o1 = h2_warm_offset(PTHB, sh, 0, (unsigned)tid, THREADS);
        asm volatile("global_load_dword %0, %2, %4\n\tglobal_load_dword %1, %3, %5"
                     : "=&v"(warm0), "=&v"(warm1) : "v"(o0), "v"(o1), "s"(PH), "s"(PTH) : "memory");
    }
#pragma unroll
    for (int c = 0; c < H2_NACT_CLASSES; ++c) amax[c * THREADS + tid] = 0.0f;
    if (!STAMP) {       // the accumulator clears HERE, while everything above is in flight (mlp_fused_step.inc)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) asm volatile("" : "+a"(aW1[a][b]));
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) asm volatile("" : "+a"(aW2[a][b]));
#pragma unroll
        for (int b = 0; b < 2; ++b) { asm volatile("" : "+a"(aW3[1][b])); asm volatile("" : "+v"(aW3[0][b])); }
        asm volatile("" : "+v"(aW4));
    }
    // the one wait of the head (fs_dma_drain's, taking the loaded values so that their loads stand in front of it)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(g_var), "+v"(g_sc), "+v"(g_b1), "+v"(g_b23), "+v"(g_b4), "+v"(warm0), "+v"(warm1) : : "memory");
    if (tid < 32) {     // loss-phase constants per output column (ppo.py:185-189) and the scale table
        const bool act = tid < MLP_NACT;
        const float L = act ? sqrtf(g_var) : 1.0f;
        c_invL[tid] = act ? 1.0f / L : 0.0f;
        c_invVar[tid] = act ? 1.0f / g_var : 0.0f;
        float hld = act ? logf(L) : 0.0f;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) hld += __shfl_xor(hld, o, 32);
        if (tid == 0) c_hld[0] = hld;
        sc[tid] = g_sc;
    }
    bias1[tid] = g_b1 * s_h1;                                             // (the epilogues add the bias times s)
    if (tid < MLP_H2) bias2[tid] = g_b23 * s_h2;
    else bias3[tid - MLP_H2] = g_b23 * s_h3;
    if (tid < MLP_OUT) bias4[tid] = g_b4;
    __syncthreads();                                                      // the scale table is in LDS
    if (tile < ntiles) {                                                  // the workgroup's first tile: converted at once
        H2XStoreOps xc0(xs, X, tid, sc[H2C_X]);
        xc0.all();
        h2_amax_fold(amax, H2C_X, tid, xc0.am);
    }
    __syncthreads();
    int par = 0;

    if (STAMP) stamp<STAMP>(reinterpret_cast<unsigned long long*>(dump.out) + ((long)blockIdx.x * 64 + 62) * FS_STAMP_SLOTS, 2);
    int grid_v = gridDim.x;
    asm volatile("" : "+v"(grid_v));
    for (; tile < ntiles; tile += __builtin_amdgcn_readfirstlane(grid_v), par ^= 1) {
        u16* Xc = X + par * H2_X_HALVES;
        u16* Xn = X + (par ^ 1) * H2_X_HALVES;
        const long row0 = tile * BM;
        const int nvalid = (int)(n - row0 < BM ? n - row0 : BM);
        int tl = tid;
        asm volatile("" : "+v"(tl));
        const int lane = tl & 63;
        const int r = lane & 31;
        float* d_h1 = DUMP ? dump.h1 + row0 * MLP_H1 : nullptr;
        float* d_h2 = DUMP ? dump.h2 + row0 * MLP_H2 : nullptr;
        float* d_h3 = DUMP ? dump.h3 + row0 * MLP_H3 : nullptr;

        if (STAMP) { stamps = reinterpret_cast<unsigned long long*>(dump.out) + ((long)blockIdx.x * 64 + tslot) * FS_STAMP_SLOTS; ++tslot; }
        stamp<STAMP>(stamps, 0);
        if (!STAMP) fs_split(n);
        // (the workgroup's first tile: requested at kernel entry.  A wave-uniform compare of 32-bit tile numbers; the loop body exists once)
        if ((int)tile != (int)blockIdx.x) h2_gemm_prefetch<MLP_IN_PAD>(w1, PH + H2_OFF_PH1, 2 * wave, lane);
        stamp<STAMP>(stamps, 1);
        if (!STAMP) fs_split(n);

        // ---- P1: layer 1, this wave's 64 columns -------------------------------------------------------------------
        WeightHead2 w4, wt4;
        {
            f32x16 hi, lo;
            WeightHead2 w1b, w2a;
            float am = 0.0f;
            const float k1 = sc[H2_FSC_INV + H2C_X] * sc[H2_FSC_INV + H2C_W1], s1 = sc[H2C_H1];
            const float k2 = sc[H2_FSC_INV + H2C_H1] * sc[H2_FSC_INV + H2C_W2], s2 = sc[H2C_H2];
            WeightHead2 w3;
            {   // layer 1's epilogues ride in MFMA gaps (dqn_fused.inc's scheme) -- column tile a's in tile b's GEMM, tile b's in the first
                // half of layer 2's GEMM, whose k-steps are ordered so that the half reads tile-a columns of H1 only (H2GemmHost MODE 1,
                // one barrier between the halves)
                f32x16 hi0, lo0;
                const float is1 = sc[H2_FSC_INV + H2C_H1];
                h2_gemm_prefetch<MLP_IN_PAD>(w1b, PH + H2_OFF_PH1, 2 * wave + 1, lane);
                h2_gemm<MLP_IN_PAD, FS_PX, false>(w1, PH + H2_OFF_PH1, 2 * wave, Xc, 0, hi0, lo0, lane);
                h2_gemm_prefetch<MLP_H2>(w2a, PH + H2_OFF_PH2, wave, lane);
                {
                    H2EluOps<FS_P1, DUMP> e(hi0, lo0, bias1, 64 * wave, H1, lane, d_h1, nvalid, k1, s1, is1);
                    h2_gemm_host<MLP_IN_PAD, FS_PX, false>(w1b, PH + H2_OFF_PH1, 2 * wave + 1, Xc, 0, hi, lo, lane, e);
                    am = e.am;
                }
                stamp<STAMP>(stamps, 2);
                if (!STAMP) fs_split(n);
                __syncthreads();                                              // every wave's tile-a columns of H1 are stored
                stamp<STAMP>(stamps, 3);
                if (!STAMP) fs_split(n);
                // ---- P2: layer 2, K = 256 in the split k order: tile b's epilogue of layer 1 in the first half's gaps --------------
                {
                    H2EluOps<FS_P1, DUMP> e(hi, lo, bias1, 64 * wave + 32, H1, lane, d_h1, nvalid, k1, s1, is1);
                    h2_gemm_host<MLP_H1, FS_P1, false, true, 2, 24, 1, 2 * MLP_H2 * (MLP_H1 / 2)>(w2a, PH + H2_OFF_PH2, wave, H1, 0, hi0, lo0, lane, e);
                    am = h2_nanmax(am, e.am);
                }
                h2_amax_fold(amax, H2C_H1, tl, am);
                hi = hi0; lo = lo0;
            }
            h2_gemm_prefetch<MLP_H2>(w3, PH + H2_OFF_PH3, wave, lane);
            am = 0.0f;
            {   // (exposed, but as the pinned ops of four interleaved chains: the loop form is one dependent chain per pair of outputs)
                H2EluOps<FS_P2, DUMP> e(hi, lo, bias2, 32 * wave, H2, lane, d_h2, nvalid, k2, s2, sc[H2_FSC_INV + H2C_H2]);
                __builtin_amdgcn_sched_barrier(0);
                fs_run_ops<0, H2EluOps<FS_P2, DUMP>::TOTAL>(e);
                __builtin_amdgcn_sched_barrier(0);
                am = e.am;
            }
            h2_amax_fold(amax, H2C_H2, tl, am);
            __syncthreads();
            stamp<STAMP>(stamps, 4);
            if (!STAMP) fs_split(n);
            // ---- P3: layer 3 (actor | critic heads stacked) ----------------------------------------------------------
            const float k3 = sc[H2_FSC_INV + H2C_H2] * sc[H2_FSC_INV + H2C_W3], s3 = sc[H2C_H3];
            h2_gemm_prefetch<32>(w4, PH + H2_OFF_PH4 + (long)(2 * wave) * 1024, 0, lane);
            h2_gemm<MLP_H2, FS_P2, false>(w3, PH + H2_OFF_PH3, wave, H2, 0, hi, lo, lane);
            am = 0.0f;
            {
                H2EluOps<FS_P2, DUMP> e(hi, lo, bias3, 32 * wave, H3, lane, d_h3, nvalid, k3, s3, sc[H2_FSC_INV + H2C_H3]);
                __builtin_amdgcn_sched_barrier(0);
                fs_run_ops<0, H2EluOps<FS_P2, DUMP>::TOTAL>(e);
                __builtin_amdgcn_sched_barrier(0);
                am = e.am;
            }
            h2_amax_fold(amax, H2C_H3, tl, am);
            // (no barrier: H3's columns 32 w .. 32 w + 31 are only ever read by the wave that wrote them -- layer 4's split-K range,
            //  dW4's operand and the dZ3 epilogue of wave w are exactly these columns -- and a wave's LDS operations complete in order)
            stamp<STAMP>(stamps, 5);
            if (!STAMP) fs_split(n);
        }
        // ---- P4: layer 4, split-K over the four waves (32 k each), partials (still carrying s_w s_h3) to LDS -------------------
        const int lrow = tl >> 3, lq = tl & 7;
        const bool lin = lrow < nvalid;
        float l_a[4], l_olp, l_adv, l_tgt;
        {
            const float* act_r = action + (row0 + lrow) * MLP_NACT + 4 * lq;
#pragma unroll
            for (int j = 0; j < 4; ++j) l_a[j] = (lin && 4 * lq + j < MLP_NACT) ? act_r[j] : 0.0f;
            l_olp = lin ? (old_logp + row0)[lrow] : 0.0f;
            l_adv = lin ? (adv + row0)[lrow] : 0.0f;
            l_tgt = lin ? (target + row0)[lrow] : 0.0f;
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            h2_gemm_prefetch<MLP_OUT>(wt4, PTH + H2_OFF_PTH4, wave, lane);
            f32x16 hi, lo;
            h2_gemm<32, FS_P2, false>(w4, PH + H2_OFF_PH4 + (long)(2 * wave) * 1024, 0, H3, 32 * wave, hi, lo, lane);
            float* pw = part + wave * (BM * MLP_OUT);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(pw + r * MLP_OUT + 4 * ((acc_n(g, lane) >> 2) ^ ((r >> 1) & 7))) =
                    make_float4(hi[4 * g] + lo[4 * g], hi[4 * g + 1] + lo[4 * g + 1], hi[4 * g + 2] + lo[4 * g + 2],
                                hi[4 * g + 3] + lo[4 * g + 3]);
        }
        __syncthreads();
        stamp<STAMP>(stamps, 6);
        if (!STAMP) fs_split(n);
        // ---- P5: outputs, loss, dZ4 (ppo.py:184-194): mlp_fused_step.inc's phase on the unscaled sums; the row's loss is loss_head.inc's
        //          ppo_row_loss with FAST_EXP (v_exp_f32 on the ratio, ~1 ulp) --------------------------------------------------------
        {
            const float k4 = sc[H2_FSC_INV + H2C_H3] * sc[H2_FSC_INV + H2C_W4], sz4 = sc[H2C_Z4];
            const int c0 = 4 * lq;
            const int cs = 4 * (lq ^ ((lrow >> 1) & 7));
            const float4 p0 = *reinterpret_cast<const float4*>(part + lrow * MLP_OUT + cs);
            const float4 p1 = *reinterpret_cast<const float4*>(part + BM * MLP_OUT + lrow * MLP_OUT + cs);
            const float4 p2 = *reinterpret_cast<const float4*>(part + 2 * BM * MLP_OUT + lrow * MLP_OUT + cs);
            const float4 p3 = *reinterpret_cast<const float4*>(part + 3 * BM * MLP_OUT + lrow * MLP_OUT + cs);
            const float4 b4v = *reinterpret_cast<const float4*>(bias4 + c0);
            const float4 iL = *reinterpret_cast<const float4*>(c_invL + c0);
            const float4 iV = *reinterpret_cast<const float4*>(c_invVar + c0);
            const float half_log_det = c_hld[0];
            const float zz[4] = {fmaf(((p0.x + p1.x) + p2.x) + p3.x, k4, b4v.x), fmaf(((p0.y + p1.y) + p2.y) + p3.y, k4, b4v.y),
                                 fmaf(((p0.z + p1.z) + p2.z) + p3.z, k4, b4v.z), fmaf(((p0.w + p1.w) + p2.w) + p3.w, k4, b4v.w)};
            const float invL[4] = {iL.x, iL.y, iL.z, iL.w}, invV[4] = {iV.x, iV.y, iV.z, iV.w};
            float y[4], xsq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = c0 + j;
                const float yv = col < MLP_NACT ? elu(zz[j]) : ((col == MLP_NACT) ? zz[j] : 0.0f);
                if (DUMP && lin) (dump.out + row0 * MLP_OUT)[frag_off(lrow, col)] = yv;
                y[j] = lin ? yv : 0.0f;
                const float xj = col < MLP_NACT ? (l_a[j] - y[j]) * invL[j] : 0.0f;
                xsq[j] = xj * xj;
            }
            const float M = fs_sum8((xsq[0] + xsq[1]) + (xsq[2] + xsq[3]));
            const float vrow = fs_sum8(lq == MLP_NACT / 4 ? y[MLP_NACT % 4] : 0.0f);
            float d[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pol = 0.0f, hub = 0.0f;
            if (lin) {
                const PpoRowLoss rl = ppo_row_loss<true>(M, half_log_det, l_olp, l_adv, vrow, l_tgt, inv_batch, clip);
                pol = rl.pol;
                hub = rl.hub;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = c0 + j;
                    if (col < MLP_NACT) d[j] = ppo_mean_dz4(rl.c, l_a[j], y[j], invV[j]);
                    else if (col == MLP_NACT) d[j] = rl.dv;
                    if (DUMP) (dump.dz4 + row0 * MLP_OUT)[frag_off(lrow, col)] = d[j];
                }
            }
            float am = 0.0f;
            h2_store4<FS_P4>(Z4, lrow, c0, make_float4(d[0] * sz4, d[1] * sz4, d[2] * sz4, d[3] * sz4), am);
            h2_amax_fold(amax, H2C_Z4, tl, am);
            if (lq == 0) { rowloss[2 * lrow] = pol; rowloss[2 * lrow + 1] = hub; }
        }
        __syncthreads();
        stamp<STAMP>(stamps, 7);
        if (!STAMP) fs_split(n);
        FsTr tr1, tr2, trx, tr4;
        fs_tr_init<FS_P1>(tr1, lane);
        fs_tr_init<FS_P2>(tr2, lane);
        fs_tr_init<FS_PX>(trx, lane);
        fs_tr_init<FS_P4>(tr4, lane);
        // ---- P6: dA3 = dZ4 . W4 -> dZ3;  dW4 += dZ4^T H3 ---------------------------------------------------------------
        if (tl < 32 && loss_part) tile_loss_sum<2>(rowloss, tl, loss_part + 2 * tile);
        WeightHead2 wt2;
        {
            f32x16 hi, lo;
            WeightHead2 wt3;
            h2_gemm<MLP_OUT, FS_P4, false>(wt4, PTH + H2_OFF_PTH4, wave, Z4, 0, hi, lo, lane);
            h2_gemm_prefetch<MLP_H3>(wt3, PTH + H2_OFF_PTH3, wave, lane);
            {   // dW4 and db4 (10 MFMAs) with the dZ3 epilogue in their gaps
                f32x16 cs;
                const f16x8 ones = h2_ones();
                H2DactOps<FS_P2, DUMP> ep3(hi, lo, H3, 32 * wave, Z3, lane, DUMP ? dump.dz3 + row0 * MLP_H3 : nullptr, nvalid,
                                           sc[H2C_Z3] * sc[H2_FSC_INV + H2C_Z4] * sc[H2_FSC_INV + H2C_W4], sc[H2_FSC_INV + H2C_H3],
                                           sc[H2_FSC_INV + H2C_Z3]);
                ep3.request(0);
                // dZ3 overwrites H3 in place: both k-steps' H3 fragments of this wave's columns are read (and pinned) before the first store
                f16x8 af3[2][2];
                h2_trws<FS_P2>(af3[0], H3, tr2, wave, 0);
                h2_trws<FS_P2>(af3[1], H3, tr2, wave, 1);
#pragma unroll
                for (int qq = 0; qq < 2; ++qq)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) asm volatile("" : "+v"(af3[qq][pl]));
#define H2_P6_HALF(S_)                                                                                                            \
                {                                                                                                                 \
                    f16x8 zf[2];                                                                                                  \
                    const f16x8 (&af)[2] = af3[S_];                                                                               \
                    h2_trns<FS_P4>(zf, Z4, tr4, 0, S_);                                                                           \
                    h2_mfma_vg(aW4, zf[0], af[1]); fs_host_gap<5 * S_ + 0, 10>(ep3);                                              \
                    h2_mfma_vg(aW4, zf[1], af[0]); fs_host_gap<5 * S_ + 1, 10>(ep3);                                              \
                    h2_mfma_vg(aW4, zf[0], af[0]); fs_host_gap<5 * S_ + 2, 10>(ep3);                                              \
                    if (S_ == 0) h2_mfma_vg0(cs, ones, zf[1]); else h2_mfma_vg(cs, ones, zf[1]);    /* db4 (every wave) */         \
                    fs_host_gap<5 * S_ + 3, 10>(ep3);                                                                             \
                    h2_mfma_vg(cs, ones, zf[0]); fs_host_gap<5 * S_ + 4, 10>(ep3);                                                \
                    fs_mfma_settle(aW4, cs);                                                                                      \
                    __builtin_amdgcn_sched_barrier(0);                                                                            \
                }
                H2_P6_HALF(0)
                H2_P6_HALF(1)
#undef H2_P6_HALF
                bs4 += fs_colsum_done(cs);
                h2_amax_fold(amax, H2C_Z3, tl, ep3.am);
            }
            __syncthreads();
            stamp<STAMP>(stamps, 8);
            if (!STAMP) fs_split(n);
            // ---- P7: dA2 = dZ3 . W3 -> dZ2 (region R);  dW3 += dZ3^T H2 --------------------------------------------------
            h2_gemm<MLP_H3, FS_P2, false>(wt3, PTH + H2_OFF_PTH3, wave, Z3, 0, hi, lo, lane);
            h2_gemm_prefetch<MLP_H2>(wt2, PTH + H2_OFF_PTH2, 2 * wave, lane);
            {
                const int nt0 = 2 * (wave >> 1), kt0 = 2 * (wave & 1);
                f32x16 cs;
                H2DactOps<FS_P2, DUMP> ep2(hi, lo, H2, 32 * wave, Z2, lane, DUMP ? dump.dz2 + row0 * MLP_H2 : nullptr, nvalid,
                                           sc[H2C_Z2] * sc[H2_FSC_INV + H2C_Z3] * sc[H2_FSC_INV + H2C_W3], sc[H2_FSC_INV + H2C_H2],
                                           sc[H2_FSC_INV + H2C_Z2]);
                ep2.request(0);
#define H2_P7_STEP(S_)                                                                                                            \
                {                                                                                                                 \
                    f16x8 zf[2][2], af[2][2];                                                                                     \
                    _Pragma("unroll") for (int a = 0; a < 2; ++a) {                                                               \
                        h2_trws<FS_P2>(zf[a], Z3, tr2, nt0 + a, S_);                                                              \
                        h2_trws<FS_P2>(af[a], H2, tr2, kt0 + a, S_);                                                              \
                    }                                                                                                             \
                    h2_dw_v_host<12 * S_ + 0, 24>(aW3[0][0], zf[0], af[0], ep2);        /* VGPR-resident tiles */                  \
                    h2_dw_host<12 * S_ + 3, 24>(aW3[1][0], zf[1], af[0], ep2);                                                    \
                    h2_dw_v_host<12 * S_ + 6, 24>(aW3[0][1], zf[0], af[1], ep2);                                                  \
                    h2_dw_host<12 * S_ + 9, 24>(aW3[1][1], zf[1], af[1], ep2);                                                    \
                    /* db3 of column tile nt0 + (wave & 1): the four waves cover the four tiles */                                \
                    if (wave & 1) { if (S_ == 0) h2_colsum_step<true, false>(cs, zf[1]); else h2_colsum_step<false>(cs, zf[1]); } \
                    else { if (S_ == 0) h2_colsum_step<true, false>(cs, zf[0]); else h2_colsum_step<false>(cs, zf[0]); }          \
                    __builtin_amdgcn_sched_barrier(0);                                                                            \
                }
                H2_P7_STEP(0)
                H2_P7_STEP(1)
#undef H2_P7_STEP
                bs3 += fs_colsum_done(cs);
                h2_amax_fold(amax, H2C_Z2, tl, ep2.am);
            }
        }
        __syncthreads();
        stamp<STAMP>(stamps, 9);
        if (!STAMP) fs_split(n);
        // ---- P8: dA1 = dZ2 . W2 with the operand roles SWAPPED -> dZ1 as transposed fragments in registers;
        //          dW2 += dZ2^T H1 and dW1 += dZ1^T X for this wave's two column tiles of H1 / dZ1 ---------------------------
        {
            WeightHead2 wt2b;
            f32x16 cs2;
            const int tile_next = (int)tile + __builtin_amdgcn_readfirstlane(grid_v);
            const bool more = tile_next < ntiles32;
            H2XStoreOps xc(xs, Xn, tl, sc[H2C_X]);
            const float q1 = sc[H2C_Z1] * sc[H2_FSC_INV + H2C_Z2] * sc[H2_FSC_INV + H2C_W2], ih1 = sc[H2_FSC_INV + H2C_H1],
                        iz1 = sc[H2_FSC_INV + H2C_Z1];
            float am1 = 0.0f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ct = 2 * wave + t;
                f16x8 z1f[2][2];
                {
                    f32x16 hi, lo;
                    if (t == 0) h2_gemm<MLP_H2, FS_P2, true>(wt2, PTH + H2_OFF_PTH2, ct, Z2, 0, hi, lo, lane);
                    else h2_gemm<MLP_H2, FS_P2, true>(wt2b, PTH + H2_OFF_PTH2, ct, Z2, 0, hi, lo, lane);
                    if (t == 0) { stamp<STAMP>(stamps, 12); if (!STAMP) fs_split(n); }
                    if (STAMP && t == 1) stamp<STAMP>(stamps, 16);
                    if (t == 0 && more) x_fetch(tile_next, tl);
                    if (STAMP && t == 0) stamp<STAMP>(stamps, 19);
                    f16x8 hf[2][2], zf[2][2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) h2_trws<FS_P1>(hf[s], H1, tr1, ct, s);
                    h2_trws<FS_P2>(zf[0], Z2, tr2, 0, 0);
                    unsigned q[2][2][4];
                    const fs_u32x4 hw[2][2] = {{__builtin_bit_cast(fs_u32x4, hf[0][0]), __builtin_bit_cast(fs_u32x4, hf[0][1])},
                                               {__builtin_bit_cast(fs_u32x4, hf[1][0]), __builtin_bit_cast(fs_u32x4, hf[1][1])}};
                    H2Dz1Ops<DUMP> ez(hi, lo, hw, q, DUMP ? dump.dz1 + row0 * MLP_H1 + ct * 1024 : nullptr, lane, nvalid, q1, ih1, iz1);
                    if (STAMP && t == 0) stamp<STAMP>(stamps, 20);
#define H2_P8_STEP(C_)                                                                                                            \
                    {                                                                                                             \
                        constexpr int c = (C_), s = c >> 2, nt = c & 3;                                                           \
                        if (c + 1 < 8) h2_trws<FS_P2>(zf[(c + 1) & 1], Z2, tr2, (c + 1) & 3, (c + 1) >> 2);                        \
                        __builtin_amdgcn_sched_barrier(0);                                                                        \
                        h2_dw_host<3 * c, 24>(aW2[nt][t], zf[c & 1], hf[s], ez);                                                  \
                        if (STAMP && t == 0 && c == 3) stamp<STAMP>(stamps, 18);                                                  \
                        if (STAMP && t == 0 && c == 0) stamp<STAMP>(stamps, 21);                                                  \
                        if (t == 0 && nt == wave) {                        /* db2 of column tile `wave` (wave-uniform branch) */   \
                            if (s == 0) h2_colsum_step<true, false>(cs2, zf[c & 1]); else h2_colsum_step<false>(cs2, zf[c & 1]);  \
                        }                                                                                                         \
                        if (STAMP && t == 0 && c <= 1) stamp<STAMP>(stamps, 22 + c);                                              \
                        __builtin_amdgcn_sched_barrier(0);                                                                        \
                    }
                    H2_P8_STEP(0) H2_P8_STEP(1) H2_P8_STEP(2) H2_P8_STEP(3) H2_P8_STEP(4) H2_P8_STEP(5) H2_P8_STEP(6) H2_P8_STEP(7)
#undef H2_P8_STEP
                    if (STAMP && t == 0) stamp<STAMP>(stamps, 17);
                    bs1[t] += ez.zsum;
                    am1 = h2_nanmax(am1, ez.am);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int p = 0; p < 2; ++p) {
                            const fs_u32x4 qq = {q[s][p][0], q[s][p][1], q[s][p][2], q[s][p][3]};
                            z1f[s][p] = __builtin_bit_cast(f16x8, qq);
                        }
                }
                if (t == 0) {
                    bs2 += fs_colsum_done(cs2);
                    fs_dma_drain();                                      // this wave's share of the next tile's rows has landed
                    h2_gemm_prefetch<MLP_H2>(wt2b, PTH + H2_OFF_PTH2, 2 * wave + 1, lane);
                }
                stamp<STAMP>(stamps, t == 0 ? 13 : 15);
                if (!STAMP) fs_split(n);
                {
                    // dW1[n tile ct][k tile kt], both k-steps back to back; the conversion of the NEXT tile's rows rides behind the 36
                    // MFMAs of the two column tiles (24 ops: one behind each of the first MFMAs)
                    f16x8 af[2][2][2];                                     // [buffer][k-step][term]
                    h2_trns<FS_PX>(af[0][0], Xc, trx, 0, 0);
                    h2_trns<FS_PX>(af[0][1], Xc, trx, 0, 1);
#define H2_DW1_KT(KT_)                                                                                                            \
                    {                                                                                                             \
                        constexpr int kt = (KT_);                                                                                 \
                        if (kt + 1 < 3) {                                                                                         \
                            h2_trns<FS_PX>(af[(kt + 1) & 1][0], Xc, trx, kt + 1, 0);                                              \
                            h2_trns<FS_PX>(af[(kt + 1) & 1][1], Xc, trx, kt + 1, 1);                                              \
                        }                                                                                                         \
                        __builtin_amdgcn_sched_barrier(0);                                                                        \
                        if (t == 0) {                                                                                             \
                            h2_dw_host<6 * kt, 36>(aW1[0][kt], z1f[0], af[kt & 1][0], xc);                                        \
                            h2_dw_host<6 * kt + 3, 36>(aW1[0][kt], z1f[1], af[kt & 1][1], xc);                                    \
                        } else {                                                                                                  \
                            h2_dw_host<18 + 6 * kt, 36>(aW1[1][kt], z1f[0], af[kt & 1][0], xc);                                   \
                            h2_dw_host<18 + 6 * kt + 3, 36>(aW1[1][kt], z1f[1], af[kt & 1][1], xc);                               \
                        }                                                                                                         \
                        __builtin_amdgcn_sched_barrier(0);                                                                        \
                    }
                    H2_DW1_KT(0) H2_DW1_KT(1) H2_DW1_KT(2)
#undef H2_DW1_KT
                }
                if (t == 0) stamp<STAMP>(stamps, 14);
            }
            h2_amax_fold(amax, H2C_Z1, tl, am1);
            if (more) h2_amax_fold(amax, H2C_X, tl, xc.am);   // (a workgroup's LAST tile converts whatever the staging block holds into a buffer nobody reads)
        }
        stamp<STAMP>(stamps, 10);
        if (!STAMP) fs_split(n);
        __syncthreads();
        stamp<STAMP>(stamps, 11);
        if (!STAMP) fs_split(n);
        // w1 is dead from P1 on.  The (empty) definition says so: without it the loop-top condition, which liveness does not see
        // through, would keep w1's 16 registers reserved through every tile for a value that only the first tile reads.
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                fs_u32x4 nothing;
                asm volatile("" : "=v"(nothing));
                w1.b[s].p[p] = __builtin_bit_cast(float4, nothing);
            }
    }
    if (STAMP) stamps = reinterpret_cast<unsigned long long*>(dump.out) + ((long)blockIdx.x * 64 + 63) * FS_STAMP_SLOTS;
    stamp<STAMP>(stamps, 0);
    if (!STAMP) fs_split(n);

    // ---- one partial slab per workgroup (the packed gradient's layout); the products leave WITH their scale factors, which workgroup
    //      0 leaves for the reduction behind the class maxima: [G * 8 + l] = 1 / (s_z s_a) of layer l + 1's dW, [G * 8 + 4 + l] = 1 / s_z (db)
    int tid_tail = tid;       // (made again from a value of its own: the lane number of the head is not kept in a register -- or spilled --
    asm volatile("" : "+v"(tid_tail));                                    //  across the tile loop for the tail)
    const int lane = tid_tail & 63;
    const unsigned G = gridDim.x, wg = blockIdx.x;
    if (wg == 0 && tid < 4) {
        const float iz = sc[H2_FSC_INV + H2C_Z1 - tid];                       // layer tid + 1: dz1 is class 7, dz4 class 4
        wsmax[(long)G * H2_NACT_CLASSES + tid] = iz * sc[H2_FSC_INV + tid];   // its input: x, h1, h2, h3 = classes 0 .. 3
        wsmax[(long)G * H2_NACT_CLASSES + 4 + tid] = iz;
    }
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(ws);
    auto write_slabs = [&](auto gc) {
        constexpr unsigned GC = decltype(gc)::value;
        constexpr unsigned S1 = fs_pad256(FS_STRIDE1), S2 = fs_pad256(FS_STRIDE2), S3 = fs_pad256(FS_STRIDE3);
        const unsigned Gn = GC ? GC : G;
        const unsigned o1 = 0, o2 = Gn * S1, o3 = Gn * (S1 + S2), o4 = Gn * (S1 + S2 + S3);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kt = 0; kt < 3; ++kt) h2_store_tile<GC>(rs, o1, G, wg, MLP_IN_PAD, 2 * wave + t, kt, aW1[t][kt], lane);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int t = 0; t < 2; ++t) h2_store_tile<GC>(rs, o2, G, wg, MLP_H1, nt, 2 * wave + t, aW2[nt][t], lane);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) h2_store_tile<GC>(rs, o3, G, wg, MLP_H2, 2 * (wave >> 1) + a, 2 * (wave & 1) + b, aW3[a][b], lane);
        h2_store_tile<GC>(rs, o4, G, wg, MLP_H3, 0, wave, aW4, lane);
        // bias gradients: lane = column (fs_colsum): db2 of column tile `wave`, db3 of tile wave, db4 (same in every wave); db1 sits in
        // the two lane halves of the swapped-role accumulators
        auto st1 = [&](unsigned lbase, unsigned p, float v) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rs, h2_slab_bytes<GC>(lbase, G, wg, p), 0, 0);
        };
        if (lane < 32) {
            st1(o2, MLP_H2 * MLP_H1 + 32 * wave + lane, bs2);
            st1(o3, MLP_H3 * MLP_H2 + 32 * wave + lane, bs3);
            if (wave == 0) st1(o4, MLP_OUT * MLP_H3 + lane, bs4);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float v = bs1[t] + __shfl_xor(bs1[t], 32, 64);
            if (lane < 32) st1(o1, MLP_H1 * MLP_IN_PAD + 32 * (2 * wave + t) + lane, v);
        }
    };
    if (G == 256u) write_slabs(std::integral_constant<unsigned, 256u>{}); else write_slabs(std::integral_constant<unsigned, 0u>{});
    // this workgroup's class maxima: wave w reduces classes 2 w and 2 w + 1 over the 256 per-thread slots
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = 2 * wave + j;
        const float* a = amax + c * THREADS;
        float m = h2_nanmax(h2_nanmax(a[lane], a[lane + 64]), h2_nanmax(a[lane + 128], a[lane + 192]));     // (a NaN survives)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = h2_nanmax(m, __shfl_xor(m, o, 64));
        if (lane == 0) wsmax[(long)wg * H2_NACT_CLASSES + c] = m;
    }
    if (STAMP) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp<STAMP>(stamps, 1);
        if (threadIdx.x == 0) stamps[2] = realtime_cu();
    }
}

// ---- the slab reduction of the fp16x2 step: mlp_grad_reduce_kernel's sum (chunked slabs, fixed order) + the scale bookkeeping ----------
// Block 0 also: takes the class maxima over the workgroups, writes the NEXT launch's scales into `fsc`, and decides whether THIS launch's
// values fit fp16: no class maximum >= 65504, none NaN (a NaN anywhere in a class reaches its maximum: h2_max3 / h2_nanmax), none
// below H2_CLASS_FLOOR (scales lagging too far above the data).  If not (or while the sticky word *ovf is set: a previous step of this update did not fit, and the optimizer must
// refuse every step from there on so that the host can redo them IN ORDER) the gradient is marked invalid (G[MLP_ERR_SLOT] = 1) and
// the step counter is not advanced.
constexpr int H2_ERR_SLOT = MLP_OFF_W1 + 76;
constexpr int H2_RED_WAVES = 16;
constexpr int H2_RED_BLOCKS = (MLP_PACKED_FLOATS / 4 + 63) / 64;          // 291
#ifndef H2_RED_FLIGHT_N
#define H2_RED_FLIGHT_N 4
#endif
constexpr int H2_RED_FLIGHT = H2_RED_FLIGHT_N;      // float4 loads of one thread in flight (slabs w, w + 16, ...)

__global__ __launch_bounds__(64 * H2_RED_WAVES) void mlp_grad_reduce_h2_kernel(const float* __restrict__ ws, int wgs, float* __restrict__ G,
                                                                               const float* __restrict__ mask, float* __restrict__ norm_ws,
                                                                               int* __restrict__ step, const float* __restrict__ wsmax,
                                                                               float* __restrict__ fsc, int* __restrict__ ovf, int freeze)
{
    __shared__ float4 red[H2_RED_WAVES][64];
    __shared__ int s_bad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    if (blockIdx.x == 0 && wave >= 1 && wave <= H2_NACT_CLASSES) {
        const int c = wave - 1;
        float m = 0.0f;
        bool nan = false;
        for (int w = lane; w < wgs; w += 64) { const float v = wsmax[(long)w * H2_NACT_CLASSES + c]; nan |= !(v == v); m = fmaxf(m, v); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        nan = __any(nan);
        if (lane == 0) {
            const float s_old = fsc[c];
            const bool over = nan || !(m < H2_F16_MAX) || (m > 0.0f && m < H2_CLASS_FLOOR);   // (the floor: fs_h2.inc)
            float s_new = s_old;
            if (nan || !(m < 3.0e38f)) s_new = s_old * 0.00390625f;                     // nothing to go by: back off by 2^-8
            else if (m > 0.0f) s_new = ldexpf(s_old, h2_target_exp(c) - ilogbf(m));     // this launch's maximum -> its class's window
            s_new = fminf(fmaxf(s_new, 0x1p-100f), 0x1p100f);
            if (!freeze) { fsc[c] = s_new; fsc[H2_FSC_INV + c] = 1.0f / s_new; }
            fsc[32 + c] = m;                                                            // (diagnostics: the maximum this launch saw)
            if (over) atomicOr(&s_bad, 1);
        }
    }
    const int q = blockIdx.x * 64 + lane;
    const int o = 4 * q;
    float4 total = make_float4(0.f, 0.f, 0.f, 0.f);
    float unscale = 1.0f;
    if (o < MLP_PACKED_FLOATS) {
        int off_w;
        long lbase;
        const long P1 = fs_pad256(FS_STRIDE1), P2 = fs_pad256(FS_STRIDE2), P3 = fs_pad256(FS_STRIDE3);
        int layer, off_b;
        if (o < MLP_OFF_W2) { layer = 0; off_w = MLP_OFF_W1; off_b = MLP_OFF_B1; lbase = 0; }
        else if (o < MLP_OFF_W3) { layer = 1; off_w = MLP_OFF_W2; off_b = MLP_OFF_B2; lbase = wgs * P1; }
        else if (o < MLP_OFF_W4) { layer = 2; off_w = MLP_OFF_W3; off_b = MLP_OFF_B3; lbase = wgs * (P1 + P2); }
        else { layer = 3; off_w = MLP_OFF_W4; off_b = MLP_OFF_B4; lbase = wgs * (P1 + P2 + P3); }
        // the slabs carry the launch's scale factors: weights s_z s_a, biases s_z (a float4 never straddles the two: offsets are multiples of 4)
        unscale = wsmax[(long)wgs * H2_NACT_CLASSES + (o < off_b ? layer : 4 + layer)];
        const int off = o - off_w;
        const float4* p4 = reinterpret_cast<const float4*>(ws + lbase + ((long)(off >> 8) * wgs) * 256 + (off & 255));
        float4 acc4[H2_RED_FLIGHT];
#pragma unroll
        for (int u = 0; u < H2_RED_FLIGHT; ++u) acc4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int w0 = wave; w0 < wgs; w0 += H2_RED_FLIGHT * H2_RED_WAVES) {
            float4 v[H2_RED_FLIGHT];
#pragma unroll
            for (int u = 0; u < H2_RED_FLIGHT; ++u) {
                const int w = w0 + u * H2_RED_WAVES;
                v[u] = w < wgs ? p4[(long)w * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < H2_RED_FLIGHT; ++u) { acc4[u].x += v[u].x; acc4[u].y += v[u].y; acc4[u].z += v[u].z; acc4[u].w += v[u].w; }
        }
#pragma unroll
        for (int st = H2_RED_FLIGHT / 2; st > 0; st >>= 1)
#pragma unroll
            for (int u = 0; u < st; ++u) { acc4[u].x += acc4[u + st].x; acc4[u].y += acc4[u + st].y; acc4[u].z += acc4[u + st].z; acc4[u].w += acc4[u + st].w; }
        total = acc4[0];
    }
    red[wave][lane] = total;
    __syncthreads();
    if (wave == 0) {
        bool bad = false;
        if (blockIdx.x == 0) {
            bad = s_bad != 0 || *ovf != 0;
            if (s_bad != 0 && lane == 0) *ovf = 1;                                      // sticky until the host clears it
        }
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < MLP_PACKED_FLOATS) {
#pragma unroll
            for (int w = 0; w < H2_RED_WAVES; ++w) { g.x += red[w][lane].x; g.y += red[w][lane].y; g.z += red[w][lane].z; g.w += red[w][lane].w; }
            g.x *= unscale; g.y *= unscale; g.z *= unscale; g.w *= unscale;
            if (o == H2_ERR_SLOT) g.x = bad ? 1.0f : 0.0f;
            *reinterpret_cast<float4*>(G + o) = g;
        }
        if (norm_ws) {
            float ss = 0.0f;
            if (o < MLP_PACKED_FLOATS) {
                const float4 mk = *reinterpret_cast<const float4*>(mask + o);
                const float a = g.x * mk.x, b = g.y * mk.y, c = g.z * mk.z, d = g.w * mk.w;
                ss = (a * a + b * b) + (c * c + d * d);
            }
            for (int off = 32; off > 0; off >>= 1) ss += __shfl_down(ss, off, 64);
            if (lane == 0) {
                norm_ws[1 + blockIdx.x] = ss;
                if (blockIdx.x == 0 && !bad) *step += 1;
            }
        }
    }
}
