// mlp_fused_step.inc — ONE persistent launch per PPO minibatch (ppo.py:184-197): forward, loss, dX chain AND the
// dW / db contribution of every 32-row tile in the workgroup that owns the tile.  bf16x3 arithmetic (mlp_layout.h).
// ---------------------------------------------------------------------------------------------------------------
// Why: the three-launch step (mlp_fwd_bwd_kernel + mlp_grad_w_b3_kernel + reduce) hands ~490 MB of activations and
// dZ through HBM for ~16 MB of true inputs (profiles/r2a_traffic.json).  Here a tile's activations and gradients
// never leave the CU:
//   * grid = one workgroup per CU (4 waves, one per SIMD, up to 512 registers each); workgroup b walks tiles
//     b, b + grid, ... (5 tiles at 40 960 rows on 256 CUs);
//   * every activation / dZ tile lives in LDS ONCE, as three bf16 term planes [32 rows][columns] (row-major): the
//     forward and dX GEMMs read it by rows (ds_read_b128: 8 consecutive k of one row = an MFMA operand fragment), the
//     dW GEMMs -- which reduce over ROWS -- read the very same image through ds_read_b64_tr_b16 (8 consecutive rows
//     of one column).  Rows have power-of-two pitches and the 16-byte slots of a row are XOR-swizzled with a function
//     of the row so that BOTH access patterns are bank-conflict free (fs_key below);
//   * dW is accumulated in registers across the workgroup's tiles: the 76 output tiles (32 x 32) of the four layers
//     are split 19 per wave (304 accumulator registers per lane), dz1 never touches LDS (its GEMM runs with the
//     operand roles swapped, so the accumulator IS the transposed fragment the dW1 MFMA wants);
//   * at the end each workgroup writes ONE partial slab in the layout of the packed gradient (297 KB); the existing
//     fixed-order reduction (mlp_grad_reduce_kernel) sums the `grid` slabs, leaves the clip-norm partials and
//     advances the step.
// HBM traffic per optimizer step: x 12 MB + 4 MB of per-row scalars in, 76 MB of slabs out and 76 MB back in.
// No cross-workgroup communication, so none of the flag / liveness machinery of mlp_fwd_bwd_kernel.
//
// Chain values (h1..h3, out, dz4..dz1) are bit-identical to forward_body<ArithB3> / backward_body<ArithB3> (same operands, same
// MFMA order, same epilogue arithmetic): the DUMP instantiation writes them to HBM in tile-fragment order for the test
// that holds the two paths together.  dW differs from mlp_grad_w_b3 only in summation order (per-CU tile sets
// instead of row slabs).
#include "fs_common.inc"
// LDS regions and who lives in them when (P0 .. P8 = the phases of a tile):
//   X   2 x [32][96] x 3 planes  the tile's input rows (P1 .. P8) and, in the other buffer, the NEXT tile's: converted from the staging block
//                             in the MFMA gaps of this tile's last dW1 product (which reads the current buffer)
//   H1  [32][256]             layer 1's activations (P1 .. P8)
//   H2  [32][128]             layer 2's activations (P2 .. P7); in P8 the raw fp32 rows of the NEXT tile are LDS-DMA'd into it (staging)
//   H3  [32][128]             layer 3's activations (P3 .. P6), overwritten IN PLACE by dZ3 (P6 .. P7): a wave's dZ3 epilogue and its dW4
//                             product touch the same 32 columns, and the product's fragments are read before the first store
//   R   [32][128]-sized       layer 4's split-K partials, fp32 [4][32][32] (P4 .. P5) | dZ4 planes behind them (P5 .. P6) | dZ2 (P7 .. P8)
constexpr int FS_OFF_X = 0;                                              // two buffers: the tile's rows and the next tile's
constexpr int FS_X_HALVES = 3 * BM * FS_PX;
constexpr int FS_OFF_H1 = FS_OFF_X + 2 * FS_X_HALVES;
constexpr int FS_OFF_H2 = FS_OFF_H1 + 3 * BM * FS_P1;
constexpr int FS_OFF_H3 = FS_OFF_H2 + 3 * BM * FS_P2;
constexpr int FS_OFF_R = FS_OFF_H3 + 3 * BM * FS_P2;
constexpr int FS_OFF_Z4 = FS_OFF_R + 4 * BM * MLP_OUT * 2;               // behind the partials (16 KB of 16-bit words)
constexpr int FS_OFF_F32 = FS_OFF_R + 3 * BM * FS_P2;                    // fp32 tail: b1 | b2 | b3 | b4 | rowloss[64] | 1/L[32] | 1/var[32] | half log det
constexpr int FS_TAIL_FLOATS = MLP_H1 + MLP_H2 + MLP_H3 + MLP_OUT + 2 * BM + 2 * MLP_OUT + 4;   // + 1/L | 1/var per column, half log det
constexpr int FS_XS_FLOATS = BM * MLP_IN;                              // raw fp32 rows of the NEXT tile, filled by LDS-DMA (in H2's region)
constexpr int FS_LDS_BYTES = FS_OFF_F32 * 2 + FS_TAIL_FLOATS * 4;        // one workgroup per CU (the 512-register waves allow no second one)
static_assert(FS_OFF_Z4 + 3 * BM * FS_P4 <= FS_OFF_F32, "split-K partials and the dZ4 planes fit region R side by side");
static_assert(FS_XS_FLOATS * 4 <= 3 * BM * FS_P2 * 2, "the staging block fits H2's region");
static_assert(FS_LDS_BYTES <= 160 * 1024, "fits one CU");

// bias + ELU epilogue (lane = row): activation -> the next GEMM's planes; DUMP: also to HBM, tile-fragment order
template <int PITCH, bool DUMP>
__device__ __forceinline__ void fs_epilogue_elu(const f32x16& hi, const f32x16& lo, const float* bias, int col0, u16* plane0,
                                                int lane, float* __restrict__ dump_tile, int nvalid)
{
    const int r = lane & 31;
    float4 y[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int nb = col0 + acc_n(g, lane);
        const float4 bv = *reinterpret_cast<const float4*>(bias + nb);
        y[g].x = elu((hi[4 * g + 0] + lo[4 * g + 0]) + bv.x);
        y[g].y = elu((hi[4 * g + 1] + lo[4 * g + 1]) + bv.y);
        y[g].z = elu((hi[4 * g + 2] + lo[4 * g + 2]) + bv.z);
        y[g].w = elu((hi[4 * g + 3] + lo[4 * g + 3]) + bv.w);
        fs_store4<PITCH>(plane0, r, nb, y[g]);
    }
    if (DUMP && dump_tile != nullptr && r < nvalid) {
        const int go = (col0 / 32) * 1024 + lane * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) GSTORE4(dump_tile + go + g * 256, y[g]);
    }
}

// The dZ epilogue (lane = row): dZ = (hi + lo) * ELU'(H), H recombined from its three term planes, dZ split into its own -- the
// arithmetic and order of backward_body<ArithB3>'s epilogue -- as 4 column groups x 11 slices
template <int PITCH, bool DUMP>
struct FsDactSlices {
    static constexpr int NS = 11;
    const f32x16& hi;
    const f32x16& lo;
    const u16* hplane0;
    u16* zplane0;
    float* dump_tile;
    int col0, lane, r, nvalid;
    uint2 ha[2], hb[2], hd[2];            // H's three term words of a group, requested a group ahead
    float hv[4];
    f32x2 v0, v1;
    float4 z;
    unsigned a0, b0, c0, a1, b1, c1;
    __device__ __forceinline__ FsDactSlices(const f32x16& hi_, const f32x16& lo_, const u16* hp, int col0_, u16* zp, int lane_,
                                            float* dump_tile_, int nvalid_)
        : hi(hi_), lo(lo_), hplane0(hp), zplane0(zp), dump_tile(dump_tile_), col0(col0_), lane(lane_), r(lane_ & 31), nvalid(nvalid_) {}
    __device__ __forceinline__ void request(int g)
    {
        const u16* q = hplane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane));
        ha[g & 1] = *reinterpret_cast<const uint2*>(q);
        hb[g & 1] = *reinterpret_cast<const uint2*>(q + fs_plane<PITCH>());
        hd[g & 1] = *reinterpret_cast<const uint2*>(q + 2 * fs_plane<PITCH>());
    }
    __device__ __forceinline__ void slice(int g, int k)
    {
        const uint2 a = ha[g & 1], b = hb[g & 1], d = hd[g & 1];
        if (k == 0) { hv[0] = fs_lo(a.x) + (fs_lo(b.x) + fs_lo(d.x)); fs_pin(hv[0]); }
        if (k == 1) { hv[1] = fs_hi(a.x) + (fs_hi(b.x) + fs_hi(d.x)); fs_pin(hv[1]); }
        if (k == 2) { hv[2] = fs_lo(a.y) + (fs_lo(b.y) + fs_lo(d.y)); fs_pin(hv[2]); }
        if (k == 3) { hv[3] = fs_hi(a.y) + (fs_hi(b.y) + fs_hi(d.y)); fs_pin(hv[3]); }
        if (k == 4) {
            if (g + 1 < 4) request(g + 1);      // (not pinned: a pin right behind a load is a wait for it)
            z.x = dact(hi[4 * g + 0] + lo[4 * g + 0], hv[0]);
            z.y = dact(hi[4 * g + 1] + lo[4 * g + 1], hv[1]);
            v0[0] = z.x; v0[1] = z.y;
            fs_pin(v0);
        }
        if (k == 5) {
            z.z = dact(hi[4 * g + 2] + lo[4 * g + 2], hv[2]);
            z.w = dact(hi[4 * g + 3] + lo[4 * g + 3], hv[3]);
            v1[0] = z.z; v1[1] = z.w;
            fs_pin(v1);
        }
        if (k == 6) {
            if (DUMP && dump_tile != nullptr && r < nvalid)
                GSTORE4(dump_tile + (col0 / 32) * 1024 + lane * 4 + g * 256, make_float4(v0[0], v0[1], v1[0], v1[1]));
            a0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v0, bf16x2));
            v0[0] -= fs_lo(a0); v0[1] -= fs_hi(a0);
            fs_pin(v0);
        }
        if (k == 7) {
            b0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v0, bf16x2));
            v0[0] -= fs_lo(b0); v0[1] -= fs_hi(b0);
            c0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v0, bf16x2));
            fs_pin(c0);
        }
        if (k == 8) {
            a1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v1, bf16x2));
            v1[0] -= fs_lo(a1); v1[1] -= fs_hi(a1);
            fs_pin(v1);
        }
        if (k == 9) {
            b1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v1, bf16x2));
            v1[0] -= fs_lo(b1); v1[1] -= fs_hi(b1);
            c1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v1, bf16x2));
            fs_pin(c1);
        }
        if (k == 10) {
            u16* q = zplane0 + fs_off<PITCH>(r, col0 + acc_n(g, lane));
            *reinterpret_cast<uint2*>(q) = make_uint2(a0, a1);
            *reinterpret_cast<uint2*>(q + fs_plane<PITCH>()) = make_uint2(b0, b1);
            *reinterpret_cast<uint2*>(q + 2 * fs_plane<PITCH>()) = make_uint2(c0, c1);
        }
    }
};
// dZ1 from the swapped-role dA1 GEMM (lane = column n, register reg = row acc_row(reg, lane)), as OPS of two interleaved chains
// (fs_common.inc) for the 48 MFMA gaps of the same column tile's dW2 product: register pair (8 s + 2 m, + 1) and word m of H1's
// three term fragments of k-step s -> word m of the three dZ1^T fragments of k-step s, which dW1 multiplies by as they are.  The
// operations on every value and their order are those of the slices this replaces (H = a + (b + d); dact; the pair's db1 term
// vs = v0 + v1 added to ONE running sum in pair order; split3x2), so every bit stays; what changes is that consecutive
// instructions belong to different pairs: the slices were one dependent chain per gap and cost 68 cycles per hosting MFMA
// against 34 without a guest.
typedef unsigned fs_u32x4 __attribute__((ext_vector_type(4)));
struct FsDz1Ex { float ha, hb, w0, w1, vs; };
template <bool DUMP>
struct FsDz1Ops {
    static constexpr int CH = 18 + FS_SPLIT_OPS, TOTAL = 8 * CH;             // 29 ops per pair, 232 per column tile
    const f32x16 &hi, &lo;
    const fs_u32x4 (&hw)[2][3];         // H1's term fragments [k-step][term], as words
    unsigned (&zq)[2][3][4];            // out: the dZ1^T fragments being built [k-step][term][word]
    float* dt;                          // DUMP: this column tile's block of the dZ1 dump
    int lane, nvalid;
    float zsum;
    FsChain k[2];
    FsDz1Ex x[2];
    __device__ __forceinline__ FsDz1Ops(const f32x16& hi_, const f32x16& lo_, const fs_u32x4 (&hw_)[2][3], unsigned (&q_)[2][3][4],
                                        float* dt_, int lane_, int nvalid_)
        : hi(hi_), lo(lo_), hw(hw_), zq(q_), dt(dt_), lane(lane_), nvalid(nvalid_), zsum(0.0f) {}
    // op i of pair c (= 4 s + m) in state slot sl
    __device__ __forceinline__ void chain_op(int c, int sl, int i)
    {
        const int s = c >> 2, m = c & 3, reg = 8 * s + 2 * m;
        FsChain& ch = k[sl];
        FsDz1Ex& e = x[sl];
        const unsigned u0 = hw[s][0][m], u1 = hw[s][1][m], u2 = hw[s][2][m];
        if (i == 0) { e.w0 = fs_lo(u1); fs_pin(e.w0); }
        if (i == 1) { e.w1 = fs_lo(u2); fs_pin(e.w1); }
        if (i == 2) { e.w0 += e.w1; fs_pin(e.w0); }
        if (i == 3) { e.ha = fs_lo(u0); fs_pin(e.ha); }
        if (i == 4) { e.ha += e.w0; fs_pin(e.ha); }
        if (i == 5) { e.w0 = fs_hi(u1); fs_pin(e.w0); }
        if (i == 6) { e.w1 = fs_hi(u2); fs_pin(e.w1); }
        if (i == 7) { e.w0 += e.w1; fs_pin(e.w0); }
        if (i == 8) { e.hb = fs_hi(u0); fs_pin(e.hb); }
        if (i == 9) { e.hb += e.w0; fs_pin(e.hb); }
        if (i == 10) { ch.t0 = hi[reg] + lo[reg]; fs_pin(ch.t0); }
        if (i == 11) { ch.t1 = hi[reg + 1] + lo[reg + 1]; fs_pin(ch.t1); }
        if (i == 12) { e.ha = fminf(e.ha, 0.0f); fs_pin(e.ha); }
        if (i == 13) { e.hb = fminf(e.hb, 0.0f); fs_pin(e.hb); }
        if (i == 14) { ch.t0 = fmaf(ch.t0, e.ha, ch.t0); fs_pin(ch.t0); }            // dact
        if (i == 15) {
            ch.t1 = fmaf(ch.t1, e.hb, ch.t1); fs_pin(ch.t1);
            if (DUMP) {
                const int ra = acc_row(reg, lane), rb = acc_row(reg + 1, lane);
                if (ra < nvalid) dt[frag_off(ra, lane & 31)] = ch.t0;
                if (rb < nvalid) dt[frag_off(rb, lane & 31)] = ch.t1;
            }
        }
        if (i == 16) { e.vs = ch.t0 + ch.t1; fs_pin(e.vs); }
        if (i >= 17 && i < 17 + FS_SPLIT_OPS) {
            const int j = i - 17;
            fs_split_op(ch, j);
            if (j == 0) zq[s][0][m] = ch.a;
            if (j == 5) zq[s][1][m] = ch.b;
            if (j == 10) zq[s][2][m] = ch.c;
        }
        // db1's running sum: the pair sum formed beside the split, added in the lightest MFMA gap (A/B: in the dact gap; not kept)
        if (i == 17 + FS_SPLIT_OPS) { zsum += e.vs; fs_pin(zsum); }
    }
    // pairs 2 pp, 2 pp + 1 interleaved: ops 2 CH pp .. 2 CH (pp + 1) - 1
    __device__ __forceinline__ void q(int t) { const int pp = t / (2 * CH), o = t % (2 * CH); chain_op(2 * pp + (o & 1), o & 1, o >> 1); }
};

// Where element p of a layer's packed-gradient block lives in the partial slabs: the slabs of the `G` workgroups are interleaved in
// 1 KiB chunks -- [chunk p >> 8][workgroup][256 floats] -- so that the reduction, whose waves each sum ONE output position over all
// workgroups, reads a contiguous run of G KiB instead of G pieces a slab apart (strides of 66 .. 132 KB: a fixed residue of the
// channel interleave); the burst that writes the slabs is 128-byte pieces either way.
constexpr long fs_pad256(long n) { return (n + 255) / 256 * 256; }
// float index of element p of a layer's block, relative to `ws`: 32-bit arithmetic throughout (all the slabs together are < 2^30
// floats), so that a store is a scalar base + a 32-bit lane offset; `lbase` = where the layer's slab region starts
__device__ __forceinline__ unsigned fs_slab(unsigned lbase, unsigned G, unsigned wg, unsigned p)
{
    return lbase + (((p >> 8) * G + wg) << 8) + (p & 255u);
}
// partial slab: tile (nt, kt) of a layer's [N][KOUT] block; lane = column k, registers = rows n
__device__ __forceinline__ void fs_store_tile(float* __restrict__ ws, unsigned lbase, unsigned G, unsigned wg, int KOUT,
                                              int nt, int kt, const f32x16& acc, int lane)
{
    const int col = kt * 32 + (lane & 31);
    if (col < KOUT) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) ws[fs_slab(lbase, G, wg, (unsigned)((nt * 32 + acc_row(reg, lane)) * KOUT + col))] = acc[reg];
    }
}

constexpr int FS_STAMP_SLOTS = 32;       // u64 per (workgroup, tile) record of the STAMP instantiation (tools/stamp_fused.py)
struct FusedDump { float *out, *h1, *h2, *h3, *dz4, *dz3, *dz2, *dz1; };   // DUMP instantiation only (tests)

constexpr long FS_STRIDE1 = (long)MLP_H1 * MLP_IN_PAD + MLP_H1, FS_STRIDE2 = (long)MLP_H2 * MLP_H1 + MLP_H2,
               FS_STRIDE3 = (long)MLP_H3 * MLP_H2 + MLP_H3, FS_STRIDE4 = (long)MLP_OUT * MLP_H3 + MLP_OUT;
static_assert(FS_STRIDE1 + FS_STRIDE2 + FS_STRIDE3 + FS_STRIDE4 == MLP_PACKED_FLOATS, "a slab is one packed gradient");

// MODE 0: the product; 1: DUMP (tests: chain values to HBM); 2: STAMP (tools/stamp_fused.py: wave 0 of every workgroup stores
// s_memtime at the phase boundaries of every tile into dump.out, viewed as u64 [workgroup][tile slot][16])
template <int MODE>
__global__ __launch_bounds__(THREADS, 1) void mlp_fused_step_kernel(
    const float* __restrict__ P, const u16* __restrict__ PB, const u16* __restrict__ PTB, const float* __restrict__ x, long n,
    const float* __restrict__ action, const float* __restrict__ old_logp, const float* __restrict__ adv,
    const float* __restrict__ target, const float* __restrict__ var, float inv_batch, float clip, float* __restrict__ ws,
    float* __restrict__ loss_part, FusedDump dump)
{
    constexpr bool DUMP = MODE == 1, STAMP = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char fs_lds_raw[];
    u16* lds = reinterpret_cast<u16*>(fs_lds_raw);
    unsigned long long* stamps = nullptr;
    int tslot = 0;
    (void)stamps; (void)tslot;
    if (STAMP) {        // record 62: kernel entry (shader clock, 100 MHz real time + CU identity), loop entry
        stamps = reinterpret_cast<unsigned long long*>(dump.out) + ((long)blockIdx.x * 64 + 62) * FS_STAMP_SLOTS;
        stamp<STAMP>(stamps, 0);
        if (!STAMP) fs_split(n);
        if (threadIdx.x == 0) stamps[1] = realtime_cu();
    }
    u16* X = lds + FS_OFF_X;
    u16* H1 = lds + FS_OFF_H1;
    u16* H2 = lds + FS_OFF_H2;
    u16* H3 = lds + FS_OFF_H3;
    u16* Z3 = H3;                                                 // dZ3 overwrites H3 in place (see the region table)
    u16* Z2 = lds + FS_OFF_R;
    float* part = reinterpret_cast<float*>(lds + FS_OFF_R);       // layer-4 split-K partials [wave][32][32]
    u16* Z4 = lds + FS_OFF_Z4;
    float* tail = reinterpret_cast<float*>(lds + FS_OFF_F32);
    float* bias1 = tail, *bias2 = tail + MLP_H1, *bias3 = bias2 + MLP_H2, *bias4 = bias3 + MLP_H3, *rowloss = bias4 + MLP_OUT;
    float* c_invL = rowloss + 2 * BM, *c_invVar = c_invL + MLP_OUT, *c_hld = c_invVar + MLP_OUT;   // loss-phase constants per column
    float* xs = reinterpret_cast<float*>(H2);                     // [32][73] fp32: the next tile's rows as they lie in HBM (H2 is dead in P8 / P0)

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long ntiles = (n + BM - 1) / BM;
    const long total = n * MLP_IN;

    // dW accumulators of this wave (persist over the workgroup's tiles) and running bias-gradient sums
    // REGISTER PLACEMENT.  hipcc emits the AGPR form of every MFMA in a kernel that may use more than 256 registers: accumulators
    // must sit in the 256 AGPRs while they are multiplied into.  19 tiles (304) + the chain GEMMs' hi / lo (32) do not fit, and
    // left to itself the allocator spills whole accumulator tiles to scratch around every GEMM (measured: ~20k cycles per tile).
    // So the chain GEMMs and FS_VTILES of the dW tiles (dW4 and part of dW3: their operands come straight from LDS) use the VGPR
    // form of the MFMA through inline asm (fs_mfma_v); the other 16 tiles fill the AGPRs exactly.
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
    float bs1[2] = {0.0f, 0.0f}, bs2 = 0.0f, bs3 = 0.0f, bs4 = 0.0f;    // running bias gradients (lane = column, see fs_colsum)

    // The next tile's input rows travel HBM -> LDS by LDS-DMA (no registers: the accumulators own the register file; holding the
    // twelve registers of a register prefetch through P8 was measured: 8 spills, +1.6k cycles per tile) into a raw fp32 staging
    // block; a tile is one contiguous, 16-byte aligned block of 32 * 73 floats = 584 16-byte pieces, and WAVE w fetches the 146
    // pieces of rows 8 w .. 8 w + 7 -- the rows its own threads convert (FsXStoreSlices), so no barrier stands between the two.
    // The ragged last tile of a batch (at most one per launch) goes through guarded loads instead.
    // The DMA is issued as inline asm: the compiler cannot tell that the staging block is disjoint from the planes the phase goes
    // on reading, and puts s_waitcnt vmcnt(0) -- the whole HBM round trip -- in front of the next LDS read behind a DMA it knows
    // of.  The wait that matters is explicit instead: fs_dma_drain() ahead of the conversion.
    typedef __attribute__((address_space(3))) void* lptr_t;
    const unsigned xs_lds = (unsigned)(unsigned long)(lptr_t)xs;               // LDS byte address of the staging block
    constexpr int XW = BM * MLP_IN / 4 / NWAVE;                                // 16-byte pieces per wave: 146
    static_assert(XW * NWAVE * 4 == BM * MLP_IN && XW > 128 && XW <= 192, "x_fetch: three DMA instructions per wave, the third partial");
    // LDS-DMA moves 16-byte pieces: `x` must be 16-byte aligned for it (a minibatch slice of the rollout ring starts k * n * 73
    // floats in: only 4-byte aligned for odd k * n).  Otherwise every tile takes the guarded 4-byte loads (wave-uniform).
    const bool x_al16 = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    auto x_fetch = [&](long tile, int tl) {      // `tl`: the thread index, opaque per tile (address arithmetic stays in place: hoisted
        const long base = tile * (BM * MLP_IN);  // out of the tile loop it lives in registers that get spilled and reloaded)
        const int w = __builtin_amdgcn_readfirstlane(tl >> 6), l = tl & 63;
        if (x_al16 && base + BM * MLP_IN <= total) {
            const float* src = x + base + 4L * (XW * w + l);
            // LDS destination of a piece = wave-uniform base (M0) + lane * 16; M0 is reserved to the compiler: saved and put back
            const unsigned dst = xs_lds + 16u * (unsigned)(XW * w);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                         "s_add_u32 m0, %1, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "s"(dst), "v"(src), "v"(src + 4 * 64) : "memory", "scc");
            if (l + 128 < XW)
                asm volatile("s_mov_b32 %0, m0\n\ts_add_u32 m0, %1, 0x800\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "s"(dst), "v"(src + 8 * 64) : "memory", "scc");
        } else {
            for (int i = l; i < 4 * XW; i += 64) xs[4 * XW * w + i] = base + 4 * XW * w + i < total ? x[base + 4 * XW * w + i] : 0.0f;
        }
    };

    long tile = blockIdx.x;
    if (tile < ntiles) x_fetch(tile, tid);
    if (tid < 32) {     // loss-phase constants per output column (ppo.py:185-189), the same for every tile
        const bool act = tid < MLP_NACT;
        const float L = act ? sqrtf(var[tid]) : 1.0f;
        c_invL[tid] = act ? 1.0f / L : 0.0f;
        c_invVar[tid] = act ? 1.0f / var[tid] : 0.0f;
        float hld = act ? logf(L) : 0.0f;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) hld += __shfl_xor(hld, o, 32);
        if (tid == 0) c_hld[0] = hld;
    }
    bias1[tid] = P[MLP_OFF_B1 + tid];
    if (tid < MLP_H2) bias2[tid] = P[MLP_OFF_B2 + tid];
    else bias3[tid - MLP_H2] = P[MLP_OFF_B3 + tid - MLP_H2];
    if (tid < MLP_OUT) bias4[tid] = P[MLP_OFF_B4 + tid];
    if (!STAMP) {
        // the 304 accumulator registers are cleared HERE, while the first tile's rows and the biases are in flight: left alone the
        // compiler sinks the clears behind the barrier, to the first use (~2k cycles of nothing but register writes per launch).
        // (Not in the diagnostic build: its stamp registers make the pins spill.)
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
    fs_dma_drain();
    if (tile < ntiles) { FsXStoreSlices xc0(xs, X, tid); xc0.all(); }   // the workgroup's first tile: converted at once
    __syncthreads();
    int par = 0;                                                         // which X buffer holds the current tile

    if (STAMP) stamp<STAMP>(reinterpret_cast<unsigned long long*>(dump.out) + ((long)blockIdx.x * 64 + 62) * FS_STAMP_SLOTS, 2);
    // the grid size, parked in a vector register: left to itself the compiler re-reads it from the dispatch packet (a scalar
    // memory round trip, ~200 cycles with nothing to hide behind) at each use inside the tile loop
    int grid_v = gridDim.x;
    asm volatile("" : "+v"(grid_v));
    for (; tile < ntiles; tile += __builtin_amdgcn_readfirstlane(grid_v), par ^= 1) {
        u16* Xc = X + par * FS_X_HALVES;
        u16* Xn = X + (par ^ 1) * FS_X_HALVES;
        const long row0 = tile * BM;
        const int nvalid = (int)(n - row0 < BM ? n - row0 : BM);
        // opaque per-iteration copy of the thread index: keeps tile-invariant address arithmetic from being hoisted out of the
        // tile loop (it would all be live across it, on top of the 304 accumulator registers)
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
        // (P0, the conversion of the tile's rows into the X planes, happened in the previous tile's last phase)
        WeightHead3 w1;
        gemm_prefetch_b3<MLP_IN_PAD>(w1, PB + MLP_OFF_PB1, 2 * wave, lane);
        stamp<STAMP>(stamps, 1);
        if (!STAMP) fs_split(n);

        // ---- P1: layer 1, this wave's 64 columns -------------------------------------------------------------------
        WeightHead3 w4, wt4;
        {
            f32x16 hi, lo;
            WeightHead3 w1b, w2a;
            fs_gemm<MLP_IN_PAD, FS_PX, false>(w1, PB + MLP_OFF_PB1, 2 * wave, Xc, 0, hi, lo, lane);
            gemm_prefetch_b3<MLP_IN_PAD>(w1b, PB + MLP_OFF_PB1, 2 * wave + 1, lane);
            fs_epilogue_elu<FS_P1, DUMP>(hi, lo, bias1, 64 * wave, H1, lane, d_h1, nvalid);
            fs_gemm<MLP_IN_PAD, FS_PX, false>(w1b, PB + MLP_OFF_PB1, 2 * wave + 1, Xc, 0, hi, lo, lane);
            gemm_prefetch_b3<MLP_H2>(w2a, PB + MLP_OFF_PB2, wave, lane);
            fs_epilogue_elu<FS_P1, DUMP>(hi, lo, bias1, 64 * wave + 32, H1, lane, d_h1, nvalid);
            stamp<STAMP>(stamps, 2);
            if (!STAMP) fs_split(n);
            __syncthreads();
            stamp<STAMP>(stamps, 3);
            if (!STAMP) fs_split(n);
            // ---- P2: layer 2 (K = 256 as the two K = 128 operands of mlp_layout.h) ----------------------------------
            WeightHead3 w2b, w3;
            gemm_prefetch_b3<MLP_H2>(w2b, PB + MLP_OFF_PB2 + 3 * MLP_H2 * (MLP_H1 / 2), wave, lane);   // the second half's first weights: a GEMM ahead
            fs_gemm<MLP_H2, FS_P1, false>(w2a, PB + MLP_OFF_PB2, wave, H1, 0, hi, lo, lane);
            fs_gemm<MLP_H2, FS_P1, false, false>(w2b, PB + MLP_OFF_PB2 + 3 * MLP_H2 * (MLP_H1 / 2), wave, H1, MLP_H1 / 2, hi, lo, lane);
            gemm_prefetch_b3<MLP_H2>(w3, PB + MLP_OFF_PB3, wave, lane);
            fs_epilogue_elu<FS_P2, DUMP>(hi, lo, bias2, 32 * wave, H2, lane, d_h2, nvalid);
            __syncthreads();
            stamp<STAMP>(stamps, 4);
            if (!STAMP) fs_split(n);
            // ---- P3: layer 3 (actor | critic heads stacked) ----------------------------------------------------------
            gemm_prefetch_b3<32>(w4, PB + MLP_OFF_PB4 + (long)(2 * wave) * 1536, 0, lane);     // layer 4's weights: a phase ahead
            fs_gemm<MLP_H2, FS_P2, false>(w3, PB + MLP_OFF_PB3, wave, H2, 0, hi, lo, lane);
            fs_epilogue_elu<FS_P2, DUMP>(hi, lo, bias3, 32 * wave, H3, lane, d_h3, nvalid);
            __syncthreads();
            stamp<STAMP>(stamps, 5);
            if (!STAMP) fs_split(n);
        }
        // ---- P4: layer 4, split-K over the four waves (32 k each), partials to LDS ---------------------------------------
        // the loss phase's per-row inputs (stored action, old log-prob, advantage, target: ppo.py:183) are requested one phase ahead:
        // one wave per SIMD has nobody to hide four dependent HBM round trips behind when the phase comes
        const int lrow = tl >> 3, lq = tl & 7;                      // loss phase: eight lanes per row, four output columns each
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
            gemm_prefetch_b3<MLP_OUT>(wt4, PTB + MLP_OFF_PTB4, wave, lane);            // dA3's weights: a phase ahead
            f32x16 hi, lo;
            fs_gemm<32, FS_P2, false>(w4, PB + MLP_OFF_PB4 + (long)(2 * wave) * 1536, 0, H3, 32 * wave, hi, lo, lane);
            // [row][32], the row's eight 16-byte chunks rotated by (row >> 1) & 7: 32 lanes writing one chunk column of 32 rows
            // (pitch 128 bytes) would otherwise meet in 8 of the 64 banks
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
        // ---- P5: outputs, loss, dZ4 (ppo.py:184-194): eight lanes per row, four output columns each; the row reductions are
        //          8-lane DPP butterflies (no LDS round trips), the dZ4 planes are written as 8-byte granules ------------------
        {
            const int c0 = 4 * lq;
            const int cs = 4 * (lq ^ ((lrow >> 1) & 7));                  // where P4 put this chunk
            const float4 p0 = *reinterpret_cast<const float4*>(part + lrow * MLP_OUT + cs);
            const float4 p1 = *reinterpret_cast<const float4*>(part + BM * MLP_OUT + lrow * MLP_OUT + cs);
            const float4 p2 = *reinterpret_cast<const float4*>(part + 2 * BM * MLP_OUT + lrow * MLP_OUT + cs);
            const float4 p3 = *reinterpret_cast<const float4*>(part + 3 * BM * MLP_OUT + lrow * MLP_OUT + cs);
            const float4 b4v = *reinterpret_cast<const float4*>(bias4 + c0);
            const float4 iL = *reinterpret_cast<const float4*>(c_invL + c0);
            const float4 iV = *reinterpret_cast<const float4*>(c_invVar + c0);
            const float half_log_det = c_hld[0];
            const float zz[4] = {(((p0.x + p1.x) + p2.x) + p3.x) + b4v.x, (((p0.y + p1.y) + p2.y) + p3.y) + b4v.y,
                                 (((p0.z + p1.z) + p2.z) + p3.z) + b4v.z, (((p0.w + p1.w) + p2.w) + p3.w) + b4v.w};
            const float invL[4] = {iL.x, iL.y, iL.z, iL.w}, invV[4] = {iV.x, iV.y, iV.z, iV.w};
            float y[4], xsq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = c0 + j;
                const float yv = col < MLP_NACT ? elu(zz[j]) : ((col == MLP_NACT) ? zz[j] : 0.0f);   // ELU on the mean (ppo.py:30), none on v
                if (DUMP && lin) (dump.out + row0 * MLP_OUT)[frag_off(lrow, col)] = yv;
                y[j] = lin ? yv : 0.0f;
                const float xj = col < MLP_NACT ? (l_a[j] - y[j]) * invL[j] : 0.0f;
                xsq[j] = xj * xj;
            }
            const float M = fs_sum8((xsq[0] + xsq[1]) + (xsq[2] + xsq[3]));
            const float vrow = fs_sum8(lq == MLP_NACT / 4 ? y[MLP_NACT % 4] : 0.0f);        // the row's value output (column 18), to all 8 lanes
            float d[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pol = 0.0f, hub = 0.0f;
            if (lin) {
                const PpoRowLoss rl = ppo_row_loss<false>(M, half_log_det, l_olp, l_adv, vrow, l_tgt, inv_batch, clip);
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
            fs_store4<FS_P4>(Z4, lrow, c0, make_float4(d[0], d[1], d[2], d[3]));
            if (lq == 0) { rowloss[2 * lrow] = pol; rowloss[2 * lrow + 1] = hub; }
        }
        __syncthreads();
        stamp<STAMP>(stamps, 7);
        if (!STAMP) fs_split(n);
        // lane offsets of the transposing reads (per row pitch): computed here, once per tile, live through P6 .. P8 only
        FsTr tr1, tr2, trx, tr4;
        fs_tr_init<FS_P1>(tr1, lane);
        fs_tr_init<FS_P2>(tr2, lane);
        fs_tr_init<FS_PX>(trx, lane);
        fs_tr_init<FS_P4>(tr4, lane);
        // ---- P6: dA3 = dZ4 . W4 -> dZ3;  dW4 += dZ4^T H3 ---------------------------------------------------------------
        if (tl < 32 && loss_part) tile_loss_sum<2>(rowloss, tl, loss_part + 2 * tile);
        WeightHead3 wt2;
        {
            f32x16 hi, lo;
            WeightHead3 wt3;
            fs_gemm<MLP_OUT, FS_P4, false>(wt4, PTB + MLP_OFF_PTB4, wave, Z4, 0, hi, lo, lane);
            gemm_prefetch_b3<MLP_H3>(wt3, PTB + MLP_OFF_PTB3, wave, lane);
            {   // dW4 and db4 (18 MFMAs) with the dZ3 epilogue in their gaps
                f32x16 cs;
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 o = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};      // eight bf16 1.0 (fs_colsum_step)
                const bf16x8 ones = __builtin_bit_cast(bf16x8, o);
                FsDactSlices<FS_P2, DUMP> ep3(hi, lo, H3, 32 * wave, Z3, lane, DUMP ? dump.dz3 + row0 * MLP_H3 : nullptr, nvalid);
                ep3.request(0);
                // dZ3 overwrites H3 in place, column group by column group: both k-steps' H3 fragments of this wave's columns are
                // read (and pinned: they must have LANDED) before the first slice stores
                bf16x8 af3[2][3];
                fs_trws<FS_P2>(af3[0], H3, tr2, wave, 0);
                fs_trws<FS_P2>(af3[1], H3, tr2, wave, 1);
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) asm volatile("" : "+v"(af3[q][pl]));
#define FS_P6_HALF(S_)                                                                                                            \
                {                                                                                                                 \
                    bf16x8 zf[3];                                                                                                 \
                    const bf16x8 (&af)[3] = af3[S_];                                                                              \
                    fs_trns<FS_P4>(zf, Z4, tr4, 0, S_);                                                                           \
                    fs_mfma_vg(aW4, zf[0], af[2]); fs_gap_spread<18, 9 * S_ + 0>(ep3);                                            \
                    fs_mfma_vg(aW4, zf[2], af[0]); fs_gap_spread<18, 9 * S_ + 1>(ep3);                                            \
                    fs_mfma_vg(aW4, zf[1], af[1]); fs_gap_spread<18, 9 * S_ + 2>(ep3);                                            \
                    fs_mfma_vg(aW4, zf[0], af[1]); fs_gap_spread<18, 9 * S_ + 3>(ep3);                                            \
                    fs_mfma_vg(aW4, zf[1], af[0]); fs_gap_spread<18, 9 * S_ + 4>(ep3);                                            \
                    fs_mfma_vg(aW4, zf[0], af[0]); fs_gap_spread<18, 9 * S_ + 5>(ep3);                                            \
                    if (S_ == 0) fs_mfma_vg0(cs, ones, zf[2]); else fs_mfma_vg(cs, ones, zf[2]);    /* db4 (every wave) */         \
                    fs_gap_spread<18, 9 * S_ + 6>(ep3);                                                                           \
                    fs_mfma_vg(cs, ones, zf[1]); fs_gap_spread<18, 9 * S_ + 7>(ep3);                                              \
                    fs_mfma_vg(cs, ones, zf[0]); fs_gap_spread<18, 9 * S_ + 8>(ep3);                                              \
                    fs_mfma_settle(aW4, cs);                                                                                      \
                    __builtin_amdgcn_sched_barrier(0);                                                                            \
                }
                FS_P6_HALF(0)
                FS_P6_HALF(1)
#undef FS_P6_HALF
                bs4 += fs_colsum_done(cs);
            }
            __syncthreads();
            stamp<STAMP>(stamps, 8);
            if (!STAMP) fs_split(n);
            // ---- P7: dA2 = dZ3 . W3 -> dZ2 (over H3);  dW3 += dZ3^T H2 --------------------------------------------------
            fs_gemm<MLP_H3, FS_P2, false>(wt3, PTB + MLP_OFF_PTB3, wave, Z3, 0, hi, lo, lane);
            gemm_prefetch_b3<MLP_H2>(wt2, PTB + MLP_OFF_PTB2, 2 * wave, lane);       // dA1's first weights: land during dW3 + the epilogue
            {
                const int nt0 = 2 * (wave >> 1), kt0 = 2 * (wave & 1);
                f32x16 cs;
                FsDactSlices<FS_P2, DUMP> ep2(hi, lo, H2, 32 * wave, Z2, lane, DUMP ? dump.dz2 + row0 * MLP_H2 : nullptr, nvalid);
                ep2.request(0);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bf16x8 zf[2][3], af[2][3];
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        fs_trws<FS_P2>(zf[a], Z3, tr2, nt0 + a, s);
                        fs_trws<FS_P2>(af[a], H2, tr2, kt0 + a, s);
                    }
#pragma unroll
                    for (int b = 0; b < 2; ++b) {                          // group 2 s + b of the dZ2 epilogue rides in the gaps
                        fs_dw_v_fill(aW3[0][b], zf[0], af[b], ep2, 2 * s + b, 0);      // VGPR-resident tiles
                        fs_dw_fill(aW3[1][b], zf[1], af[b], ep2, 2 * s + b, 6);
                    }
                    // db3 of column tile nt0 + (wave & 1): the four waves cover the four tiles
                    if (wave & 1) { if (s == 0) fs_colsum_step<true>(cs, zf[1]); else fs_colsum_step<false>(cs, zf[1]); }
                    else { if (s == 0) fs_colsum_step<true>(cs, zf[0]); else fs_colsum_step<false>(cs, zf[0]); }
                    __builtin_amdgcn_sched_barrier(0);
                }
                bs3 += fs_colsum_done(cs);
            }
        }
        __syncthreads();
        stamp<STAMP>(stamps, 9);
        if (!STAMP) fs_split(n);
        // ---- P8: dA1 = dZ2 . W2 with the operand roles SWAPPED -> dZ1 as transposed fragments in registers;
        //          dW2 += dZ2^T H1 and dW1 += dZ1^T X for this wave's two column tiles of H1 / dZ1 ---------------------------
        {
            // Per column tile ct = 2 wave + t of layer 1:  dA1 GEMM (swapped roles: the accumulator holds dA1^T fragments)  ->
            // dW2[.][ct] (48 MFMAs: four n' tiles x two k-steps) WITH the dZ1 epilogue of the tile in its gaps  ->  dW1[ct][.].
            // The epilogue is pure vector work (recombine H1, ELU', split into three terms: ~27 instructions per value pair) and one
            // wave per SIMD has nobody else to run under it: cut into six slices per pair, one slice goes behind each MFMA of the
            // independent dW2 product, where the matrix pipe's 32 cycles cover it.  The H1 fragments dW2 multiplies by ARE the ones
            // the epilogue recombines (same column tile, same k-steps), so they are read once.
            WeightHead3 wt2b;
            f32x16 cs2;
            const bool more = tile + __builtin_amdgcn_readfirstlane(grid_v) < ntiles;      // this workgroup has another tile
            FsXStoreSlices xc(xs, Xn, tl);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ct = 2 * wave + t;                               // column tile of layer 1 (n of dW1, k of dW2)
                bf16x8 z1f[2][3];
                {
                    f32x16 hi, lo;
                    if (t == 0) fs_gemm<MLP_H2, FS_P2, true>(wt2, PTB + MLP_OFF_PTB2, ct, Z2, 0, hi, lo, lane);
                    else fs_gemm<MLP_H2, FS_P2, true>(wt2b, PTB + MLP_OFF_PTB2, ct, Z2, 0, hi, lo, lane);
                    // the next tile's rows, requested HERE: behind the GEMM whose weight ring counts its own loads (older DMAs in
                    // flight would hold every ring wait for the HBM round trip) and ahead of 84 MFMAs that load nothing; drained
                    // by fs_dma_drain() at the end of the phase
                    if (t == 0) { stamp<STAMP>(stamps, 12); if (!STAMP) fs_split(n); }
                    if (STAMP && t == 1) stamp<STAMP>(stamps, 16);
                    if (t == 0 && more) x_fetch(tile + __builtin_amdgcn_readfirstlane(grid_v), tl);
                    bf16x8 hf[2][3], zf[2][3];
#pragma unroll
                    for (int s = 0; s < 2; ++s) fs_trws<FS_P1>(hf[s], H1, tr1, ct, s);
                    fs_trws<FS_P2>(zf[0], Z2, tr2, 0, 0);
                    unsigned q[2][3][4];                                   // the dZ1 fragments being built: [k-step][term][word]
                    const fs_u32x4 hw[2][3] = {{__builtin_bit_cast(fs_u32x4, hf[0][0]), __builtin_bit_cast(fs_u32x4, hf[0][1]),
                                                __builtin_bit_cast(fs_u32x4, hf[0][2])},
                                               {__builtin_bit_cast(fs_u32x4, hf[1][0]), __builtin_bit_cast(fs_u32x4, hf[1][1]),
                                                __builtin_bit_cast(fs_u32x4, hf[1][2])}};
                    FsDz1Ops<DUMP> ez(hi, lo, hw, q, DUMP ? dump.dz1 + row0 * MLP_H1 + ct * 1024 : nullptr, lane, nvalid);
                    // c = 4 s + nt: dW2[n' tile nt][k tile ct], k-step s; the dZ1 epilogue's ops ride in the 48 gaps (pairs c, c + 1 of
                    // accumulator registers interleaved over the twelve gaps of dW2 steps c, c + 1)
#define FS_P8_STEP(C_)                                                                                                            \
                    {                                                                                                             \
                        constexpr int c = (C_), s = c >> 2, nt = c & 3;                                                           \
                        if (c + 1 < 8) fs_trws<FS_P2>(zf[(c + 1) & 1], Z2, tr2, (c + 1) & 3, (c + 1) >> 2);                        \
                        __builtin_amdgcn_sched_barrier(0);                                                                        \
                        fs_dw_host<6 * c, 48>(aW2[nt][t], zf[c & 1], hf[s], ez);                                                  \
                        if (STAMP && t == 0 && c == 3) stamp<STAMP>(stamps, 18);                                                  \
                        if (t == 0 && nt == wave) {                        /* db2 of column tile `wave` (wave-uniform branch) */   \
                            if (s == 0) fs_colsum_step<true>(cs2, zf[c & 1]); else fs_colsum_step<false>(cs2, zf[c & 1]);         \
                        }                                                                                                         \
                        __builtin_amdgcn_sched_barrier(0);                                                                        \
                    }
                    FS_P8_STEP(0) FS_P8_STEP(1) FS_P8_STEP(2) FS_P8_STEP(3) FS_P8_STEP(4) FS_P8_STEP(5) FS_P8_STEP(6) FS_P8_STEP(7)
#undef FS_P8_STEP
                    if (STAMP && t == 0) stamp<STAMP>(stamps, 17);
                    bs1[t] += ez.zsum;
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int p = 0; p < 3; ++p) {
                            const fs_u32x4 qq = {q[s][p][0], q[s][p][1], q[s][p][2], q[s][p][3]};
                            z1f[s][p] = __builtin_bit_cast(bf16x8, qq);
                        }
                }
                if (t == 0) {
                    bs2 += fs_colsum_done(cs2);
                    // this wave's share of the next tile's rows has landed (requested ~3k cycles ago, ahead of 54 MFMAs)
                    // (A/B: drained only before the second column tile's dW1, which then hosts the whole conversion -- neutral,
                    // 125.8 vs 126.0 us, same box: the drain is not what column tile 0's dW2 waits for)
                    fs_dma_drain();
                    gemm_prefetch_b3<MLP_H2>(wt2b, PTB + MLP_OFF_PTB2, 2 * wave + 1, lane);      // lands during dW1 of tile 0
                }
                stamp<STAMP>(stamps, t == 0 ? 13 : 15);
                if (!STAMP) fs_split(n);
                {
                    // dW1[n tile ct][k tile kt]: both k-steps back to back.  Behind the MFMAs rides the conversion of the NEXT
                    // tile's rows (staging -> the other X buffer): both column tiles host it, 36 slices over 72 MFMAs, three per dW1
                    // k-step (in a workgroup's LAST tile the slices convert whatever the staging block holds into a buffer nobody reads:
                    // cheaper than a second copy of the 72 MFMAs without them)
                    bf16x8 af[2][2][3];                                    // [buffer][k-step][term]
                    fs_trns<FS_PX>(af[0][0], Xc, trx, 0, 0);
                    fs_trns<FS_PX>(af[0][1], Xc, trx, 0, 1);
#pragma unroll
                    for (int kt = 0; kt < 3; ++kt) {
                        if (kt + 1 < 3) {
                            fs_trns<FS_PX>(af[(kt + 1) & 1][0], Xc, trx, kt + 1, 0);
                            fs_trns<FS_PX>(af[(kt + 1) & 1][1], Xc, trx, kt + 1, 1);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        fs_dw_fill3(aW1[t][kt], z1f[0], af[kt & 1][0], xc, 18 * t + 6 * kt);
                        fs_dw_fill3(aW1[t][kt], z1f[1], af[kt & 1][1], xc, 18 * t + 6 * kt + 3);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (t == 0) stamp<STAMP>(stamps, 14);
            }
        }
        stamp<STAMP>(stamps, 10);
        if (!STAMP) fs_split(n);
        __syncthreads();            // every wave is done with X, H1 and dZ2 before the next tile overwrites them, and the next X is whole
        stamp<STAMP>(stamps, 11);
        if (!STAMP) fs_split(n);
    }
    if (STAMP) stamps = reinterpret_cast<unsigned long long*>(dump.out) + ((long)blockIdx.x * 64 + 63) * FS_STAMP_SLOTS;
    stamp<STAMP>(stamps, 0);
    if (!STAMP) fs_split(n);

    // ---- one partial slab per workgroup, laid out like the packed gradient (weights then biases per layer) ----------------
    const int lane = tid & 63;
    const unsigned G = gridDim.x, wg = blockIdx.x;
    constexpr unsigned S1 = fs_pad256(FS_STRIDE1), S2 = fs_pad256(FS_STRIDE2), S3 = fs_pad256(FS_STRIDE3);
    const unsigned o1 = 0, o2 = G * S1, o3 = G * (S1 + S2), o4 = G * (S1 + S2 + S3);      // the layers' slab regions (each G slabs)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) fs_store_tile(ws, o1, G, wg, MLP_IN_PAD, 2 * wave + t, kt, aW1[t][kt], lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int t = 0; t < 2; ++t) fs_store_tile(ws, o2, G, wg, MLP_H1, nt, 2 * wave + t, aW2[nt][t], lane);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) fs_store_tile(ws, o3, G, wg, MLP_H2, 2 * (wave >> 1) + a, 2 * (wave & 1) + b, aW3[a][b], lane);
    fs_store_tile(ws, o4, G, wg, MLP_H3, 0, wave, aW4, lane);
    // bias gradients: lane = column (fs_colsum): db2 of column tile `wave`, db3 of tile 2 (wave >> 1) + (wave & 1) = wave, db4 (same in
    // every wave); db1 sits in the two lane halves of the swapped-role accumulators
    if (lane < 32) {
        ws[fs_slab(o2, G, wg, MLP_H2 * MLP_H1 + 32 * wave + lane)] = bs2;
        ws[fs_slab(o3, G, wg, MLP_H3 * MLP_H2 + 32 * wave + lane)] = bs3;
        if (wave == 0) ws[fs_slab(o4, G, wg, MLP_OUT * MLP_H3 + lane)] = bs4;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float v = bs1[t] + __shfl_xor(bs1[t], 32, 64);
        if (lane < 32) ws[fs_slab(o1, G, wg, MLP_H1 * MLP_IN_PAD + 32 * (2 * wave + t) + lane)] = v;
    }
    if (STAMP) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp<STAMP>(stamps, 1);
        if (!STAMP) fs_split(n);
        if (threadIdx.x == 0) stamps[2] = realtime_cu();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The rollout's policy for ONE 32-env tile in the style of the fused step (ppo.py:213-220: Net.pi + Net.v on the tile's
// observation rows, sampling, log-prob, clipping): the X / H1 / H2 / H3 images as swizzled three-term planes in LDS, the chain GEMMs
// of the fused step (fs_gemm, the same MFMA order and epilogues: every value equals forward_body<ArithB3>'s, bit for bit), layer 4 as
// split-K partials, then forward_body<ArithB3>'s last phase (outputs, sampling on the 32 lanes of a row).  For the one-launch rollout at
// one workgroup per CU (rollout_all_kernel): the tile's rows come from the fp32 block the env step of the same workgroup left in
// LDS (`obs`, in H2's region: the conversion precedes the first store into H2), or from HBM row `x` for the first step; the
// clipped actions also go to `acts` in LDS for the env step that follows.  ~20 % fewer cycles than forward_body<ArithB3> (its 136-column
// pitches, builtin MFMAs behind a compiler-scheduled ring and two-half layer 1 / 2 interleave were tuned for three workgroups per CU).
constexpr int FR_OFF_X = 0;
constexpr int FR_OFF_H1 = FR_OFF_X + FS_X_HALVES;
constexpr int FR_OFF_H2 = FR_OFF_H1 + 3 * BM * FS_P1;
constexpr int FR_OFF_H3 = FR_OFF_H2 + 3 * BM * FS_P2;
constexpr int FR_OFF_PART = FR_OFF_H3 + 3 * BM * FS_P2;                  // fp32 [4][32][32] split-K partials
constexpr int FR_OFF_F32 = FR_OFF_PART + 4 * BM * MLP_OUT * 2;           // fp32: b1 | b2 | b3 | b4 | sqrt(var)[32] | log sqrt(var)[32] | var now [32] | acts [32][18]
constexpr int FR_TAIL_FLOATS = MLP_H1 + MLP_H2 + MLP_H3 + MLP_OUT + 3 * 32 + BM * MLP_NACT + 4;   // + sum of log sqrt(var)
constexpr int FR_LDS_BYTES = FR_OFF_F32 * 2 + FR_TAIL_FLOATS * 4;
static_assert(BM * MLP_IN * 4 <= 3 * BM * FS_P2 * 2, "the observation block fits H2's region");

struct FrLds {
    u16 *X, *H1, *H2, *H3;
    float *part, *bias1, *bias2, *bias3, *bias4, *sd, *lg, *varcur, *acts, *hld, *obs;
    __device__ __forceinline__ explicit FrLds(u16* lds)
        : X(lds + FR_OFF_X), H1(lds + FR_OFF_H1), H2(lds + FR_OFF_H2), H3(lds + FR_OFF_H3),
          part(reinterpret_cast<float*>(lds + FR_OFF_PART)), bias1(reinterpret_cast<float*>(lds + FR_OFF_F32)), bias2(bias1 + MLP_H1),
          bias3(bias2 + MLP_H2), bias4(bias3 + MLP_H3), sd(bias4 + MLP_OUT), lg(sd + 32), varcur(lg + 32), acts(varcur + 32),
          hld(acts + BM * MLP_NACT), obs(reinterpret_cast<float*>(lds + FR_OFF_H2)) {}
};

// biases -> LDS, once per launch (the caller's barrier publishes them)
__device__ __forceinline__ void policy_tile_fs_setup(const FrLds& L, const float* __restrict__ P)
{
    const int tid = threadIdx.x;
    L.bias1[tid] = P[MLP_OFF_B1 + tid];
    if (tid < MLP_H2) L.bias2[tid] = P[MLP_OFF_B2 + tid];
    else L.bias3[tid - MLP_H2] = P[MLP_OFF_B3 + tid - MLP_H2];
    if (tid < MLP_OUT) L.bias4[tid] = P[MLP_OFF_B4 + tid];
}

// x != nullptr: the tile's rows are read from HBM (row-major [n][73]); nullptr: they lie in L.obs.  Ends with a barrier: L.acts
// and every HBM row store have been issued by all waves when it returns (the stores are not waited for).
// `w1`: the head of layer 1's first column tile (policy_tile_fs_head), requested by the caller BEFORE the env step that precedes
// this call: the weights are the same every step, and their L2 round trip then hides under the physics.
// (A/B: the whole weight ring a phase ahead, WeightHeadT<4>, measured SLOWER in the same box: 22.7 vs 21.9 us per env step)
__device__ __forceinline__ void policy_tile_fs_head(WeightHeadT<2>& w1, const u16* __restrict__ PB)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    gemm_prefetch_b3<MLP_IN_PAD>(w1, PB + MLP_OFF_PB1, 2 * wave, threadIdx.x & 63);
}
// NORM: the observation block is normalised in place (obs_norm_apply) under norm_tab (LDS, published by an earlier barrier)
// before it is converted; the env step writes the next raw block over it.
template <bool STAMP = false, bool NORM = false>
__device__ __forceinline__ void policy_tile_fs(const FrLds& L, const long tile, const u16* __restrict__ PB, const float* __restrict__ x,
                                               const long n, float* __restrict__ v_out, const float* __restrict__ smp_eps,
                                               float* __restrict__ smp_act, float* __restrict__ smp_logp, const WeightHeadT<2>& w1,
                                               unsigned long long* stamps = nullptr, const float* norm_tab = nullptr)
{
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tl = tid;
    asm volatile("" : "+v"(tl));
    const int lane = tl & 63, r = lane & 31;
    const long row0 = tile * BM;
    const int nvalid = (int)(n - row0 < BM ? n - row0 : BM);
    // last phase: eight lanes per row, four output columns each (the layout of the fused step's loss phase).  The sampling noise
    // of this thread's four slots is requested now
    const int lrow = tl >> 3, lq = tl & 7;
    const bool lin = lrow < nvalid;
    float eps_pre[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        eps_pre[j] = (lin && 4 * lq + j < MLP_NACT) ? (smp_eps + row0 * MLP_NACT)[lrow * MLP_NACT + 4 * lq + j] : 0.0f;
    if (x != nullptr) {     // first step of a rollout: HBM -> the fp32 block, each wave the eight rows its own threads convert
        const long total = n * MLP_IN, base = tile * (BM * MLP_IN) + 584L * wave;
        for (int i = lane; i < 584; i += 64) L.obs[584 * wave + i] = base + i < total ? x[base + i] : 0.0f;
    }
    static_assert(BM * MLP_IN == 4 * 584, "eight rows per wave");
    // this thread's sampling constants of the CURRENT variance (ppo.py:215-219; the caller decays L.varcur once per step)
    if (tid < 32) {
        const float v = tid < MLP_NACT ? L.varcur[tid] : 1.0f;
        const float s = sqrtf(v);
        L.sd[tid] = s;
        float lg = tid < MLP_NACT ? logf(s) : 0.0f;
        L.lg[tid] = lg;
        // sum_j log sqrt(var_j): the same for every row; summed ONCE, in the order of the 32-lane xor butterfly that
        // forward_body<ArithB3> runs per row (bit-identical log-probs)
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) lg += __shfl_xor(lg, o, 32);
        if (tid == 0) L.hld[0] = lg;
    }
    if (NORM) {     // exactly the elements this thread's conversion reads (FsXStoreSlices' map), so no barrier stands between
        float* row = L.obs + (tl >> 3) * FS_IN;
        const int c0 = 12 * (tl & 7);
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (c0 + j < FS_IN) row[c0 + j] = obs_norm_apply(row[c0 + j], norm_tab[c0 + j], norm_tab[FS_IN + c0 + j], norm_tab[2 * FS_IN]);
    }
    { FsXStoreSlices xc(L.obs, L.X, tl); xc.all(); }
    __syncthreads();
    stamp<STAMP>(stamps, 1);
    WeightHeadT<2> w4;
    {
        f32x16 hi, lo;
        WeightHeadT<2> w1b, w2a;
        fs_gemm<MLP_IN_PAD, FS_PX, false>(w1, PB + MLP_OFF_PB1, 2 * wave, L.X, 0, hi, lo, lane);
        gemm_prefetch_b3<MLP_IN_PAD>(w1b, PB + MLP_OFF_PB1, 2 * wave + 1, lane);
        fs_epilogue_elu<FS_P1, false>(hi, lo, L.bias1, 64 * wave, L.H1, lane, nullptr, nvalid);
        fs_gemm<MLP_IN_PAD, FS_PX, false>(w1b, PB + MLP_OFF_PB1, 2 * wave + 1, L.X, 0, hi, lo, lane);
        gemm_prefetch_b3<MLP_H2>(w2a, PB + MLP_OFF_PB2, wave, lane);
        fs_epilogue_elu<FS_P1, false>(hi, lo, L.bias1, 64 * wave + 32, L.H1, lane, nullptr, nvalid);
        __syncthreads();
        stamp<STAMP>(stamps, 2);
        WeightHeadT<2> w2b, w3;
        gemm_prefetch_b3<MLP_H2>(w2b, PB + MLP_OFF_PB2 + 3 * MLP_H2 * (MLP_H1 / 2), wave, lane);
        fs_gemm<MLP_H2, FS_P1, false>(w2a, PB + MLP_OFF_PB2, wave, L.H1, 0, hi, lo, lane);
        fs_gemm<MLP_H2, FS_P1, false, false>(w2b, PB + MLP_OFF_PB2 + 3 * MLP_H2 * (MLP_H1 / 2), wave, L.H1, MLP_H1 / 2, hi, lo, lane);
        gemm_prefetch_b3<MLP_H2>(w3, PB + MLP_OFF_PB3, wave, lane);
        fs_epilogue_elu<FS_P2, false>(hi, lo, L.bias2, 32 * wave, L.H2, lane, nullptr, nvalid);
        __syncthreads();
        stamp<STAMP>(stamps, 3);
        gemm_prefetch_b3<32>(w4, PB + MLP_OFF_PB4 + (long)(2 * wave) * 1536, 0, lane);
        fs_gemm<MLP_H2, FS_P2, false>(w3, PB + MLP_OFF_PB3, wave, L.H2, 0, hi, lo, lane);
        fs_epilogue_elu<FS_P2, false>(hi, lo, L.bias3, 32 * wave, L.H3, lane, nullptr, nvalid);
        __syncthreads();
        stamp<STAMP>(stamps, 4);
    }
    {   // layer 4, split-K over the four waves (32 k each), partials chunk-rotated (no bank conflicts)
        f32x16 hi, lo;
        fs_gemm<32, FS_P2, false>(w4, PB + MLP_OFF_PB4 + (long)(2 * wave) * 1536, 0, L.H3, 32 * wave, hi, lo, lane);
        float* pw = L.part + wave * (BM * MLP_OUT);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(pw + r * MLP_OUT + 4 * ((acc_n(g, lane) >> 2) ^ ((r >> 1) & 7))) =
                make_float4(hi[4 * g] + lo[4 * g], hi[4 * g + 1] + lo[4 * g + 1], hi[4 * g + 2] + lo[4 * g + 2],
                            hi[4 * g + 3] + lo[4 * g + 3]);
    }
    __syncthreads();
    stamp<STAMP>(stamps, 5);
    // outputs + sampling (ppo.py:213-220): forward_body<ArithB3>'s last phase re-laid on eight lanes per row, four output columns each --
    // ONE pass, 16-byte LDS reads, and the row's Mahalanobis sum as an 8-lane DPP butterfly (no LDS round trips) in the pairing
    // order of the 32-lane xor butterfly (columns pair as (0,1),(2,3) in the lane, then lanes ^1, ^2, ^4): bit-identical sums
    {
        const int c0 = 4 * lq;
        const int cs = 4 * (lq ^ ((lrow >> 1) & 7));                  // where the split-K stores put this chunk
        const float4 p0 = *reinterpret_cast<const float4*>(L.part + lrow * MLP_OUT + cs);
        const float4 p1 = *reinterpret_cast<const float4*>(L.part + BM * MLP_OUT + lrow * MLP_OUT + cs);
        const float4 p2 = *reinterpret_cast<const float4*>(L.part + 2 * BM * MLP_OUT + lrow * MLP_OUT + cs);
        const float4 p3 = *reinterpret_cast<const float4*>(L.part + 3 * BM * MLP_OUT + lrow * MLP_OUT + cs);
        const float4 b4 = *reinterpret_cast<const float4*>(L.bias4 + c0);
        const float4 s4 = *reinterpret_cast<const float4*>(L.sd + c0);
        const float hld = L.hld[0];
        const float zz[4] = {(((p0.x + p1.x) + p2.x) + p3.x) + b4.x, (((p0.y + p1.y) + p2.y) + p3.y) + b4.y,
                             (((p0.z + p1.z) + p2.z) + p3.z) + b4.z, (((p0.w + p1.w) + p2.w) + p3.w) + b4.w};
        const float sdv[4] = {s4.x, s4.y, s4.z, s4.w};
        float a[4], xsq[4], yv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = c0 + j;
            const float y = (col < MLP_NACT) ? elu(zz[j]) : ((col == MLP_NACT) ? zz[j] : 0.0f);   // ELU on the mean (ppo.py:30), none on v
            yv[j] = y;
            a[j] = 0.0f; xsq[j] = 0.0f;
            if (col < MLP_NACT && lin) {
                a[j] = y + sdv[j] * eps_pre[j];
                const float xj = (a[j] - y) / sdv[j];
                xsq[j] = xj * xj;
            }
        }
        const float M = fs_sum8((xsq[0] + xsq[1]) + (xsq[2] + xsq[3]));
        if (lin) {
            if (v_out && lq == MLP_NACT / 4) (v_out + row0)[lrow] = yv[MLP_NACT % 4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < MLP_NACT) {
                    const float ac = fminf(fmaxf(a[j], -1.0f), 1.0f);
                    (smp_act + row0 * MLP_NACT)[lrow * MLP_NACT + c0 + j] = ac;
                    L.acts[lrow * MLP_NACT + c0 + j] = ac;
                }
            if (lq == 0) (smp_logp + row0)[lrow] = gauss_logp(M, hld);
        }
    }
    __syncthreads();
}
