// mlp_gemm.inc — tile GEMMs on the matrix cores and their epilogues (included by mlp_mfma.hip, inside its
// anonymous namespace): fp32 MFMA runs, the bf16x3 variant, accumulator-fragment layout helpers.
typedef float f32x16 __attribute__((ext_vector_type(16)));
// 16-byte store of a register group to a saved tensor (nontemporal stores measured 4-6 % slower)
#define GSTORE4(ptr, v) (*reinterpret_cast<float4*>(ptr) = (v))

// Accesses to the saved tensors that one workgroup hands to ANOTHER inside a launch (mlp_fwd_bwd_kernel).
// COH = true: through a buffer descriptor with the sc1 bit -- stores write through the XCD's L2 to
// memory, loads bypass the reading CU's L1 -- which, with every storing wave's vmcnt(0) + barrier before an
// sc1 flag store and an sc1 poll + barrier before the loads, is the fence-free hand-off form of the
// microarchitecture guide ("Valid forms", table row 1).  COH = false: plain 16-byte accesses.
// `base` is a wave-uniform pointer (a tile's first row), `off` a small per-lane offset in floats.
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int AUX_SC1 = 16;        // gfx940+ buffer cache-policy bit 4
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* base)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}
template <bool COH>
__device__ __forceinline__ void gstore4(float* base, int off, const float4& v)
{
    if (COH) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), tile_rsrc(base), off * 4, 0, AUX_SC1);
    else *reinterpret_cast<float4*>(base + off) = v;
}
template <bool COH>
__device__ __forceinline__ float4 gload4(const float* base, int off)
{
    if (COH) return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(base), off * 4, 0, AUX_SC1));
    return *reinterpret_cast<const float4*>(base + off);
}
template <bool COH>
__device__ __forceinline__ void gstore1(float* base, int off, float v)
{
    if (COH) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), tile_rsrc(base), off * 4, 0, AUX_SC1);
    else base[off] = v;
}
template <bool COH>
__device__ __forceinline__ float gload1(const float* base, int off)
{
    if (COH) return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(tile_rsrc(base), off * 4, 0, AUX_SC1));
    return base[off];
}

constexpr int BM = 32;          // rows per workgroup
constexpr int NWAVE = 4;
constexpr int THREADS = 64 * NWAVE;

// ELU as torch evaluates it: x > 0 ? x : exp(x) - 1 (ELU.cpp), with the hardware exp2 path
// (v_exp_f32, ~1 ulp on exp): absolute error vs expm1 <= ~1.2e-7, inside the stated 2e-5 tolerance.
__device__ __forceinline__ float elu(float x) { return x > 0.0f ? x : __expf(x) - 1.0f; }
// dA * ELU'(H) with H the saved OUTPUT: ELU' = min(H, 0) + 1, so the product is one min and one fma
// (dA * min(H, 0) + dA, rounded once) instead of compare, select, add, multiply
__device__ __forceinline__ float dact(float da, float h) { return fmaf(da, fminf(h, 0.0f), da); }

// acc[t] (+)= W[col tile t][K] * A[32 rows x K]^T for this wave's NT column tiles.  The WEIGHTS are
// the MFMA "A" operand and the activations the "B" operand, so the 32x32 result tile is
// C[n][row]: a lane owns ONE row (lane&31) and, per group of four accumulator registers, FOUR
// CONSECUTIVE output columns n = 8*(reg>>2) + 4*(lane>>5) + (reg&3) -- which makes the epilogue's
// LDS traffic 16-byte vectors instead of scalars.
//   lds_in : [32][K+4] floats (row-major, k contiguous)
//   Wf     : this layer's weights in fragment order (mlp_layout.h): [col tile][K/8][64 lanes][4];
//            `tile0` = first column tile of this wave.  One wave-instruction = one contiguous KiB.
// k mapping: MFMA step s = 4*kq+q multiplies k = 4*kq+q (lanes 0..31) and k = K/2+4*kq+q (32..63).
// Measured on MI355X (tools/mfma_valu_overlap.hip): VALU, LDS and VMEM instructions do NOT execute under
// a running MFMA of the same SIMD -- every v_mov / address add / s_waitcnt stall in a GEMM loop is
// matrix-pipe time lost.  So the k loop is straight-line code: fully unrolled over a ring of four
// NAMED operand sets (compile-time indices -> registers, no copies), each set reloaded right
// after the four MFMAs that consumed it, i.e. three sets (768 matrix cycles) ahead of its next
// use; sched_barriers pin that order so the scheduler can neither hoist the loads (register
// blow-up) nor sink them (exposed L2 latency).  The first MFMA of an accumulator takes the
// constant 0 as its C operand, so no accumulator clearing is issued either.
//
// The first two weight k-quads of a GEMM are requested AHEAD of it: a caller issues `gemm_prefetch`
// before the previous layer's epilogue / barrier so the L2 round trip (1-2 k cycles, once per layer
// per tile) hides under that work instead of opening every MFMA run.
#ifndef TUNE_RING
#define TUNE_RING 4
#endif
#ifndef TUNE_ARING
#define TUNE_ARING 2
#endif
constexpr int RING = TUNE_RING, HEAD = 2, ARING = TUNE_ARING;      // weight sets (L2 latency), head sets, activation sets (LDS latency)
template <int NT>
struct WeightHead { float4 b[HEAD][NT]; };

template <int K, int NT>
__device__ __forceinline__ void gemm_prefetch(WeightHead<NT>& w, const float* __restrict__ Wf, int tile0, int lane)
{
    static_assert(K / 8 >= RING, "at least RING k-quads");
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float* bp = Wf + (long)(tile0 + t) * (K / 8) * 256 + lane * 4;
#pragma unroll
        for (int s = 0; s < HEAD; ++s) w.b[s][t] = *reinterpret_cast<const float4*>(bp + 256 * s);
    }
}

// ZERO: the accumulators start from 0 (their incoming value is ignored); otherwise they are added to.
template <int K, int NT, bool ZERO = true>
__device__ __forceinline__ void tile_gemm(const WeightHead<NT>& head, const float* __restrict__ Wf, int tile0,
                                          const float* lds_in, f32x16 (&acc)[NT], int lane)
{
    constexpr int K8 = K / 8;
    const int r = lane & 31, h = lane >> 5;
    const float* ap = lds_in + r * (K + 4) + h * (K / 2);
    const float* bp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bp[t] = Wf + (long)(tile0 + t) * K8 * 256 + lane * 4;
    float4 b[RING][NT], a[ARING];
#pragma unroll
    for (int s = 0; s < RING; ++s) {
        if (s < ARING) a[s] = *reinterpret_cast<const float4*>(ap + 4 * s);
#pragma unroll
        for (int t = 0; t < NT; ++t)
            b[s][t] = s < HEAD ? head.b[s][t] : *reinterpret_cast<const float4*>(bp[t] + 256 * s);
    }
#pragma unroll
    for (int kq = 0; kq < K8; ++kq) {
        const int s = kq % RING, sa = kq % ARING;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (ZERO && kq == 0) {
                const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s][t].x, a[sa].x, z, 0, 0, 0);
            } else {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s][t].x, a[sa].x, acc[t], 0, 0, 0);
            }
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s][t].y, a[sa].y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s][t].z, a[sa].z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s][t].w, a[sa].w, acc[t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kq + RING < K8) {
#pragma unroll
            for (int t = 0; t < NT; ++t) b[s][t] = *reinterpret_cast<const float4*>(bp[t] + 256 * (kq + RING));
        }
        if (kq + ARING < K8) a[sa] = *reinterpret_cast<const float4*>(ap + 4 * (kq + ARING));
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int K, int NT, bool ZERO = true>
__device__ __forceinline__ void tile_gemm(const float* __restrict__ Wf, int tile0, const float* lds_in,
                                          f32x16 (&acc)[NT], int lane)
{
    WeightHead<NT> head;
    gemm_prefetch<K, NT>(head, Wf, tile0, lane);
    tile_gemm<K, NT, ZERO>(head, Wf, tile0, lds_in, acc, lane);
}

// C/D layout of the 32x32 tile with the operand roles above: lane holds row (lane&31) and output
// columns n = 8*g + 4*(lane>>5) + j for register 4*g + j.
__device__ __forceinline__ int acc_n(int g, int lane) { return 8 * g + 4 * (lane >> 5); }
// Saved activations and dZ tensors ([rows][N], written by these epilogues, read back by the
// backward epilogues and the dW kernel) live in HBM in TILE-FRAGMENT order: per 32-row tile and
// 32-column tile one block of 1024 floats laid out [g][lane][4] exactly like the accumulator
// fragments, so a wave's store or load of one register group is one contiguous KiB (row-major rows
// would be 32-byte pieces of 32 different lines: measured ~30 us of the fused launch).  Offset of
// (row, col) inside its 32 x 32 block; blocks follow each other [row tile][column tile].
__device__ __forceinline__ int frag_off(int row, int col) { return ((col >> 3) * 64 + ((col >> 2) & 1) * 32 + row) * 4 + (col & 3); }
// generic C/D map (A operand indexes rows): row (reg&3) + 8*(reg>>2) + 4*(lane>>5), column lane&31
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// ---------------------------------------------------------------------------------------------
// bf16x3 GEMM path: the same tile GEMMs on v_mfma_f32_32x32x16_bf16 with both operands split into
// three bf16 terms (mlp_layout.h).  Six MFMAs of 8 passes per 16-wide k block replace eight fp32
// MFMAs of 16 passes: 192 instead of 512 matrix cycles, and (tools/bf16x3_gemm.hip) a smaller
// error than the fp32 MFMA chain because each instruction sums its 16 products before rounding.
// The large term w0*x0 accumulates in `hi`, the five small ones in `lo`; the epilogue adds them.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;
struct Frag3 { float4 p[3]; };                                   // one operand fragment: 3 terms x 8 bf16
__device__ __forceinline__ bf16x8 as_bf16x8(const float4& v) { return __builtin_bit_cast(bf16x8, v); }

constexpr int B3_PAD = 8;                                        // LDS row pitch (K + 8) bf16 = 4 banks past a multiple of 64
constexpr int B3_RING = 4, B3_HEAD = 2, B3_ARING = 2;
template <int K> constexpr int b3_plane() { return BM * (K + B3_PAD); }   // 16-bit words per term plane of a [32][K] tile

// the first HEAD k-steps of a GEMM's weights, requested a phase ahead (HEAD = 2 where registers are scarce -- the training
// kernels --, 4 = the whole ring in the rollout's policy, whose waves have registers to spare)
template <int HEAD>
struct WeightHeadT { Frag3 b[HEAD]; static constexpr int N = HEAD; };
typedef WeightHeadT<B3_HEAD> WeightHead3;

template <int K, int HEAD>
__device__ __forceinline__ void gemm_prefetch_b3(WeightHeadT<HEAD>& w, const u16* __restrict__ Wb, int tile0, int lane)
{
    const u16* bp = Wb + (long)tile0 * (K / 16) * 1536 + lane * 8;
#pragma unroll
    for (int s = 0; s < HEAD; ++s)
        if (s < K / 16) {
#pragma unroll
            for (int p = 0; p < 3; ++p) w.b[s].p[p] = *reinterpret_cast<const float4*>(bp + s * 1536 + p * 512);
        }
}

// (hi, lo) (+)= W[col tile][K] * A[32 rows x K]^T; lds_in = term 0 plane of the activation tile
// ([32][K + 8] bf16 per plane, planes b3_plane<K>() apart); Wb = this operand's planes.
template <int K, bool ZERO = true>
__device__ __forceinline__ void tile_gemm_b3(const WeightHead3& head, const u16* __restrict__ Wb, int tile0,
                                             const u16* lds_in, f32x16& hi, f32x16& lo, int lane)
{
    constexpr int K16 = K / 16;
    constexpr int RING = K16 < B3_RING ? K16 : B3_RING;
    constexpr int ARING = K16 < B3_ARING ? K16 : B3_ARING;
    const int r = lane & 31, h = lane >> 5;
    const u16* ap = lds_in + r * (K + B3_PAD) + 8 * h;
    const u16* bp = Wb + (long)tile0 * K16 * 1536 + lane * 8;
    Frag3 b[RING], a[ARING];
#pragma unroll
    for (int s = 0; s < RING; ++s) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if (s < ARING) a[s].p[p] = *reinterpret_cast<const float4*>(ap + p * b3_plane<K>() + 16 * s);
            b[s].p[p] = s < B3_HEAD ? head.b[s].p[p] : *reinterpret_cast<const float4*>(bp + s * 1536 + p * 512);
        }
    }
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < K16; ++kb) {
        const int s = kb % RING, sa = kb % ARING;
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 w0 = as_bf16x8(b[s].p[0]), w1 = as_bf16x8(b[s].p[1]), w2 = as_bf16x8(b[s].p[2]);
        const bf16x8 x0 = as_bf16x8(a[sa].p[0]), x1 = as_bf16x8(a[sa].p[1]), x2 = as_bf16x8(a[sa].p[2]);
        lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x2, (ZERO && kb == 0) ? z : lo, 0, 0, 0);
        hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x0, (ZERO && kb == 0) ? z : hi, 0, 0, 0);
        lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, x0, lo, 0, 0, 0);
        lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x1, lo, 0, 0, 0);
        lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x1, lo, 0, 0, 0);
        lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x0, lo, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (kb + RING < K16) {
#pragma unroll
            for (int p = 0; p < 3; ++p) b[s].p[p] = *reinterpret_cast<const float4*>(bp + (kb + RING) * 1536 + p * 512);
        }
        if (kb + ARING < K16) {
#pragma unroll
            for (int p = 0; p < 3; ++p) a[sa].p[p] = *reinterpret_cast<const float4*>(ap + p * b3_plane<K>() + 16 * (kb + ARING));
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// x = a + b + c exactly, each a bf16 (round to nearest even): the terms of the split
__device__ __forceinline__ void split3(float x, u16& a, u16& b, u16& c)
{
    const __bf16 t0 = (__bf16)x;
    const float r1 = x - (float)t0;
    const __bf16 t1 = (__bf16)r1;
    const float r2 = r1 - (float)t1;
    const __bf16 t2 = (__bf16)r2;
    a = __builtin_bit_cast(u16, t0); b = __builtin_bit_cast(u16, t1); c = __builtin_bit_cast(u16, t2);
}

// the same split for two values at once, terms returned as packed bf16 pairs (x in the low half):
// one v_cvt_pk_bf16_f32 per term, a shift and a mask to widen a pair back to fp32
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3x2(float x, float y, unsigned& a, unsigned& b, unsigned& c)
{
    f32x2 v = {x, y};
    a = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    v[0] -= __builtin_bit_cast(float, a << 16);
    v[1] -= __builtin_bit_cast(float, a & 0xffff0000u);
    b = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    v[0] -= __builtin_bit_cast(float, b << 16);
    v[1] -= __builtin_bit_cast(float, b & 0xffff0000u);
    c = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// four consecutive columns of one row -> the three term planes of an LDS tile (8-byte stores)
template <int K>
__device__ __forceinline__ void store_split4(u16* lds_plane0, int row, int col, const float4& y)
{
    unsigned a0, b0, c0, a1, b1, c1;
    split3x2(y.x, y.y, a0, b0, c0);
    split3x2(y.z, y.w, a1, b1, c1);
    u16* q = lds_plane0 + row * (K + B3_PAD) + col;
    *reinterpret_cast<uint2*>(q) = make_uint2(a0, a1);
    *reinterpret_cast<uint2*>(q + b3_plane<K>()) = make_uint2(b0, b1);
    *reinterpret_cast<uint2*>(q + 2 * b3_plane<K>()) = make_uint2(c0, c1);
}

// bias + ELU epilogue of the bf16x3 path: hi + lo, activation to HBM as fp32 (the backward and dW
// read it) and to the LDS tile of the next GEMM as three bf16 terms.  N = width of the LDS tile.
template <int N, int NG = N, bool COH = false>
__device__ __forceinline__ void epilogue_elu_b3(const f32x16& hi, const f32x16& lo, const float* __restrict__ bias, int col0,
                                                u16* lds_plane0, int lane, float* __restrict__ gtile, int nvalid)
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
        store_split4<N>(lds_plane0, r, nb, y[g]);
    }
    if (gtile != nullptr && r < nvalid) {
        const int go = (col0 / 32) * 1024 + lane * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) gstore4<COH>(gtile, go + g * 256, y[g]);
    }
}

// bias + ELU epilogue: writes the activation tile to LDS (the next layer's operand), 16 bytes per
// store, and -- when `gdst` is given -- the same 16 bytes to the saved-activation rows in HBM.  A
// wave's four stores of one column tile touch the same 32 lines (one 128-byte line per row) and
// together fill them, so L2 merges them into full-line writes; no LDS read-back pass is needed.
// `gtile` points at this tile's first row of the destination (a wave-uniform pointer); lanes
// address it with small 32-bit offsets, and all stores sit under ONE predicate (`nvalid` rows of
// the tile exist): 64-bit per-lane address arithmetic and per-store exec masking are issue slots
// the matrix pipe does not get back.
template <int N, int NT, int NG = N, bool COH = false>
__device__ __forceinline__ void epilogue_elu(const f32x16 (&acc)[NT], const float* __restrict__ bias, int col0,
                                             float* lds_out, int lane, float* __restrict__ gtile, int nvalid)
{
    const int r = lane & 31;
    float4 y[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int nb = col0 + 32 * t + acc_n(g, lane);
            const float4 bv = *reinterpret_cast<const float4*>(bias + nb);
            y[t][g].x = elu(acc[t][4 * g + 0] + bv.x);
            y[t][g].y = elu(acc[t][4 * g + 1] + bv.y);
            y[t][g].z = elu(acc[t][4 * g + 2] + bv.z);
            y[t][g].w = elu(acc[t][4 * g + 3] + bv.w);
            *reinterpret_cast<float4*>(lds_out + r * (N + 4) + nb) = y[t][g];
        }
    }
    if (gtile != nullptr && r < nvalid) {
        const int go = (col0 / 32) * 1024 + lane * 4;             // column tile col0/32 of this row tile, fragment order
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) gstore4<COH>(gtile, go + t * 1024 + g * 256, y[t][g]);
    }
}

// dZ = dA * ELU'(H).  H is read from the saved activations in exactly the accumulator layout (a
// lane owns row lane&31 and four consecutive columns per register group): one 16-byte load per
// group, requested before the GEMM whose epilogue consumes it.  The four loads of a column tile
// touch one 128-byte line per row, so L1 serves three of them.
template <int NT>
struct HFrag { float4 v[NT][4]; };

template <int N, int NT, bool COH = false>
__device__ __forceinline__ void hfrag_load(HFrag<NT>& hf, const float* __restrict__ htile, int nvalid, int col0, int lane)
{
    // the saved activations are in tile-fragment order (frag_off, above): this wave's four loads of a
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
