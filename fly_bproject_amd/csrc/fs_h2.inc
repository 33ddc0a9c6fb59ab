// fs_h2.inc — the fp16x2 arithmetic's building blocks for the fused-step kernels (mlp_fused_h2.inc: the PPO optimizer step; dqn_fused_h2.inc:
// the DQN update): two fp16 terms per operand (x s = h0 + h1, s a power of two per tensor class), three v_mfma_f32_32x32x16_f16
// products per k block, the split / recombine helpers (v_cvt_pk_f16_f32, v_fma_mix_f32), the running-maximum fold, transposing
// fragment reads on two planes, dW / column-sum products with guests in their gaps.  Included after fs_common.inc (swizzle, FsTr,
// fs_host_gap, fs_mfma_settle ...); see mlp_fused_h2.inc's header for the arithmetic and the scales.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
struct Frag2 { float4 p[2]; };
__device__ __forceinline__ f16x8 as_f16x8(const float4& v) { return __builtin_bit_cast(f16x8, v); }
template <int HEAD> struct WeightHeadH { Frag2 b[HEAD]; static constexpr int N = HEAD; };
typedef WeightHeadH<2> WeightHead2;
#ifndef H2_RING
#define H2_RING 4
#endif


// scale table
constexpr int H2C_X = 0, H2C_H1 = 1, H2C_H2 = 2, H2C_H3 = 3, H2C_Z4 = 4, H2C_Z3 = 5, H2C_Z2 = 6, H2C_Z1 = 7, H2C_W1 = 8, H2C_W2 = 9, H2C_W3 = 10,
              H2C_W4 = 11, H2_NACT_CLASSES = 8, H2_FSC_INV = 16, H2_FSC_FLOATS = 48;
// Where a class maximum is steered (scaled): activations (x, h1 .. h3) into [2^7, 2^8) -- 256x below fp16's largest number; their maxima
// move by <= 4 binades from one minibatch to the next (tools/h2_scale_trace.py, real updates) --; gradients (dz4 .. dz1) into [2^2, 2^3):
// the PPO surrogate (ppo_row_loss, loss_head.inc) is unclipped on one side (A < 0, ratio large: ppo.py:191-193), so a few rows carry gradients 10^3 .. 10^5 x the
// rest and a class maximum RISES by up to 10.5 binades from one launch to the next (tools/h2_scale_trace.py 30 8192); 13 binades of
// headroom cover that.  What the low target costs: an element has an absolute error of max(2^-25, 2^-24 |scaled|), i.e. full
// precision down to 2^-2 .. 2^-3 of its class maximum and 2^-27 OF THE MAXIMUM below.  That is NOT enough where a few rows carry the
// maximum and the rest dominate a sum over rows: on minibatches of the training loop whose max / median row ||dz4|| is 10^4 .. 10^5,
// dW3 / db3 / dW4 / db4 come out 3e-5 .. 1e-4 off float64 under scales calibrated to the minibatch (the chain itself stays <= 2.2e-6; the
// scales the loop itself had, lagging low, give ~2e-6): tests/test_h2_real_minibatches_gpu.py, profiles/h2_real_minibatches.txt.
// Raising the target does not fix it within the headroom: 2^6 (16x the precision, 9 binades of headroom) overflowed in 3 of 30
// updates of the trace and made the benchmark 9 % slower through the bf16x3 redo.
constexpr int H2_TARGET_EXP_ACT = 7, H2_TARGET_EXP_GRAD = 2;
__host__ __device__ constexpr int h2_target_exp(int c) { return c < 4 ? H2_TARGET_EXP_ACT : H2_TARGET_EXP_GRAD; }
constexpr float H2_F16_MAX = 65504.0f;
// Scales lagging HIGH: a class maximum that falls k binades between two launches meets scales 2^k too large, and its elements lose k
// bits above the second term's fixed absolute quantum (fp16's subnormal step, 2^-24).  Measured on the PPO step with the gradient
// classes' scales 2^k too large (tests/test_h2_edges_gpu.py, profiles/h2_lagging_scales.txt), worst chain / dW / db error relative to
// its fp64 scale: k = 4: 2.3e-6, k = 6: 5.5e-6, k = 8: 2.0e-5, k = 11: 1.6e-4 (activations 8 binades low: 3.5e-7).  Real updates do
// land there: in 1875 launches of the benchmark's run, 20 had a gradient class maximum below 2^-4 of |scaled value|, 1 below 2^-6,
// none below 2^-7.  A refusal redoes the rest of the update in bf16x3 (a floor at 2^-4 refused 7 of 25 updates: 36 % slower), so
// the floor sits below what training produces: mlp_grad_reduce_h2_kernel refuses a launch (the overflow path) only when a class
// maximum of |scaled value| is nonzero and below H2_CLASS_FLOOR = 2^-8 -- more than 10 binades under the gradient window (accepted
// error up to ~1e-4), more than 15 under the activation window.
constexpr float H2_CLASS_FLOOR = 0x1p-8f;

// ---- the three products ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void h2_mfma_v(f32x16& acc, const f16x8& a, const f16x8& b)
{
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void h2_mfma_v0(f32x16& acc, const f16x8& a, const f16x8& b)
{
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
// guarded: an operand may have been written by a vector instruction just before (fs_common.inc, fs_mfma_vg)
__device__ __forceinline__ void h2_mfma_vg(f32x16& acc, const f16x8& a, const f16x8& b)
{
    asm volatile("s_nop 3\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void h2_mfma_vg0(f32x16& acc, const f16x8& a, const f16x8& b)
{
    asm volatile("s_nop 3\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}

template <int K, int HEAD>
__device__ __forceinline__ void h2_gemm_prefetch(WeightHeadH<HEAD>& w, const u16* __restrict__ Wh, int tile0, int lane)
{
    const u16* bp = Wh + (long)tile0 * (K / 16) * 1024 + lane * 8;
#pragma unroll
    for (int s = 0; s < HEAD; ++s)
        if (s < K / 16) {
#pragma unroll
            for (int p = 0; p < 2; ++p) w.b[s].p[p] = *reinterpret_cast<const float4*>(bp + s * 1024 + p * 512);
        }
}

// (hi, lo) (+)= W[column tile][K] . A[32 rows][k0 .. k0 + K)^T on the two planes at `act` (pitch PITCH, swizzled): fs_gemm's structure
// (ring of weight fragments streamed from L2, activation fragments from LDS, asm MFMAs in the VGPR form).  The sums carry the factor
// s_w s_a.  SWAP as in fs_gemm.
template <int K, int PITCH, bool SWAP, bool ZERO = true, int HEAD = 2>
__device__ __forceinline__ void h2_gemm(const WeightHeadH<HEAD>& head, const u16* __restrict__ Wh, int tile0, const u16* act, int k0,
                                        f32x16& hi, f32x16& lo, int lane)
{
    constexpr int K16 = K / 16;
    constexpr int RING = K16 < H2_RING ? K16 : H2_RING;
    constexpr int ARING = K16 < 2 ? K16 : 2;
    const int r = lane & 31;
    const int key = fs_key<PITCH>(r);
    const int sh = (k0 >> 3) + (lane >> 5);
    const u16* arow = act + r * PITCH;
    const u16* bp = Wh + (long)tile0 * K16 * 1024 + lane * 8;
    Frag2 b[RING], a[ARING];
    auto aload = [&](Frag2& f, int kb) {
        const u16* q = arow + (((sh + 2 * kb) ^ key) << 3);
#pragma unroll
        for (int p = 0; p < 2; ++p) f.p[p] = *reinterpret_cast<const float4*>(q + p * fs_plane<PITCH>());
    };
#pragma unroll
    for (int s = 0; s < RING; ++s) {
        if (s < ARING) aload(a[s], s);
#pragma unroll
        for (int p = 0; p < 2; ++p)
            b[s].p[p] = s < HEAD ? head.b[s].p[p] : *reinterpret_cast<const float4*>(bp + s * 1024 + p * 512);
    }
#pragma unroll
    for (int kb = 0; kb < K16; ++kb) {
        const int s = kb % RING, sa = kb % ARING;
        __builtin_amdgcn_sched_barrier(0);
        const f16x8 w0 = as_f16x8(b[s].p[0]), w1 = as_f16x8(b[s].p[1]);
        const f16x8 x0 = as_f16x8(a[sa].p[0]), x1 = as_f16x8(a[sa].p[1]);
        if (ZERO && kb == 0) {
            if (!SWAP) { h2_mfma_v0(lo, w0, x1); h2_mfma_v0(hi, w0, x0); } else { h2_mfma_v0(lo, x1, w0); h2_mfma_v0(hi, x0, w0); }
        } else {
            if (!SWAP) { h2_mfma_v(lo, w0, x1); h2_mfma_v(hi, w0, x0); } else { h2_mfma_v(lo, x1, w0); h2_mfma_v(hi, x0, w0); }
        }
        if (!SWAP) h2_mfma_v(lo, w1, x0); else h2_mfma_v(lo, x0, w1);
        __builtin_amdgcn_sched_barrier(0);
        if (kb + RING < K16) {
#pragma unroll
            for (int p = 0; p < 2; ++p) b[s].p[p] = *reinterpret_cast<const float4*>(bp + (kb + RING) * 1024 + p * 512);
        }
        if (kb + ARING < K16) aload(a[sa], kb + ARING);
    }
    fs_mfma_settle(hi, lo);
    __builtin_amdgcn_sched_barrier(0);
}

// ---- the two-term split ---------------------------------------------------------------------------------------------------------
// y - (float)h and (float)h0 + (float)h1 in ONE instruction each (v_fma_mix_f32 reads fp16 halves as fp32 operands; both results are
// exact: tools/f16_probe.hip)
__device__ __forceinline__ float h2_resid_lo(unsigned a, float y) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(a), "v"(y)); return r; }
__device__ __forceinline__ float h2_resid_hi(unsigned a, float y) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(a), "v"(y)); return r; }
__device__ __forceinline__ float h2_sum_lo(unsigned a, unsigned b) { float r; asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float h2_sum_hi(unsigned a, unsigned b) { float r; asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ unsigned h2_cvt2(float x, float y)
{
    const f32x2 v = {x, y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
}
// max(m, |a|, |b|) as ONE instruction (fmaxf chains compile to canonicalising v_max_f32 pairs).  v_maximum3_f32 (IEEE 754-2019
// maximum), not v_max3_f32: a NaN operand makes the result NaN instead of being dropped, so a NaN anywhere in a class reaches the
// class maximum, and from there the reduction's NaN test (which refuses the step).  The maxima are folded on with h2_nanmax for the
// same reason: fmaxf (maxNum) would drop the NaN again.
__device__ __forceinline__ float h2_max3(float m, float a, float b)
{
    float r;
    asm("v_maximum3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float h2_nanmax(float a, float b)
{
    float r;
    asm("v_maximum3_f32 %0, %1, %2, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (x, y) ALREADY scaled -> the pair's two packed terms
__device__ __forceinline__ void h2_split2(float x, float y, unsigned& a, unsigned& b)
{
    a = h2_cvt2(x, y);
    b = h2_cvt2(h2_resid_lo(a, x), h2_resid_hi(a, y));
}
// four consecutive columns of one row (scaled) -> the two term planes (8-byte stores); `am` = the running maximum of |scaled value|
template <int PITCH>
__device__ __forceinline__ void h2_store4(u16* plane0, int r, int c, const float4& ys, float& am)
{
    unsigned a0, b0, a1, b1;
    h2_split2(ys.x, ys.y, a0, b0);
    h2_split2(ys.z, ys.w, a1, b1);
    am = h2_max3(am, ys.x, ys.y);
    am = h2_max3(am, ys.z, ys.w);
    u16* q = plane0 + fs_off<PITCH>(r, c);
    *reinterpret_cast<uint2*>(q) = make_uint2(a0, a1);
    *reinterpret_cast<uint2*>(q + fs_plane<PITCH>()) = make_uint2(b0, b1);
}

// transposed operand fragments of the two planes from precomputed lane offsets (fs_trq3's addresses)
template <int PITCH, int S>
__device__ __forceinline__ void h2_trq(f16x8 (&f)[2], const u16* tbase, const FsTr& t, int xw)
{
    typedef __attribute__((address_space(3))) s16x4* lds_ptr;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const u16* a = tbase + 16 * S * PITCH + (t.lo ^ xw);
    const u16* b = tbase + 16 * S * PITCH + (t.hi ^ xw);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + p * fs_plane<PITCH>()));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(b + p * fs_plane<PITCH>()));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        f[p] = __builtin_bit_cast(f16x8, v);
    }
}
template <int PITCH>
__device__ __forceinline__ void h2_trws(f16x8 (&f)[2], const u16* buf, const FsTr& t, int T, int s)   // wide pitch, column tile T
{
    if (s == 0) h2_trq<PITCH, 0>(f, buf + 32 * (T & ~3), t, 32 * (T & 3)); else h2_trq<PITCH, 1>(f, buf + 32 * (T & ~3), t, 32 * (T & 3));
}
template <int PITCH>
__device__ __forceinline__ void h2_trns(f16x8 (&f)[2], const u16* buf, const FsTr& t, int T, int s)   // narrow pitch
{
    if (s == 0) h2_trq<PITCH, 0>(f, buf + 32 * T, t, 0); else h2_trq<PITCH, 1>(f, buf + 32 * T, t, 0);
}

// dW tile [n'][k] += dZ^T A over one k-step of 16 rows: the two small products, then the large one, into ONE accumulator; behind
// each MFMA gap J0 .. J0 + 2 of GAPS of a guest's ops (fs_host_gap).  AGPR-resident tiles (builtin MFMAs) and the VGPR form.
template <int J0, int GAPS, class E>
__device__ __forceinline__ void h2_dw_host(f32x16& acc, const f16x8 (&z)[2], const f16x8 (&a)[2], E& e)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(z[0], a[1], acc, 0, 0, 0); fs_host_gap<J0 + 0, GAPS>(e);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(z[1], a[0], acc, 0, 0, 0); fs_host_gap<J0 + 1, GAPS>(e);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(z[0], a[0], acc, 0, 0, 0); fs_host_gap<J0 + 2, GAPS>(e);
}
template <int J0, int GAPS, class E>
__device__ __forceinline__ void h2_dw_v_host(f32x16& acc, const f16x8 (&z)[2], const f16x8 (&a)[2], E& e)
{
    h2_mfma_vg(acc, z[0], a[1]); fs_host_gap<J0 + 0, GAPS>(e);
    h2_mfma_vg(acc, z[1], a[0]); fs_host_gap<J0 + 1, GAPS>(e);
    h2_mfma_vg(acc, z[0], a[0]); fs_host_gap<J0 + 2, GAPS>(e);
    fs_mfma_settle(acc);
}
struct H2NoGuest { static constexpr int TOTAL = 0; __device__ __forceinline__ void q(int) {} };
// the same three products with nothing in their gaps (the compiler schedules the fragment reads around them)
__device__ __forceinline__ void h2_dw(f32x16& acc, const f16x8 (&z)[2], const f16x8 (&a)[2])
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(z[0], a[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(z[1], a[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(z[0], a[0], acc, 0, 0, 0);
}

// db: column sums of a dZ tile through an all-ones operand (fs_colsum_step): two planes, two MFMAs per k-step
__device__ __forceinline__ f16x8 h2_ones()
{
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 o = {0x3c003c00u, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u};      // eight fp16 1.0
    return __builtin_bit_cast(f16x8, o);
}
// SETTLE = false: nothing but a later column-sum step (an MFMA accumulating on t) touches t next -- the LAST step of a sum settles
template <bool FIRST, bool SETTLE = true>
__device__ __forceinline__ void h2_colsum_step(f32x16& t, const f16x8 (&z)[2])
{
    const f16x8 ones = h2_ones();
    if (FIRST) h2_mfma_vg0(t, ones, z[1]); else h2_mfma_vg(t, ones, z[1]);
    h2_mfma_vg(t, ones, z[0]);
    if (SETTLE) fs_mfma_settle(t);
}

// fold an epilogue's maximum into this thread's slot of class c's table
__device__ __forceinline__ void h2_amax_fold(float* amax, int c, int tl, float am)
{
    float* p = amax + c * THREADS + tl;
    *p = h2_nanmax(*p, am);
}


// staging (raw fp32 rows) -> the X planes of the NEXT tile as ops for dW1's gaps (FsXStoreSlices): 3 granules x 8 ops
struct H2XStoreOps {
    static constexpr int NS = 8, TOTAL = 3 * NS;
    const float* src;
    u16* dst;
    int rr, c0;
    float sx, am;
    float v[4];
    unsigned a0, b0, a1, b1;
    __device__ __forceinline__ H2XStoreOps(const float* xs, u16* xn, int tl, float sx_)
        : src(xs + (tl >> 3) * FS_IN + 12 * (tl & 7)), dst(xn), rr(tl >> 3), c0(12 * (tl & 7)), sx(sx_), am(0.0f) {}
    __device__ __forceinline__ void op(int g, int k)
    {
        if (k == 0) { v[0] = src[4 * g + 0]; v[1] = src[4 * g + 1]; v[2] = src[4 * g + 2]; v[3] = src[4 * g + 3]; }
        if (k == 1) {
            const int c = c0 + 4 * g;
            v[0] = c + 0 < FS_IN ? v[0] * sx : 0.0f; v[1] = c + 1 < FS_IN ? v[1] * sx : 0.0f;
            fs_pin(v[0]); fs_pin(v[1]);
        }
        if (k == 2) {
            const int c = c0 + 4 * g;
            v[2] = c + 2 < FS_IN ? v[2] * sx : 0.0f; v[3] = c + 3 < FS_IN ? v[3] * sx : 0.0f;
            fs_pin(v[2]); fs_pin(v[3]);
        }
        if (k == 3) { a0 = h2_cvt2(v[0], v[1]); a1 = h2_cvt2(v[2], v[3]); fs_pin(a0); fs_pin(a1); }
        if (k == 4) { b0 = h2_cvt2(h2_resid_lo(a0, v[0]), h2_resid_hi(a0, v[1])); fs_pin(b0); }
        if (k == 5) { b1 = h2_cvt2(h2_resid_lo(a1, v[2]), h2_resid_hi(a1, v[3])); fs_pin(b1); }
        if (k == 6) { am = h2_max3(am, v[0], v[1]); am = h2_max3(am, v[2], v[3]); fs_pin(am); }
        if (k == 7) {
            u16* p = dst + fs_off<FS_PX>(rr, c0 + 4 * g);
            *reinterpret_cast<uint2*>(p) = make_uint2(a0, a1);
            *reinterpret_cast<uint2*>(p + fs_plane<FS_PX>()) = make_uint2(b0, b1);
        }
    }
    __device__ __forceinline__ void q(int t) { op(t / NS, t % NS); }
    __device__ __forceinline__ void all()
    {
#pragma unroll
        for (int t = 0; t < TOTAL; ++t) q(t);
    }
};


// h2_gemm with a guest (FsGemmHost on two planes): behind MFMA j of the GEMM's 3 K/16 the guest E runs its ops
// [j TOTAL / HOST_GAPS, (j + 1) TOTAL / HOST_GAPS).  MODE 1 (K = 256, the operand produced two 32-column tiles per wave): the k-steps over
// every wave's tile-a columns first, ONE workgroup barrier, then the tile-b columns -- the producing layer's tile-b epilogue rides in the
// first half (HOST_GAPS = 24).  MODE 2 (the k range is this wave's OWN two tiles, natural order): no barrier, the second half's
// activation fragments are read when the first half is through.  (The order of the k-steps changes the order of the fp32 additions.)
// BSPLIT != 0: the weight operand lies as TWO K / 2 operands (the PPO step's layer 2: mlp_fused_h2.inc), the second BSPLIT 16-bit words
// behind the first: k block kb of column tile t at (kb / (K16 / 2)) BSPLIT + (t K16 / 2 + kb % (K16 / 2)) 1024.
// E2: a second guest in the gaps the first leaves free (HOST_GAPS .. 3 K / 16 - 1: with MODE 1 / 2 the whole second half).
template <int K, int PITCH, bool SWAP, bool ZERO, class E, int HOST_GAPS = 3 * (K / 16), int MODE = 0, int BSPLIT = 0, class E2 = H2NoGuest>
struct H2GemmHost {
    static constexpr bool SPLIT = MODE == 1;
    static constexpr int K16 = K / 16, GAPS = 3 * K16, HALF = K16 / 2;
    static constexpr int RING = K16 < H2_RING ? K16 : H2_RING;
    static constexpr int ARING = K16 < 2 ? K16 : 2;
    static_assert(!SPLIT || K16 == 16, "the split order is written for K = 256");
    static_assert(HOST_GAPS <= GAPS && (MODE == 0 || HOST_GAPS <= 3 * HALF), "the guest must be done when the second half begins");
    Frag2 b[RING], a[ARING];
    const u16 *arow, *bp;
    int sh, key;
    f32x16 &hi, &lo;
    E& e;
    E2& e2;
    __device__ __forceinline__ H2GemmHost(f32x16& hi_, f32x16& lo_, E& e_, E2& e2_) : hi(hi_), lo(lo_), e(e_), e2(e2_) {}
    static constexpr int kblock(int i) { return !SPLIT ? i : (i < HALF ? 4 * (i >> 1) + (i & 1) : 4 * ((i - HALF) >> 1) + 2 + (i & 1)); }
    __device__ __forceinline__ void aload(Frag2& f, int kb)
    {
        const u16* q = arow + (((sh + 2 * kb) ^ key) << 3);
#pragma unroll
        for (int p = 0; p < 2; ++p) f.p[p] = *reinterpret_cast<const float4*>(q + p * fs_plane<PITCH>());
    }
    __device__ __forceinline__ void bload(Frag2& f, int kb)
    {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            f.p[p] = *reinterpret_cast<const float4*>(bp + (BSPLIT ? (kb / HALF) * BSPLIT + (kb % HALF) * 1024 : kb * 1024) + p * 512);
    }
    template <int J>
    __device__ __forceinline__ void gap()
    {
        if constexpr (J < HOST_GAPS) {
            constexpr int T0 = J * E::TOTAL / HOST_GAPS, T1 = (J + 1) * E::TOTAL / HOST_GAPS;
            __builtin_amdgcn_sched_barrier(0);
            fs_run_ops<T0, T1>(e);
            __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (E2::TOTAL > 0) {
            constexpr int R = GAPS - HOST_GAPS, J2 = J - HOST_GAPS;
            constexpr int T0 = J2 * E2::TOTAL / R, T1 = (J2 + 1) * E2::TOTAL / R;
            __builtin_amdgcn_sched_barrier(0);
            fs_run_ops<T0, T1>(e2);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <int I>
    __device__ __forceinline__ void steps()
    {
        if constexpr (I < K16) {
            constexpr int s = I % RING, sa = I % ARING;
            if constexpr (MODE != 0 && I == HALF) {
                if (SPLIT) __syncthreads();
#pragma unroll
                for (int u = 0; u < ARING; ++u)
                    if (HALF + u < K16) aload(a[(HALF + u) % ARING], kblock(HALF + u));
            }
            __builtin_amdgcn_sched_barrier(0);
            const f16x8 w0 = as_f16x8(b[s].p[0]), w1 = as_f16x8(b[s].p[1]);
            const f16x8 x0 = as_f16x8(a[sa].p[0]), x1 = as_f16x8(a[sa].p[1]);
            if constexpr (ZERO && I == 0) {
                if (!SWAP) { h2_mfma_v0(lo, w0, x1); gap<0>(); h2_mfma_v0(hi, w0, x0); } else { h2_mfma_v0(lo, x1, w0); gap<0>(); h2_mfma_v0(hi, x0, w0); }
            } else {
                if (!SWAP) { h2_mfma_v(lo, w0, x1); gap<3 * I>(); h2_mfma_v(hi, w0, x0); } else { h2_mfma_v(lo, x1, w0); gap<3 * I>(); h2_mfma_v(hi, x0, w0); }
            }
            gap<3 * I + 1>();
            if (!SWAP) h2_mfma_v(lo, w1, x0); else h2_mfma_v(lo, x0, w1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (I + RING < K16) bload(b[s], kblock(I + RING));
            if constexpr (I + ARING < K16 && !(MODE != 0 && I < HALF && I + ARING >= HALF)) aload(a[sa], kblock(I + ARING));
            gap<3 * I + 2>();
            steps<I + 1>();
        }
    }
};
template <int K, int PITCH, bool SWAP, bool ZERO = true, int HEAD = 2, int HOST_GAPS = 3 * (K / 16), int MODE = 0, int BSPLIT = 0, class E, class E2>
__device__ __forceinline__ void h2_gemm_host2(const WeightHeadH<HEAD>& head, const u16* __restrict__ Wh, int tile0, const u16* act, int k0,
                                              f32x16& hi, f32x16& lo, int lane, E& e, E2& e2)
{
    typedef H2GemmHost<K, PITCH, SWAP, ZERO, E, HOST_GAPS, MODE, BSPLIT, E2> G;
    static_assert(E2::TOTAL == 0 || HOST_GAPS < G::GAPS, "the second guest needs gaps of its own");
    G g(hi, lo, e, e2);
    const int r = lane & 31;
    g.key = fs_key<PITCH>(r);
    g.sh = (k0 >> 3) + (lane >> 5);
    g.arow = act + r * PITCH;
    g.bp = Wh + (long)tile0 * (BSPLIT ? G::HALF : G::K16) * 1024 + lane * 8;
    static_assert(MODE != 1 || HEAD <= 2, "a head is the first k-steps IN ORDER: 0, 1 are the split order's first two as well");
#pragma unroll
    for (int s = 0; s < G::RING; ++s) {
        if (s < G::ARING && (MODE == 0 || s < G::HALF)) g.aload(g.a[s], G::kblock(s));
        if (s < HEAD) {
#pragma unroll
            for (int p = 0; p < 2; ++p) g.b[s].p[p] = head.b[s].p[p];
        } else {
            g.bload(g.b[s], G::kblock(s));
        }
    }
    g.template steps<0>();
    fs_mfma_settle(hi, lo);
    __builtin_amdgcn_sched_barrier(0);
}

// the two-term split of a scaled pair as single-instruction ops (i = 0 .. 4), the running maximum among them
struct H2Chain { float t0, t1, u0, u1; unsigned a, b; };
constexpr int H2_SPLIT_OPS = 5;
__device__ __forceinline__ void h2_split_op(H2Chain& c, float& am, int i)
{
    if (i == 0) { c.a = h2_cvt2(c.t0, c.t1); fs_pin(c.a); }
    if (i == 1) { am = h2_max3(am, c.t0, c.t1); fs_pin(am); }
    if (i == 2) { c.u0 = h2_resid_lo(c.a, c.t0); fs_pin(c.u0); }
    if (i == 3) { c.u1 = h2_resid_hi(c.a, c.t1); fs_pin(c.u1); }
    if (i == 4) { c.b = h2_cvt2(c.u0, c.u1); fs_pin(c.b); }
}
template <int K, int PITCH, bool SWAP, bool ZERO = true, int HEAD = 2, int HOST_GAPS = 3 * (K / 16), int MODE = 0, int BSPLIT = 0, class E>
__device__ __forceinline__ void h2_gemm_host(const WeightHeadH<HEAD>& head, const u16* __restrict__ Wh, int tile0, const u16* act, int k0,
                                             f32x16& hi, f32x16& lo, int lane, E& e)
{
    H2NoGuest none;
    h2_gemm_host2<K, PITCH, SWAP, ZERO, HEAD, HOST_GAPS, MODE, BSPLIT>(head, Wh, tile0, act, k0, hi, lo, lane, e, none);
}
