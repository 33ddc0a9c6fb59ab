// fs_common.inc — the building blocks of the "fused step" kernels (mlp_fused_step.inc: the PPO optimizer step and the rollout's
// policy; dqn_fused.inc: the DQN update): swizzled three-term bf16 plane images in LDS that serve BOTH the row-wise reads of the
// chain GEMMs (ds_read_b128) and the transposing reads of the dW products (ds_read_b64_tr_b16), the VGPR-form MFMA through inline
// asm, the chain GEMM over a ring of weight fragments (fs_gemm), dW / column-sum products, the machinery that slices an epilogue
// into MFMA gaps, the x-row conversion slices, and small helpers.  Included inside the including file's anonymous namespace,
// after mlp_gemm.inc (BM, THREADS, Frag3, WeightHeadT, split3x2, acc_n / acc_row, ...).  FS_IN = input columns of a row (73).
#ifndef FS_IN
#define FS_IN 73
#endif
#ifndef FS_RING
#define FS_RING 4
#endif
typedef short s16x4 __attribute__((ext_vector_type(4)));                 // (the same typedef as grad_w_b3.inc's: redeclaration is fine)
constexpr int FS_PX = 96, FS_P1 = 256, FS_P2 = 128, FS_P4 = 32;          // row pitches (bf16 elements) of X, H1, H2/H3/dZ3/dZ2, dZ4
// Swizzle: physical 16-byte slot = logical slot ^ fs_key(row).
//  pitch a multiple of 256 B (H1, H2, ...): every row starts on bank 0; key = ((r & 3) << 2) | ((r >> 2) & 3) moves
//    the 64-byte window by r & 3 (the four rows of a transposing read then cover the four bank quarters) and the slot
//    inside the window by (r >> 2) & 3 (the 16 rows a ds_read_b128 lane group holds -- {0-3, 12-15, 20-27} or
//    {4-11, 16-19, 28-31} -- get 16 different keys);
//  pitch 192 B or 64 B (X, dZ4): consecutive rows already start in different bank quarters; key = (r >> 2) & 3.
template <int PITCH>
__device__ __forceinline__ int fs_key(int r)
{
    if (PITCH % 128 == 0) return ((r & 3) << 2) | ((r >> 2) & 3);
    return (r >> 2) & 3;
}
// element offset of (row, column) inside one term plane
template <int PITCH>
__device__ __forceinline__ int fs_off(int r, int c) { return r * PITCH + ((((c >> 3) ^ fs_key<PITCH>(r))) << 3) + (c & 7); }
template <int PITCH> constexpr int fs_plane() { return BM * PITCH; }

// MFMA in its VGPR form, by inline asm.  hipcc gives every MFMA of a kernel that may use more than 256 registers the AGPR
// form (accumulator in the 256 AGPRs); this kernel keeps 16 dW tiles there for its whole life (256), so the chain GEMMs'
// accumulators (and three more dW tiles) must be multiplied into where they are: in VGPRs.  What the compiler does not know
// about an asm MFMA is the hazard between its result and a following VALU read: fs_mfma_settle() pads it (once per GEMM).
// Dependent MFMAs on one accumulator need no padding (the compiler's own streams have none either), and every operand of
// these MFMAs comes from a load (LDS / global), which the compiler's s_waitcnt logic tracks through asm operands.
__device__ __forceinline__ void fs_mfma_v(f32x16& acc, const bf16x8& a, const bf16x8& b)
{
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void fs_mfma_v0(f32x16& acc, const bf16x8& a, const bf16x8& b)
{
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
// the same, guarded: for MFMAs whose operands may have been written by a vector instruction just before (a register copy, a
// materialised constant) -- the compiler pads that hazard for its own MFMAs only
__device__ __forceinline__ void fs_mfma_vg(f32x16& acc, const bf16x8& a, const bf16x8& b)
{
    asm volatile("s_nop 3\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void fs_mfma_vg0(f32x16& acc, const bf16x8& a, const bf16x8& b)
{
    asm volatile("s_nop 3\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
// The accumulators pass THROUGH the padding as in/out operands: a read of them can then not be scheduled above it.
__device__ __forceinline__ void fs_mfma_settle(f32x16& acc) { asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(acc)); }
__device__ __forceinline__ void fs_mfma_settle(f32x16& a, f32x16& b) { asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(a), "+v"(b)); }

// (hi, lo) (+)= W[column tile][K] . A[32 rows][k0 .. k0 + K)^T, A = the three planes at `act` (pitch PITCH, swizzled).
// SWAP = false: weights are the MFMA A operand -> result C[n][row] (lane = row, register groups = 4 consecutive n);
// SWAP = true: activations are the A operand -> C[row][n] (lane = n, registers = rows acc_row(reg, lane)).
template <int K, int PITCH, bool SWAP, bool ZERO = true, int HEAD = B3_HEAD>
__device__ __forceinline__ void fs_gemm(const WeightHeadT<HEAD>& head, const u16* __restrict__ Wb, int tile0, const u16* act, int k0,
                                        f32x16& hi, f32x16& lo, int lane)
{
    constexpr int K16 = K / 16;
    constexpr int RING = K16 < FS_RING ? K16 : FS_RING;
    constexpr int ARING = K16 < B3_ARING ? K16 : B3_ARING;
    const int r = lane & 31;
    const int key = fs_key<PITCH>(r);
    const int sh = (k0 >> 3) + (lane >> 5);                       // logical slot of k block 0 for this lane half
    const u16* arow = act + r * PITCH;
    const u16* bp = Wb + (long)tile0 * K16 * 1536 + lane * 8;
    Frag3 b[RING], a[ARING];
    auto aload = [&](Frag3& f, int kb) {
        const u16* q = arow + (((sh + 2 * kb) ^ key) << 3);
#pragma unroll
        for (int p = 0; p < 3; ++p) f.p[p] = *reinterpret_cast<const float4*>(q + p * fs_plane<PITCH>());
    };
#pragma unroll
    for (int s = 0; s < RING; ++s) {
        if (s < ARING) aload(a[s], s);
#pragma unroll
        for (int p = 0; p < 3; ++p)
            b[s].p[p] = s < HEAD ? head.b[s].p[p] : *reinterpret_cast<const float4*>(bp + s * 1536 + p * 512);
    }
#pragma unroll
    for (int kb = 0; kb < K16; ++kb) {
        const int s = kb % RING, sa = kb % ARING;
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 w0 = as_bf16x8(b[s].p[0]), w1 = as_bf16x8(b[s].p[1]), w2 = as_bf16x8(b[s].p[2]);
        const bf16x8 x0 = as_bf16x8(a[sa].p[0]), x1 = as_bf16x8(a[sa].p[1]), x2 = as_bf16x8(a[sa].p[2]);
        // (the pairing of terms and their order per accumulator are those of tile_gemm_b3: bit-identical sums)
        if (ZERO && kb == 0) {
            if (!SWAP) { fs_mfma_v0(lo, w0, x2); fs_mfma_v0(hi, w0, x0); } else { fs_mfma_v0(lo, x2, w0); fs_mfma_v0(hi, x0, w0); }
        } else {
            if (!SWAP) { fs_mfma_v(lo, w0, x2); fs_mfma_v(hi, w0, x0); } else { fs_mfma_v(lo, x2, w0); fs_mfma_v(hi, x0, w0); }
        }
        if (!SWAP) { fs_mfma_v(lo, w2, x0); fs_mfma_v(lo, w1, x1); fs_mfma_v(lo, w0, x1); fs_mfma_v(lo, w1, x0); }
        else { fs_mfma_v(lo, x0, w2); fs_mfma_v(lo, x1, w1); fs_mfma_v(lo, x1, w0); fs_mfma_v(lo, x0, w1); }
        __builtin_amdgcn_sched_barrier(0);
        if (kb + RING < K16) {
#pragma unroll
            for (int p = 0; p < 3; ++p) b[s].p[p] = *reinterpret_cast<const float4*>(bp + (kb + RING) * 1536 + p * 512);
        }
        if (kb + ARING < K16) aload(a[sa], kb + ARING);
    }
    fs_mfma_settle(hi, lo);
    __builtin_amdgcn_sched_barrier(0);
}

// fs_gemm with a guest: behind MFMA j of the GEMM's 6 K/16 the guest E runs its slices [j TOTAL / GAPS, (j + 1) TOTAL / GAPS)
// (e.q(t) = slice t, written so that every index folds once the k loop is unrolled).  The guest is vector / LDS
// work that does not depend on this GEMM -- the epilogue of the PREVIOUS column tile (whose accumulators the caller keeps in a
// second register pair), or the fp32 -> planes conversion of the next pass's rows: one wave per SIMD has nobody else to run it
// under, and a chain MFMA leaves ~33 cycles of which the weight / activation loads use a few issue slots.
// (the k loop is a template recursion, not an unrolled loop: with the guest's slices inside, the loop body is too large for the
// unroller's budget BEFORE the slice indices have folded, and a rolled loop would index the fragment rings dynamically -> scratch)
// HOST_GAPS: the guest is spread over the FIRST HOST_GAPS gaps only (default: all).
// MODE 1 (K = 256, an operand produced two 32-column tiles per wave: columns 64 w .. + 31 = "tile a", + 32 .. + 63 = "tile b" of wave
//   w): the k-steps over every wave's tile-a columns come first, then ONE workgroup barrier, then the tile-b columns.  That lets the
//   producing layer's tile-b epilogue ride in the first half as the guest (HOST_GAPS = 48) instead of standing exposed in front of a
//   barrier: when the barrier falls every wave's guest has stored its tile-b columns.  (The caller's barrier in front of this GEMM
//   covers the tile-a columns.)  The order of the k-steps changes the order of the fp32 additions, nothing else.
// MODE 2 (the k range is this wave's OWN two tiles, natural order): no barrier, but the second half's activation fragments are read
//   only when the first half is through -- the guest in the first half's gaps is what stores them.
template <int K, int PITCH, bool SWAP, bool ZERO, class E, int HOST_GAPS = 6 * (K / 16), int MODE = 0>
struct FsGemmHost {
    static constexpr bool SPLIT = MODE == 1;
    static constexpr int K16 = K / 16, GAPS = 6 * K16, HALF = K16 / 2;
    static constexpr int RING = K16 < FS_RING ? K16 : FS_RING;
    static constexpr int ARING = K16 < B3_ARING ? K16 : B3_ARING;
    static_assert(!SPLIT || K16 == 16, "the split order is written for K = 256");
    static_assert(HOST_GAPS <= GAPS && (MODE == 0 || HOST_GAPS <= 6 * HALF), "the guest must be done when the second half begins");
    // the split order visits every k block once, tile-a blocks (4 w, 4 w + 1) in the first half, tile-b blocks (4 w + 2, 4 w + 3) after
    static constexpr bool order_ok()
    {
        unsigned seen = 0;
        for (int i = 0; i < K16; ++i) {
            const int kb = kblock(i);
            if (kb < 0 || kb >= K16 || ((seen >> kb) & 1u)) return false;
            if (MODE == 1 && ((kb & 2) != 0) != (i >= HALF)) return false;
            seen |= 1u << kb;
        }
        return true;
    }
    Frag3 b[RING], a[ARING];
    const u16 *arow, *bp;
    int sh, key;
    f32x16 &hi, &lo;
    E& e;
    __device__ __forceinline__ FsGemmHost(f32x16& hi_, f32x16& lo_, E& e_) : hi(hi_), lo(lo_), e(e_) {}
    // k block of step i
    static constexpr int kblock(int i) { return !SPLIT ? i : (i < HALF ? 4 * (i >> 1) + (i & 1) : 4 * ((i - HALF) >> 1) + 2 + (i & 1)); }
    static_assert(order_ok(), "k-step order");
    __device__ __forceinline__ void aload(Frag3& f, int kb)
    {
        const u16* q = arow + (((sh + 2 * kb) ^ key) << 3);
#pragma unroll
        for (int p = 0; p < 3; ++p) f.p[p] = *reinterpret_cast<const float4*>(q + p * fs_plane<PITCH>());
    }
    __device__ __forceinline__ void bload(Frag3& f, int kb)
    {
#pragma unroll
        for (int p = 0; p < 3; ++p) f.p[p] = *reinterpret_cast<const float4*>(bp + kb * 1536 + p * 512);
    }
    template <int J>
    __device__ __forceinline__ void gap()
    {
        if constexpr (J < HOST_GAPS) {
            constexpr int T0 = J * E::TOTAL / HOST_GAPS, T1 = (J + 1) * E::TOTAL / HOST_GAPS;
            __builtin_amdgcn_sched_barrier(0);
            run<T0, T1>();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <int T, int TE>
    __device__ __forceinline__ void run()
    {
        if constexpr (T < TE) { e.q(T); run<T + 1, TE>(); }
    }
    template <int I>
    __device__ __forceinline__ void steps()
    {
        if constexpr (I < K16) {
            constexpr int s = I % RING, sa = I % ARING;
            if constexpr (MODE != 0 && I == HALF) {
                // every wave's guest has stored its tile-b columns; the activation fragments of the second half are read from here on
                if (SPLIT) __syncthreads();
#pragma unroll
                for (int u = 0; u < ARING; ++u)
                    if (HALF + u < K16) aload(a[(HALF + u) % ARING], kblock(HALF + u));
            }
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8 w0 = as_bf16x8(b[s].p[0]), w1 = as_bf16x8(b[s].p[1]), w2 = as_bf16x8(b[s].p[2]);
            const bf16x8 x0 = as_bf16x8(a[sa].p[0]), x1 = as_bf16x8(a[sa].p[1]), x2 = as_bf16x8(a[sa].p[2]);
            if constexpr (ZERO && I == 0) {
                if (!SWAP) { fs_mfma_v0(lo, w0, x2); gap<0>(); fs_mfma_v0(hi, w0, x0); } else { fs_mfma_v0(lo, x2, w0); gap<0>(); fs_mfma_v0(hi, x0, w0); }
            } else {
                if (!SWAP) { fs_mfma_v(lo, w0, x2); gap<6 * I>(); fs_mfma_v(hi, w0, x0); } else { fs_mfma_v(lo, x2, w0); gap<6 * I>(); fs_mfma_v(hi, x0, w0); }
            }
            gap<6 * I + 1>();
            if (!SWAP) {
                fs_mfma_v(lo, w2, x0); gap<6 * I + 2>(); fs_mfma_v(lo, w1, x1); gap<6 * I + 3>();
                fs_mfma_v(lo, w0, x1); gap<6 * I + 4>(); fs_mfma_v(lo, w1, x0);
            } else {
                fs_mfma_v(lo, x0, w2); gap<6 * I + 2>(); fs_mfma_v(lo, x1, w1); gap<6 * I + 3>();
                fs_mfma_v(lo, x1, w0); gap<6 * I + 4>(); fs_mfma_v(lo, x0, w1);
            }
            __builtin_amdgcn_sched_barrier(0);
            // (the ring refills go out BEFORE the k-step's last gap: their issue slots are the gap's too)
            if constexpr (I + RING < K16) bload(b[s], kblock(I + RING));
            if constexpr (I + ARING < K16 && !(MODE != 0 && I < HALF && I + ARING >= HALF)) aload(a[sa], kblock(I + ARING));
            gap<6 * I + 5>();
            steps<I + 1>();
        }
    }
};
template <int K, int PITCH, bool SWAP, bool ZERO = true, int HEAD = B3_HEAD, int HOST_GAPS = 6 * (K / 16), int MODE = 0, class E>
__device__ __forceinline__ void fs_gemm_host(const WeightHeadT<HEAD>& head, const u16* __restrict__ Wb, int tile0, const u16* act, int k0,
                                             f32x16& hi, f32x16& lo, int lane, E& e)
{
    typedef FsGemmHost<K, PITCH, SWAP, ZERO, E, HOST_GAPS, MODE> G;
    G g(hi, lo, e);
    const int r = lane & 31;
    g.key = fs_key<PITCH>(r);
    g.sh = (k0 >> 3) + (lane >> 5);
    g.arow = act + r * PITCH;
    g.bp = Wb + (long)tile0 * G::K16 * 1536 + lane * 8;
    static_assert(MODE != 1 || HEAD <= 2, "a head is the first k-steps IN ORDER: 0, 1 are the split order's first two as well");
#pragma unroll
    for (int s = 0; s < G::RING; ++s) {
        if (s < G::ARING && (MODE == 0 || s < G::HALF)) g.aload(g.a[s], G::kblock(s));
        if (s < HEAD) {
#pragma unroll
            for (int p = 0; p < 3; ++p) g.b[s].p[p] = head.b[s].p[p];
        } else {
            g.bload(g.b[s], G::kblock(s));
        }
    }
    g.template steps<0>();
    fs_mfma_settle(hi, lo);
    __builtin_amdgcn_sched_barrier(0);
}

// ops [T0, T1) of a guest, and the gap J of GAPS behind any MFMA (the LDS-fed dW products host guests too)
template <int T, int TE, class E>
__device__ __forceinline__ void fs_run_ops(E& e)
{
    if constexpr (T < TE) { e.q(T); fs_run_ops<T + 1, TE>(e); }
}
template <int J, int GAPS, class E>
__device__ __forceinline__ void fs_host_gap(E& e)
{
    __builtin_amdgcn_sched_barrier(0);
    fs_run_ops<J * E::TOTAL / GAPS, (J + 1) * E::TOTAL / GAPS>(e);
    __builtin_amdgcn_sched_barrier(0);
}
// fs_dw (below) with gaps J0 .. J0 + 5 of GAPS behind its six MFMAs
template <int J0, int GAPS, class E>
__device__ __forceinline__ void fs_dw_host(f32x16& acc, const bf16x8 (&z)[3], const bf16x8 (&a)[3], E& e)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[2], acc, 0, 0, 0); fs_host_gap<J0 + 0, GAPS>(e);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[2], a[0], acc, 0, 0, 0); fs_host_gap<J0 + 1, GAPS>(e);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[1], acc, 0, 0, 0); fs_host_gap<J0 + 2, GAPS>(e);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[1], acc, 0, 0, 0); fs_host_gap<J0 + 3, GAPS>(e);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[0], acc, 0, 0, 0); fs_host_gap<J0 + 4, GAPS>(e);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[0], acc, 0, 0, 0); fs_host_gap<J0 + 5, GAPS>(e);
}

// four consecutive columns of one row -> the three term planes (8-byte stores)
template <int PITCH>
__device__ __forceinline__ void fs_store4(u16* plane0, int r, int c, const float4& y)
{
    unsigned a0, b0, c0, a1, b1, c1;
    split3x2(y.x, y.y, a0, b0, c0);
    split3x2(y.z, y.w, a1, b1, c1);
    u16* q = plane0 + fs_off<PITCH>(r, c);
    *reinterpret_cast<uint2*>(q) = make_uint2(a0, a1);
    *reinterpret_cast<uint2*>(q + fs_plane<PITCH>()) = make_uint2(b0, b1);
    *reinterpret_cast<uint2*>(q + 2 * fs_plane<PITCH>()) = make_uint2(c0, c1);
}
// a packed bf16 pair widened back to two floats (t0 + (t1 + t2) of the three terms is exact: it IS the fp32 value that was split)
__device__ __forceinline__ float fs_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float fs_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// Transposed operand fragment of one term plane: lane l gets column c0 + (l & 31), k-step s (rows 16 s .. 16 s + 15) in the
// order element j <-> row 16 s + 8 (j >> 2) + 4 (l >> 5) + (j & 3) -- the order in which a 32x32 accumulator with its ROWS in the
// registers (acc_row) holds them, so that tr-read fragments and converted accumulators can meet in one MFMA.
// (The defining form of the address arithmetic; the kernel reads through fs_trq3 below, which computes the same addresses.)
template <int PITCH>
__device__ __forceinline__ bf16x8 fs_trfrag(const u16* plane, int c0, int s, int lane)
{
    const int i = lane & 15, g = (lane >> 4) & 1, h = lane >> 5;
    const int row = 16 * s + 4 * h + (i >> 2);
    const int gran = 4 * g + (i & 3);                                // 8-byte granule inside the 64-byte window at c0
    const int slot = (c0 >> 3) + (gran >> 1);
    typedef __attribute__((address_space(3))) s16x4* lds_ptr;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_ptr)(plane + row * PITCH + ((slot ^ fs_key<PITCH>(row)) << 3) + (gran & 1) * 4));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_ptr)(plane + (row + 8) * PITCH + ((slot ^ fs_key<PITCH>(row + 8)) << 3) + (gran & 1) * 4));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}
// The same fragment from PRECOMPUTED lane offsets.  With key = ((r & 3) << 2) | ((r >> 2) & 3) and r = 16 s + 4 h + m (+ 8 for the
// second row block) the swizzled element offset of column tile T is
//     (4 h + m (+ 8)) PITCH + 8 ((gran >> 1) ^ h') + 4 (gran & 1)   [lane part, no s, no T: ONE register per row block]
//     ^ 32 (T & 3)                                                   [the 64-byte window: an isolated bit field, so the XOR of the
//                                                                     key acts on the offset itself; m is folded into the lane part]
//     + 16 s PITCH + 32 (T & ~3) + plane / buffer offsets            [wave-uniform or compile-time: the instruction's offset field]
// Two registers per pitch and at most two v_xor per fragment SET replace ~6 vector instructions per READ (240 reads per tile).
struct FsTr { int lo, hi; };
template <int PITCH>
__device__ __forceinline__ void fs_tr_init(FsTr& t, int lane)
{
    const int i = lane & 15, g = (lane >> 4) & 1, h = lane >> 5, m = i >> 2;
    const int gran = 4 * g + (i & 3);
    const int win = (PITCH % 128 == 0) ? 32 * m : 0;             // narrow pitches rotate the window by themselves (fs_key)
    t.lo = (4 * h + m) * PITCH + 8 * ((gran >> 1) ^ h) + 4 * (gran & 1) + win;
    t.hi = (4 * h + m + 8) * PITCH + 8 * ((gran >> 1) ^ ((h + 2) & 3)) + 4 * (gran & 1) + win;
}
// `tbase` = plane 0 of the buffer + 32 (T & ~3) (wide pitches) or + 32 T (narrow ones); `xw` = 32 (T & 3) (wide) or 0
template <int PITCH, int S>
__device__ __forceinline__ void fs_trq3(bf16x8 (&f)[3], const u16* tbase, const FsTr& t, int xw)
{
    typedef __attribute__((address_space(3))) s16x4* lds_ptr;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const u16* a = tbase + 16 * S * PITCH + (t.lo ^ xw);
    const u16* b = tbase + 16 * S * PITCH + (t.hi ^ xw);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + p * fs_plane<PITCH>()));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(b + p * fs_plane<PITCH>()));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        f[p] = __builtin_bit_cast(bf16x8, v);
    }
}
template <int PITCH>
__device__ __forceinline__ void fs_trws(bf16x8 (&f)[3], const u16* buf, const FsTr& t, int T, int s)   // wide pitch, column tile T
{
    if (s == 0) fs_trq3<PITCH, 0>(f, buf + 32 * (T & ~3), t, 32 * (T & 3)); else fs_trq3<PITCH, 1>(f, buf + 32 * (T & ~3), t, 32 * (T & 3));
}
template <int PITCH>
__device__ __forceinline__ void fs_trns(bf16x8 (&f)[3], const u16* buf, const FsTr& t, int T, int s)   // narrow pitch
{
    if (s == 0) fs_trq3<PITCH, 0>(f, buf + 32 * T, t, 0); else fs_trq3<PITCH, 1>(f, buf + 32 * T, t, 0);
}

// dW tile [n'][k] += dZ^T A over one k-step of 16 rows: the six product terms, smallest first, into ONE accumulator
__device__ __forceinline__ void fs_dw(f32x16& acc, const bf16x8 (&z)[3], const bf16x8 (&a)[3])
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[2], a[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[0], acc, 0, 0, 0);
}

// db: the column sums of a dZ tile over its 32 rows, from the transposed fragments the dW GEMM reads anyway: a product with an
// all-ones operand puts sum_rows dZ[row][n] into every register of lane n (three term planes, two k-steps: six MFMAs into a
// transient accumulator).  One persistent register per column tile instead of one per (row-in-tile, column) slot, and no
// cross-lane reduction on the vector pipe.
template <bool FIRST>
__device__ __forceinline__ void fs_colsum_step(f32x16& t, const bf16x8 (&z)[3])
{
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 o = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};      // eight bf16 1.0
    const bf16x8 ones = __builtin_bit_cast(bf16x8, o);
    if (FIRST) fs_mfma_vg0(t, ones, z[2]); else fs_mfma_vg(t, ones, z[2]);
    fs_mfma_vg(t, ones, z[1]);
    fs_mfma_vg(t, ones, z[0]);
    fs_mfma_settle(t);
}
__device__ __forceinline__ float fs_colsum_done(f32x16& t) { return t[0]; }

// "this value exists HERE": the optimizer otherwise sinks pure vector arithmetic out of the MFMA gap it was written into
__device__ __forceinline__ void fs_pin(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void fs_pin(unsigned& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void fs_pin(f32x2& x) { asm volatile("" : "+v"(x)); }

// ---- vector work in the shadow of the matrix pipe ---------------------------------------------------------------------------
// One wave per SIMD has nobody to run an epilogue under: after a GEMM the matrix pipe idles while ~60 vector instructions per
// four outputs recombine H, apply ELU' and split the result into its three bf16 terms.  Where an INDEPENDENT MFMA stream is at
// hand (the dW product of the layer above, whose operands lie in LDS already) the epilogue is cut into slices of four to six
// instructions and one slice is issued behind each MFMA: the pipe's 32 cycles cover ~24 cycles of other issue.  Every slice ends
// in fs_pin() of what it produced ("this value exists HERE"): pure arithmetic is otherwise sunk out of the gap by the optimizer;
// sched_barriers on both sides keep the machine scheduler from undoing the placement.
__device__ __forceinline__ void fs_pin(uint2& x) { asm volatile("" : "+v"(x)); }

// ---- epilogues as single-instruction ops (the pieces every such epilogue shares; see dqn_fused.inc for the measurements) -------------
// One wave per SIMD pays ~8 cycles for a vector instruction that needs the result of the one before it and ~4.5 for an independent one;
// behind an MFMA about four independent instructions are free.  An epilogue is therefore written as OPS -- one instruction each,
// pinned where it is written -- of CHAINS (one pair of adjacent outputs each), issued so that consecutive instructions belong to
// different chains.
struct FsChain { float t0, t1, u0, u1; unsigned a, b, c; };
__device__ __forceinline__ unsigned fs_cvt2(float x, float y)
{
    const f32x2 v = {x, y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// (t0, t1) -> three packed bf16 terms a, b, c: split3x2, one instruction per op (i literal: 0 .. 10)
__device__ __forceinline__ void fs_split_op(float& t0, float& t1, float& u0, float& u1, unsigned& a, unsigned& b, unsigned& c, int i)
{
    if (i == 0) { a = fs_cvt2(t0, t1); fs_pin(a); }
    if (i == 1) { u0 = fs_lo(a); fs_pin(u0); }
    if (i == 2) { u1 = fs_hi(a); fs_pin(u1); }
    if (i == 3) { t0 -= u0; fs_pin(t0); }
    if (i == 4) { t1 -= u1; fs_pin(t1); }
    if (i == 5) { b = fs_cvt2(t0, t1); fs_pin(b); }
    if (i == 6) { u0 = fs_lo(b); fs_pin(u0); }
    if (i == 7) { u1 = fs_hi(b); fs_pin(u1); }
    if (i == 8) { t0 -= u0; fs_pin(t0); }
    if (i == 9) { t1 -= u1; fs_pin(t1); }
    if (i == 10) { c = fs_cvt2(t0, t1); fs_pin(c); }
}
__device__ __forceinline__ void fs_split_op(FsChain& k, int i) { fs_split_op(k.t0, k.t1, k.u0, k.u1, k.a, k.b, k.c, i); }
constexpr int FS_SPLIT_OPS = 11;

// gap J of GAPS: slices [J TOTAL / GAPS, (J + 1) TOTAL / GAPS) of the epilogue's 4 x NS (template recursion: every slice call
// with literal indices, so the epilogue's state stays in registers)
template <int Q, int QEND, class E>
__device__ __forceinline__ void fs_slices(E& e)
{
    if constexpr (Q < QEND) { e.slice(Q / E::NS, Q % E::NS); fs_slices<Q + 1, QEND>(e); }
}
template <int GAPS, int J, class E>
__device__ __forceinline__ void fs_gap_spread(E& e)
{
    constexpr int TOTAL = 4 * E::NS;
    __builtin_amdgcn_sched_barrier(0);
    fs_slices<J * TOTAL / GAPS, (J + 1) * TOTAL / GAPS>(e);
    __builtin_amdgcn_sched_barrier(0);
}
// staging (raw fp32 rows) -> the X planes of the NEXT tile, as slices for the MFMA gaps of dW1 (3 granules x 12 slices: granule g behind
// the two k-steps of dW1's k tile g).  Thread t handles row t >> 3, columns 12 (t & 7) + 4 g .. + 3: a wave converts exactly the eight
// rows its own LDS-DMA fetched (x_fetch), so its own vmcnt(0) is all the ordering the reads need.  Columns past the 73 inputs are stored
// as zeros -- that is what keeps the K padding of layer 1 (columns 73 .. 95) zero, in both buffers, without a clearing pass.
struct FsXStoreSlices {
    const float* src;       // staging: row (t >> 3), column 12 (t & 7)
    u16* dst;               // plane 0 of the buffer being filled
    int rr, c0;
    float r0, r1, r2, r3;
    f32x2 v0, v1;
    unsigned a0, b0, c0w, a1, b1, c1w;
    __device__ __forceinline__ FsXStoreSlices(const float* xs, u16* xn, int tl)
        : src(xs + (tl >> 3) * FS_IN + 12 * (tl & 7)), dst(xn), rr(tl >> 3), c0(12 * (tl & 7)) {}
    __device__ __forceinline__ void slice(int g, int k)
    {
        if (k == 0) { r0 = src[4 * g + 0]; r1 = src[4 * g + 1]; r2 = src[4 * g + 2]; r3 = src[4 * g + 3]; }
        if (k == 2) {
            const int c = c0 + 4 * g;
            v0[0] = c + 0 < FS_IN ? r0 : 0.0f; v0[1] = c + 1 < FS_IN ? r1 : 0.0f;
            v1[0] = c + 2 < FS_IN ? r2 : 0.0f; v1[1] = c + 3 < FS_IN ? r3 : 0.0f;
            fs_pin(v0); fs_pin(v1);
        }
        if (k == 3) { a0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v0, bf16x2)); v0[0] -= fs_lo(a0); v0[1] -= fs_hi(a0); fs_pin(v0); }
        if (k == 4) {
            b0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v0, bf16x2)); v0[0] -= fs_lo(b0); v0[1] -= fs_hi(b0);
            c0w = __builtin_bit_cast(unsigned, __builtin_convertvector(v0, bf16x2)); fs_pin(c0w);
        }
        if (k == 5) { a1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v1, bf16x2)); v1[0] -= fs_lo(a1); v1[1] -= fs_hi(a1); fs_pin(v1); }
        if (k == 6) {
            b1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v1, bf16x2)); v1[0] -= fs_lo(b1); v1[1] -= fs_hi(b1);
            c1w = __builtin_bit_cast(unsigned, __builtin_convertvector(v1, bf16x2)); fs_pin(c1w);
        }
        if (k == 7) *reinterpret_cast<uint2*>(dst + fs_off<FS_PX>(rr, c0 + 4 * g)) = make_uint2(a0, a1);
        if (k == 8) *reinterpret_cast<uint2*>(dst + fs_off<FS_PX>(rr, c0 + 4 * g) + fs_plane<FS_PX>()) = make_uint2(b0, b1);
        if (k == 9) *reinterpret_cast<uint2*>(dst + fs_off<FS_PX>(rr, c0 + 4 * g) + 2 * fs_plane<FS_PX>()) = make_uint2(c0w, c1w);
    }
    __device__ __forceinline__ void all()          // the whole conversion at once (the first tile of a workgroup)
    {
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int k = 0; k < 10; ++k) slice(g, k);
    }
};
#define FS_GAP(E_, G_, K_) do { __builtin_amdgcn_sched_barrier(0); (E_).slice((G_), (K_)); __builtin_amdgcn_sched_barrier(0); } while (0)

// fs_dw, and its VGPR-tile form (asm MFMAs, settled at the end), with slices k0 .. k0 + 5 of group g of an epilogue behind their six MFMAs
template <class E>
__device__ __forceinline__ void fs_dw_fill(f32x16& acc, const bf16x8 (&z)[3], const bf16x8 (&a)[3], E& e, int g, int k0)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[2], acc, 0, 0, 0); FS_GAP(e, g, k0 + 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[2], a[0], acc, 0, 0, 0); FS_GAP(e, g, k0 + 1);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[1], acc, 0, 0, 0); FS_GAP(e, g, k0 + 2);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[1], acc, 0, 0, 0); FS_GAP(e, g, k0 + 3);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[0], acc, 0, 0, 0); FS_GAP(e, g, k0 + 4);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[0], acc, 0, 0, 0); FS_GAP(e, g, k0 + 5);
}
// fs_dw with three slices q0 .. q0 + 2 of an epilogue whose slices are numbered 12 g + k, behind its first, third and fifth MFMA
template <class E>
__device__ __forceinline__ void fs_dw_fill3(f32x16& acc, const bf16x8 (&z)[3], const bf16x8 (&a)[3], E& e, int q0)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[2], acc, 0, 0, 0); FS_GAP(e, q0 / 12, q0 % 12);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[2], a[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[1], acc, 0, 0, 0); FS_GAP(e, (q0 + 1) / 12, (q0 + 1) % 12);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[1], a[0], acc, 0, 0, 0); FS_GAP(e, (q0 + 2) / 12, (q0 + 2) % 12);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(z[0], a[0], acc, 0, 0, 0);
}
template <class E>
__device__ __forceinline__ void fs_dw_v_fill(f32x16& acc, const bf16x8 (&z)[3], const bf16x8 (&a)[3], E& e, int g, int k0)
{
    fs_mfma_vg(acc, z[0], a[2]); FS_GAP(e, g, k0 + 0);
    fs_mfma_vg(acc, z[2], a[0]); FS_GAP(e, g, k0 + 1);
    fs_mfma_vg(acc, z[1], a[1]); FS_GAP(e, g, k0 + 2);
    fs_mfma_vg(acc, z[0], a[1]); FS_GAP(e, g, k0 + 3);
    fs_mfma_vg(acc, z[1], a[0]); FS_GAP(e, g, k0 + 4);
    fs_mfma_vg(acc, z[0], a[0]); FS_GAP(e, g, k0 + 5);
    fs_mfma_settle(acc);
}

// all-reduce over 8 consecutive lanes (half a DPP row), every lane gets the same bits; the pairing (lane ^ 1, ^ 2, then the
// two quads) is the xor-butterfly's, so sums come out bit for bit as the 32-lane butterfly of backward_body<ArithB3> leaves them
__device__ __forceinline__ float fs_sum8(float x)
{
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true));   // row_half_mirror
    return x;
}

// all LDS-DMA of this wave has landed (the DMA is issued by inline asm, so the compiler's own wait counts do not cover it)
__device__ __forceinline__ void fs_dma_drain() { asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); }

// A basic-block boundary the compiler cannot remove (a scalar branch on a condition that is never true but not provably so).
// The register allocator and the pre-RA scheduler work per region: with the whole of a phase in ONE block hipcc's scheduler
// front-loads the phase's LDS reads and the allocator then spills accumulator tiles around them (171 spilled registers, ~60k
// cycles per tile); cut at the points where the diagnostic build happens to branch for its stamps, the same source allocates
// with 10 spills and runs ~48k cycles per tile.
__device__ __forceinline__ void fs_split(long never_negative)
{
    if (never_negative < 0) asm volatile("s_nop 0");
}

