// mlp_adam.inc — clip_grad_norm_ + Adam on the packed parameters, refresh of the fragment-ordered copies.
// ---------------------------------------------------------------------------------------------
// Optimizer step (ppo.py:196-199): clip_grad_norm_(max_norm) + Adam (torch defaults: no weight
// decay, no amsgrad) over the packed parameter buffer, plus the refresh of the transposed weights
// the next backward pass streams.  Two small launches: per-block sums of squares of the masked,
// scaled gradient (fixed order: deterministic), then the update, where every block re-adds the
// 73 block sums in the same order and so derives the same clip coefficient.  The step counter
// lives in device memory (incremented by the first launch), so both are graph-capturable.
// (round 5 A/B, rocprof in the optimizer loop: 1024-thread blocks 5.6 us, 256-thread blocks 6.15 us -- more blocks re-add the norm
//  partials and ramp up; not kept.)
constexpr int ADAM_THREADS = 1024;
constexpr int ADAM_WAVES = ADAM_THREADS / 64;
constexpr int ADAM_BLOCKS = (MLP_PACKED_FLOATS + ADAM_THREADS - 1) / ADAM_THREADS;   // 73

// fp16x2 weight-scale bookkeeping in the scale table `fsc` (include/flyhip.h, h2_scales), beside the class scales:
//   [H2_SINCE + par]   applied steps whose planes were split under the current weight scales (a float);
//   [H2_WMAX + par * H2_WMAX_SLOTS + w]   max |w| over the 64 packed elements 64 w .. 64 w + 63 as an applied step left them
//                      (0 for a group of biases: every region boundary is a multiple of 64, so a group is all weights or all biases).
// par = the parity of the applied-step count: the step that takes the count to s writes slot s & 1 and reads slot (s - 1) & 1, which
// the applied step before it wrote -- no word is both read and written by one launch, and a refused step writes nothing.
constexpr int H2_SINCE = 40;
constexpr int H2_WMAX = 64;
constexpr int H2_WMAX_SLOTS = (MLP_PACKED_FLOATS + 63) / 64;                        // 1161
constexpr int H2_TABLE_FLOATS = H2_WMAX + 2 * H2_WMAX_SLOTS;                        // 2386 = MLP_H2_SCALE_FLOATS_ABI
__device__ __forceinline__ int h2_group_layer(int w)      // weight layer of packed group w, -1: biases
{
    const int o = 64 * w;
    return o < MLP_OFF_B1 ? 0 : o < MLP_OFF_W2 ? -1 : o < MLP_OFF_B2 ? 1 : o < MLP_OFF_W3 ? -1 : o < MLP_OFF_B3 ? 2 : o < MLP_OFF_W4 ? -1
         : o < MLP_OFF_B4 ? 3 : -1;
}
__device__ __forceinline__ float h2_wave_max(float x)     // max over the wave's 64 lanes of x >= 0 (order-free, exact), wave-uniform
{
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true)));
    const int b = __builtin_bit_cast(int, x);           // (each row of 16 lanes holds its maximum)
    return fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))),
                 fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48))));
}
static_assert(MLP_OFF_B1 % 64 == 0 && MLP_OFF_W2 % 64 == 0 && MLP_OFF_B2 % 64 == 0 && MLP_OFF_W3 % 64 == 0 && MLP_OFF_B3 % 64 == 0 &&
              MLP_OFF_W4 % 64 == 0 && MLP_OFF_B4 % 64 == 0, "a 64-element group (one wave of the apply kernel) lies in one region");

__global__ __launch_bounds__(ADAM_THREADS) void mlp_adam_norm_kernel(const float* __restrict__ G,
                                                                     const float* __restrict__ mask, float grad_scale,
                                                                     float* __restrict__ norm_ws, int* __restrict__ step,
                                                                     const int* __restrict__ grad_invalid)
{
    __shared__ float red[ADAM_WAVES];
    if (G[MLP_ERR_SLOT] != 0.0f) return;                    // some rank's gradient is invalid: no step anywhere (mlp_grad_w.inc)
    if (grad_invalid && *grad_invalid != 0) return;         // this rank's exchange gave up on a peer (dp_allreduce_p2p's err word)
    const int tid = threadIdx.x;
    const int i = blockIdx.x * ADAM_THREADS + tid;
    float ss = 0.0f;
    if (i < MLP_PACKED_FLOATS) { const float g = G[i] * grad_scale * mask[i]; ss = g * g; }
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) {
        float t = 0.0f;
        for (int w = 0; w < ADAM_WAVES; ++w) t += red[w];
        norm_ws[1 + blockIdx.x] = t;
        if (blockIdx.x == 0) *step += 1;
    }
}

__global__ __launch_bounds__(ADAM_THREADS) void mlp_adam_apply_kernel(float* __restrict__ P, float* __restrict__ PF,
                                                                      float* __restrict__ PT,
                                                                      const int* __restrict__ idx_f,
                                                                      const int* __restrict__ idx_t,
                                                                      const float* __restrict__ G,
                                                                      const float* __restrict__ mask,
                                                                      float* __restrict__ m, float* __restrict__ v,
                                                                      const int* __restrict__ step, float lr, float beta1,
                                                                      float beta2, float eps, float max_norm,
                                                                      float grad_scale, float* __restrict__ norm_ws,
                                                                      int nparts, float part_scale,
                                                                      u16* __restrict__ PB, u16* __restrict__ PTB,
                                                                      const int* __restrict__ idx_fb,
                                                                      const int* __restrict__ idx_tb,
                                                                      int* __restrict__ step_out,
                                                                      const int* __restrict__ grad_invalid,
                                                                      u16* __restrict__ PH, u16* __restrict__ PTH,
                                                                      float* __restrict__ fsc, int h2_period)
{
    __shared__ float s_coef, s_step_size, s_bc2_sqrt;
    __shared__ float red[ADAM_WAVES];
    __shared__ float s_wscale[4];
    __shared__ unsigned s_wmax[4];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // step_out != nullptr (data-parallel ranks: the gradient arrives from an all-reduce, nothing has prepared the
    // norm): ONE launch does everything -- every block sums the whole masked gradient itself (297 KB from L2, the
    // same fixed order in every block and on every rank) and the step counter ping-pongs: all blocks read *step,
    // block 0 writes *step_out, so no block can see a counter another block has already advanced.
    const bool self_norm = step_out != nullptr;
    // ONE memory round trip: every address is known at entry, so everything the launch reads is requested here, before the first
    // wait -- the words the refusal check needs, the step counter, the fp16x2 bookkeeping, this thread's element with all four
    // of its destination indices and its layer's weight scale, and its norm partial (self_norm: the first trip of the gradient
    // sum).  Only stores wait for the check.  (A dead thread of the last block reads element 0: no branch around a load.)
    const int i = blockIdx.x * ADAM_THREADS + tid;
    const bool live = i < MLP_PACKED_FLOATS;
    const int ic = live ? i : 0;
    // An optional buffer that is not passed reads a word of one that is, and the value is dropped: a branch around a load would put
    // a wait (for its condition, for its kernel argument) between the requests.
    const int* invalid_p = grad_invalid ? grad_invalid : step;
    const float* tab = PH ? fsc : norm_ws;
    const int* ifb = PB ? idx_fb : idx_f;
    const int* itb = PB ? idx_tb : idx_t;
    const int layer = ic < MLP_OFF_W2 ? 0 : ic < MLP_OFF_W3 ? 1 : ic < MLP_OFF_W4 ? 2 : 3;
    const float err_mark = G[MLP_ERR_SLOT];
    const int invalid_w = *invalid_p, step_in = *step;
    const float s0 = tab[H2_SINCE], s1 = tab[H2_SINCE + 1];     // (both words: the loads need not wait for *step)
    const float mk = mask[ic], g_in = G[ic], m_in = m[ic], v_in = v[ic], p_in = P[ic];
    const int jf_in = idx_f[ic], jt_in = idx_t[ic], kf_in = ifb[ic], kt_in = itb[ic];
    const float wscale = tab[8 + layer];                        // (a rescale step derives its own below and does not use this)
    const float part0 = norm_ws[1 + (tid < nparts ? tid : 0)];
    const float4* g4 = reinterpret_cast<const float4*>(G);
    const float4* m4 = reinterpret_cast<const float4*>(mask);
    const int q0 = self_norm ? tid : 0;                         // (the other forms drop it: one line per wave)
    const float4 ga = g4[q0], ka = m4[q0];
    const int invalid = grad_invalid ? invalid_w : 0;
    const int jf = live ? jf_in : -1, jt = live ? jt_in : -1;
    const int kf = PB ? kf_in : -1, kt = PB ? kt_in : -1;
    // (the scalar words -- and the kernel arguments only the stores use -- are held to this point, or their requests drift down to
    // their first use, one round trip each behind a wait)
    asm volatile("" :: "s"(err_mark), "s"(invalid_w), "s"(step_in), "s"(s0), "s"(s1), "s"(PF), "s"(PT), "s"(PTB), "s"(PTH), "s"(h2_period),
                 "s"(eps), "s"(max_norm), "s"(part_scale));
    // bias corrections of torch.optim.Adam, once per workgroup (two powf per thread otherwise): they need the step counter and
    // nothing else, so lane 0 of waves 1 and 2 works them out, one powf each, side by side, while the element loads are still
    // in flight and apart from wave 0, which has the norm.  (Only LDS is written: a refused step leaves no trace.)
    const int step_now = self_norm ? step_in + 1 : step_in;     // applied steps once this one is (norm_ready: already advanced)
    if (wave == 1 && (tid & 63) == 0) s_step_size = lr / (1.0f - powf(beta1, (float)step_now));
    if (wave == 2 && (tid & 63) == 0) s_bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step_now));
    // the one wait: everything requested above has to have arrived here, so no request can sink below the check
    asm volatile("" :: "v"(mk), "v"(g_in), "v"(m_in), "v"(v_in), "v"(p_in), "v"(jf_in), "v"(jt_in), "v"(kf_in), "v"(kt_in), "v"(wscale),
                 "v"(part0), "v"(ga.x), "v"(ka.x));
    // fail closed: weights and moments never see an invalid gradient.  `grad_invalid` (optional) is a device word that whoever
    // produced G sets when G is not what it should be -- dp_allreduce_p2p's err word: ANY of its workgroups that gave up on a
    // peer sets it, so a gradient that is only PARTLY reduced is refused too (the mark inside G covers only the block that owns it).
    // Nothing has been stored yet.
    if (err_mark != 0.0f || invalid != 0) {
        if (self_norm && blockIdx.x == 0 && tid == 0) *step_out = step_in;
        return;
    }
    {   // every block re-adds the same partial sums in the same order: identical clip coefficient
        float t = 0.0f;
        if (self_norm) {
            static_assert(MLP_PACKED_FLOATS / 4 >= ADAM_THREADS, "every thread has a first trip");
            float4 g = ga, k = ka;
            for (int q = tid;;) {
                const float a = g.x * grad_scale * k.x, b = g.y * grad_scale * k.y, c = g.z * grad_scale * k.z, d = g.w * grad_scale * k.w;
                t += (a * a + b * b) + (c * c + d * d);
                q += ADAM_THREADS;
                if (q >= MLP_PACKED_FLOATS / 4) break;
                g = g4[q]; k = m4[q];
            }
        } else {
            if (tid < nparts) t += part0;
            for (int b = tid + ADAM_THREADS; b < nparts; b += ADAM_THREADS) t += norm_ws[1 + b];
        }
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = t;
    }
    // fp16x2 weight planes: layer l's weights are split as w s_l = h0 + h1 under a scale that stays fixed between two RESCALE steps.
    // The count of applied steps since the scales were derived lives in the table (H2_SINCE), so a refused step neither counts nor
    // uses up a rescale: the first APPLIED step that finds the count at h2_period (the host: min(64, 0.9 / (3.2 lr))) rescales.  A
    // rescale step derives s_l from the weights as they stand BEFORE this step: the per-group maxima the previous applied step
    // published (H2_WMAX, the slot of the other parity: no block of this launch writes it; mlp_h2_rescale seeds both), the same in
    // every block -- max(max |w_l|, 2^-4) -> [2^11, 2^12), 16x below fp16's largest value.  An Adam step moves a weight by at most
    // lr (1 - beta1) / sqrt(1 - beta2) = 3.2 lr, so over the <= h2_period + 1 steps a scale serves a weight travels < 0.21, while
    // overflowing needs it to grow to 16 max(max |w_l|, 2^-4) >= 1: it cannot.
    const int par = step_now & 1;
    bool rescale = false;
    if (PH) {
        const int since = (int)(par ? s0 : s1);
        rescale = since >= h2_period;
        if (blockIdx.x == 0 && tid == 0) fsc[H2_SINCE + par] = rescale ? 1.0f : (float)(since + 1);
    }
    if (PH && rescale) {    // (once per h2_period steps: the one dependent load a step may keep, the maxima table)
        if (tid < 4) s_wmax[tid] = 0u;
        __syncthreads();
        float mx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* wm = fsc + H2_WMAX + (par ^ 1) * H2_WMAX_SLOTS;
        for (int w = tid; w < H2_WMAX_SLOTS; w += ADAM_THREADS) {
            const int l = h2_group_layer(w);
            const float a = wm[w];
#pragma unroll
            for (int k = 0; k < 4; ++k) mx[k] = l == k ? fmaxf(mx[k], a) : mx[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float m = mx[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            if ((tid & 63) == 0 && m > 0.0f) atomicMax(&s_wmax[k], __float_as_uint(m));     // (non-negative floats order like their bits)
        }
        __syncthreads();
        if (tid < 4) {
            const float m = fminf(fmaxf(__uint_as_float(s_wmax[tid]), 0x1p-4f), 0x1p60f);
            const float sc = ldexpf(1.0f, 11 - ilogbf(m));
            s_wscale[tid] = sc;
            if (blockIdx.x == 0) { fsc[8 + tid] = sc; fsc[16 + 8 + tid] = 1.0f / sc; }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.0f;
        for (int w = 0; w < ADAM_WAVES; ++w) t += red[w];
        t *= part_scale;                                    // partials of the unscaled gradient: scale^2
        const float norm = sqrtf(t);
        const float coef = max_norm / (norm + 1e-6f);          // torch.nn.utils.clip_grad_norm_
        s_coef = coef < 1.0f ? coef : 1.0f;
        if (blockIdx.x == 0) norm_ws[0] = norm;
        if (self_norm && blockIdx.x == 0) *step_out = step_now;
    }
    __syncthreads();
    float p = 0.0f;
    if (live) {
        const float coef = s_coef * grad_scale;
        const float step_size = s_step_size;
        const float bc2_sqrt = s_bc2_sqrt;
        const float g = g_in * coef * mk;
        const float mi = beta1 * m_in + (1.0f - beta1) * g;
        const float vi = beta2 * v_in + (1.0f - beta2) * g * g;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p = p_in - mk * (step_size * (mi / denom));
        P[i] = p;
        // keep the fragment-ordered copies the kernels stream in step with the master weights
        if (jf >= 0) PF[jf] = p;
        if (jt >= 0) PT[jt] = p;
        if (PB) {       // and the three-term bf16 planes of the bf16x3 GEMM path
            u16 a, b, c;
            split3(p, a, b, c);
            if (kf >= 0) { PB[kf] = a; PB[kf + 512] = b; PB[kf + 1024] = c; }
            if (kt >= 0) { PTB[kt] = a; PTB[kt + 512] = b; PTB[kt + 1024] = c; }
        }
        if (PH && kf >= 0) {    // and the two-term fp16 planes of the fp16x2 step (PB's layout with 1024-word blocks instead of 1536), under
            // the layer's scale
            const float ps = p * (rescale ? s_wscale[layer] : wscale);
            const _Float16 h0 = (_Float16)ps;
            const _Float16 h1 = (_Float16)(ps - (float)h0);
            const u16 a = __builtin_bit_cast(u16, h0), b = __builtin_bit_cast(u16, h1);
            const int hf = (kf / 1536) * 1024 + kf % 1536;
            PH[hf] = a; PH[hf + 512] = b;
            if (kt >= 0) { const int ht = (kt / 1536) * 1024 + kt % 1536; PTH[ht] = a; PTH[ht + 512] = b; }
        }
    }
    if (PH) {   // publish this wave's max |w| of the weights it leaves, for the next rescale step (a wave is one group of 64)
        const int w = i >> 6;
        float mw = 0.0f;
        if (h2_group_layer(w) >= 0) mw = h2_wave_max(fabsf(p));        // (wave-uniform branch)
        if ((tid & 63) == 0 && w < H2_WMAX_SLOTS) fsc[H2_WMAX + par * H2_WMAX_SLOTS + w] = mw;
    }
}

// The same scales and BOTH plane buffers from the master weights as they stand, without an optimizer step: for a policy whose weights
// changed out of band (a loaded checkpoint, PackedPolicy.refresh).  One block, 74 272 elements, ~100 us: never on the training path
// (there mlp_adam_apply_kernel's rescale steps do it).
constexpr int H2_RESCALE_THREADS = 1024;
__global__ __launch_bounds__(H2_RESCALE_THREADS) void mlp_h2_rescale_kernel(const float* __restrict__ P, const int* __restrict__ idx_fb,
                                                                            const int* __restrict__ idx_tb, u16* __restrict__ PH,
                                                                            u16* __restrict__ PTH, float* __restrict__ fsc)
{
    __shared__ unsigned s_max[4];
    __shared__ float s_scale[4];
    const int tid = threadIdx.x;
    if (tid < 4) s_max[tid] = 0u;
    __syncthreads();
    float mine[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = tid; i < MLP_PACKED_FLOATS; i += H2_RESCALE_THREADS)
        if (idx_fb[i] >= 0) {
            const int layer = i < MLP_OFF_W2 ? 0 : i < MLP_OFF_W3 ? 1 : i < MLP_OFF_W4 ? 2 : 3;
            const float a = fabsf(P[i]);
#pragma unroll
            for (int l = 0; l < 4; ++l) mine[l] = layer == l ? fmaxf(mine[l], a) : mine[l];
        }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        float m = mine[l];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if ((tid & 63) == 0 && m > 0.0f) atomicMax(&s_max[l], __float_as_uint(m));     // (non-negative floats order like their bits)
    }
    __syncthreads();
    if (tid < 4) {
        const float mx = fminf(fmaxf(__uint_as_float(s_max[tid]), 0x1p-4f), 0x1p60f);
        const float sc = ldexpf(1.0f, 11 - ilogbf(mx));
        s_scale[tid] = sc;
        fsc[8 + tid] = sc;
        fsc[16 + 8 + tid] = 1.0f / sc;
    }
    __syncthreads();
    // seed what the next mlp_adam_apply_kernel reads, whichever parity it takes: no applied step since the scales were derived, and
    // the per-group maxima of the weights as they stand
    if (tid < 2) fsc[H2_SINCE + tid] = 0.0f;
    for (int w = tid; w < H2_WMAX_SLOTS; w += H2_RESCALE_THREADS) {
        float m = 0.0f;
        if (h2_group_layer(w) >= 0)
            for (int j = 64 * w; j < 64 * w + 64; ++j) m = fmaxf(m, fabsf(P[j]));
        fsc[H2_WMAX + w] = m;
        fsc[H2_WMAX + H2_WMAX_SLOTS + w] = m;
    }
    for (int i = tid; i < MLP_PACKED_FLOATS; i += H2_RESCALE_THREADS) {
        const int kf = idx_fb[i];
        if (kf < 0) continue;
        const int layer = i < MLP_OFF_W2 ? 0 : i < MLP_OFF_W3 ? 1 : i < MLP_OFF_W4 ? 2 : 3;
        const float ps = P[i] * s_scale[layer];
        const _Float16 h0 = (_Float16)ps;
        const _Float16 h1 = (_Float16)(ps - (float)h0);
        const u16 a = __builtin_bit_cast(u16, h0), b = __builtin_bit_cast(u16, h1);
        const int hf = (kf / 1536) * 1024 + kf % 1536;
        PH[hf] = a; PH[hf + 512] = b;
        const int kt = idx_tb[i];
        if (kt >= 0) { const int ht = (kt / 1536) * 1024 + kt % 1536; PTH[ht] = a; PTH[ht + 512] = b; }
    }
}
