// loss_head.inc — the loss heads of the update kernels, ONCE: device code only, no kernels.  Included (inside the file's
// anonymous namespace) by mlp_mfma.hip, mlp_fused_h2.hip and dqn_mfma.hip in front of mlp_gemm.inc, and by dqn_kernels.hip and
// ppo_kernels.hip.  The loss is edited HERE and nowhere else: the three-launch, fused bf16x3 and fused f16x2 paths are held
// bit-equal to each other by the tests, which they stay only as long as they share these lines.
//
//   huber / huber_grad     every update kernel (PPO value term, DQN TD term), through the two row functions below
//   gauss_logp             ppo_row_loss and the rollout's sampling epilogues (mlp_forward.inc, mlp_fused_step.inc)
//   ppo_row_loss           the loss phase of backward_body, both arithmetics (ppo_loss_phase, mlp_backward.inc: mlp_backward_dx*
//   ppo_mean_dz4           and mlp_fwd_bwd_kernel) and phase P5 of mlp_fused_step_kernel and mlp_fused_step_h2_kernel
//   dqn_action_index       dqn_huber_td_kernel (dqn_kernels.hip), dqn_td_kernel (dqn_mfma.hip), dqn_chain_kernel (dqn_fused.inc)
//   dqn_td_row             and dqn_chain_h2_kernel (dqn_fused_h2.inc)
//   tile_loss_sum          the seven kernel bodies that leave one loss partial per 32-row tile (all of the above but
//                          dqn_huber_td_kernel, whose 64-lane block reduction is another thing)
// The fused kernels keep their own plumbing around these calls (how the layer-4 sums are formed and where dZ goes): they sit
// at the register limit, and wrapping the plumbing in shared functions changed their SGPR spills (profiles/loss_head_isa.txt).
// ---------------------------------------------------------------------------------------------------------------------

constexpr float GAUSS_DIM_LOG_2PI = 33.08178959434617f;            // 18 ln 2 pi: the action space has 18 dimensions

// log-density of a diagonal Gaussian from the Mahalanobis term M and half the log-determinant (ppo.py:215-219)
__device__ __forceinline__ float gauss_logp(float M, float half_log_det) { return -0.5f * (GAUSS_DIM_LOG_2PI + M) - half_log_det; }

// smooth_l1 with beta = 1 and its derivative.  The kink belongs to the linear branch (|dv| < 1 is strict), where both
// branches and both derivatives agree.
__device__ __forceinline__ float huber(float dv) { return fabsf(dv) < 1.0f ? 0.5f * dv * dv : fabsf(dv) - 0.5f; }
__device__ __forceinline__ float huber_grad(float dv) { return fminf(fmaxf(dv, -1.0f), 1.0f); }

// derivative of ELU expressed through its OUTPUT y: 1 for y > 0, y + 1 otherwise
__device__ __forceinline__ float elu_grad_from_out(float y) { return y > 0.0f ? 1.0f : y + 1.0f; }

// One row of the PPO loss (ppo.py:191-194),
//     -min(ratio A, clamp(ratio, 1-c, 1+c) A) + huber(v - target),   ratio = exp(logp - old_logp),
// and its gradient, with torch's subgradient choices: min() splits a tie evenly between its arguments, clamp() passes
// gradient on the CLOSED interval [1-c, 1+c].
//   c    d loss / d logp (the batch mean's 1/B included)          pol  the row's policy term
//   dv   d loss / d v    (likewise)                               hub  the row's Huber term
// FAST_EXP: the ratio through v_exp_f32 (__expf, ~1 ulp) -- the f16x2 kernel only; the bf16x3 kernel keeps expf for bit
// equality with the three-launch path.
struct PpoRowLoss { float c, dv, pol, hub; };
template <bool FAST_EXP>
__device__ __forceinline__ PpoRowLoss ppo_row_loss(float M, float half_log_det, float old_logp, float A, float v, float target,
                                                   float inv_batch, float clip)
{
    const float logp = gauss_logp(M, half_log_det);
    const float ratio = FAST_EXP ? __expf(logp - old_logp) : expf(logp - old_logp);
    const float s1 = ratio * A;
    const float rc = fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
    const float s2 = rc * A;
    const float in_range = (ratio >= 1.0f - clip && ratio <= 1.0f + clip) ? 1.0f : 0.0f;
    float dmin;                                    // d min(s1,s2) / d ratio
    if (s1 < s2) dmin = A;
    else if (s1 > s2) dmin = A * in_range;
    else dmin = 0.5f * (A + A * in_range);
    const float dv = v - target;
    PpoRowLoss r;
    r.c = -inv_batch * ratio * dmin;
    r.dv = inv_batch * huber_grad(dv);
    r.pol = -fminf(s1, s2);
    r.hub = huber(dv);
    return r;
}

// dZ4 of a mean column: d loss / d(pre-ELU mean) from the row's c, the stored action a, the mean y = ELU(z) and 1 / var
__device__ __forceinline__ float ppo_mean_dz4(float c, float a, float y, float inv_var)
{
    return c * (a - y) * inv_var * elu_grad_from_out(y);
}

// The discrete action a stored action in [-1, 1] stands for: torch.round (half to even) of its position among the `nact`
// bins, clamped (dqn.py:70).  The MFMA kernels pass the constant DQN_NACT, dqn_huber_td_kernel its run-time table width.
__device__ __forceinline__ int dqn_action_index(float act, int nact)
{
    const float a01 = 0.5f * (act + 1.0f);
    const int idx = (int)rintf(a01 * (float)(nact - 1));
    return idx < 0 ? 0 : (idx >= nact ? nact - 1 : idx);
}

// One row of the DQN TD loss (dqn.py:72-79): hub = huber(q - target), dq = d mean(hub) / d q (no operand scale applied)
struct DqnTdRow { float hub, dq; };
__device__ __forceinline__ DqnTdRow dqn_td_row(float q_val, float reward, float discount, float qn_max, float done, float inv_B)
{
    const float target = reward + discount * qn_max * done;
    const float dv = q_val - target;
    DqnTdRow r;
    r.hub = huber(dv);
    r.dq = inv_B * huber_grad(dv);
    return r;
}

// Fixed-order sum of the 32 rows' loss terms of a tile: lane t < 32 of one wave brings row t's NTERMS terms
// (rowloss[NTERMS * t ..]; PPO: policy, Huber; DQN: Huber), lane 0 stores the sums to out[0 .. NTERMS).  The callers keep
// their own guards (which lanes, whether the partials are wanted at all).
template <int NTERMS>
__device__ __forceinline__ void tile_loss_sum(const float* rowloss, int t, float* __restrict__ out)
{
    static_assert(NTERMS == 1 || NTERMS == 2, "Huber term, or policy term + Huber term");
    float pol = rowloss[NTERMS * t], hub = rowloss[NTERMS * t + NTERMS - 1];
    for (int o = 16; o > 0; o >>= 1) {
        if (NTERMS == 2) pol += __shfl_down(pol, o, 32);
        hub += __shfl_down(hub, o, 32);
    }
    if (t == 0) {
        if (NTERMS == 2) out[0] = pol;
        out[NTERMS - 1] = hub;
    }
}
