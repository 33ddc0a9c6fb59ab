// time_scan.h — the pieces shared by the backward "one wave per env, time on lanes" kernels (PPO_GAE_SCAN: the reference GAE's
// scan in ppo_kernels.hip, plain and value-normalising, and gae_episodic_scan_kernel): device code only.
//
// The 64 lanes of a wave own 64 consecutive chunks of L = ceil(T / 64) steps of the time axis [0, T), lane 0 the LAST one, so a
// scan towards higher lanes runs backwards in time.  A lane whose chunk lies before t = 0 (T < 64, or a ragged T) owns the empty
// range: t_hi <= t_lo = 0.
//
// The forward kernels (reward_returns_scan_kernel, episode_stats_scan_kernel: lane 0 owns the EARLIEST chunk) keep their own
// bounds and scans: the scans combine by other rules (float64 with an exact zero; segments), and taking the bounds from a
// function here cost reward_returns_scan_kernel two SGPRs and 0.6 - 1 % of its time (profiles/rollout_idioms_isa.txt).
#pragma once
#include <hip/hip_runtime.h>

struct TimeChunk {
    long t_lo, t_hi;    // the lane's steps: t_lo <= t < t_hi
};

__device__ __forceinline__ TimeChunk reverse_chunk(long T, int lane)
{
    const long L = (T + 63) / 64;
    TimeChunk c;
    c.t_hi = T - (long)lane * L;
    c.t_lo = (c.t_hi - L > 0) ? c.t_hi - L : 0;
    return c;
}

// Over its chunk a lane's recurrence is the affine map X -> S + m X (S: the chunk run from a zero carry, m: the product of its
// steps' multipliers).  With lane 0 first, the value after chunk l given a zero carry into chunk 0 is X_l = S_l + m_l X_{l-1}: a
// linear recurrence over lanes, solved by a 6-step Kogge-Stone inclusive scan of (m, S) pairs on shuffles.  Returns X_{l-1}, the
// carry that enters this lane's chunk; 0 for lane 0.  Only these 63 carries are re-associated against the sequential loop.
__device__ __forceinline__ float affine_carry(float m, float S, int lane)
{
    float sm = m, sv = S;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float pm = __shfl_up(sm, o, 64), pv = __shfl_up(sv, o, 64);
        if (lane >= o) { sv = sv + sm * pv; sm = sm * pm; }
    }
    const float carry = __shfl_up(sv, 1, 64);
    return lane == 0 ? 0.0f : carry;
}
