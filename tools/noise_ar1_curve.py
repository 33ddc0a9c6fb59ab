#!/usr/bin/env python3
"""What temporally correlated exploration noise (PPO action_noise="ar1") does to training: ITERS iterations at N envs, seed 0,
with `--action_noise white`, with `ar1` at `--noise_rho 0.5` and at 0.9.  Per run: every score line; per sampled iteration the
mean step reward and the mean return / length of the episodes finished since the previous sample (`Fly.episode_stats()`), and
the count of fp16x2 updates that overflowed their scales and were redone in bf16x3 so far (`h2_overflows`).

    python tools/noise_ar1_curve.py [ITERS (200)] [N (8192)]

Evidence from one seed, not a threshold."""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402


def run(iters, n, noise, rho):
    torch.manual_seed(0)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        agent = PPO(make_args(n, action_noise=noise, noise_rho=rho))
    T = agent.rollout_size
    print("action_noise=%s%s  num_envs=%d  rollout_size=%d  gemm=%s step_gemm=%s"
          % (noise, "  noise_rho=%g" % rho if noise == "ar1" else "", n, T, agent.policy.gemm, agent.policy.step_gemm))
    total_ret = total_len = total_cnt = 0.0
    for it in range(iters):
        with contextlib.redirect_stdout(log):
            for _ in range(T):
                agent.run()
        if it % max(1, iters // 20) == 0 or it == iters - 1:
            ret, length, cnt = agent.env.episode_stats(reset=True)
            if cnt:
                total_ret, total_len, total_cnt = total_ret + ret * cnt, total_len + length * cnt, total_cnt + cnt
            print("iter %4d  mean step reward %.4f  finished episodes %7d  mean return %.3f  mean length %.1f  h2_overflows %d"
                  % (it, float(agent.all_reward.mean()), cnt, ret, length, agent.policy.h2_overflows), flush=True)
    with contextlib.redirect_stdout(log):
        agent.flush_log()
    if total_cnt:
        print("over the run: %d finished episodes, mean return %.3f, mean length %.1f"
              % (total_cnt, total_ret / total_cnt, total_len / total_cnt))
    print("optimizer steps %d; h2_overflows %d" % (agent.optim_step, agent.policy.h2_overflows))
    print("score lines:")
    for ln in log.getvalue().splitlines():
        if ln.startswith("Steps:"):
            print("  " + ln)
    agent.exit()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    for noise, rho in (("white", 0.5), ("ar1", 0.5), ("ar1", 0.9)):
        run(iters, n, noise, rho)
        print()


if __name__ == "__main__":
    main()
