#!/usr/bin/env python3
"""What the episode-aware advantage estimate (PPO gae="episodic") does to training: ITERS iterations at N envs, seed 0, with
`--gae reference` and with `--gae episodic`.  Per run: every score line; per sampled iteration the mean step reward and the mean
return / length of the episodes finished since the previous sample (`Fly.episode_stats()`); for the episodic run also the share
of rollout rows that ended, timed out and were stale in the last rollout.

    python tools/gae_curve.py [ITERS (200)] [N (8192)]

Evidence from one seed, not a threshold."""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402


def run(iters, n, gae):
    torch.manual_seed(0)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        agent = PPO(make_args(n, gae=gae))
    T = agent.rollout_size
    print("gae=%s  num_envs=%d  rollout_size=%d  max_episode_length=%d  gemm=%s step_gemm=%s"
          % (gae, n, T, agent.env.max_episode_length, agent.policy.gemm, agent.policy.step_gemm))
    total_ret = total_len = total_cnt = 0.0
    for it in range(iters):
        with contextlib.redirect_stdout(log):
            for _ in range(T):
                agent.run()
        if it % max(1, iters // 20) == 0 or it == iters - 1:
            ret, length, cnt = agent.env.episode_stats(reset=True)
            if cnt:
                total_ret, total_len, total_cnt = total_ret + ret * cnt, total_len + length * cnt, total_cnt + cnt
            print("iter %4d  mean step reward %.4f  finished episodes %7d  mean return %.3f  mean length %.1f  max|target| %.4g"
                  % (it, float(agent.all_reward.mean()), cnt, ret, length, float(agent._target.abs().max())), flush=True)
    with contextlib.redirect_stdout(log):
        agent.flush_log()
    if total_cnt:
        print("over the run: %d finished episodes, mean return %.3f, mean length %.1f"
              % (total_cnt, total_ret / total_cnt, total_len / total_cnt))
    if gae == "episodic":
        ended = agent._reset_rows != 0
        timeout = ended & (agent._progress_rows >= agent.env.max_episode_length - 1)
        stale = torch.cat([(agent._ended_prev != 0).unsqueeze(0), ended[:-1]])
        print("last rollout: %.4f of the rows ended (%.4f timed out), %.4f were stale"
              % (float(ended.float().mean()), float(timeout.float().mean()), float(stale.float().mean())))
    print("optimizer steps %d; h2_overflows %d" % (agent.optim_step, agent.policy.h2_overflows))
    print("score lines:")
    for ln in log.getvalue().splitlines():
        if ln.startswith("Steps:"):
            print("  " + ln)
    agent.exit()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    for gae in ("reference", "episodic"):
        run(iters, n, gae)
        print()


if __name__ == "__main__":
    main()
