#!/usr/bin/env python3
"""What reward scaling (PPO normalize_reward) does to training: ITERS iterations at N envs, seed 0, with the flag off and on,
alone and under `--lambda_returns --gae episodic`.  Per sampled iteration: the mean step reward (raw units, comparable between
the runs), the running scale r, and the largest |critic target| and |advantage| the update saw; at the end the number of
updates in which an fp16x2 step was refused (`policy.h2_overflows`) and every score line.

    python tools/reward_norm_curve.py [ITERS (200)] [N (8192)]

Evidence from one seed, not a threshold."""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402


def run(iters, n, on, **kw):
    torch.manual_seed(0)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        agent = PPO(make_args(n, normalize_reward=on, **kw))
    T = agent.rollout_size
    print("normalize_reward=%s %s num_envs=%d  rollout_size=%d  gemm=%s step_gemm=%s" % (on, kw or "", n, T, agent.policy.gemm,
                                                                                        agent.policy.step_gemm))
    max_tg = max_adv = 0.0
    for it in range(iters):
        with contextlib.redirect_stdout(log):
            for _ in range(T):
                agent.run()
        # what the update of this iteration saw: targets and advantages are still in place
        atg, aadv = float(agent._target.abs().max()), float(agent.all_advantage.abs().max())
        max_tg, max_adv = max(max_tg, atg), max(max_adv, aadv)
        if it % max(1, iters // 20) == 0 or it == iters - 1:
            scale = "  r %.5g  S_r count %.0f var %.5g" % (float(agent.reward_scale), float(agent.reward_count),
                                                           float(agent.reward_var)) if on else ""
            print("iter %4d  mean step reward %.4f  max|target| %.4g  max|advantage| %.4g%s"
                  % (it, float(agent.all_reward.mean()), atg, aadv, scale), flush=True)
    with contextlib.redirect_stdout(log):
        agent.flush_log()
    print("over the run: max|target seen by the update| %.4g  max|advantage| %.4g" % (max_tg, max_adv))
    print("optimizer steps %d; h2_overflows (updates in which an fp16x2 step was refused and redone in bf16x3): %d"
          % (agent.optim_step, agent.policy.h2_overflows))
    print("score lines:")
    for ln in log.getvalue().splitlines():
        if ln.startswith("Steps:"):
            print("  " + ln)
    agent.exit()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    for kw in ({}, dict(lambda_returns=True, gae="episodic")):
        for on in (False, True):
            run(iters, n, on, **kw)
            print()


if __name__ == "__main__":
    main()
