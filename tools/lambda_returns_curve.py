#!/usr/bin/env python3
"""What the lambda-return critic target (PPO --lambda_returns) does to training: ITERS iterations at N envs,
seed 0, as `trainer.py --num_envs N --headless True --max_steps ITERS * rollout_size` runs them, without and with
`--lambda_returns`, and both again with `--normalize_value`; then the same four under `--gae episodic`.  Per run: every score
line; per sampled iteration the mean step reward, the mean return / length of the episodes finished since the previous sample
and the smallest and largest target (reward units; max |target| is the larger magnitude) of the rollout just trained on; the
final score.

    python tools/lambda_returns_curve.py [ITERS (200)] [N (8192)]

Evidence from one seed, not a threshold."""
import contextlib
import io
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import trainer  # noqa: E402
from fly_bproject_amd import options  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402


def run(iters, n, flags):
    T = (options.MINI_BATCH_SIZE // n) * options.CHUNK_NUMBER
    argv = ["--num_envs", str(n), "--headless", "True", "--max_steps", str(iters * T)] + flags
    args = trainer.parse_args(argv)
    args.rank, args.world_size = 0, 1
    torch.manual_seed(args.seed)                            # trainer.main's seeding
    random.seed(args.seed)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        agent = PPO(args)
    assert agent.rollout_size == T
    print("trainer.py %s   (rollout_size=%d gemm=%s step_gemm=%s)" % (" ".join(argv), T, agent.policy.gemm, agent.policy.step_gemm))
    peak = 0.0
    for it in range(iters):
        with contextlib.redirect_stdout(log):
            for _ in range(T):
                agent.run()
        if it % max(1, iters // 20) == 0 or it == iters - 1:
            ret, length, cnt = agent.env.episode_stats(reset=True)
            lo, hi = float(agent._target.min()), float(agent._target.max())
            top = max(-lo, hi)
            peak = max(peak, top)
            print("iter %4d  mean step reward %.4f  finished episodes %7d  mean return %.3f  mean length %.1f  max|target| %.4g  "
                  "(targets in [%.4g, %.4g])" % (it, float(agent.all_reward.mean()), cnt, ret, length, top, lo, hi), flush=True)
    assert agent.run_step == args.max_steps
    with contextlib.redirect_stdout(log):
        agent.flush_log()
    lines = [ln for ln in log.getvalue().splitlines() if ln.startswith("Steps:")]
    print("optimizer steps %d; h2_overflows %d; max|target| over the sampled iterations %.4g" % (agent.optim_step, agent.policy.h2_overflows, peak))
    if agent.normalize_value:
        print("value statistics: count %.0f mean %.4f var %.4f" % (float(agent.value_count), float(agent.value_mean), float(agent.value_var)))
    print("final score: %s" % lines[-1])
    print("score lines:")
    for ln in lines:
        print("  " + ln)
    agent.exit()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    print("python tools/lambda_returns_curve.py %d %d -- one MI355X, one seed; evidence, not a threshold" % (iters, n))
    for gae in ([], ["--gae", "episodic"]):
        for flags in ([], ["--lambda_returns"], ["--normalize_value"], ["--normalize_value", "--lambda_returns"]):
            run(iters, n, gae + flags)
            print()
    # the advantages that go with fast-growing values are large: the same under --normalize_advantage
    for flags in ([], ["--lambda_returns"], ["--normalize_value", "--lambda_returns"]):
        run(iters, n, ["--gae", "episodic", "--normalize_advantage"] + flags)
        print()


if __name__ == "__main__":
    main()
