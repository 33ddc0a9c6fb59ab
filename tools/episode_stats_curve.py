#!/usr/bin/env python3
"""What the episode statistics (PPO --episode_stats) show of a training run: ITERS iterations at N envs, seed 0,
as `trainer.py --num_envs N --headless True --episode_stats --max_steps ITERS * rollout_size` runs them, without and with
`--gae episodic`.  Per run: per sampled iteration the mean step reward of the rollout beside the episodes closed since the
previous sample (count, mean / min / max return, mean length, share of time-outs; the difference of two `total` sets), the
totals of the whole run, and every score line with its suffix.

    python tools/episode_stats_curve.py [ITERS (200)] [N (8192)]

An observation from one seed, not a claim of improvement."""
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
    argv = ["--num_envs", str(n), "--headless", "True", "--episode_stats", "--max_steps", str(iters * T)] + flags
    args = trainer.parse_args(argv)
    args.rank, args.world_size = 0, 1
    torch.manual_seed(args.seed)                            # trainer.main's seeding
    random.seed(args.seed)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        agent = PPO(args)
    assert agent.rollout_size == T
    print("trainer.py %s   (rollout_size=%d gemm=%s step_gemm=%s)" % (" ".join(argv), T, agent.policy.gemm, agent.policy.step_gemm))
    seen = dict(episodes=0, ret=0.0, length=0.0, timeouts=0)
    for it in range(iters):
        with contextlib.redirect_stdout(log):
            for _ in range(T):
                agent.run()
        if it % max(1, iters // 20) == 0 or it == iters - 1:
            tot = agent.episode_stats()["total"]
            k = tot["episodes"] - seen["episodes"]
            ret = tot["return_mean"] * tot["episodes"] if tot["episodes"] else 0.0
            length = tot["length_mean"] * tot["episodes"] if tot["episodes"] else 0.0
            if k:
                since = "episodes %7d  mean return %9.3f  mean length %7.1f  timeouts %5.1f%%" % (
                    k, (ret - seen["ret"]) / k, (length - seen["length"]) / k, 100.0 * (tot["timeouts"] - seen["timeouts"]) / k)
            else:
                since = "episodes %7d" % 0
            print("iter %4d  mean step reward %.4f  since the previous sample: %s" % (it, float(agent.all_reward.mean()), since), flush=True)
            seen = dict(episodes=tot["episodes"], ret=ret, length=length, timeouts=tot["timeouts"])
    assert agent.run_step == args.max_steps
    with contextlib.redirect_stdout(log):
        agent.flush_log()
    tot = agent.episode_stats()["total"]
    print("whole run: %s" % ", ".join("%s %.6g" % (k, v) for k, v in tot.items()))
    print("optimizer steps %d; h2_overflows %d" % (agent.optim_step, agent.policy.h2_overflows))
    lines = [ln for ln in log.getvalue().splitlines() if ln.startswith("Steps:")]
    print("score lines:")
    for ln in lines:
        print("  " + ln)
    agent.exit()


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    print("python tools/episode_stats_curve.py %d %d -- one MI355X, one seed; an observation, not a claim of improvement" % (iters, n))
    for flags in ([], ["--gae", "episodic"]):
        run(iters, n, flags)
        print()


if __name__ == "__main__":
    main()
