#!/usr/bin/env python3
"""What the update diagnostics (PPO --update_stats) show of a training run: ITERS iterations at N envs, seed 0,
as `trainer.py --num_envs N --headless True --update_stats --max_steps ITERS * rollout_size` runs them, once with the defaults
and once with `--lambda_returns --gae episodic` (the configuration DESIGN.md 3.3g reports as not training the standing task).
Per run: per sampled iteration the mean step reward of the rollout beside that update's `last` set (approximate KL, k1, clip
fraction, ratio range, explained variance, the two loss terms, the targets' mean and standard deviation, the largest
|advantage|), the totals of the whole run, and every score line with its suffix.

    python tools/update_stats_curve.py [OUT (profiles/update_stats_curve.txt)] [ITERS (200)] [N (8192)]

An observation from one seed, not a claim about causes."""
import contextlib
import io
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import trainer  # noqa: E402
from fly_bproject_amd import options  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402


def run(say, iters, n, flags):
    T = (options.MINI_BATCH_SIZE // n) * options.CHUNK_NUMBER
    argv = ["--num_envs", str(n), "--headless", "True", "--update_stats", "--max_steps", str(iters * T)] + flags
    args = trainer.parse_args(argv)
    args.rank, args.world_size = 0, 1
    torch.manual_seed(args.seed)                            # trainer.main's seeding
    random.seed(args.seed)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        agent = PPO(args)
    assert agent.rollout_size == T
    say("trainer.py %s   (rollout_size=%d gemm=%s step_gemm=%s)" % (" ".join(argv), T, agent.policy.gemm, agent.policy.step_gemm))
    for it in range(iters):
        with contextlib.redirect_stdout(log):
            for _ in range(T):
                agent.run()
        if it % max(1, iters // 20) == 0 or it == iters - 1:
            e = agent.update_stats()["last"]
            say("iter %4d  mean step reward %8.4f  KL %.5f (k1 %.5f)  clip %5.1f%%  ratio [%.3f, %.3f]  EV %7.3f  policy loss %9.4f  "
                "value loss %8.4f  target %8.3f +- %7.3f  max |A| %8.2f  nonfinite %d"
                % (it, float(agent.all_reward.mean()), e["approx_kl"], e["kl_k1"], 100 * e["clip_fraction"], e["ratio_min"],
                   e["ratio_max"], e["explained_variance"], e["policy_loss"], e["value_loss"], e["target_mean"], e["target_std"],
                   e["adv_absmax"], e["nonfinite"]))
    assert agent.run_step == args.max_steps
    with contextlib.redirect_stdout(log):
        agent.flush_log()
    say("whole run: %s" % ", ".join("%s %.6g" % (k, v) for k, v in agent.update_stats()["total"].items()))
    say("optimizer steps %d; h2_overflows %d" % (agent.optim_step, agent.policy.h2_overflows))
    say("score lines:")
    for ln in log.getvalue().splitlines():
        if ln.startswith("Steps:"):
            say("  " + ln)
    agent.exit()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "update_stats_curve.txt")
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("python tools/update_stats_curve.py -- %d iterations, %d envs, one MI355X, one seed; an observation, not a claim about causes"
        % (iters, n))
    for flags in ([], ["--lambda_returns", "--gae", "episodic"]):
        run(say, iters, n, flags)
        say("")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
