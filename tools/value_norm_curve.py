#!/usr/bin/env python3
"""What value normalisation (PPO normalize_value) does to training: ITERS iterations at N envs, seed 0, with the flag off and
on.  Per run: every score line; per sampled iteration the largest |critic output| and |regression target| the update saw (in
the units the critic works in), the largest raw target, and the running statistics; at the end the critic's explained variance
on the last rollout (in reward units) and the number of updates in which an fp16x2 step was refused (`policy.h2_overflows`).

    python tools/value_norm_curve.py [ITERS (200)] [N (8192)]

Evidence from one seed, not a threshold."""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402


def run(iters, n, on):
    torch.manual_seed(0)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        agent = PPO(make_args(n, normalize_value=on))
    T = agent.rollout_size
    print("normalize_value=%s  num_envs=%d  rollout_size=%d  gemm=%s step_gemm=%s" % (on, n, T, agent.policy.gemm,
                                                                                      agent.policy.step_gemm))
    max_v = max_y = max_tg = 0.0
    for it in range(iters):
        with contextlib.redirect_stdout(log):
            for _ in range(T):
                agent.run()
        # what the update of this iteration saw: the value ring and the targets are still in place
        seen = agent._target_norm if on else agent._target
        av, ay, atg = float(agent._v_ring.abs().max()), float(seen.abs().max()), float(agent._target.abs().max())
        max_v, max_y, max_tg = max(max_v, av), max(max_y, ay), max(max_tg, atg)
        if it % max(1, iters // 20) == 0 or it == iters - 1:
            stats = "  S_v count %.0f mean %.4f var %.4f" % tuple(float(x) for x in agent._value_stats) if on else ""
            print("iter %4d  mean step reward %.4f  max|critic output| %.4g  max|target seen| %.4g  max|raw target| %.4g%s"
                  % (it, float(agent.all_reward.mean()), av, ay, atg, stats), flush=True)
    with contextlib.redirect_stdout(log):
        agent.flush_log()
    with torch.no_grad():
        tg = agent._target[..., 0].double()
        vd = agent.denormalize_value(agent._v_ring[:T, :, 0]).double()
        # the ring was denormalised under the table committed BEFORE the last update; denormalize_value uses the one after it
        ev = 1.0 - float((tg - vd).var() / tg.var())
    print("over the run: max|critic output| %.4g  max|target seen by the update| %.4g  max|raw target| %.4g"
          % (max_v, max_y, max_tg))
    print("explained variance of the critic on the last rollout (reward units, committed table): %.4f" % ev)
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
    for on in (False, True):
        run(iters, n, on)
        print()


if __name__ == "__main__":
    main()
