#!/usr/bin/env python3
"""The reward-scaling kernels at the two shapes the trainer runs them at, beside `ppo_td_gae` of the same shape
for scale: REPS launches each of ppo_reward_returns in BOTH forms (lane = env and the scan), ppo_value_norm_merge over its sets,
ppo_reward_scale and ppo_td_gae, at 8192 x 80 and 16 x 40960, on synthetic rows with an end at one row in 50.  Meant to run
under the profiler, which names and times the kernels:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/reward_norm_cost.py [REPS (50)]

Alone it prints a host-clock figure per launch (a synchronise around REPS launches), which includes the launch overhead."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fly_bproject_amd import _lib  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    api, ext, dev = _lib.api(), _lib.ext(), "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    for n, T, gae_mode in ((8192, 80, 0), (16, 40960, 4)):
        reward = torch.rand((T, n), device=dev, generator=gen) * 4 - 2
        reset = (torch.rand((T, n), device=dev, generator=gen) < 0.02).to(torch.long)
        v = torch.randn((T + 1, n), device=dev, generator=gen)
        done = torch.ones(n, device=dev)
        target, adv, scaled = (torch.empty((T, n), device=dev) for _ in range(3))
        carry, carry_next = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(2))
        sets = torch.zeros((_lib.VALUE_NORM_SETS, _lib.VALUE_NORM_SET), dtype=torch.float64, device=dev)
        stats = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
        stats_next, table = torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(4, device=dev)

        def returns(mode):
            return lambda: ext.ppo_reward_returns(reward, reset, 0.99, T, n, carry, carry_next, sets, mode, None)

        def merge():
            api.ppo_value_norm_merge(stats, sets, _lib.VALUE_NORM_SETS, stats_next, table, None)

        def scale():
            ext.ppo_reward_scale(reward, T * n, table, 10.0, scaled, None)

        def gae():
            api.ppo_td_gae(reward, v[:T], v[1:], done, 0.99, 0.95, T, n, target, adv, gae_mode, None)

        for name, f in (("ppo_reward_returns (lane = env)", returns(0)), ("ppo_reward_returns (scan)", returns(4)),
                        ("ppo_value_norm_merge", merge), ("ppo_reward_scale", scale), ("ppo_td_gae", gae)):
            for _ in range(5):
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            print("%d envs x %d steps: %-32s %8.2f us per launch by the host clock (%d launches, launch overhead included)"
                  % (n, T, name, 1e6 * (time.perf_counter() - t0) / reps, reps), flush=True)
        print("  running scale after the launches: r = %.6g" % float(table[2]))


if __name__ == "__main__":
    main()
