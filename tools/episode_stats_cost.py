#!/usr/bin/env python3
"""The episode-statistics kernels at the two shapes the trainer runs them at, beside `ppo_td_gae` of the same
shape for scale: REPS launches each of ppo_episode_stats (lane = env at 8192 x 80, the scan form at 16 x 40960),
ppo_episode_stats_merge and ppo_td_gae on synthetic rows with an end at one row in 50.  Meant to run under the profiler, which
names and times the kernels:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/episode_stats_cost.py [REPS (50)]

Alone it prints a host-clock figure per launch (a synchronise around REPS launches), which includes the launch overhead."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fly_bproject_amd import _lib  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    lib, dev, p = _lib.load(), "cuda:0", _lib.ptr
    gen = torch.Generator(device=dev).manual_seed(0)
    for n, T, mode in ((8192, 80, 0), (16, 40960, 4)):
        reward = torch.rand((T, n), device=dev, generator=gen) * 4 - 2
        reset = (torch.rand((T, n), device=dev, generator=gen) < 0.02).to(torch.long)
        progress = torch.randint(0, 1200, (T, n), device=dev, generator=gen)
        v = torch.randn((T + 1, n), device=dev, generator=gen)
        done = torch.ones(n, device=dev)
        target, adv = torch.empty((T, n), device=dev), torch.empty((T, n), device=dev)
        carry_ret = torch.zeros(n, dtype=torch.float64, device=dev)
        carry_len = torch.zeros(n, dtype=torch.long, device=dev)
        sets = torch.zeros((_lib.EPISODE_SETS, _lib.EPISODE_SET), dtype=torch.float64, device=dev)
        inf = float("inf")
        window = torch.tensor([0.0, 0.0, 0.0, inf, -inf, 0.0, inf, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
        total = window.clone()

        def stats():
            _lib.check(lib.ppo_episode_stats(p(reward), p(reset), p(progress), 1000, T, n, p(carry_ret), p(carry_len), p(sets), mode,
                                             None), "ppo_episode_stats")

        def merge():
            _lib.check(lib.ppo_episode_stats_merge(p(sets), _lib.EPISODE_SETS, p(window), p(total), None), "ppo_episode_stats_merge")

        def gae():
            _lib.check(lib.ppo_td_gae(p(reward), p(v[:T]), p(v[1:]), p(done), C.c_float(0.99), C.c_float(0.95), T, n, p(target),
                                      p(adv), mode, None), "ppo_td_gae")

        for name, f in (("ppo_episode_stats", stats), ("ppo_episode_stats_merge", merge), ("ppo_td_gae", gae)):
            for _ in range(5):
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            print("%d envs x %d steps, mode %d: %-24s %8.2f us per launch by the host clock (%d launches, launch overhead included)"
                  % (n, T, mode, name, 1e6 * (time.perf_counter() - t0) / reps, reps), flush=True)
        print("  episodes closed per launch: %d" % int((reset != 0).sum()))


if __name__ == "__main__":
    main()
