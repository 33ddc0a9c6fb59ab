#!/usr/bin/env python3
"""What per-env physics domain randomisation (Fly.set_randomization) costs on the GPU: the default one-launch rollout per env
step at 8192 and 16384 envs in three forms -- randomisation off, on with unit ranges (the DR kernels, every multiplier 1), on
with trainer.py's default ranges -- alternated in one process so that the forms see the same clocks.  Prints one JSON line.

    python tools/dr_cost.py [reps (5)] [rounds (5)]"""
import contextlib
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd.fly import DR_DEFAULT_RANGES, DR_NAMES  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402

FORMS = {"off": None, "unit": {n: (1.0, 1.0) for n in DR_NAMES}, "default": DR_DEFAULT_RANGES}


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps       # ms


def measure(n, reps, rounds):
    agents = {}
    for name, ranges in FORMS.items():
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            ag = PPO(make_args(n))
            if ranges is not None:
                ag.env.set_randomization(ranges, seed=1)
            for _ in range(ag.rollout_size):            # one iteration: warm, and an update
                ag.run()
            ag.flush_log()
        agents[name] = ag
    T = agents["off"].rollout_size
    roll = {k: [] for k in FORMS}
    for _ in range(rounds):
        for name in FORMS:
            roll[name].append(timed(agents[name]._launch_rollout, reps))
    best = {k: min(v) for k, v in roll.items()}
    out = {"num_envs": n, "rollout_size": T, "gemm": agents["off"].policy.gemm}
    for k in FORMS:
        out["us_per_env_step_" + k] = round(1e3 * best[k] / T, 3)
    out["unit_over_off"] = round(best["unit"] / best["off"], 4)
    out["default_over_off"] = round(best["default"] / best["off"], 4)
    out["rollout_ms_all_reps"] = {k: [round(x, 4) for x in v] for k, v in roll.items()}
    draws = agents["default"].env.env_param_draws
    out["draws_per_env_mean_default"] = round(float(draws.float().mean()), 2)
    for a in agents.values():
        a.exit()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    print(json.dumps({"forms": list(FORMS), "results": [measure(n, reps, rounds) for n in (8192, 16384)]}))


if __name__ == "__main__":
    main()
