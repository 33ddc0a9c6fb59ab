#!/usr/bin/env python3
"""What observation normalisation (PPO normalize_obs) costs on the GPU: the statistics pass and the merge per update, and the
one-launch rollout with its NORM instantiation against the plain one, alternated in the same process.  Prints one JSON line.

    python tools/obs_norm_cost.py [N envs (8192)] [reps (20)]

HBM roofline of the pass: it reads the raw ring [T+1][N][73] and writes the normalised copy, 2 x (T+1) N 73 x 4 bytes."""
import contextlib
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402

HBM_TBS = 8.0       # MI355X HBM3E peak, TB/s


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps       # ms


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    agents = {}
    for norm in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            ag = PPO(make_args(n, normalize_obs=norm))
            for _ in range(ag.rollout_size):            # one iteration: warm, statistics merged once
                ag.run()
            ag.flush_log()
        agents[norm] = ag
    T = agents[True].rollout_size
    roll = {False: [], True: []}
    for _ in range(5):                                  # alternated: the two forms see the same clocks
        for norm in (False, True):
            roll[norm].append(timed(agents[norm]._launch_rollout, max(1, reps // 5)))
    ag = agents[True]
    pass_ms = timed(ag._obs_norm_pass, reps)
    merge_ms = timed(ag._merge_obs_stats, reps)
    nbytes = 2 * (T + 1) * n * 73 * 4
    plain, normed = min(roll[False]), min(roll[True])
    out = {"num_envs": n, "rollout_size": T, "gemm": ag.policy.gemm,
           "rollout_ms_plain": round(plain, 4), "rollout_ms_norm": round(normed, 4),
           "us_per_env_step_plain": round(1e3 * plain / T, 3), "us_per_env_step_norm": round(1e3 * normed / T, 3),
           "norm_over_plain": round(normed / plain, 4),
           "rollout_ms_all_reps": {"plain": [round(x, 4) for x in roll[False]], "norm": [round(x, 4) for x in roll[True]]},
           "pass_ms": round(pass_ms, 4), "pass_bytes": nbytes, "pass_TBps": round(nbytes / pass_ms / 1e9, 3),
           "pass_roofline_ms": round(nbytes / (HBM_TBS * 1e12) * 1e3, 4), "merge_ms": round(merge_ms, 4)}
    for a in agents.values():
        a.exit()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
