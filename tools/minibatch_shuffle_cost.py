#!/usr/bin/env python3
"""What shuffled PPO minibatches (PPO minibatch="shuffled") cost on the GPU: the gather launch alone, per minibatch, on a real
rollout (the 15 windows of an epoch, back to back: issue + run); beside it, in the same run and alternated with it, a plain
device copy of the same byte count (the staging set onto a second one) as the yardstick; and the whole iteration (rollout +
update) with `minibatch` reference and shuffled -- the two agents alternated in the same process, HIP events, warm-up excluded.
Prints one JSON line per env count.

    python tools/minibatch_shuffle_cost.py [reps (20)] [N envs ... (8192)]"""
import contextlib
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402

ROW_BYTES = 4 * (73 + 18 + 3)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps       # ms


def iteration(ag):
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(ag.rollout_size):
            ag.run()
        ag.flush_log()


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(sorted(xs)[len(xs) // 2], 4), "max": round(max(xs), 4)}


def measure(n, reps):
    agents = {}
    for mode in ("reference", "shuffled"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agents[mode] = PPO(make_args(n, minibatch=mode))
        for _ in range(3):                                  # warm-up: three whole iterations each
            iteration(agents[mode])
    it = {"reference": [], "shuffled": []}
    for r in range(10):                                     # alternated, and the order swapped every round
        for mode in (("reference", "shuffled") if r % 2 == 0 else ("shuffled", "reference")):
            it[mode].append(timed(lambda: iteration(agents[mode]), max(1, reps // 4)))
    ag = agents["shuffled"]
    T = ag.rollout_size
    rows = ag.mini_chunk_size * n
    data = (ag.all_obs, ag.all_acts, ag.all_log_prob, ag._target, ag.all_advantage)
    twin = [torch.empty_like(x) for x in ag._mb_stage]
    key = [0]

    def gather_epoch():                                     # the 15 windows of one epoch, a new key every time
        key[0] += 1
        for w in range(15):
            ag._gather_minibatch(key[0], w * rows, rows, *data)

    def copy_epoch():
        for _ in range(15):
            for dst, src in zip(twin, ag._mb_stage):
                dst.copy_(src)

    def copy_one_epoch():                                   # the same bytes in ONE copy launch per minibatch
        for _ in range(15):
            flat_b.copy_(flat_a)

    flat_a = torch.zeros(rows * ROW_BYTES // 4, device=ag.device)
    flat_b = torch.empty_like(flat_a)
    launches = {}
    for r in range(7):                                      # alternated; the first round is the warm-up
        for name, fn in (("ppo_minibatch_gather", gather_epoch), ("copy_five_tensors", copy_epoch),
                         ("copy_one_tensor_same_bytes", copy_one_epoch)):
            t = 1e3 * timed(fn, reps) / 15
            if r:
                launches.setdefault(name, []).append(t)
    med = {k: spread(v)["median"] for k, v in it.items()}
    lm = {k: spread(v)["median"] for k, v in launches.items()}
    out = {"num_envs": n, "rollout_size": T, "rows_per_minibatch": rows, "gemm": ag.policy.gemm, "reps": reps,
           "bytes_read_and_written_per_minibatch": 2 * rows * ROW_BYTES,
           "us_per_minibatch": {k: spread(v) for k, v in launches.items()},
           "gather_GBps_read_plus_write": round(2 * rows * ROW_BYTES / (lm["ppo_minibatch_gather"] * 1e3), 1),
           "gather_over_one_copy": round(lm["ppo_minibatch_gather"] / lm["copy_one_tensor_same_bytes"], 3),
           "iteration_ms": {k: spread(v) for k, v in it.items()},
           "iteration_delta_us_median": round(1e3 * (med["shuffled"] - med["reference"]), 2),
           "iteration_delta_us_per_optimizer_step": round(1e3 * (med["shuffled"] - med["reference"]) / 75, 2),
           "iteration_reference_spread_us": round(1e3 * (max(it["reference"]) - min(it["reference"])), 2),
           "h2_overflows": {k: a.policy.h2_overflows for k, a in agents.items()}}
    for a in agents.values():
        a.exit()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    sizes = [int(x) for x in sys.argv[2:]] or [8192]
    for n in sizes:
        print(json.dumps(measure(n, reps)), flush=True)


if __name__ == "__main__":
    main()
