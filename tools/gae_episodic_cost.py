#!/usr/bin/env python3
"""What the episode-aware advantage estimate (PPO gae="episodic") costs on the GPU: its launch against ppo_td_gae in the
reference's mode 0 (an unchanged kernel: tools/kernel_resources.py --isa-digest) on the same rollout, back to back, and the
whole iteration (rollout + update) with `gae` reference and episodic -- the two agents alternated in the same process, HIP
events, warm-up excluded.  Prints one JSON line per env count.

    python tools/gae_episodic_cost.py [reps (20)] [N envs ... (8192)]"""
import contextlib
import ctypes as C
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import make_args  # noqa: E402
from fly_bproject_amd import _lib  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402


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
    for gae in ("reference", "episodic"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agents[gae] = PPO(make_args(n, gae=gae))
        for _ in range(3):                                  # warm-up: three whole iterations each
            iteration(agents[gae])
    it = {"reference": [], "episodic": []}
    for r in range(10):                                     # alternated, and the order swapped every round
        for gae in (("reference", "episodic") if r % 2 == 0 else ("episodic", "reference")):
            it[gae].append(timed(lambda: iteration(agents[gae]), max(1, reps // 4)))
    ag, ref = agents["episodic"], agents["reference"]
    T, lib = ag.rollout_size, ag._lib
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    done = ref.all_done.to(torch.float32).contiguous()

    def gae_reference():
        lib.ppo_td_gae(p(ref.all_reward), p(ref._v_ring[:T]), p(ref._v_ring[1:]), p(done), C.c_float(0.99), C.c_float(0.95),
                       C.c_int64(T), C.c_int64(n), p(ref._target), p(ref.all_advantage), 0, _lib.stream_ptr())

    def gae_episodic():
        lib.ppo_td_gae_episodic(p(ag.all_reward), p(ag._v_ring[:T]), p(ag._v_ring[1:]), p(ag._reset_rows), p(ag._progress_rows),
                                p(ag._ended_prev), C.c_int64(ag.env.max_episode_length), C.c_float(0.99), C.c_float(0.95),
                                C.c_int64(T), C.c_int64(n), p(ag._target), p(ag.all_advantage), 0, _lib.stream_ptr())

    launches = {}
    for r in range(5):                                      # alternated; back to back: issue + run
        for name, fn in (("ppo_td_gae_mode0", gae_reference), ("ppo_td_gae_episodic", gae_episodic)):
            timed(fn, 5)
            launches.setdefault(name, []).append(1e3 * timed(fn, 10 * reps))
    med = {k: spread(v)["median"] for k, v in it.items()}
    out = {"num_envs": n, "rollout_size": T, "gemm": ag.policy.gemm, "reps": reps,
           "launch_us": {k: spread(v) for k, v in launches.items()},
           "bytes_read_per_row": {"ppo_td_gae_mode0": 12, "ppo_td_gae_episodic": 28},
           "bytes_moved": {"ppo_td_gae_mode0": (12 + 8) * T * n + 4 * n, "ppo_td_gae_episodic": (28 + 8) * T * n + 8 * n},
           "iteration_ms": {k: spread(v) for k, v in it.items()},
           "iteration_delta_us_median": round(1e3 * (med["episodic"] - med["reference"]), 2),
           "iteration_reference_spread_us": round(1e3 * (max(it["reference"]) - min(it["reference"])), 2),
           "episodic_launch_share_of_iteration": round(spread(launches["ppo_td_gae_episodic"])["median"] / (1e3 * med["episodic"]), 5),
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
