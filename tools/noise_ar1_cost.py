#!/usr/bin/env python3
"""What temporally correlated exploration noise (PPO action_noise="ar1") costs on the GPU: the filter launch alone on the
rollout's noise buffer (ppo_noise_ar1 over `_eps_all`, T x 18 N floats in place; issue + run); beside it, in the same run and
alternated with it, a plain device copy of the same byte count between two buffers as the yardstick, and the white draw
(`normal_`) it follows; and the whole iteration (rollout + update) with `action_noise` white and ar1 -- the two agents alternated
in the same process, HIP events, warm-up excluded.  Prints one JSON line per env count.

    python tools/noise_ar1_cost.py [reps (20)] [N envs ... (8192)]"""
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
    for mode in ("white", "ar1"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agents[mode] = PPO(make_args(n, action_noise=mode))
        for _ in range(3):                                  # warm-up: three whole iterations each
            iteration(agents[mode])
    it = {"white": [], "ar1": []}
    for r in range(10):                                     # alternated, and the order swapped every round
        for mode in (("white", "ar1") if r % 2 == 0 else ("ar1", "white")):
            it[mode].append(timed(lambda: iteration(agents[mode]), max(1, reps // 4)))
    ag = agents["ar1"]
    T, cols = ag.rollout_size, n * ag.num_acts
    lib = _lib.load()
    eps, carry = ag._eps_all, ag._noise_carry
    twin = torch.empty_like(eps)
    gen = torch.Generator(device=ag.device)
    gen.manual_seed(1)

    def filter_():
        _lib.check(lib.ppo_noise_ar1(C.c_void_p(eps.data_ptr()), C.c_void_p(carry.data_ptr()), C.c_int64(T), C.c_int64(cols),
                                     C.c_float(ag.noise_rho), _lib.stream_ptr()), "ppo_noise_ar1")

    def copy_():
        twin.copy_(eps)

    def draw_():
        eps.normal_(generator=gen)

    def draw_and_filter():                                  # what _draw_noise issues per rollout
        draw_()
        filter_()

    launches = {}
    for r in range(7):                                      # alternated; the first round is the warm-up
        for name, fn in (("ppo_noise_ar1", filter_), ("copy_same_bytes", copy_), ("normal_", draw_),
                         ("normal_then_ppo_noise_ar1", draw_and_filter)):
            t = 1e3 * timed(fn, reps)
            if r:
                launches.setdefault(name, []).append(t)
    med = {k: spread(v)["median"] for k, v in it.items()}
    lm = {k: spread(v)["median"] for k, v in launches.items()}
    nbytes = 4 * T * cols
    out = {"num_envs": n, "rollout_size": T, "columns": cols, "noise_rho": ag.noise_rho, "gemm": ag.policy.gemm, "reps": reps,
           "bytes_read_and_written_per_launch": 2 * nbytes,
           "us_per_launch": {k: spread(v) for k, v in launches.items()},
           "filter_GBps_read_plus_write": round(2 * nbytes / (lm["ppo_noise_ar1"] * 1e3), 1),
           "filter_over_copy": round(lm["ppo_noise_ar1"] / lm["copy_same_bytes"], 3),
           "filter_behind_the_draw_us": round(lm["normal_then_ppo_noise_ar1"] - lm["normal_"], 2),
           "iteration_ms": {k: spread(v) for k, v in it.items()},
           "iteration_delta_us_median": round(1e3 * (med["ar1"] - med["white"]), 2),
           "iteration_white_spread_us": round(1e3 * (max(it["white"]) - min(it["white"])), 2),
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
