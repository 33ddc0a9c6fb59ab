#!/usr/bin/env python3
"""What value normalisation (PPO normalize_value) costs on the GPU: make_data() + the commit with the flag off and on, the three
new launches one by one against today's GAE launch, and the whole iteration (rollout + update) both ways -- the two agents
alternated in the same process, HIP events, warm-up excluded.  Prints one JSON line per env count.

    python tools/value_norm_cost.py [reps (20)] [N envs ... (8192 16384)]

The reference is the flag-off path of the same build: it launches what the code launched before the flag existed."""
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


def make_data_and_commit(ag):
    # as inside a training iteration: the rollout left v(obs_t) in the value ring, make_data evaluates the last row only
    ag._v_have, ag._v_version = ag.rollout_size, ag.policy.version
    ag.make_data()
    if ag.normalize_value:
        ag._commit_value_stats()


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(sorted(xs)[len(xs) // 2], 4), "max": round(max(xs), 4)}


def measure(n, reps):
    agents = {}
    for on in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agents[on] = PPO(make_args(n, normalize_value=on))
        for _ in range(3):                                  # warm-up: three whole iterations each
            iteration(agents[on])
    T = agents[True].rollout_size
    md, it = {False: [], True: []}, {False: [], True: []}
    for r in range(10):                                     # alternated, and the order swapped every round
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            md[on].append(timed(lambda: make_data_and_commit(agents[on]), reps))
    for r in range(10):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            it[on].append(timed(lambda: iteration(agents[on]), max(1, reps // 4)))
    ag, off = agents[True], agents[False]
    lib = ag._lib
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    done = ag.all_done.to(torch.float32).contiguous()
    v = ag._v_ring

    def gae_plain():
        lib.ppo_td_gae(p(off.all_reward), p(off._v_ring[:T]), p(off._v_ring[1:]), p(done), C.c_float(0.99), C.c_float(0.95),
                       C.c_int64(T), C.c_int64(n), p(off._target), p(off.all_advantage), 0, _lib.stream_ptr())

    def gae_vnorm():
        lib.ppo_td_gae_vnorm(p(ag.all_reward), p(v[:T]), p(v[1:]), p(done), p(ag._value_table), C.c_float(0.99), C.c_float(0.95),
                             C.c_int64(T), C.c_int64(n), p(ag._target), p(ag.all_advantage), p(ag._value_sets), 0,
                             _lib.stream_ptr())

    def merge():
        lib.ppo_value_norm_merge(p(ag._value_stats), p(ag._value_sets), C.c_int64(_lib.VALUE_NORM_SETS), p(ag._value_stats_next),
                                 p(ag._value_table_next), _lib.stream_ptr())

    def apply():
        lib.ppo_value_norm_apply(p(ag._target), C.c_int64(T * n), p(ag._value_table_next), p(ag._target_norm), _lib.stream_ptr())

    launches = {}
    for name, fn in (("ppo_td_gae", gae_plain), ("ppo_td_gae_vnorm", gae_vnorm), ("ppo_value_norm_merge", merge),
                     ("ppo_value_norm_apply", apply)):
        timed(fn, 5)
        launches[name + "_us"] = round(1e3 * min(timed(fn, reps) for _ in range(5)), 2)     # back to back: issue + run
    out = {"num_envs": n, "rollout_size": T, "gemm": ag.policy.gemm, "reps": reps,
           "make_data_commit_ms": {"off": spread(md[False]), "on": spread(md[True])},
           "make_data_commit_delta_us_median": round(1e3 * (spread(md[True])["median"] - spread(md[False])["median"]), 2),
           "iteration_ms": {"off": spread(it[False]), "on": spread(it[True])},
           "iteration_delta_us_median": round(1e3 * (spread(it[True])["median"] - spread(it[False])["median"]), 2),
           "iteration_off_spread_us": round(1e3 * (max(it[False]) - min(it[False])), 2),
           "launches": launches, "bytes_touched_by_the_new_launches": (5 + 2) * T * n * 4,
           "h2_overflows": {"off": off.policy.h2_overflows, "on": ag.policy.h2_overflows}}
    for a in agents.values():
        a.exit()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    sizes = [int(x) for x in sys.argv[2:]] or [8192, 16384]
    for n in sizes:
        print(json.dumps(measure(n, reps)), flush=True)


if __name__ == "__main__":
    main()
