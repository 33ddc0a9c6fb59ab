"""What a save costs with and without --save_state: host wall time of PPO.save() at a rollout boundary, the
device idle before it starts, median of --reps, the two forms alternated in one process; and the size of the files.

    python tools/save_state_cost.py                  # 8192 envs, every opt-in on
    python tools/save_state_cost.py --weights_only   # the weights-only save alone (runs on a tree without --save_state too)
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--weights_only", action="store_true")
    opt = ap.parse_args()
    from fly_bproject_amd.ppo import PPO
    tmp = tempfile.mkdtemp(prefix="save_state_cost_")
    args = types.SimpleNamespace(
        sim_device="cuda:0", num_envs=opt.num_envs, headless=True, testing=False, save=True, load=False, record=False,
        save_freq=10 ** 9, save_path=os.path.join(tmp, "s_"), load_path=None, seed=0, rank=0, world_size=1, variant="bigGrav",
        reward="standing", normalize_obs=True, normalize_value=True, normalize_advantage=True, gae="episodic",
        minibatch="shuffled", action_noise="ar1", randomize=True, save_state=False)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(args)
        for _ in range(agent.rollout_size):
            agent.run()
        agent.flush_log()
    forms = [False] if opt.weights_only else [False, True]
    times = {f: [] for f in forms}
    for rep in range(opt.reps + 1):                         # the first round warms the file system and the allocator
        for f in forms:
            args.save_state = f
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.save("t")
            dt = time.perf_counter() - t0
            if rep:
                times[f].append(dt * 1e3)
    for f in forms:
        print("save() %s: median %.2f ms (%s)" % ("with save_state" if f else "weights only   ", statistics.median(times[f]),
                                                   " ".join("%.2f" % t for t in times[f])))
    for name in sorted(os.listdir(tmp)):
        print("%s: %d bytes" % (name, os.path.getsize(os.path.join(tmp, name))))
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)
    agent.exit()


if __name__ == "__main__":
    main()
