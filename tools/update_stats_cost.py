#!/usr/bin/env python3
"""What the update diagnostics (PPO --update_stats) cost at N envs (default 8192: 80 steps, 655 360 rows), by
HIP events in one process: the probe's three launches one by one (the forward of the updated network over the rollout's rows,
ppo_update_stats, ppo_update_stats_merge), REPS launches each, and one whole update() with the probe and without it,
alternated PAIRS times on the same rollout.  By bytes alone the reduction reads 160 B x rows (a floor, not a prediction); the
forward is rows x 138 112 FLOP.

    python tools/update_stats_cost.py [OUT (profiles/update_stats_cost.txt)] [N (8192)] [REPS (20)] [PAIRS (6)]
"""
import contextlib
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import trainer  # noqa: E402
from fly_bproject_amd import _lib  # noqa: E402
from fly_bproject_amd.ppo import PPO  # noqa: E402

FORWARD_FLOP_PER_ROW = 138112


def event_ms(f, reps):
    """Mean milliseconds of one f() over `reps` calls between two HIP events, after three warm-up calls."""
    for _ in range(3):
        f()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "update_stats_cost.txt")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    pairs = int(sys.argv[4]) if len(sys.argv) > 4 else 6
    args = trainer.parse_args(["--num_envs", str(n), "--headless", "True", "--update_stats"])
    args.rank, args.world_size = 0, 1
    torch.manual_seed(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(args)
        for _ in range(2 * agent.rollout_size):             # two rollouts with their updates: real rows, a trained-on network
            agent.run()
        agent.flush_log()
    T = agent.rollout_size
    rows = T * n
    say("python tools/update_stats_cost.py -- one MI355X, %d envs x %d steps = %d rows, gemm=%s step_gemm=%s; HIP events"
        % (n, T, rows, agent.policy.gemm, agent.policy.step_gemm))
    obs, acts, logp, target, adv = agent.all_obs, agent.all_acts, agent.all_log_prob, agent._target, agent.all_advantage
    api = _lib.update_stats_api()
    stream = _lib.stream_ptr()
    mu, v = agent.policy.forward(obs)
    ms_fwd = event_ms(lambda: agent.policy.forward(obs), reps)
    ms_red = event_ms(lambda: api.ppo_update_stats(mu, acts, logp, adv, v, target, agent._action_var, agent.clip, rows,
                                                   agent._us_sets, stream), reps)
    ms_mrg = event_ms(lambda: api.ppo_update_stats_merge(agent._us_sets, _lib.UPDATE_STATS_SETS, agent._us_last, agent._us_window,
                                                         agent._us_total, stream), reps)
    say("  forward over the rollout's rows (mlp_forward, mu and v)   %9.1f us   %.1f TFLOP/s of its %.1f GFLOP"
        % (1e3 * ms_fwd, rows * FORWARD_FLOP_PER_ROW / (ms_fwd * 1e-3) / 1e12, rows * FORWARD_FLOP_PER_ROW / 1e9))
    say("  ppo_update_stats (256 workgroups, flat 16-byte loads)     %9.1f us   %.2f TB/s of its %.1f MB"
        % (1e3 * ms_red, rows * 160 / (ms_red * 1e-3) / 1e12, rows * 160 / 1e6))
    say("  ppo_update_stats_merge (one workgroup, 256 sets)          %9.1f us" % (1e3 * ms_mrg))
    # one whole update() on the same rollout, the probe on and off in turn
    with contextlib.redirect_stdout(io.StringIO()):
        agent.prepare()
    on, off = [], []
    for k in range(pairs + 1):
        for flag, acc in ((True, on), (False, off)):
            agent._update_stats = flag
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            agent.update()
            b.record()
            b.synchronize()
            if k:                                           # the first pair warms up
                acc.append(a.elapsed_time(b))
    agent._update_stats = True
    m_on, m_off = sum(on) / len(on), sum(off) / len(off)
    say("  update() with the probe    %s  ms   mean %.3f" % (" ".join("%.3f" % x for x in on), m_on))
    say("  update() without it        %s  ms   mean %.3f" % (" ".join("%.3f" % x for x in off), m_off))
    say("  the probe adds %.3f ms to an update of %.3f ms: %.1f%% (the rollout that goes with an update is not in these figures)"
        % (m_on - m_off, m_off, 100.0 * (m_on - m_off) / m_off))
    with contextlib.redirect_stdout(io.StringIO()):
        agent.exit()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
