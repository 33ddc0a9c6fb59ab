"""Synthetic rollout sequences for the make_data chain (tests/make_data_ref.py): what three consecutive rollouts leave before
make_data, with the properties the real ones have and that a wiring mistake needs in order to show.

  * rewards of non-unit scale (mean about 3, std about 2) that drift from rollout to rollout (mean + 2.5 k, scale x 1.6^k):
    the return statistics move, so a stale S_r, table or carry is a different number;
  * critic outputs in normalised units (unit scale, correlated along time), drawn anew per rollout;
  * an episode process as the env's: an env whose flag is up performs its reset in the next step (progress 1 behind it), the
    flag rises at progress max_episode_length - 1 = 36 (a time-out) or at a fall; reset_buf = 1 everywhere at the very start.
    Envs 0 and 1 never fall, env 2 falls in the LAST row of every rollout, env 3 in the FIRST row of every rollout, the rest
    fall with a per-env probability of up to 6 % per step -- so episodes straddle both rollout boundaries, some end exactly at
    them, and T = 160 is no multiple of 36;
  * a raw observation ring whose columns have their own offsets and scales and drift too; row 0 of rollout k + 1 is row T of
    rollout k, as in the agent's ring.
Everything is float32 / int64 as the agent holds it; one numpy Generator per (shape, seed, rank)."""
import numpy as np

from tests import make_data_ref as M

SHAPES = [(160, 64), (2176, 12)]
MAXLEN = 37
K = 73

ALL_ON = dict(normalize_reward=True, normalize_obs=True, normalize_value=True, lambda_returns=True, normalize_advantage=True,
              gae="episodic", minibatch="shuffled")


def sequence(T, N, iterations=3, seed=0, rank=0):
    """[raw] of `iterations` consecutive rollouts of one rank (tests/make_data_ref.py's `raw`)."""
    rng = np.random.default_rng([seed, T, N, rank])
    p_fall = np.where(np.arange(N) < 4, 0.0, rng.uniform(0.0, 0.06, N))
    col_off, col_scale = rng.normal(0, 3, K), np.exp(rng.uniform(-2, 2, K))
    flag = np.ones(N, np.int64)                                  # reset_buf = 1 everywhere at the very start
    progress = np.zeros(N, np.int64)
    last_row = None
    out = []
    for k in range(iterations):
        reset_start = flag.copy()
        reset, prog = np.zeros((T, N), np.int64), np.zeros((T, N), np.int64)
        fell = np.zeros((T, N), bool)
        for t in range(T):
            progress = np.where(flag != 0, 0, progress) + 1
            fall = rng.random(N) < p_fall
            if N > 3:
                fall[2] = t == T - 1
                fall[3] = t == 0
            flag = ((progress >= MAXLEN - 1) | fall).astype(np.int64)
            reset[t], prog[t], fell[t] = flag, progress, fall & (progress < MAXLEN - 1)
        scale = 1.6 ** k
        reward = 3.0 + 2.5 * k + 2.0 * scale * rng.standard_normal((T, N)) - 4.0 * scale * fell
        z = rng.standard_normal((T + 1, N))
        values = np.empty((T + 1, N))
        values[0] = z[0]
        for t in range(1, T + 1):
            values[t] = 0.9 * values[t - 1] + np.sqrt(1 - 0.81) * z[t]
        values += 0.3 * k
        ring = (col_off + 0.5 * k + col_scale * (1.0 + 0.2 * k) * rng.standard_normal((T + 1, N, K))).astype(np.float32)
        if last_row is not None:
            ring[0] = last_row
        last_row = ring[T].copy()
        out.append({"ring": ring, "reward": reward.astype(np.float32), "values": values.astype(np.float32),
                    "reset": reset, "progress": prog, "reset_start": reset_start,
                    "done": (1 - reset[T - 1]).astype(np.float32)})
    return out


def run(chain, seq):
    """The chain over the whole sequence, committing behind every iteration: -> [out]."""
    outs = []
    for raw in seq:
        outs.append(chain.step(raw))
        chain.commit()
    return outs


def chains(options, T, N, **kw):
    """(chain64, chain32) of the same options."""
    return M.Chain(options, T, N, MAXLEN, precision="64", **kw), M.Chain(options, T, N, MAXLEN, precision="32", **kw)


def pose_as_agent(chain, seq, mb_seed=0):
    """The iterations tests/make_data_capture.py captures on a live agent, made by a float32 `chain` (one rank) instead: what
    the GPU checks are themselves checked with, on a right chain and on wrongly wired ones."""
    from tests import minibatch_ref as MB
    T, N, opt = chain.T, chain.N, chain.opt
    rows = (T // 16) * N
    rng = np.random.default_rng(5)

    def state():
        s = chain.state()
        out = {k: np.asarray(v).copy() for k, v in s.items() if k not in ("carry", "ended_prev", "update")}
        if "carry" in s:
            out["carry"] = s["carry"][0].copy()
        if opt["minibatch"] == "shuffled":
            out["update"] = s["update"]
        if opt["gae"] == "episodic" and s["ended_prev"][0] is not None:
            out["ended_prev"] = s["ended_prev"][0].copy()
        return out

    its = []
    for k, raw in enumerate(seq):
        before = state()
        before.setdefault("ended_prev", raw["reset_start"].copy())
        o = chain.step(raw)
        if chain.wiring["ended_prev"] == "stale":
            before["ended_prev"] = o["ended_prev"].copy()
        acts = rng.standard_normal((T, N, 18)).astype(np.float32)
        logp = rng.standard_normal((T, N)).astype(np.float32)
        returned = [np.asarray(o["obs"]), acts, logp, np.asarray(o["target"])[..., None], np.asarray(o["advantage"])[..., None]]
        sc = {"target": o["target_raw"], "advantage_raw": o["advantage_raw"]}
        if opt["normalize_reward"]:
            sc.update(scaled=o["reward_scaled"], S_r_next=o["S_r_next"], rnorm_table_next=o["rnorm_table_next"],
                      carry_next=o["carry_next"])
        if opt["normalize_obs"]:
            sc["obs_norm"] = o["obs_norm"]
        if opt["normalize_value"]:
            n, mean, var = o["value_moments"]
            sc.update(target_norm=o["target_norm"], S_v_next=o["S_v_next"], value_table_next=o["value_table_next"],
                      value_sets=np.array([[n, mean, var * n], [0.0, 0.0, 0.0]]))
        steps = {}
        if k in (0, 2):
            flat = (returned[0].reshape(T * N, -1), acts.reshape(T * N, -1), logp.reshape(-1), returned[4].reshape(-1),
                    returned[3].reshape(-1))
            for step in (0, 14, 15, 74):
                epoch, window = divmod(step, 15)
                if opt["minibatch"] == "shuffled":
                    steps[step] = MB.gather_ref(*flat, mb_seed, int(o["epoch_keys"][epoch]), window * rows, rows)[0]
                else:
                    mc = T // 16
                    steps[step] = [x[window * mc * N:(window + 1) * mc * N] for x in flat]
        chain.commit()
        its.append({"before": before, "raw": raw, "returned": returned, "scratch": sc, "after": state(), "steps": steps})
    info = {"T": T, "N": N, "scan": False, "reward_clip": chain.reward_clip, "obs_clip": chain.obs_clip, "mb_seed": mb_seed,
            "mb_rows": rows, "mini_chunk": T // 16, "options": {k: opt[k] for k in M.OPTIONS}}
    return info, its
