"""The float64 reference of the DQN training loop (`DQN.run()` / `DQN.update()`; reference UselessFiles/dqn.py:64-126) on the
replay ring's own rows.  CPU only, numpy float64, no HIP; tests/test_dqn_loop_ref_cpu.py holds it to torch, the GPU test
tests/test_dqn_loop_gpu.py holds the loop to it.

Three parts:
  * the batch an update trains on: the sampled ring slots' rows, concatenated in slot order (`batch`, `chunks`);
  * the update on that batch: Huber-TD loss and its gradient, written out layer by layer (`loss_and_grad`), with the count of
    (row, unit) pairs next to LeakyReLU's kink (`kink_pairs`: the margin of tests/test_dqn_h2_gpu.py::_kink_reference);
    the optimizer is tests/adam_ref.dqn_adam_soft;
  * the loop around it: what every `run()` must leave in the ring, bit for bit, given what the env, `act` and the sampler did
    (`check_transcript`), and the eps-greedy action of the float64 Q values with the rows that any fp32 arithmetic may decide
    either way left out (`expected_actions`).

A transcript is a dict {"capacity", "mini_batch_size", "steps": [record, ...]}; record t (1-based, the loop's `run_step`) holds
numpy arrays of what the loop saw and left:
    run_step, eps                         the step counter in front of the step and the epsilon `act` was passed
    obs_before                            the env's observation in front of the step
    act_obs, coin, rand, action           what `act` was given, the two draws it left, what it returned
    step_obs, step_reward, step_reset     the env's buffers as the step left them, BEFORE the reset
    row                                   (obs, action, reward, next_obs, done): ring slot (t - 1) % capacity after the step
    head, count, size                     of the ring after the step
    slot_lists                            the slot lists the sampler returned to this step's own update (none, or one)
    ring_before_update                    optional: the whole ring in front of this step's update, {field: [capacity, N, ...]}
"""
import numpy as np

from tests import dqn_head_ref as HR

F = np.float32
NACT = HR.NACT
KINK_K = 32                 # the GEMM term of the ambiguity margins: the constant of tests/test_dqn_h2_gpu.py (asserted equal there)
FIELDS = ("obs", "action", "reward", "next_obs", "done")
DISCOUNT = 0.99


def epsilon(run_step):
    """dqn.py:104."""
    return max(0.01, 0.8 - 0.01 * (run_step / 20))


# ---------------------------------------------------------------------------------------------------------------------
# the batch
def chunks(ring, slots):
    """One `(obs, action, reward, next_obs, done)` row block per sampled slot, in slot order (numpy arrays or tensors)."""
    return [tuple(ring[k][int(s)] for k in FIELDS) for s in slots]


def batch(ring, slots):
    """The update's batch: the slots' rows concatenated in slot order.  -> (obs, act, rew, nxt, done) numpy arrays."""
    cs = chunks(ring, slots)
    return tuple(np.concatenate([np.asarray(c[i]) for c in cs]) for i in range(5))


# ---------------------------------------------------------------------------------------------------------------------
# the update
def _leaky(z):
    s = np.where(z > 0, 1.0, 0.01)
    return z * s, s


def loss_and_grad(w, wt, b, discount=DISCOUNT):
    """Huber-TD loss (mean over the batch) and its gradient [dW1, db1, dW2, db2, dW3, db3] in float64 on the fp32 weights
    `w` (online) and `wt` (target), each (W1, b1, W2, b2, W3, b3) in torch's [out, in] layout.  LeakyReLU' from the sign of
    the float64 pre-activation (1 for z > 0, 0.01 otherwise: torch's rule).  Also returns the intermediates."""
    obs, act, rew, nxt, done = b
    W1, b1, W2, b2, W3, b3 = (np.asarray(a, np.float64) for a in w)
    x = np.asarray(obs, np.float64)
    z1 = x @ W1.T + b1
    a1, s1 = _leaky(z1)
    z2 = a1 @ W2.T + b2
    a2, s2 = _leaky(z2)
    Q = a2 @ W3.T + b3
    Qn, _ = HR.forward64(wt, nxt)
    h = HR.head(Q, Qn, act, rew, done, discount=discount, H2=a2)
    dA2 = h["dZ3"] @ W3[:NACT]
    dZ2 = dA2 * s2
    dA1 = dZ2 @ W2
    dZ1 = dA1 * s1
    grads = [dZ1.T @ x, dZ1.sum(0), dZ2.T @ a1, dZ2.sum(0), h["dW3"], h["db3"]]
    return h["loss"], grads, dict(x=x, z1=z1, z2=z2, a1=a1, a2=a2, Q=Q, Qn=Qn, dA1=dA1, dA2=dA2, head=h)


def kink_pairs(w, mid, s_h1=2.0 ** 40, s_h2=2.0 ** 40):
    """(ambiguous, all) (row, unit) pairs of the two hidden layers under the margin of _kink_reference:
    |z64| <= max(KINK_K 2^-24 (sum |x| |w| + |b|), 2^-25 / s_H, 2^-25 / (0.01 s_H)).  The default scales make the sign-loss
    term vanish (bf16x3 and the per-step path have no scales): only the GEMM term is left."""
    W1, b1, W2, b2 = (np.abs(np.asarray(a, np.float64)) for a in w[:4])
    g = 2.0 ** -24 * KINK_K
    m1 = np.maximum(g * (np.abs(mid["x"]) @ W1.T + b1), 2.0 ** -25 / (0.01 * s_h1))
    m2 = np.maximum(g * (np.abs(mid["a1"]) @ W2.T + b2), 2.0 ** -25 / (0.01 * s_h2))
    return int((np.abs(mid["z1"]) <= m1).sum() + (np.abs(mid["z2"]) <= m2).sum()), mid["z1"].size + mid["z2"].size


# ---------------------------------------------------------------------------------------------------------------------
# the action
def expected_actions(w, obs, coin, rand, eps):
    """The eps-greedy action of the float64 Q values of `obs` under the fp32 weights `w`, with the recorded draws.
    -> (action fp32 [n], left_out bool [n], {"tie": rows, "edge": rows}).

    Left out are the rows any fp32 arithmetic may decide either way:
      tie    greedy rows (coin >= eps) whose float64 maximum is not clear of another column: Q[top] - Q[j] <= m[top] + m[j]
             with m = KINK_K 2^-24 (sum |a2| |w3| + |b3|), the forward's own rounding as _kink_reference takes it;
      edge   rows whose coin is within one fp32 ulp of fp32(eps).
    Rows on the random branch (coin < eps, strict, in fp32) are held exactly whatever their Q values."""
    Q, a2 = HR.forward64(w, obs)
    W3, b3 = np.abs(np.asarray(w[4], np.float64)), np.abs(np.asarray(w[5], np.float64))
    m = 2.0 ** -24 * KINK_K * (np.abs(a2) @ W3.T + b3)
    rows = np.arange(Q.shape[0])
    top = HR.first_argmax(Q, NACT)
    close = (Q[rows, top][:, None] - Q) <= (m[rows, top][:, None] + m)
    close[rows, top] = False
    coin = np.asarray(coin, F)
    e = F(eps)
    edge = np.abs(coin.astype(np.float64) - float(e)) <= float(np.spacing(e))
    explore = coin < e
    tie = close.any(1) & ~explore
    want = HR.eps_greedy(Q, coin, rand, eps, NACT)
    return want, tie | edge, {"tie": int(tie.sum()), "edge": int(edge.sum()), "explore": int(explore.sum())}


# ---------------------------------------------------------------------------------------------------------------------
# the loop
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_transcript(tr, reset_rewrites_obs=False):
    """Every rule `DQN.run()` must keep, bit for bit (module docstring for the record's fields).  Raises AssertionError naming
    the rule and the step; returns {"reset_envs", "done0_rows", "updates"}.

    `reset_rewrites_obs`: whether the env's reset repacks the observations of the envs it resets.  `Fly`'s does not -- nor does the
    reference's (fly.py:446-480 restores the simulation state only; the oracle's `reset_masked` takes no observation buffer): the
    observation a step starts from is the one the previous step left, for EVERY env, and the new episode's first own observation
    is packed by the next step.  An env whose reset does repack them must differ there on exactly the envs that reset."""
    cap, mbs = int(tr["capacity"]), int(tr["mini_batch_size"])
    assert cap > mbs, "the ring must hold more steps than an update samples"
    steps = tr["steps"]
    last_writer = {}
    reset_envs = done0 = updates = 0
    for i, r in enumerate(steps):
        t = i + 1
        h = (t - 1) % cap
        tag = "step %d (slot %d): " % (t, h)
        assert int(r["run_step"]) == t, tag + "run_step"
        assert float(r["eps"]) == epsilon(t), tag + "epsilon is max(0.01, 0.8 - 0.01 run_step / 20)"
        obs, action, reward, next_obs, done = r["row"]
        assert _same(obs, r["obs_before"]), tag + "obs[h] is the env's observation in front of the step"
        assert _same(r["act_obs"], r["obs_before"]), tag + "act sees the env's observation in front of the step"
        assert _same(action, r["action"]), tag + "action[h] is what act returned"
        assert _same(reward, r["step_reward"]), tag + "reward[h] is what the step left"
        assert _same(next_obs, r["step_obs"]), tag + "next_obs[h] is what the step left, before the reset"
        want_done = (1.0 - np.asarray(r["step_reset"]).astype(np.float64)).astype(F)
        assert _same(done, want_done), tag + "done[h] == 1 - reset_buf of the step, before the reset clears it"
        assert int(r["head"]) == t % cap, tag + "head follows commit()"
        assert int(r["count"]) == min(t, cap) == int(r["size"]), tag + "count / size() follow commit()"
        last_writer[h] = i
        flagged = np.asarray(r["step_reset"]) != 0
        done0 += int(flagged.sum())
        if i + 1 < len(steps):
            nxt = np.asarray(steps[i + 1]["obs_before"])
            carried = (nxt == np.asarray(r["step_obs"])).all(1) & ~np.isnan(nxt).any(1)
            assert carried[~flagged].all(), tag + "an env that did not reset starts the next step from this step's next_obs"
            if reset_rewrites_obs:
                assert not carried[flagged].any(), tag + "an env that reset starts the next step from its reset observation"
            else:
                assert carried[flagged].all(), tag + "the reset leaves the observation buffer alone: next_obs carries over for every env"
            reset_envs += int(flagged.sum())
        lists = r["slot_lists"]
        if int(r["count"]) > mbs:
            assert len(lists) == 1, tag + "one update per step once size() > mini_batch_size"
            s = [int(x) for x in lists[0]]
            assert len(s) == mbs and len(set(s)) == mbs and all(0 <= x < int(r["count"]) for x in s), \
                tag + "a slot list has mini_batch_size distinct entries below count"
            updates += 1
            ring = r.get("ring_before_update")
            if ring is not None:
                for slot, j in last_writer.items():
                    for k, want in zip(FIELDS, steps[j]["row"]):
                        assert _same(ring[k][slot], want), tag + "slot %d in front of the update is what step %d left (%s)" % (slot, j + 1, k)
        else:
            assert len(lists) == 0, tag + "no update before size() > mini_batch_size"
    assert reset_envs > 0, "no env reset during the transcript: the reset rules were not exercised"
    return {"reset_envs": reset_envs, "done0_rows": done0, "updates": updates}
