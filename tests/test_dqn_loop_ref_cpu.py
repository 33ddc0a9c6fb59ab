"""CPU: tests/dqn_loop_ref.py, the float64 reference of the DQN training loop, held to torch and to a plain Python loop -- so that
what tests/test_dqn_loop_gpu.py holds `DQN.run()` / `DQN.update()` to is itself pinned where there is no GPU.

  * the explicit float64 gradient is torch autograd's (float64) on a batch assembled from a synthetic ring that has wrapped;
  * tests/adam_ref.dqn_adam_soft over ten chained updates is torch.optim.Adam + the product's own `soft_update` in float64;
  * the slot-to-batch assembly honours slot order and wrap;
  * the ring-transcript checker accepts the transcript of a plain Python loop over a stub env with `ReplayBuffer(device="cpu")`
    and rejects each of the three corruptions the loop could suffer without a weight turning non-finite;
  * the exclusion caps of the GPU test are reachable: on observation-like rows the eps-greedy tie margin and the kink margin leave
    out far less than their caps (2 % of the rows, 1e-4 of the pairs)."""
import numpy as np
import pytest
import torch

from tests import adam_ref
from tests import dqn_head_ref as HR
from tests import dqn_loop_ref as LR

F = np.float32
IN, H, NACT = 73, 256, 18


def _net(rng, bias3=0.0):
    W1, b1 = HR._linear_init(rng, H, IN)
    W2, b2 = HR._linear_init(rng, H, H)
    W3, b3 = HR._linear_init(rng, NACT, H)
    return (W1, b1, W2, b2, W3, (b3 + F(bias3)).astype(F))


def _observation_like(rng, n):
    """Rows shaped like `Fly` observations: columns of very different ranges (a height near 1.2, velocities of a few units, angles
    over the circle, projections in [-1, 1], joint positions in [-1, 1], joint velocities of tens) and six contact flags that are
    exactly 0 or 1, a third of the velocity columns exactly 0 (an env at rest)."""
    x = np.zeros((n, IN), F)
    x[:, 0] = 1.2 + 0.2 * rng.standard_normal(n)
    x[:, 1:7] = 3.0 * rng.standard_normal((n, 6))
    x[:, 7:10] = rng.uniform(-np.pi, np.pi, (n, 3))
    x[:, 10:13] = rng.uniform(-1, 1, (n, 3))
    x[:, 13:31] = rng.uniform(-1, 1, (n, 18))
    x[:, 31:49] = 20.0 * rng.standard_normal((n, 18)) * (rng.uniform(size=(n, 1)) > 1 / 3)
    x[:, 49:67] = rng.uniform(-1, 1, (n, 18))
    x[:, 67:73] = rng.uniform(size=(n, 6)) > 0.5
    return x


def _synthetic_ring(rng, cap, n, writes):
    """A ring written `writes` > cap times (so it wrapped): every slot holds the rows of its LAST writer; ~15 % done == 0 rows."""
    ring = {k: np.zeros((cap, n) + ((IN,) if k in ("obs", "next_obs") else ()), F) for k in LR.FIELDS}
    for t in range(writes):
        h = t % cap
        ring["obs"][h] = _observation_like(rng, n)
        ring["next_obs"][h] = _observation_like(rng, n)
        ring["action"][h] = rng.uniform(-1, 1, n)
        ring["reward"][h] = 2.0 * rng.standard_normal(n)
        ring["done"][h] = rng.uniform(size=n) > 0.15
    return ring


def test_slot_to_batch_assembly_honours_slot_order_and_wrap():
    rng = np.random.default_rng(0)
    cap, n = 5, 7
    ring = _synthetic_ring(rng, cap, n, 13)                     # wrapped twice: head at 3
    slots = [4, 0, 2]                                           # across the wrap, not sorted
    obs, act, rew, nxt, done = LR.batch(ring, slots)
    assert obs.shape == (3 * n, IN) and act.shape == (3 * n,)
    for i, s in enumerate(slots):
        sl = slice(i * n, (i + 1) * n)
        assert np.array_equal(obs[sl], ring["obs"][s]) and np.array_equal(nxt[sl], ring["next_obs"][s])
        assert np.array_equal(act[sl], ring["action"][s]) and np.array_equal(rew[sl], ring["reward"][s])
        assert np.array_equal(done[sl], ring["done"][s])
    assert not np.array_equal(obs, LR.batch(ring, sorted(slots))[0])       # the order is the list's, not the ring's
    cs = LR.chunks({k: torch.from_numpy(v) for k, v in ring.items()}, slots)
    assert all(torch.equal(c[0], torch.from_numpy(ring["obs"][s])) for c, s in zip(cs, slots))


def test_explicit_gradient_is_autograd_in_float64():
    """Batch from a wrapped synthetic ring, duplicate-free slots, done == 0 rows: loss and all six tensors against torch autograd
    (float64, smooth_l1_loss, the target under no_grad) to 1e-8 of each tensor's scale."""
    rng = np.random.default_rng(1)
    ring = _synthetic_ring(rng, 7, 96, 24)
    slots = [6, 1, 3, 0, 5]
    assert len(set(slots)) == len(slots)
    b = LR.batch(ring, slots)
    assert (b[4] == 0).any() and (b[4] == 1).any()
    w, wt = _net(rng), _net(rng, bias3=0.05)
    loss, grads, mid = LR.loss_and_grad(w, wt, b)
    tw = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in w]
    tt = [torch.tensor(a, dtype=torch.float64) for a in wt]

    def fwd(p, x):
        lk = torch.nn.functional.leaky_relu
        return lk(lk(x @ p[0].T + p[1]) @ p[2].T + p[3]) @ p[4].T + p[5]
    obs, act, rew, nxt, done = (torch.from_numpy(a) for a in b)
    idx = torch.round(0.5 * (act + 1) * 17).long()
    q = fwd(tw, obs.double())[torch.arange(obs.shape[0]), idx]
    with torch.no_grad():
        target = rew.double() + 0.99 * fwd(tt, nxt.double()).max(1)[0] * done.double()
    tl = torch.nn.functional.smooth_l1_loss(q, target)
    auto = torch.autograd.grad(tl, tw)
    assert abs(loss - float(tl.detach())) <= 1e-12 * abs(float(tl.detach()))
    assert (np.abs(mid["head"]["hub"]) > 0.5).any() and (np.abs(mid["head"]["hub"]) < 0.5).any()      # both Huber branches
    for g, a in zip(grads, auto):
        a = a.numpy()
        assert g.shape == a.shape and np.abs(g - a).max() <= 1e-8 * np.abs(a).max()


def test_dqn_adam_soft_chained_is_torch_adam_plus_soft_update():
    """Ten chained updates: adam_ref.dqn_adam_soft (all-ones mask) against torch.optim.Adam(lr 3e-4) and the product's own
    `soft_update(tau 0.995)` on a float64 module."""
    from fly_bproject_amd.dqn import soft_update
    torch.manual_seed(0)
    rng = np.random.default_rng(2)
    net, tgt = torch.nn.Linear(40, 30).double(), torch.nn.Linear(40, 30).double()
    opt = torch.optim.Adam(net.parameters(), lr=3e-4)
    flat = lambda m: np.concatenate([p.detach().numpy().reshape(-1) for p in m.parameters()])   # noqa: E731
    P, Pt = flat(net), flat(tgt)
    m, v = np.zeros_like(P), np.zeros_like(P)
    mask = np.ones_like(P)
    for step in range(10):
        G = rng.standard_normal(P.size) * 10.0 ** rng.uniform(-6, 0, P.size)
        o = 0
        for p in net.parameters():
            p.grad = torch.from_numpy(G[o:o + p.numel()].reshape(p.shape).copy())
            o += p.numel()
        opt.step()
        soft_update(net, tgt, 0.995)
        P, Pt, m, v = adam_ref.dqn_adam_soft(P, Pt, G, m, v, step, mask)
        assert np.abs(P - flat(net)).max() <= 1e-13 * np.abs(P).max(), step
        assert np.abs(Pt - flat(tgt)).max() <= 1e-13 * np.abs(Pt).max(), step
    st = opt.state[next(iter(net.parameters()))]
    n0 = next(iter(net.parameters())).numel()
    assert np.abs(m[:n0] - st["exp_avg"].numpy().reshape(-1)).max() <= 1e-13 * np.abs(m).max()
    assert np.abs(v[:n0] - st["exp_avg_sq"].numpy().reshape(-1)).max() <= 1e-13 * np.abs(v).max()


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
class _StubEnv:
    """An env with `Fly`'s loop-facing surface on the CPU: `step` leaves obs / reward / reset flags (an env flags itself every
    `period` steps, staggered), `reset_async` clears the flags and -- `rewrites` -- repacks the flagged envs' observations (`Fly`'s
    reset, like the reference's, does not: then next_obs stored before or after the reset is the same row)."""

    def __init__(self, n, seed, period=5, rewrites=True):
        self.rng = np.random.default_rng(seed)
        self.n, self.period, self.rewrites = n, period, rewrites
        self.obs_buf = torch.zeros(n, IN)
        self.reward_buf = torch.zeros(n)
        self.reset_buf = torch.ones(n, dtype=torch.long)
        self.progress = np.arange(n) % period

    def step(self, actions):
        self.obs_buf.copy_(torch.from_numpy(_observation_like(self.rng, self.n)) + actions[:, :1])
        self.reward_buf.copy_(torch.from_numpy(self.rng.standard_normal(self.n).astype(F)))
        self.progress += 1
        self.reset_buf.copy_(torch.from_numpy((self.progress % self.period == 0).astype(np.int64)))

    def reset_async(self):
        k = self.reset_buf != 0
        if self.rewrites:
            self.obs_buf[k] = torch.from_numpy(_observation_like(self.rng, int(k.sum())))
        self.reset_buf.zero_()


def _plain_loop(steps=17, n=6, cap=5, mbs=3, bug=None, rewrites=True):
    """dqn.py:102-126 as a plain Python loop (random actions; the action rule has a test of its own) -> transcript.
    bug: "next_obs_after_reset" | "done_from_cleared_flags" | "late_publish_after_wrap": one corruption of the loop each."""
    from fly_bproject_amd.dqn import ReplayBuffer
    rb = ReplayBuffer(n, IN, "cpu", buffer_limit=cap, seed=0)
    assert rb.capacity == cap
    env = _StubEnv(n, 3, rewrites=rewrites)
    rng = np.random.default_rng(4)
    recs, pending_commit = [], False
    for t in range(1, steps + 1):
        if pending_commit:
            rb.commit()
            pending_commit = False
        r = {"run_step": t, "eps": LR.epsilon(t), "obs_before": env.obs_buf.numpy().copy()}
        o, a, rw, no, d = rb.slot()
        o.copy_(env.obs_buf)
        r["act_obs"] = o.numpy().copy()
        r["coin"], r["rand"] = rng.uniform(size=n).astype(F), rng.uniform(size=n).astype(F)
        act = torch.from_numpy(F(2.0) * (r["rand"] - F(0.5)))
        r["action"] = act.numpy().copy()
        a.copy_(act)
        env.step(a.unsqueeze(-1).expand(-1, 18).contiguous())
        r["step_obs"], r["step_reward"], r["step_reset"] = (x.numpy().copy() for x in (env.obs_buf, env.reward_buf, env.reset_buf))
        if bug == "next_obs_after_reset":
            rw.copy_(env.reward_buf); torch.sub(1.0, env.reset_buf, out=d)
            env.reset_async()
            no.copy_(env.obs_buf)
        else:
            no.copy_(env.obs_buf); rw.copy_(env.reward_buf)
            if bug == "done_from_cleared_flags":
                env.reset_async()
                torch.sub(1.0, env.reset_buf, out=d)
            else:
                torch.sub(1.0, env.reset_buf, out=d)
                env.reset_async()
        if bug == "late_publish_after_wrap" and t > cap:
            pending_commit = True
        else:
            rb.commit()
        r["slot_lists"] = []
        if rb.size() > mbs:
            r["ring_before_update"] = {k: getattr(rb, k).numpy().copy() for k in LR.FIELDS}
            r["slot_lists"].append(rb.sample_slots(mbs))
        r["row"] = tuple(x.numpy().copy() for x in (o, a, rw, no, d))
        r["head"], r["count"], r["size"] = rb.head, rb.count, rb.size()
        recs.append(r)
    return {"capacity": cap, "mini_batch_size": mbs, "steps": recs}


@pytest.mark.parametrize("rewrites", [False, True])
def test_transcript_checker_accepts_a_plain_loop(rewrites):
    stats = LR.check_transcript(_plain_loop(rewrites=rewrites), reset_rewrites_obs=rewrites)
    assert stats["updates"] == 17 - 3 and stats["reset_envs"] > 0 and stats["done0_rows"] > 0
    rule = "an env that reset starts the next step from its reset observation" if not rewrites else "the reset leaves the observation buffer alone"
    with pytest.raises(AssertionError, match=rule):             # and it knows which kind of env it is looking at
        LR.check_transcript(_plain_loop(rewrites=rewrites), reset_rewrites_obs=not rewrites)


@pytest.mark.parametrize("bug,rule", [("next_obs_after_reset", r"next_obs\[h\] is what the step left, before the reset"),
                                      ("done_from_cleared_flags", r"done\[h\] == 1 - reset_buf of the step"),
                                      ("late_publish_after_wrap", r"head follows commit\(\)")])
def test_transcript_checker_rejects_each_corruption(bug, rule):
    with pytest.raises(AssertionError, match=rule):
        LR.check_transcript(_plain_loop(bug=bug), reset_rewrites_obs=True)
    if bug != "next_obs_after_reset":       # (where the reset leaves the observations alone, that order changes no stored value)
        with pytest.raises(AssertionError, match=rule):
            LR.check_transcript(_plain_loop(bug=bug, rewrites=False))
    else:
        LR.check_transcript(_plain_loop(bug=bug, rewrites=False))


def test_transcript_checker_sees_a_stale_slot_in_front_of_an_update():
    tr = _plain_loop(rewrites=False)
    r = tr["steps"][9]
    r["ring_before_update"]["reward"][(r["head"] + 1) % tr["capacity"]][0] += 1.0
    with pytest.raises(AssertionError, match="in front of the update"):
        LR.check_transcript(tr)


# ---- the exclusion caps ------------------------------------------------------------------------------------------------------------
def test_exclusion_caps_are_reachable_on_observation_like_rows():
    """The GPU test fails a case that leaves out more than 2 % of its rows (ties, coin edge) or whose ambiguous kink pairs pass 1e-4
    of all pairs.  On 4096 observation-like rows under default-initialised weights both shares are far below their caps; the
    random branch is held whatever the Q values; a row made an exact tie and a coin put on fp32(eps) are left out."""
    rng = np.random.default_rng(5)
    n = 4096
    w = _net(rng)
    x = _observation_like(rng, n)
    coin, rand = rng.uniform(size=n).astype(F), rng.uniform(size=n).astype(F)
    eps = LR.epsilon(40)
    want, out, cnt = LR.expected_actions(w, x, coin, rand, eps)
    share_rows = out.mean()
    _, _, mid = LR.loss_and_grad(w, w, (x, rand * 2 - 1, rand, x, np.ones(n, F)))
    amb, pairs = LR.kink_pairs(w, mid)
    amb_h2, _ = LR.kink_pairs(w, mid, s_h1=2.0 ** 7 / np.abs(mid["a1"]).max(), s_h2=2.0 ** 7 / np.abs(mid["a2"]).max())
    print("\neps-greedy rows left out: %d of %d (%.2e; %d ties, %d on the coin edge); ambiguous kink pairs: %d of %d (%.2e), "
          "%d under fp16x2 scales" % (int(out.sum()), n, share_rows, cnt["tie"], cnt["edge"], amb, pairs, amb / pairs, amb_h2))
    assert share_rows <= 0.002 and amb <= 0.5e-4 * pairs and amb_h2 <= 0.5e-4 * pairs
    explore = coin < F(eps)
    assert 0.5 * n < explore.sum() < n
    assert np.array_equal(want[explore], F(2.0) * (rand[explore] - F(0.5)))
    greedy = ~explore & ~out
    Q, _ = HR.forward64(w, x)
    assert np.array_equal(want[greedy], F(2.0) * (np.argmax(Q, 1).astype(F)[greedy] / F(17) - F(0.5)))
    # a constant last layer: every greedy row is an 18-way tie and is left out; a coin on fp32(eps) is left out on either branch
    w0 = w[:4] + (np.zeros_like(w[4]), np.full_like(w[5], 0.25))
    coin[:2] = F(eps), np.nextafter(F(eps), F(0))
    _, out0, cnt0 = LR.expected_actions(w0, x, coin, rand, eps)
    assert out0[:2].all() and out0[~(coin < F(eps))].all() and not out0[2:][(coin < F(eps))[2:]].any()
    assert cnt0["edge"] == 2
