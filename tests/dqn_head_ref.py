"""A stand-alone restatement of the DQN head (reference UselessFiles/dqn.py:68-79 and :89-100) in plain numpy: the three
decisions the head takes per row -- the target max over the 18 real columns of a Q row padded to 32, the first argmax over
the same columns, the bin a stored action stands for -- and the TD / Huber row rule behind them.  It shares no code with
oracle/ or the kernels.

Everything DISCRETE follows the fp32 rule as specified (the position of an action among the bins is formed in fp32, product
by product, and rounded half to even; the eps-greedy action is formed in fp32); everything CONTINUOUS is float64 unless the
caller asks for the fp32 row rule (`dtype=np.float32`: numpy rounds every operation on its own, which is what a kernel
built without floating-point contraction does).

`mutant=` names one wrong decision each (tests/test_dqn_head_ref_cpu.py shows that every one of them moves the reference by
>= 100x the bounds the GPU tests assert, on the batch of `edge_batch`):
    "pad"          max / argmax over all 32 columns, the padded ones reading 0
    "half_away"    the bin by rounding half away from zero
    "affine"       the bin from 8.5 act + 8.5 (for 18 bins) in float64 instead of the two fp32 products
    "no_clamp"     no clamp of the bin (saturated only where Python indexing needs it: [-nact, nact - 1], negative wraps)
    "ignore_done"  the target keeps the bootstrap term of finished rows
    "coin_le"      explores on coin <= eps instead of coin < eps
"""
import numpy as np

F = np.float32
NACT, OUT, IN, H, TILE = 18, 32, 73, 256, 32
SPECIAL_ACTIONS = (0.0, -0.0, 1.0, -1.0, 1.5, -1.5)
# What tests/test_dqn_head_edges_gpu.py asserts of the three update paths against `head` (the bounds of
# test_h2_gradient_error_against_float64_beside_bf16x3): |loss - loss64| <= LOSS_RTOL |loss64| (and every per-tile sum
# likewise), max |g - g64| <= L3_RTOL max |g64| for db3 and dW3.  tests/test_dqn_head_ref_cpu.py holds every mutant to
# 100x these, so the two files cannot drift apart.
LOSS_RTOL, L3_RTOL = 2e-6, 2e-5
SEED = 14     # the batch the tests use: with this draw the row maximum moves between columns 0 and 13 in both networks


# ---------------------------------------------------------------------------------------------------------------------
# the discrete rules
def action_position(act_f32, nact):
    """fp32: 0.5 * (act + 1), then * (nact - 1) -- two separately rounded products of one separately rounded sum."""
    a = np.asarray(act_f32, F)
    return (F(0.5) * (a + F(1.0))) * F(nact - 1)


def action_index(act_f32, nact, mutant=None):
    if mutant == "affine":
        half = 0.5 * (nact - 1)
        pos = half * np.asarray(act_f32, F).astype(np.float64) + half
    else:
        pos = action_position(act_f32, nact).astype(np.float64)
    if mutant == "half_away":
        idx = np.sign(pos) * np.floor(np.abs(pos) + 0.5)
    else:
        idx = np.rint(pos)                                   # half to even, as torch.round
    lo = -nact if mutant == "no_clamp" else 0
    return np.clip(idx, lo, nact - 1).astype(np.int64)


def _columns(q, nact, mutant):
    q = np.asarray(q)
    real = q[:, :nact]
    if mutant == "pad":
        return np.concatenate([real, np.zeros((q.shape[0], OUT - nact), real.dtype)], 1)
    return real


def masked_max(q, nact, mutant=None):
    """Row maximum over the columns < nact only."""
    return _columns(q, nact, mutant).max(1)


def first_argmax(q, nact, mutant=None):
    """The FIRST maximal column among the columns < nact (np.argmax returns the first)."""
    return np.argmax(_columns(q, nact, mutant), 1)


def eps_greedy(q, coin, rand, eps, nact, mutant=None):
    """dqn.py:89-100 in fp32: idx / (nact - 1), mixed with `rand` where coin < eps (strict), mapped to [-1, 1]."""
    true_act = first_argmax(q, nact, mutant).astype(F) / F(nact - 1)
    coin, rand = np.asarray(coin, F), np.asarray(rand, F)
    explore = (coin <= F(eps)) if mutant == "coin_le" else (coin < F(eps))
    a = np.where(explore, rand, true_act).astype(F)
    return F(2.0) * (a - F(0.5))


# ---------------------------------------------------------------------------------------------------------------------
# the continuous rule
def td_rows(q_val, reward, qn_max, done, discount, inv_B, dtype=np.float64, mutant=None):
    """One row each: target = reward + (discount * qn_max) * done, dv = q_val - target; Huber with beta = 1 whose kink belongs
    to the linear branch (|dv| < 1 strict); dq = clamp(dv, -1, 1) * inv_B.  Returns (hub, dq) in `dtype`."""
    t = np.dtype(dtype).type
    q_val, reward, qn_max, done = (np.asarray(x).astype(dtype) for x in (q_val, reward, qn_max, done))
    if mutant == "ignore_done":
        done = np.ones_like(done)
    target = reward + (t(discount) * qn_max) * done
    dv = q_val - target
    hub = np.where(np.abs(dv) < t(1.0), (t(0.5) * dv) * dv, np.abs(dv) - t(0.5))
    dq = t(inv_B) * np.minimum(np.maximum(dv, t(-1.0)), t(1.0))
    return hub.astype(dtype), dq.astype(dtype)


def head(Q, Qn, act, reward, done, discount=0.99, nact=NACT, H2=None, tile=TILE, mutant=None):
    """The head of one update batch on float64 Q tables: the loss (mean over the B rows), one loss SUM per `tile` rows, dZ3
    [B, nact], and with the float64 last hidden layer H2 [B, 256]: db3 = dZ3.sum(0), dW3 = dZ3^T H2."""
    Q, Qn = np.asarray(Q, np.float64), np.asarray(Qn, np.float64)
    B = Q.shape[0]
    rows = np.arange(B)
    idx = action_index(act, nact, mutant)
    q_val = Q[:, :nact][rows, idx]
    qn_max = masked_max(Qn, nact, mutant)
    hub, dq = td_rows(q_val, np.asarray(reward, F), qn_max, np.asarray(done, F), discount, 1.0 / B, mutant=mutant)
    pad = (-B) % tile
    out = dict(loss=float(hub.sum() / B), loss_part=np.concatenate([hub, np.zeros(pad)]).reshape(-1, tile).sum(1), idx=idx,
               hub=hub, dq=dq)
    dZ3 = np.zeros((B, nact))
    dZ3[rows, idx] = dq
    out["dZ3"] = dZ3
    if H2 is not None:
        out["db3"] = dZ3.sum(0)
        out["dW3"] = dZ3.T @ np.asarray(H2, np.float64)
    return out


def forward64(w, x):
    """The Q-network (Linear 73-256, LeakyReLU 0.01, Linear 256-256, LeakyReLU, Linear 256-18) in float64 on fp32 weights
    `w` = (W1, b1, W2, b2, W3, b3) in torch's [out, in] layout.  Returns (Q [n, 18], H2 [n, 256])."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(a, np.float64) for a in w)
    z = np.asarray(x, np.float64) @ W1.T + b1
    h = np.where(z > 0, z, 0.01 * z)
    z = h @ W2.T + b2
    h2 = np.where(z > 0, z, 0.01 * z)
    return h2 @ W3.T + b3, h2


# ---------------------------------------------------------------------------------------------------------------------
# the inputs
def _ulp_step(v, k):
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf), dtype=F)
    return v


def edge_actions(nact=NACT):
    """The special actions (+-0, +-1, +-1.5: bin centres, both clamps) and, for every bin edge k + 0.5, the fp32 value of
    (2k + 1) / (nact - 1) - 1 with its +-1..4 ulp neighbours: 6 + 9 (nact - 1) fp32 actions (159 for 18 bins)."""
    acts = [F(a) for a in SPECIAL_ACTIONS]
    for k in range(nact - 1):
        centre = F((2 * k + 1) / (nact - 1) - 1.0)
        acts += [_ulp_step(centre, d) for d in range(-4, 5)]
    return np.array(acts, F)


def on_half_position(act_f32, nact=NACT):
    """Rows whose fp32 position is EXACTLY k + 0.5: where half-to-even and half-away differ."""
    pos = action_position(act_f32, nact).astype(np.float64)
    return pos - np.floor(pos) == 0.5


def bias_pattern(name, nact=NACT):
    """Last-layer biases that make every Q row negative: "mod" = -1 - 0.25 ((7a) mod 18), whose runner-up columns are far
    apart; "asc" / "desc" = -1 .. -18 strictly ascending / descending (steps of 1: the network's own contribution to a Q
    value is a few tenths) so that the row maximum is at column 17 / column 0 on every row."""
    a = np.arange(nact)
    if name == "mod":
        return (-1.0 - 0.25 * ((7 * a) % 18)).astype(F)
    if name == "asc":
        return (-1.0 - 1.0 * (nact - 1 - a)).astype(F)
    if name == "desc":
        return (-1.0 - 1.0 * a).astype(F)
    raise ValueError(name)


def _linear_init(rng, n_out, n_in):
    """The distribution of torch's default nn.Linear init: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weights and biases."""
    b = 1.0 / np.sqrt(n_in)
    return rng.uniform(-b, b, (n_out, n_in)).astype(F), rng.uniform(-b, b, n_out).astype(F)


def edge_batch(seed=SEED, pattern="mod"):
    """160 rows on which the head's decisions are all visible: every online and every target Q row entirely negative (so a
    max or argmax that sees a padded 0 is wrong on EVERY row), the actions of `edge_actions` (>= 62 exactly on a bin edge,
    4 beyond the clamp), ~30 % of the rows finished, rewards N(0, 2) so both Huber branches occur.  The target's last-layer
    bias is the online one minus 0.125.  Returns a dict of fp32 arrays: obs, nxt [160, 73], act, rew, done [160], `w` and
    `wt` (W1, b1, W2, b2, W3, b3 of the online and the target network)."""
    rng = np.random.default_rng(seed)
    acts = edge_actions(NACT)
    B = (len(acts) + TILE - 1) // TILE * TILE
    act = np.concatenate([acts, rng.uniform(-1, 1, B - len(acts)).astype(F)])
    nets = []
    for shift in (0.0, 0.125):
        W1, b1 = _linear_init(rng, H, IN)
        W2, b2 = _linear_init(rng, H, H)
        W3, _ = _linear_init(rng, NACT, H)
        nets.append((W1, b1, W2, b2, W3, (bias_pattern(pattern) - F(shift)).astype(F)))
    obs, nxt = rng.standard_normal((B, IN)).astype(F), rng.standard_normal((B, IN)).astype(F)
    rew = (2.0 * rng.standard_normal(B)).astype(F)
    done = (rng.uniform(size=B) > 0.3).astype(F)
    b = dict(obs=obs, nxt=nxt, act=act, rew=rew, done=done, w=nets[0], wt=nets[1], pattern=pattern)
    # the batch's guarantees, on the float64 forward
    Q, _ = forward64(b["w"], obs)
    Qn, _ = forward64(b["wt"], nxt)
    assert Q.max() < 0 and Qn.max() < 0, "every online and target Q row must be entirely negative"
    assert int(on_half_position(act).sum()) >= 62
    assert 0.2 < 1.0 - done.mean() < 0.4
    if pattern != "mod":
        col = NACT - 1 if pattern == "asc" else 0
        assert (np.argmax(Q, 1) == col).all() and (np.argmax(Qn, 1) == col).all()
    return b
