"""CPU: the stand-alone DQN head reference of tests/dqn_head_ref.py against torch (float64 autograd of the reference's own
loss, dqn.py:68-79) and the oracle, the guarantees of its edge batch, and its SENSITIVITY: every one-decision mutant of the
reference (a max or argmax that sees the padded columns, another rounding rule for the bin, no clamp, `done` ignored, coin
<= eps) moves the reference by at least 100x the bounds tests/test_dqn_head_edges_gpu.py asserts -- which is what makes
those bounds mean something."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import dqn_head_ref as R

F = np.float32
# the bounds tests/test_dqn_head_edges_gpu.py asserts: a mutant must be 100x above them
GPU_LOSS_RTOL, GPU_L3_RTOL = R.LOSS_RTOL, R.L3_RTOL


@pytest.fixture(scope="module")
def batch():
    b = R.edge_batch()
    Q, H2 = R.forward64(b["w"], b["obs"])
    Qn, _ = R.forward64(b["wt"], b["nxt"])
    return dict(b, Q=Q, Qn=Qn, H2=H2, ref=R.head(Q, Qn, b["act"], b["rew"], b["done"], H2=H2))


def _torch_net(w):
    net = torch.nn.Sequential(torch.nn.Linear(73, 256), torch.nn.LeakyReLU(), torch.nn.Linear(256, 256), torch.nn.LeakyReLU(),
                              torch.nn.Linear(256, 18)).double()
    with torch.no_grad():
        for p, a in zip(net.parameters(), w):
            p.copy_(torch.from_numpy(np.asarray(a, np.float64)))
    return net


def test_edge_batch_keeps_its_guarantees(batch):
    """Conditions on the INPUTS, by the reference alone: every online and target Q row entirely negative in all three bias
    patterns (asserted by edge_batch itself), >= 62 rows exactly on a bin edge, both clamps, both Huber branches, finished and
    unfinished rows, and a row maximum that moves between columns (to column 17 / column 0 in the two ordered patterns)."""
    act, Q, Qn = batch["act"], batch["Q"], batch["Qn"]
    assert act.shape == (160,) and batch["obs"].shape == (160, 73)
    assert Q.max() < 0 and Qn.max() < 0
    half = R.on_half_position(act)
    assert half.sum() >= 62 and half[0] and half[1]                      # +-0.0 sit on 8.5
    assert np.signbit(act[1]) and not np.signbit(act[0])
    assert (act > 1).sum() == 1 and (act < -1).sum() == 1
    assert set(R.action_index(act, 18)) == set(range(18)) - {9}          # every bin but 9: 0's neighbours are subnormal, all ON 8.5
    on_edge = R.action_position(act[half], 18).astype(np.float64) - 0.5
    assert set(on_edge) >= set(range(4, 17))                             # rows exactly ON the edges 4.5 .. 16.5 (below, fp32 is finer)
    assert (~half[6:159]).sum() >= 40                                    # and the neighbourhoods have rows off their edge
    assert 40 <= (batch["done"] == 0).sum() <= 56
    dv = batch["ref"]["dq"] * 160
    assert (np.abs(dv) < 1).sum() >= 16 and (np.abs(dv) == 1).sum() >= 64
    assert len(np.unique(np.argmax(Q, 1))) >= 2 and len(np.unique(np.argmax(Qn, 1))) >= 2
    for pattern, col in (("asc", 17), ("desc", 0)):
        b = R.edge_batch(pattern=pattern)                               # (asserts negativity and the column itself)
        assert np.array_equal(b["act"], act) and (np.diff(b["w"][5]) != 0).all()
        assert R.first_argmax(R.forward64(b["w"], b["obs"])[0], 18)[0] == col


@pytest.mark.parametrize("nact", [18, 5, 2])
def test_action_index_is_torch_round_then_clamp(nact):
    act = np.concatenate([R.edge_actions(nact), np.linspace(-2, 2, 101).astype(F)])
    t = torch.from_numpy(act)
    want = torch.round(0.5 * (t + 1) * (nact - 1)).clamp(0, nact - 1).long().numpy()
    assert np.array_equal(R.action_index(act, nact), want)
    assert R.on_half_position(R.edge_actions(nact), nact).sum() >= (62 if nact == 18 else nact - 1)


def test_head_equals_float64_autograd(batch):
    """loss, net.4.weight.grad and net.4.bias.grad of smooth_l1_loss(q[b, idx], r + 0.99 max q_target(next) done) in float64."""
    b = batch
    q, qt = _torch_net(b["w"]), _torch_net(b["wt"])
    obs, nxt, rew, done = (torch.from_numpy(b[k]).double() for k in ("obs", "nxt", "rew", "done"))
    idx = torch.round(0.5 * (torch.from_numpy(b["act"]) + 1) * 17).clamp(0, 17).long()
    q_val = q(obs)[torch.arange(160), idx]
    with torch.no_grad():
        target = rew + 0.99 * qt(nxt).max(1)[0] * done
    loss = torch.nn.functional.smooth_l1_loss(q_val, target)
    loss.backward()
    ref, loss = b["ref"], loss.item()
    assert abs(ref["loss"] - loss) <= 1e-12 * abs(loss)
    assert abs(ref["loss_part"].sum() / 160 - loss) <= 1e-12 * abs(loss) and ref["loss_part"].shape == (5,)
    for got, want in ((ref["dW3"], q[4].weight.grad.numpy()), (ref["db3"], q[4].bias.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(b["Q"] - q(obs).detach().numpy()).max() <= 1e-12 * np.abs(b["Q"]).max()


def test_fp32_row_rule_agrees_with_the_oracle(batch):
    """On in-range actions (the oracle does not clamp): dq of the fp32 row rule against oracle.dqn_huber_td at the tolerances
    of test_oracle_huber_td_matches_reference (the oracle divides by B where the rule multiplies by 1 / B: one ulp)."""
    b = batch
    keep = np.abs(b["act"]) <= 1
    q, qn = b["Q"][keep].astype(F), b["Qn"][keep].astype(F)
    act, rew, done = b["act"][keep], b["rew"][keep], b["done"][keep]
    B = int(keep.sum())
    dq_o, loss_o = O.dqn_huber_td(q, act, rew, qn, done)
    idx = R.action_index(act, 18)
    hub, dq = R.td_rows(q[np.arange(B), idx], rew, R.masked_max(qn, 18), done, 0.99, F(1.0) / F(B), dtype=F)
    assert hub.dtype == F and dq.dtype == F
    full = np.zeros((B, 18), F)
    full[np.arange(B), idx] = dq
    np.testing.assert_allclose(full, dq_o, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(hub.astype(np.float64).sum() / B, loss_o, rtol=1e-6)


def _moved(mut, ref):
    return (abs(mut["loss"] - ref["loss"]) / abs(ref["loss"]),
            np.abs(mut["db3"] - ref["db3"]).max() / np.abs(ref["db3"]).max(),
            np.abs(mut["dW3"] - ref["dW3"]).max() / np.abs(ref["dW3"]).max())


def test_every_mutant_moves_the_reference_100x_beyond_the_gpu_bounds(batch):
    """On the edge batch (relative to |loss| and to each tensor's largest entry; measured with the batch's seed):
        pad          loss 23 %     db3 30 %   dW3 40 %
        half_away    loss 0.095 %  db3 62 %   dW3 75 %    (39 rows change their bin)
        affine       loss 2.5 %    db3 47 %   dW3 47 %    (27 rows)
        ignore_done  loss 8.3 %    db3 28 %   dW3 30 %
    Each of the four is >= 100x the GPU bound on the loss AND on both layer-3 tensors.  no_clamp changes the bin of the row
    with act = -1.5 (and with it dZ3); coin_le and pad change eps_greedy's output outright."""
    b, ref = batch, batch["ref"]
    table = {}
    for m in ("pad", "half_away", "affine", "ignore_done", "no_clamp"):
        table[m] = _moved(R.head(b["Q"], b["Qn"], b["act"], b["rew"], b["done"], H2=b["H2"], mutant=m), ref)
    print("\nmutant: relative change of loss, db3, dW3")
    for m, v in table.items():
        print("  %-12s %.3g %.3g %.3g" % ((m,) + v))
    for m in ("pad", "half_away", "affine", "ignore_done"):
        d_loss, d_b, d_w = table[m]
        assert d_loss >= 100 * GPU_LOSS_RTOL and d_b >= 100 * GPU_L3_RTOL and d_w >= 100 * GPU_L3_RTOL, (m, table[m])
    # the rebinned rows are the rows on an edge, and only those
    half = R.on_half_position(b["act"])
    for m, rows in (("half_away", 39), ("affine", 27)):
        moved = R.action_index(b["act"], 18, m) != R.action_index(b["act"], 18)
        assert moved.sum() >= rows - 2 and not (moved & ~half).any(), (m, int(moved.sum()))
    # no_clamp: the row beyond -1 takes another bin outright (and the gradient follows)
    moved = R.action_index(b["act"], 18, "no_clamp") != R.action_index(b["act"], 18)
    assert moved.sum() == 1 and b["act"][moved][0] == F(-1.5) and table["no_clamp"][1] >= 100 * GPU_L3_RTOL
    # eps_greedy: a coin exactly at eps is greedy; an all-negative row's argmax is not a padded column
    q = b["Q"].astype(F)
    coin, rand = np.full(160, 0.25, F), np.full(160, 0.75, F)
    want = R.eps_greedy(q, coin, rand, 0.25, 18)
    assert np.array_equal(want, F(2) * (R.first_argmax(q, 18).astype(F) / F(17) - F(0.5)))
    assert (R.eps_greedy(q, coin, rand, 0.25, 18, "coin_le") != want).all()
    padded = R.eps_greedy(q, coin, rand, 0.25, 18, "pad")
    assert (padded != want).all() and (padded > 1).all()                # column 18 of 17: an action outside [-1, 1]
    assert (np.abs(want) <= 1).all()
