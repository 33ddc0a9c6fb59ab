"""GPU: the DQN head where the rest of the suite never looks -- Q rows that are entirely NEGATIVE (the padded columns 18..31 of
a Q row read exactly 0: a max or argmax that lost its `< 18` mask is right whenever one real Q value is positive, which is
every row the other tests draw), stored actions exactly ON a bin edge (fp32 position k + 0.5: round half to even) and beyond
the clamp, rows with done = 0, a coin exactly equal to eps, ragged row counts, rows followed by NaN in their allocation.

All five kernels that carry a copy of the column mask (dqn_act_kernel, dqn_td_kernel, dqn_chain_kernel, dqn_chain_h2_kernel
and the two run-time-width table kernels) against tests/dqn_head_ref.py, a plain numpy restatement that is itself held to
float64 autograd and shown to be sensitive (tests/test_dqn_head_ref_cpu.py: every one-decision mutant moves it by >= 100x the
bounds below).

Bounds (R.LOSS_RTOL, R.L3_RTOL: the project's measured ones against float64, test_h2_gradient_error_against_float64_beside_
bf16x3): loss within 2e-6 relative; db3 and dW3 within 2e-5 of their largest entry.  A per-tile loss sum is held to 2e-6 of
max(that sum, the batch's mean row term): a ragged tile can hold ONE row next to the parabola's vertex (row 32 of the batch:
|dv| = 0.04, term 9e-4), whose own relative rounding 2 d|dv| / |dv| is 2e-6 from fp32's 4e-8 on dv alone (measured: 2.07e-6
of its own sum on the fp32-MFMA path, and the same from an fp32 evaluation on the CPU); what the per-tile check is for -- a
row in the wrong tile, a padded row in the sum -- moves a tile by a whole row term.  Measured on an MI355X
(profiles/dqn_head_edges.txt): every path is at least 24x inside every bound, so none was re-measured; builds with a
20-column mask, coin <= eps or round-half-away fail this file at the figures of the reference's own mutants."""
import math

import numpy as np
import pytest
import torch

from tests import dqn_head_ref as R
from tests.test_dqn import _bare_dqn
from tests.test_dqn_h2_gpu import _restore, _state, _views

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
SENTINEL = 7.0
LAST_U = F(1.0 - 2.0 ** -24)          # the largest fp32 below 1: the top of a uniform draw


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _poisoned(a, tail=32):
    """`a` on the GPU at the front of an allocation whose following `tail` rows are NaN: whatever reads past the rows it was
    given carries NaN into its result."""
    a = np.ascontiguousarray(a, F)
    buf = torch.full((a.shape[0] + tail,) + a.shape[1:], NAN, device="cuda:0")
    buf[:a.shape[0]] = torch.from_numpy(a).to("cuda:0")
    view = buf[:a.shape[0]]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def _out(*shape):
    return torch.full(shape, SENTINEL, device="cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# a. the table kernels through the ABI
def _td_inputs(B, A, seed):
    rng = np.random.default_rng(seed)
    q = -(0.125 + 2.0 * np.abs(rng.standard_normal((B, A)))).astype(F)
    qn = -(0.125 + 2.0 * np.abs(rng.standard_normal((B, A)))).astype(F)
    if B > 3:
        qn[1], qn[2] = -0.0, 0.0                                 # rows entirely -0.0 / entirely 0.0
        qn[3], q[3] = -1.5, -2.25                                # A-way ties below zero
    edges = R.edge_actions(A)
    act = rng.permutation(edges)[np.arange(B) % len(edges)]
    if B > 8:
        act[4:8] = 1.5, -1.5, 0.0, -0.0                          # both clamps and both zeros whatever the draw left out
    rew = (2.0 * rng.standard_normal(B)).astype(F)
    done = (rng.uniform(size=B) > 0.3).astype(F)
    return q, qn, act, rew, done


@pytest.mark.parametrize("B,A", [(1, 18), (63, 18), (65, 18), (255, 18), (257, 18), (513, 18), (65, 2), (65, 5)])
def test_huber_td_table_kernel_on_negative_rows_and_bin_edges(B, A):
    """dqn_huber_td: dq bit-equal to the fp32 row rule (the same fp32 operations in the same order; the build has
    -ffp-contract=off), each loss_part[block] within 8 2^-24 of the float64 sum of its block's row terms (six shuffle levels
    and two adds of non-negative terms), rows >= B of a partial last block add nothing and nothing is written past row B."""
    from fly_bproject_amd import _lib
    q, qn, act, rew, done = _td_inputs(B, A, 100 * A + B)
    assert q.max() < 0 and qn.max() <= 0 and (B < 8 or (done == 0).any())
    idx = R.action_index(act, A)
    hub, dq = R.td_rows(q[np.arange(B), idx], rew, R.masked_max(qn, A), done, F(0.99), F(1.0) / F(B), dtype=F)
    want = np.zeros((B, A), F)
    want[np.arange(B), idx] = dq
    blocks = (B + 255) // 256
    want_parts = [hub[256 * i:256 * (i + 1)].astype(np.float64).sum() for i in range(blocks)]
    g = [_poisoned(x) for x in (q, act, rew, qn, done)]
    got, parts = _out(B + 32, A), _out(blocks + 1)
    _lib.check(_lib.load().dqn_huber_td(g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), g[4].data_ptr(),
                                        0.99, A, B, got.data_ptr(), parts.data_ptr(), None), "dqn_huber_td")
    torch.cuda.synchronize()
    got, parts = got.cpu().numpy(), parts.cpu().numpy().astype(np.float64)
    assert np.array_equal(_bits(got[:B]), _bits(want))
    assert (got[B:] == SENTINEL).all() and parts[blocks] == SENTINEL
    for i in range(blocks):
        print("B %d A %d block %d: loss_part %.9g, float64 sum %.9g" % (B, A, i, parts[i], want_parts[i]))
        assert abs(parts[i] - want_parts[i]) <= 8 * 2.0 ** -24 * want_parts[i], (i, parts[i], want_parts[i])
    if B > 8:
        assert (act > 1).any() and (act < -1).any() and R.on_half_position(act, A).sum() >= 2


@pytest.mark.parametrize("n", [1, 255, 257])
def test_eps_greedy_table_kernel_on_negative_rows_ties_and_the_coin_at_eps(n):
    """dqn_eps_greedy bit-equal to the reference: all-negative rows, ties among negative values (the first index wins), rows
    entirely -0.0, coin == eps exactly at eps = 0.25 (greedy: the comparison is strict), eps = 0 and eps = 1, rand at both ends
    of a uniform draw."""
    from fly_bproject_amd import _lib
    rng = np.random.default_rng(n)
    q = -(0.125 + 2.0 * np.abs(rng.standard_normal((n, 18)))).astype(F)
    if n > 8:
        q[2, 5] = q[2, 9] = q[2, 17] = -0.0625                   # a three-way tie for the maximum: 5 wins
        q[3] = -3.0                                              # an 18-way tie: 0 wins
        q[4] = -0.0
        q[5, 17] = -0.03125                                      # the maximum in the last real column
    coin = rng.uniform(size=n).astype(F)
    coin[::3] = 0.25
    coin[1::7] = np.nextafter(F(0.25), F(0))
    coin[4::11] = LAST_U
    coin[5::13] = 0.0
    rand = rng.uniform(size=n).astype(F)
    rand[::2] = 0.0
    rand[1::4] = LAST_U
    g = [_poisoned(x) for x in (q, coin, rand)]
    greedy = F(2.0) * (R.first_argmax(q, 18).astype(F) / F(17) - F(0.5))
    for eps in (0.25, 0.0, 1.0):
        out = _out(n + 32)
        _lib.check(_lib.load().dqn_eps_greedy(g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), eps, 18, out.data_ptr(), n, None),
                   "dqn_eps_greedy")
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.array_equal(_bits(out[:n]), _bits(R.eps_greedy(q, coin, rand, eps, 18))), eps
        assert (out[n:] == SENTINEL).all() and (np.abs(out[:n]) <= 1).all()
        if eps == 0.25:
            assert np.array_equal(out[:n][coin == F(0.25)], greedy[coin == F(0.25)])          # coin == eps: greedy
        elif eps == 0.0:
            assert np.array_equal(out[:n], greedy)                                            # coin = 0 included
        else:
            assert np.array_equal(out[:n], F(2.0) * (rand - F(0.5)))
    if n > 8:
        assert np.array_equal(greedy[2:6], F(2.0) * (np.array([5, 0, 0, 17], F) / F(17) - F(0.5)))


# ---------------------------------------------------------------------------------------------------------------------
# b. dqn_act and dqn_forward on the three bias patterns
_NETS = {}


def _load(d, b):
    with torch.no_grad():
        for net, w in ((d.q, b["w"]), (d.q_target, b["wt"])):
            for p, a in zip(net.parameters(), w):
                p.copy_(torch.from_numpy(a))
    d.packed.refresh()
    return d


def _net(pattern):
    """One network pair per bias pattern for the launches that do not change it."""
    if pattern not in _NETS:
        b = R.edge_batch(pattern=pattern)
        _NETS[pattern] = (_load(_bare_dqn(rows=64), b), b, R.forward64(b["w"], b["obs"])[0])
    return _NETS[pattern]


@pytest.mark.parametrize("pattern", ["mod", "asc", "desc"])
@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_act_on_all_negative_q_rows(n, pattern):
    """dqn_act with its optional q_out buffer (DQN.act passes none): the actions bit-equal to the reference's eps_greedy on the
    launch's OWN Q table, that table against the float64 forward at test_mfma_q_network_forward_matches_torch's tolerance and
    entirely negative; greedy actions are +1 everywhere under the ascending bias and -1 under the descending one (a padded
    column's 0 would win every row); no action outside [-1, 1]; rows past n (NaN) are neither read into a result nor written."""
    from fly_bproject_amd import _lib
    d, b, Q64 = _net(pattern)
    pk = d.packed
    rng = np.random.default_rng(n)
    coin = rng.uniform(size=n).astype(F)
    coin[::3] = 0.25
    coin[1::5] = np.nextafter(F(0.25), F(0))
    rand = rng.uniform(size=n).astype(F)
    rand[1::2] = LAST_U
    x, gc, gr = _poisoned(b["obs"][:n]), _poisoned(coin), _poisoned(rand)
    for eps in (0.25, 0.0):
        act, q = _out(n + 32), _out(n + 32, 18)
        _lib.check(_lib.load().dqn_act(pk.P.data_ptr(), pk.PF.data_ptr(), x.data_ptr(), n, gc.data_ptr(), gr.data_ptr(), eps,
                                       act.data_ptr(), q.data_ptr(), None), "dqn_act")
        torch.cuda.synchronize()
        act, q = act.cpu().numpy(), q.cpu().numpy()
        assert (act[n:] == SENTINEL).all() and (q[n:] == SENTINEL).all()
        act, q = act[:n], q[:n]
        assert np.isfinite(q).all() and (q < 0).all()
        np.testing.assert_allclose(q, Q64[:n], rtol=2e-5, atol=2e-5)
        assert np.array_equal(_bits(act), _bits(R.eps_greedy(q, coin, rand, eps, 18))), eps
        assert (np.abs(act) <= 1).all()
        if eps == 0.0 and pattern != "mod":
            assert (act == (1.0 if pattern == "asc" else -1.0)).all()


@pytest.mark.parametrize("pattern", ["mod", "asc", "desc"])
@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_forward_reads_no_row_past_its_count(n, pattern):
    """dqn_forward on rows at the front of an allocation whose following 32 rows are NaN: no NaN reaches q_out, nothing is
    written past row n, the table agrees with the float64 forward."""
    from fly_bproject_amd import _lib
    d, b, Q64 = _net(pattern)
    pk = d.packed
    x, q = _poisoned(b["obs"][:n]), _out(n + 32, 18)
    _lib.check(_lib.load().dqn_forward(pk.P.data_ptr(), pk.PF.data_ptr(), x.data_ptr(), n, q.data_ptr(), None), "dqn_forward")
    torch.cuda.synchronize()
    q = q.cpu().numpy()
    assert (q[n:] == SENTINEL).all() and np.isfinite(q[:n]).all() and (q[:n] < 0).all()
    np.testing.assert_allclose(q[:n], Q64[:n], rtol=2e-5, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------------
# c. the three update paths on the edge batch
_REF = {}


def _reference(n):
    """`head` on the first n rows of the edge batch, from the float64 forward of the same weights (computed once per n)."""
    if "batch" not in _REF:
        b = R.edge_batch()
        Q, H2 = R.forward64(b["w"], b["obs"])
        _REF["batch"] = (b, Q, H2, R.forward64(b["wt"], b["nxt"])[0])
    b, Q, H2, Qn = _REF["batch"]
    if n not in _REF:
        _REF[n] = R.head(Q[:n], Qn[:n], b["act"][:n], b["rew"][:n], b["done"][:n], H2=H2[:n])
    return b, _REF[n]


def _chunks(b, split):
    """The batch's rows as row blocks of `split` rows, each in an allocation of its own followed by 32 NaN rows."""
    out, r = [], 0
    for n in split:
        out.append(tuple(_poisoned(b[k][r:r + n]) for k in ("obs", "act", "rew", "nxt", "done")))
        r += n
    return out


def _update(b, fused, split):
    """One DQN.update of the rows in `split` on the path `fused` names (False: the per-step fp32-MFMA launches).  The per-step
    workspace is NaN-filled in front of the call; f16x2 is calibrated on the same rows first and runs under h2_freeze
    (tests/test_dqn_h2_gpu.py).  Returns (the DQN, the loss, the per-tile loss sums in row order)."""
    d = _load(_bare_dqn(rows=160, fused=bool(fused), gemm=fused or "f16x2"), b)
    d.mini_batch_size = 8                        # a loss row per chunk for up to 8 chunks: update() must not reallocate
    d._alloc_workspace(160)
    chunks = _chunks(b, split)
    takes_fused = bool(fused) and len(set(split)) == 1 and split[0] % 32 == 0
    if takes_fused and fused == "f16x2":
        st = _state(d)
        d.update(chunks)
        torch.cuda.synchronize()
        assert d.h2_calibrated and d.h2_overflows == 0
        _restore(d, st)
        d.h2_freeze = True
    ws = (d._h1, d._h2, d._dz1, d._dz2, d._dz3)
    for t in ws:
        t.fill_(NAN)
    loss = float(d.update(chunks))
    torch.cuda.synchronize()
    assert all(t is u for t, u in zip(ws, (d._h1, d._h2, d._dz1, d._dz2, d._dz3)))       # (the poisoned workspace was the one used)
    if takes_fused:
        tiles = d._fu_loss[:sum(split) // 32].cpu().numpy()
        assert d.h2_calibrated == (fused == "f16x2")
    else:
        tiles = np.concatenate([d._loss_part[i, :(n + 31) // 32].cpu().numpy() for i, n in enumerate(split)])
        assert not d.h2_calibrated and getattr(d, "_fu_rows", 0) == 0                    # no fused launch was made
    return d, loss, tiles


def _check(d, loss, tiles, ref, label):
    """One update against `head`: prints the measured errors (loss, worst per-tile sum against max(its own sum, the mean row
    term) and against its own sum alone, db3, dW3) and returns (what is out of bounds: a list to assert empty once every path
    of a test has been printed, db3)."""
    G = d.packed.G
    bad = []
    if not bool(torch.isfinite(G).all()):
        bad.append("%s: NaN or Inf in G" % label)
    if not bool((G[d.packed.grad_mask == 0] == 0).all()):
        bad.append("%s: a padded entry of G is not 0" % label)
    if d.h2_overflows != 0 or not math.isfinite(loss):
        bad.append("%s: overflows %d, loss %r" % (label, d.h2_overflows, loss))
    v = _views(G)
    dW3, db3 = v[4].double().cpu().numpy(), v[5].double().cpu().numpy()
    assert tiles.shape == ref["loss_part"].shape, label
    e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
    d_tile = np.abs(tiles.astype(np.float64) - ref["loss_part"])
    e_tile = float((d_tile / np.maximum(ref["loss_part"], ref["loss"])).max())
    e_own = float((d_tile / ref["loss_part"]).max())
    e_b = float(np.abs(db3 - ref["db3"]).max() / np.abs(ref["db3"]).max())
    e_w = float(np.abs(dW3 - ref["dW3"]).max() / np.abs(ref["dW3"]).max())
    print("%-34s loss %.2e  worst tile %.2e (of its own sum %.2e)  db3 %.2e  dW3 %.2e" % (label, e_loss, e_tile, e_own, e_b, e_w))
    for name, e, bound in (("loss", e_loss, R.LOSS_RTOL), ("tile", e_tile, R.LOSS_RTOL), ("db3", e_b, R.L3_RTOL), ("dW3", e_w, R.L3_RTOL)):
        if not e <= bound:
            bad.append("%s: %s off by %.3g > %.3g" % (label, name, e, bound))
    return bad, db3


@pytest.mark.parametrize("split", [(160,), (32,) * 5], ids=["one_chunk", "five_chunks"])
def test_update_paths_on_the_edge_batch(split):
    """The 160 rows of the edge batch as one chunk and as 5 x 32, through the per-step launches and the two fused
    arithmetics, against `head` on the float64 forward: the loss, every per-tile loss sum, db3 and dW3 (read from the packed
    gradient), no NaN or Inf anywhere in G, G's padded entries exactly 0, no overflow; and the three paths leave the same set
    of non-zero db3 entries -- the bins are the same (every bin but 9: 0's fp32 neighbours all round 8.5 to 8)."""
    b, ref = _reference(160)
    print()
    hit, bad = {}, []
    for fused in (False, "bf16x3", "f16x2"):
        d, loss, tiles = _update(b, fused, split)
        problems, db3 = _check(d, loss, tiles, ref, "%s %s" % (fused or "per-step fp32", "x".join(map(str, split))))
        bad += problems
        hit[fused] = db3 != 0
    assert not bad, bad
    want = ref["db3"] != 0
    assert want.sum() == 17 and not want[9]
    for fused, nz in hit.items():
        assert np.array_equal(nz, want), fused


@pytest.mark.parametrize("n", [1, 31, 33, 96])
def test_per_step_launches_on_ragged_prefixes(n):
    """The first n rows of the edge batch through dqn_td_step + dqn_grad_w: the rows of a ragged tile past n are NaN in the
    inputs' allocations and in the workspace, and must not reach the loss sums or the gradient."""
    b, ref = _reference(n)
    print()
    d, loss, tiles = _update(b, False, (n,))
    bad, _ = _check(d, loss, tiles, ref, "per-step fp32, first %d rows" % n)
    assert not bad, bad


def test_mixed_split_falls_through_to_the_per_step_launches():
    """32 + 64 + 64 rows with fused_update = True: row blocks of unequal size are not the fused launches' shape, the update
    must take the per-step launches (no fused launch, no fp16x2 calibration) and give the batch's gradient."""
    b, ref = _reference(160)
    print()
    d, loss, tiles = _update(b, "f16x2", (32, 64, 64))
    assert d.fused_update and d.update_gemm == "f16x2"
    bad, _ = _check(d, loss, tiles, ref, "fused asked, 32+64+64 -> per-step")
    assert not bad, bad
