"""GPU: the DQN update's fp16x2 arithmetic (csrc/dqn_fused_h2.inc; reference UselessFiles/dqn.py:64-85) beyond the parity cases of
tests/test_dqn.py, which run every fused-update test in both arithmetics: its error against float64 beside bf16x3's, the scale
windows and the weight planes `dqn_fused_update_h2` leaves, and the refusal path (an update whose values do not fit fp16 under the
lagged scales is formed again by the bf16x3 launches: bit for bit what an undisturbed bf16x3 update leaves)."""
import math

import numpy as np
import pytest
import torch

from tests.test_dqn import _bare_dqn

pytestmark = pytest.mark.gpu


def _batch(parts, n, seed):
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda:0", generator=g)   # noqa: E731
    u = lambda *s: torch.rand(*s, device="cuda:0", generator=g)   # noqa: E731
    return [(r(n, 73), u(n) * 2 - 1, r(n) * 2, r(n, 73), (u(n) > 0.1).float()) for _ in range(parts)]


def _perturb_target(d):
    with torch.no_grad():
        for p_ in d.q_target.parameters():
            p_.add_(0.05 * torch.randn_like(p_))
    d.packed.refresh()


KINK_K = 32           # the GEMM term of the ambiguity margin: z's rounding is taken as at most 32 2^-24 of sum |x| |w| + |b|


def _kink_reference(d, chunks, s_h1, s_h2, flip=None):
    """The update's gradient in float64 with LeakyReLU' taken from sign(z64) (1 for z64 > 0, 0.01 otherwise: torch's rule), and the
    signed effect of every unit next to LeakyReLU's kink taking the other slope.

    A unit's slope is read by the kernel from the sign of the leading fp16 term of its activation h s_H (s_H = the class scale of
    H1 or H2 in that launch's table).  It can differ from sign(z64) for two reasons only:
      - the GEMM rounds z.  Both operands are split into two fp16 terms (relative error <= 2^-22 each, the dropped lo x lo product
        another 2^-22) and summed in fp32 over at most 256 products (sqrt(256) 2^-24 typical, more in the worst order); layer 2's
        input carries layer 1's rounding, a relative error of the same size in sum |a1| |w2|.  KINK_K 2^-24 (sum |x| |w| + |b|)
        = 2^-19 of the absolute sum covers all of that with a factor of 4 or more;
      - the leading term loses the sign: h s_H rounds to +-0.0 when |h s_H| <= 2^-25 (half fp16's smallest subnormal), i.e. for
        0 < z <= 2^-25 / s_H on the positive side and for 0 > z >= -2^-25 / (0.01 s_H) on the negative side (h = 0.01 z).
    A (row, unit) pair is AMBIGUOUS when |z64| <= max(KINK_K 2^-24 (sum |x| |w| + |b|), 2^-25 / s_H, 2^-25 / (0.01 s_H)).  Either
    slope is right there to the arithmetic's own rounding: taking the other one moves dZ by (s' - s) dA = +-0.99 dA, and with it a
    row of dW / db -- a layer-2 pair also the row's dA1, i.e. ALL of dW1 and db1 through layer 1's slope.  That last term is why the
    allowance is not a per-element sum of |moves|: one ambiguous layer-2 pair would put ~1e-3 of dW1's scale under every element
    and leave dW1 unchecked.  Instead each pair's signed effect on the six tensors is returned, and _beyond takes out the effects of
    the pairs the kernel evidently flipped.

    Expected count: z1 and z2 have a density of about 1 at zero, the margins are ~1e-6 .. 1e-5, so about 2e-5 of the (row, unit)
    pairs or fewer are ambiguous.

    flip = (layer, row, unit): the reference takes the OTHER slope for that one pair (the negative control).
    Returns (gradient [dW1, db1, dW2, db2, dW3, db3], the effects of flipping each ambiguous pair [P, shape] per tensor, P, total
    pairs, margins and |z|)."""
    obs, act, rew, nxt, done = (torch.cat([c[i] for c in chunks]).double() for i in range(5))
    w1, b1, w2, b2, w3, b3 = (t.detach().double() for t in d.q.parameters())
    B = obs.shape[0]
    rows = torch.arange(B, device=obs.device)
    z1 = obs @ w1.T + b1
    a1 = torch.where(z1 > 0, z1, 0.01 * z1)
    z2 = a1 @ w2.T + b2
    a2 = torch.where(z2 > 0, z2, 0.01 * z2)
    q = a2 @ w3.T + b3
    tn = [t.detach().double() for t in d.q_target.parameters()]
    ht = nxt @ tn[0].T + tn[1]
    ht = torch.where(ht > 0, ht, 0.01 * ht) @ tn[2].T + tn[3]
    qt = torch.where(ht > 0, ht, 0.01 * ht) @ tn[4].T + tn[5]
    idx = torch.round(0.5 * (torch.cat([c[1] for c in chunks]) + 1) * 17).long()      # (in fp32, as the kernel and _grad64 round)
    diff = q[rows, idx] - (rew + 0.99 * qt.max(1)[0] * done)
    dz3 = torch.zeros_like(q)
    dz3[rows, idx] = diff.clamp(-1.0, 1.0) / B                           # smooth_l1 (beta 1), mean over the batch
    slope = [torch.where(z > 0, 1.0, 0.01).double() for z in (z1, z2)]
    if flip is not None:
        layer, r, u = flip
        slope[layer - 1][r, u] = 1.01 - slope[layer - 1][r, u]
    da2 = dz3 @ w3
    dz2 = da2 * slope[1]
    da1 = dz2 @ w2
    dz1 = da1 * slope[0]
    want = [dz1.T @ obs, dz1.sum(0), dz2.T @ a1, dz2.sum(0), dz3.T @ a2, dz3.sum(0)]
    gemm = 2.0 ** -24 * KINK_K
    m1 = torch.clamp(gemm * (obs.abs() @ w1.abs().T + b1.abs()), min=max(2.0 ** -25 / s_h1, 2.0 ** -25 / (0.01 * s_h1)))
    m2 = torch.clamp(gemm * (a1.abs() @ w2.abs().T + b2.abs()), min=max(2.0 ** -25 / s_h2, 2.0 ** -25 / (0.01 * s_h2)))
    amb1, amb2 = z1.abs() <= m1, z2.abs() <= m2
    # the signed change of all six tensors if the kernel took the other slope for one ambiguous pair, one row per pair
    r1, u1 = torch.nonzero(amb1, as_tuple=True)
    r2, u2 = torch.nonzero(amb2, as_tuple=True)
    d1 = (1.01 - 2 * slope[0][r1, u1]) * da1[r1, u1]                     # dZ1 moves by (s' - s) dA1 at (r, u)
    d2 = (1.01 - 2 * slope[1][r2, u2]) * da2[r2, u2]                     # dZ2 moves by (s' - s) dA2 at (r, j) ...
    dz1_2 = d2[:, None] * w2[u2] * slope[0][r2]                          # ... and dZ1's row r by that times W2[j] and layer 1's slope
    P = r1.numel() + r2.numel()
    eff = [torch.zeros((P,) + w.shape, dtype=torch.float64, device=obs.device) for w in want]
    i1, i2 = torch.arange(r1.numel(), device=obs.device), r1.numel() + torch.arange(r2.numel(), device=obs.device)
    eff[0][i1, u1] = d1[:, None] * obs[r1]
    eff[1][i1, u1] = d1
    eff[0][i2] = dz1_2[:, :, None] * obs[r2][:, None, :]
    eff[1][i2] = dz1_2
    eff[2][i2, u2] = d2[:, None] * a1[r2]
    eff[3][i2, u2] = d2
    return want, eff, P, 2 * B * 256, (m1, m2, z1.abs(), z2.abs(), da1.abs())


def _beyond(G, want, eff, tensors=range(6), most=16):
    """Per parameter tensor: max |g - g64| / max |g64| after the kink pairs the kernel evidently took the other slope for are
    accounted for.  Greedy: the pair whose signed effect `eff` (_kink_reference) removes the most of the worst relative error is
    taken while it at least halves it (at most `most` pairs) -- a real error is not the exact rank-one pattern of one such pair.
    Returns (errors per tensor in `tensors`, pairs taken)."""
    tensors = list(tensors)
    got = _views(G)
    scale = [float(want[t].abs().max()) for t in tensors]
    R = torch.cat([((got[t].double() - want[t]) / sc).reshape(-1) for t, sc in zip(tensors, scale)])
    # (an explicit width: a batch with NO ambiguous pair has eff of zero rows, which reshape(0, -1) cannot size)
    D = torch.cat([(eff[t] / sc).reshape(eff[t].shape[0], want[t].numel()) for t, sc in zip(tensors, scale)], 1)
    taken = []
    cur = float(R.abs().max())
    while D.shape[0] and len(taken) < most:
        cand = (R[None] - D).abs().max(1)[0]
        best = int(cand.argmin())
        if not float(cand[best]) < 0.5 * cur:
            break
        R = R - D[best]
        cur = float(cand[best])
        D[best] = float("inf")
        taken.append(best)
    out, o = [], 0
    for t in tensors:
        n = want[t].numel()
        out.append(float(R[o:o + n].abs().max()))
        o += n
    return out, len(taken)


def _grad64(d, chunks):
    """The update's gradient by torch autograd in float64 on the same weights and rows."""
    import copy
    obs, act, rew, nxt, done = (torch.cat([c[i] for c in chunks]).double() for i in range(5))
    q, qt = copy.deepcopy(d.q).double(), copy.deepcopy(d.q_target).double()
    B = obs.shape[0]
    idx = torch.round(0.5 * (act.float() + 1) * 17).long()
    q_val = q(obs)[torch.arange(B), idx]
    with torch.no_grad():
        target = rew + 0.99 * qt(nxt).max(1)[0] * done
    loss = torch.nn.functional.smooth_l1_loss(q_val, target)
    return torch.autograd.grad(loss, list(q.parameters())), float(loss)


def _views(G):
    return [G[:256 * 80].view(256, 80)[:, :73], G[20480:20736], G[20736:86272].view(256, 256), G[86272:86528],
            G[86528:94720].view(32, 256)[:18], G[94720:94738]]


def _state(d):
    pk = d.packed
    return [t.clone() for t in (pk.P, pk.P_tgt, pk.exp_avg, pk.exp_avg_sq, pk.step)]


def _restore(d, st):
    pk = d.packed
    for dst, src in zip((pk.P, pk.P_tgt, pk.exp_avg, pk.exp_avg_sq, pk.step), st):
        dst.copy_(src)
    pk.refresh()


def test_h2_gradient_error_against_float64_beside_bf16x3():
    """4 x 8192 rows as drawn -- none replaced; the batch on which an fp16x2 unit next to LeakyReLU's kink once moved dW1 by 2.6e-3
    of its scale.  Against the float64 gradient once the ambiguous (row, unit) pairs the kernel took the other slope for are
    accounted for (_kink_reference with the scales of the fp16x2 launch, _beyond): per parameter tensor max |g - g64| / max |g64| of
    the fp16x2 update <= 2e-5 and <= twice the fp32-MFMA per-step path's (the reference's numerics) + 2e-6; bf16x3 printed beside.  The
    ambiguous pairs are few (<= 1e-4 of all; about 2e-5 expected).  The loss within 2e-6.  Negative control: the same check against a
    reference that takes the other slope for ONE pair that is not ambiguous (|z64| >= 10x its margin) must fail."""
    torch.manual_seed(2)
    chunks = _batch(4, 8192, 21)
    errs, grads = {}, {}
    for gemm, fused in (("f16x2", True), ("bf16x3", True), ("f32", False)):
        torch.manual_seed(2)
        d = _bare_dqn(rows=8192, fused=fused, gemm=gemm if fused else "f16x2")
        _perturb_target(d)
        if gemm == "f16x2":
            st = _state(d)
            d.update(chunks); torch.cuda.synchronize()       # calibrates; the update leaves the scales of these rows ...
            _restore(d, st)
            d.h2_freeze = True                               # ... and the measured update runs under exactly those
            sc = d.packed.h2_scales.cpu()
            s_h1, s_h2 = float(sc[1]), float(sc[2])
            want, eff, n_amb, pairs, (m1, _, z1, _, da1) = _kink_reference(d, chunks, s_h1, s_h2)
            auto, loss64 = _grad64(d, chunks)                # (the explicit reference is autograd's gradient)
            for a, w in zip(auto, want):
                assert float((a - w).abs().max()) <= 1e-8 * float(w.abs().max())
            # the negative control's reference: a layer-1 pair far from its margin, the one whose flip moves dW1 most
            obs = torch.cat([c[0] for c in chunks]).double()
            clear = z1 >= 10 * m1
            effect = torch.where(clear, da1 * obs.abs().max(1, keepdim=True)[0], torch.zeros_like(da1))
            r, u = divmod(int(effect.argmax()), effect.shape[1])
            assert bool(clear[r, u])
            want_f, eff_f, _, _, _ = _kink_reference(d, chunks, s_h1, s_h2, flip=(1, r, u))
            P0 = d.packed.P.clone()
        assert torch.equal(d.packed.P, P0)                   # (the same weights in all three)
        loss = d.update(chunks)
        torch.cuda.synchronize()
        assert abs(float(loss) - loss64) <= 2e-6 * abs(loss64) + 1e-9, gemm
        grads[gemm] = d.packed.G.clone()
        errs[gemm] = _beyond(grads[gemm], want, eff)
        assert d.h2_overflows == 0
    print("\nambiguous (row, unit) pairs: %d of %d (s_H1 %g, s_H2 %g, KINK_K %d)" % (n_amb, pairs, s_h1, s_h2, KINK_K))
    print("max |g - g64| / max |g64| per tensor, kink pairs the kernel flipped taken out:",
          {k: (["%.2e" % e for e in v[0]], "%d flipped" % v[1]) for k, v in errs.items()})
    assert 0 < n_amb <= 1e-4 * pairs, n_amb
    for e_h2, e_f32 in zip(errs["f16x2"][0], errs["f32"][0]):
        assert e_h2 <= 2e-5 and e_h2 <= 2 * e_f32 + 2e-6, errs
    forced, _ = _beyond(grads["f16x2"], want_f, eff_f)
    print("negative control (layer 1, row %d, unit %d, |z64| %.3g = %.0fx its margin, slope flipped in the reference):" % (
        r, u, float(z1[r, u]), float(z1[r, u] / m1[r, u])), ["%.2e" % e for e in forced])
    assert max(forced) > 2e-5, forced


def test_h2_scales_land_in_their_windows_and_planes_hold_the_weights():
    """After an update: the maxima of |scaled value| the launch recorded lie in their class's window once the scales have seen the same
    rows (activations [2^7, 2^8), gradients [2^2, 2^3), weights [2^11, 2^12)); the two-term planes reproduce every weight to 2^-21
    relative to its layer's maximum, online and target, forward and transposed."""
    from fly_bproject_amd import dqn as D
    from fly_bproject_amd.policy import H2_TARGET_EXP_ACT, H2_TARGET_EXP_GRAD
    torch.manual_seed(4)
    d = _bare_dqn(rows=4096, fused=True)
    _perturb_target(d)
    chunks = _batch(3, 4096, 5)
    st = _state(d)
    d.update(chunks)                # calibrates (two passes) + the update
    _restore(d, st)
    d.update(chunks)                # the same rows under the scales the first update left
    torch.cuda.synchronize()
    sc = d.packed.h2_scales.cpu().numpy()
    assert d.h2_overflows == 0 and int(d.packed.h2_overflow) == 0
    for c in (0, 1, 2):
        assert 2.0 ** H2_TARGET_EXP_ACT <= sc[32 + c] < 2.0 ** (H2_TARGET_EXP_ACT + 1), (c, sc[32 + c])
    for c in (5, 6):
        assert 2.0 ** H2_TARGET_EXP_GRAD <= sc[32 + c] < 2.0 ** (H2_TARGET_EXP_GRAD + 1), (c, sc[32 + c])
    np.testing.assert_array_equal(sc[:16] * sc[16:32], np.ones(16, np.float32))
    assert all(np.log2(s) == np.round(np.log2(s)) for s in sc[:14] if s > 0)          # powers of two
    # weights: s_l max|w_l| in [2^11, 2^12) (the planes were made from the weights in front of the LAST update: restore them)
    _restore(d, st)
    d.h2_freeze = True
    d.update(chunks)
    _restore(d, st)
    torch.cuda.synchronize()
    pk = d.packed
    layers = ((D.OFF_W1, D.OFF_B1), (D.OFF_W2, D.OFF_B2), (D.OFF_W3, D.OFF_B3))
    sc = pk.h2_scales.cpu().numpy()
    for which, (master, planes_f) in enumerate(((pk.P, pk.QH), (pk.P_tgt, pk.QH_tgt))):
        for l, (a, b) in enumerate(layers):
            s = float(sc[8 + 3 * which + l])
            m = float(master[a:b].abs().max())
            # max(max |w|, 2^-4) -> [2^11, 2^12): nn.Linear(256, .)'s init is U(-1/16, 1/16), its maximum sits just under the floor
            assert s == 2.0 ** (11 - math.floor(math.log2(max(m, 0.0625)))) and s * m < 2.0 ** 12
            assert float(sc[32 + 8 + 3 * which + l]) == m
            idx = pk.idx_fb[a:b].long()
            hf = (idx // 1536) * 1024 + idx % 1536
            got = (planes_f[hf].view(torch.float16).double() + planes_f[hf + 512].view(torch.float16).double()) / s
            assert float((got - master[a:b].double()).abs().max()) <= 2.0 ** -21 * m, (which, l)
    for l, (a, b) in enumerate(layers[1:], start=1):
        s = float(sc[8 + l])
        idx = pk.idx_tb[a:b].long()
        ht = (idx // 1536) * 1024 + idx % 1536
        got = (pk.QTH[ht].view(torch.float16).double() + pk.QTH[ht + 512].view(torch.float16).double()) / s
        assert float((got - pk.P[a:b].double()).abs().max()) <= 2.0 ** -21 * float(pk.P[a:b].abs().max()), l


@pytest.mark.parametrize("cls", [0, 2, 6])
def test_h2_overflow_is_refused_and_the_update_redone_in_bf16x3(cls):
    """A lagged scale 2^14 too large (class X, H2 or dZ1): the launch's maximum does not fit fp16, the device word is set, `DQN.update`
    forms the gradient again with the bf16x3 launches -- the packed gradient, the loss and the networks afterwards are bit for bit
    what a bf16x3 update leaves -- and the NEXT update calibrates again and runs in fp16x2."""
    torch.manual_seed(6)
    chunks = _batch(2, 4096, 9)
    ref = _bare_dqn(rows=4096, fused=True, gemm="bf16x3")
    _perturb_target(ref)
    st = _state(ref)
    l_ref = float(ref.update(chunks)); torch.cuda.synchronize()
    g_ref, p_ref, pt_ref = ref.packed.G.clone(), ref.packed.P.clone(), ref.packed.P_tgt.clone()

    d = _bare_dqn(rows=4096, fused=True, gemm="f16x2")
    _restore(d, st)
    d.update(chunks); torch.cuda.synchronize()               # calibrated
    assert d.h2_calibrated and d.h2_overflows == 0
    _restore(d, st)
    with torch.no_grad():
        d.packed.h2_scales[cls] *= 2.0 ** 14
        d.packed.h2_scales[16 + cls] /= 2.0 ** 14
    l = float(d.update(chunks)); torch.cuda.synchronize()
    assert d.h2_overflows == 1 and not d.h2_calibrated and int(d.packed.h2_overflow) == 0
    assert l == l_ref and torch.equal(d.packed.G, g_ref) and torch.equal(d.packed.P, p_ref) and torch.equal(d.packed.P_tgt, pt_ref)
    # the next update calibrates again and is an fp16x2 update
    g_b3_next = None
    l2 = float(d.update(chunks)); torch.cuda.synchronize()
    assert d.h2_overflows == 1 and d.h2_calibrated
    ref.update(chunks); torch.cuda.synchronize()
    g_b3_next = ref.packed.G
    m = d.packed.grad_mask > 0
    assert float((d.packed.G - g_b3_next)[m].abs().max()) <= 2e-5 * float(g_b3_next[m].abs().max()) and np.isfinite(l2)
    assert not torch.equal(d.packed.G, g_b3_next)           # (it really ran the other arithmetic)


def test_h2_update_is_independent_of_the_grid():
    """One workgroup per CU or a quarter of them: the partial slabs are summed in a fixed order per grid, so two grids differ only in
    summation order -- to 2e-6 of the gradient's scale -- and each is deterministic run to run.  (Smaller grid: fewer rows than CUs x 32.)"""
    torch.manual_seed(8)
    d = _bare_dqn(rows=2048, fused=True)
    _perturb_target(d)
    st = _state(d)
    big = _batch(8, 2048, 3)                 # 512 tiles on 256 workgroups
    d.update(big); _restore(d, st)
    d.h2_freeze = True
    d.update(big); torch.cuda.synchronize(); g_a = d.packed.G.clone(); _restore(d, st)
    d.update(big); torch.cuda.synchronize(); g_b = d.packed.G.clone(); _restore(d, st)
    assert torch.equal(g_a, g_b)
    # the same rows as 64-tile updates (grid = 64 workgroups), averaged
    acc = torch.zeros_like(g_a)
    for i in range(8):
        d.update(big[i:i + 1]); torch.cuda.synchronize(); acc += d.packed.G / 8; _restore(d, st)
    m = d.packed.grad_mask > 0
    assert float((acc - g_a)[m].abs().max()) <= 2e-5 * float(g_a[m].abs().max())
    assert d.h2_overflows == 0


def test_h2_overflow_in_the_training_loop_is_refused_on_the_device_and_settled_later():
    """`DQN.run()`'s own updates do not synchronise with the host (a blocking read per env step drains the launch queue): the optimizer
    launch takes the overflow word as `grad_invalid`, the host looks at a copy of it when a later update begins.  A lagged scale pushed
    2^14 too high between two env steps: the updates from there on are refused ON THE DEVICE (nothing moves, the step counter stays),
    the host finds out within the next steps, clears the word, forms as many updates in bf16x3 and goes on in fp16x2 -- at the end every
    env step has had its update and the networks are finite."""
    import contextlib
    import io
    from fly_bproject_amd.dqn import DQN
    from tests.hip_helpers import make_args
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = DQN(make_args(256, dqn_mini_batch_size=8, replay_steps=16))
        for _ in range(14):
            agent.run()
    torch.cuda.synchronize()
    assert agent.update_gemm == "f16x2" and agent.h2_calibrated and agent.h2_overflows == 0
    issued0 = agent._updates_issued
    assert issued0 == 14 - 8 and int(agent.packed.step) == issued0
    p_before = agent.packed.P.clone()
    with torch.no_grad():
        agent.packed.h2_scales[0] *= 2.0 ** 14
        agent.packed.h2_scales[16] /= 2.0 ** 14
    with contextlib.redirect_stdout(io.StringIO()):
        agent.run()                                      # this update overflows: refused on the device
    torch.cuda.synchronize()
    assert int(agent.packed.h2_overflow) == 1 and int(agent.packed.step) == issued0 and torch.equal(agent.packed.P, p_before)
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(4):
            agent.run()                                  # the host notices, redoes the refused updates in bf16x3, calibrates, goes on
        agent._h2_poll(block=True)                       # (at the latest here)
        agent.run()                                      # and an fp16x2 update again: calibrates first
        agent._h2_poll(block=True)
    torch.cuda.synchronize()
    assert agent.h2_overflows >= 1 and int(agent.packed.h2_overflow) == 0 and agent.h2_calibrated
    assert agent._updates_issued == issued0 + 6 and int(agent.packed.step) == issued0 + 6
    assert not torch.equal(agent.packed.P, p_before) and all(torch.isfinite(q).all() for q in agent.q.parameters())
    agent.exit()


def test_h2_dw2_from_the_record_against_float64():
    """The dW2 kernel rebuilds dZ2 from a 2.3 KB record per tile (dq s_z2 and the action per row, LeakyReLU' flags) instead of
    reading its 32 KB plane image: the layer-2 weight gradient against float64 on every row (<= 2e-6 of its scale once the ambiguous
    layer-2 pairs the kernel flipped are accounted for, _beyond: the rebuilt dZ2 is the correctly rounded fp32 product, its flags
    those of the chain); 5 x 4096 rows: workgroups walk tiles across chunk boundaries."""
    torch.manual_seed(12)
    chunks = _batch(5, 4096, 31)
    d = _bare_dqn(rows=4096, fused=True)
    _perturb_target(d)
    st = _state(d)
    d.update(chunks); _restore(d, st)                    # calibrated
    d.h2_freeze = True
    sc = d.packed.h2_scales.cpu()
    want, eff, n_amb, pairs, _ = _kink_reference(d, chunks, float(sc[1]), float(sc[2]))
    d.update(chunks); torch.cuda.synchronize()
    assert n_amb <= 1e-4 * pairs, n_amb
    (err,), flipped = _beyond(d.packed.G, want, eff, tensors=[2])
    print("\nambiguous (row, unit) pairs: %d of %d, %d flipped; dW2 error %.2e of its scale" % (n_amb, pairs, flipped, err))
    assert err <= 2e-6


def test_h2_dw2_record_takes_the_slope_where_the_leading_term_is_negative_zero():
    """Layer-2 units whose pre-activation is a tiny negative number in every arithmetic: W2's row zero and b2 = -2^-30, so z2 is
    exactly -2^-30 and LeakyReLU' is 0.01.  0.01 |z2| s_H2 is under 2^-25, so H2's leading fp16 term is -0.0: the LeakyReLU' flags of
    the dW2 record must take the slope there, as the chain's dA1 does (a flag that reads -0.0 as positive makes these rows of dW2
    100x too large).  Their rows of dW2 and entries of db2 against float64 with the slope 0.01: within 1e-5 of their own largest
    entry.  (W2's zero rows keep the units out of dA1: only the record decides.)"""
    torch.manual_seed(14)
    chunks = _batch(2, 4096, 41)
    d = _bare_dqn(rows=4096, fused=True)
    _perturb_target(d)
    units = [0, 37, 101, 200]
    with torch.no_grad():
        d.q.net[2].weight[units] = 0.0
        d.q.net[2].bias[units] = -2.0 ** -30
    d.packed.refresh()
    st = _state(d)
    d.update(chunks); _restore(d, st)                    # calibrated
    d.h2_freeze = True
    sc = d.packed.h2_scales.cpu()
    assert 0.01 * 2.0 ** -30 * float(sc[2]) < 2.0 ** -25, float(sc[2])
    want, _, _, _, _ = _kink_reference(d, chunks, float(sc[1]), float(sc[2]))
    d.update(chunks); torch.cuda.synchronize()
    assert d.h2_overflows == 0
    v = _views(d.packed.G)
    errs = [float((v[t].double()[units] - want[t][units]).abs().max() / want[t][units].abs().max()) for t in (2, 3)]
    print("\nlayer-2 units at z2 = -2^-30 (s_H2 %g): dW2 rows %.2e, db2 %.2e of their largest entry" % (float(sc[2]), *errs))
    assert max(errs) <= 1e-5, errs
