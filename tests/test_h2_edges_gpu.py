"""GPU (-m gpu): the bookkeeping of the fp16x2 optimizer step outside its MFMA loops, at the edges the calibrated steady state of
tests/test_fused_h2_gpu.py never reaches: the RESCALE step of mlp_adam_step (weights crossing a power of two on that very step, a
rescale step that is refused), activation / gradient scales lagging far above the data, and a NaN or inf in the data (the step is
refused on the device, in the PPO step and in the DQN update)."""
import pytest
import torch

from tests.test_dqn_h2_gpu import _batch, _perturb_target, _restore, _state
from tests.test_fused_h2_gpu import _errs, _fp64_chain
from tests.test_fused_step_gpu import WIDTH, _chain
from tests.test_mlp_train_gpu import DEV, _setup

pytestmark = pytest.mark.gpu


def _layer_bounds():
    from fly_bproject_amd.policy import OFF_B1, OFF_B2, OFF_B3, OFF_B4, OFF_W1, OFF_W2, OFF_W3, OFF_W4
    return ((OFF_W1, OFF_B1), (OFF_W2, OFF_B2), (OFF_W3, OFF_B3), (OFF_W4, OFF_B4))


def _assert_planes_follow(pol, scales):
    """PH / PTH hold exactly split_f16x2(P, s_l) under the layer scales `scales` for every weight that has a plane."""
    from fly_bproject_amd.policy import OFF_W2, OFF_W3, OFF_W4, PACKED, split_f16x2
    bounds = (0, OFF_W2, OFF_W3, OFF_W4, PACKED)
    layer_scale = torch.ones(PACKED, device=DEV)
    for l in range(4):
        layer_scale[bounds[l]:bounds[l + 1]] = scales[l]
    for name, buf, src, dst in (("PH", pol.PH, pol._src_fb, pol._dst_fb), ("PTH", pol.PTH, pol._src_tb, pol._dst_tb)):
        dh = (dst // 1536) * 1024 + dst % 1536
        for term, plane in enumerate(split_f16x2(pol.P[src], layer_scale[src])):
            bad = torch.nonzero(buf[dh + 512 * term] != plane).squeeze(-1)
            assert bad.numel() == 0, (name, term, bad.numel(), src[bad[:8]].tolist())


def _layer_max(P):
    return [float(P[a:b].abs().max()) for a, b in _layer_bounds()]


def _snapshot(pol):
    ts = (pol.P, pol.PF, pol.PT, pol.PB, pol.PTB, pol.PH, pol.PTH, pol.G, pol.exp_avg, pol.exp_avg_sq, pol._step2, pol._norm_ws,
          pol.h2_scales)
    return [t.clone() for t in ts], pol._step_idx


def _restore_snapshot(pol, snap):
    ts = (pol.P, pol.PF, pol.PT, pol.PB, pol.PTB, pol.PH, pol.PTH, pol.G, pol.exp_avg, pol.exp_avg_sq, pol._step2, pol._norm_ws,
          pol.h2_scales)
    for dst, src in zip(ts, snap[0]):
        dst.copy_(src)
    pol._step_idx = snap[1]


@pytest.mark.parametrize("mode", ["norm_ready", "self_norm"])
def test_h2_rescale_step_derives_the_scales_from_the_weights_before_it(mode):
    """A rescale step on which the largest weights of W2 and W3 cross 2^-3 (set to +-(2^-3 - lr/2), one per Adam block of the layer,
    against their gradient's sign: the first Adam step moves each by lr).  The published scale of every layer is the one of the
    weights BEFORE the step, the planes are a bit-exact split of the weights AFTER it under that scale -- in every block -- and ten
    repeats of the same step from the same state leave the same bits."""
    from fly_bproject_amd.policy import H2_INV, H2_SINCE, H2_W0, h2_weight_scale
    n = 4099
    net, ref, pol, batch = _setup(n, 41, gemm="f16x2")
    pol.minibatch_grad(*batch, 0.2, fuse_norm=mode == "norm_ready")
    torch.cuda.synchronize()
    assert int(pol.h2_overflow) == 0 and int(pol.step) == (1 if mode == "norm_ready" else 0)
    lr, k = pol.lr, 2.0 ** -3
    crossing = {}
    with torch.no_grad():
        for l in (1, 2):
            a, b = _layer_bounds()[l]
            assert float(pol.P[a:b].abs().max()) < k - lr
            picked = []
            for blk in range(a // 1024, (b - 1) // 1024 + 1):         # the element of each Adam block with the largest |gradient|
                lo, hi = max(a, blk * 1024), min(b, blk * 1024 + 1024)
                j = lo + int(pol.G[lo:hi].abs().argmax())
                assert float(pol.G[j].abs()) > 1e-6
                picked.append(j)
            idx = torch.tensor(picked, device=DEV)
            pol.P[idx] = -torch.sign(pol.G[idx]) * (k - lr / 2)
            crossing[l] = idx
        pol.refresh()                                                  # (fragment copies and planes of the weights as now set)
        pol.h2_scales[H2_W0:H2_W0 + 4] *= 2.0                          # stale scales: the step must publish fresh ones ...
        pol.h2_scales[H2_INV + H2_W0:H2_INV + H2_W0 + 4] *= 0.5
        pol.h2_scales[H2_SINCE:H2_SINCE + 2] = 64.0                    # ... because a rescale is due
    before = pol.P.clone()
    want = [h2_weight_scale(m) for m in _layer_max(before)]
    snap = _snapshot(pol)
    first = None
    for rep in range(10):
        if rep:
            _restore_snapshot(pol, snap)
        pol.adam_step(norm_ready=mode == "norm_ready", self_norm=mode == "self_norm")
        torch.cuda.synchronize()
        assert int(pol.step) == 1
        got = [float(s) for s in pol.h2_scales[H2_W0:H2_W0 + 4].cpu()]
        if rep == 0:
            for l in (1, 2):                                           # the test bites: the weights crossed on this step
                assert float(pol.P[crossing[l]].abs().min()) > k, l
                assert h2_weight_scale(_layer_max(pol.P)[l]) == want[l] / 2, l
            assert got == want, (got, want)
            inv = [float(s) for s in pol.h2_scales[H2_INV + H2_W0:H2_INV + H2_W0 + 4].cpu()]
            assert all(s * i == 1.0 for s, i in zip(got, inv))
            _assert_planes_follow(pol, got)
            first = [t.clone() for t in (pol.P, pol.PH, pol.PTH, pol.PB, pol.exp_avg, pol.exp_avg_sq, pol.h2_scales)]
        else:
            for name, a, b in zip(("P", "PH", "PTH", "PB", "m", "v", "scales"), first,
                                  (pol.P, pol.PH, pol.PTH, pol.PB, pol.exp_avg, pol.exp_avg_sq, pol.h2_scales)):
                assert torch.equal(a, b), (rep, name)
    # the next step is not a rescale: it splits under the scales just published
    pol.minibatch_grad(*batch, 0.2, fuse_norm=mode == "norm_ready")
    pol.adam_step(norm_ready=mode == "norm_ready", self_norm=mode == "self_norm")
    torch.cuda.synchronize()
    assert int(pol.step) == 2 and [float(s) for s in pol.h2_scales[H2_W0:H2_W0 + 4].cpu()] == want
    _assert_planes_follow(pol, want)


def test_h2_refused_rescale_step_leaves_the_rescale_to_the_next_applied_step():
    """A rescale is due, the scales are stale (2x too large: they still fit), and the step is refused (its producer marked the gradient
    invalid): nothing changes.  The next step that IS applied rescales: fresh scales, planes split under them."""
    from fly_bproject_amd.policy import H2_INV, H2_SINCE, H2_W0, h2_weight_scale
    n = 4099
    net, ref, pol, batch = _setup(n, 43, gemm="f16x2")
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):                                                 # two ordinary steps
        pol.minibatch_grad(*batch, 0.2)
        pol.adam_step(self_norm=True, grad_invalid=word)
    torch.cuda.synchronize()
    assert int(pol.step) == 2
    with torch.no_grad():
        pol.h2_scales[H2_W0:H2_W0 + 4] *= 2.0
        pol.h2_scales[H2_INV + H2_W0:H2_INV + H2_W0 + 4] *= 0.5
        pol.h2_scales[H2_SINCE:H2_SINCE + 2] = 64.0
    keep = [t.clone() for t in (pol.P, pol.PH, pol.PTH, pol.exp_avg, pol.exp_avg_sq)]
    pol.minibatch_grad(*batch, 0.2)
    stale = pol.h2_scales.clone()
    word.fill_(1)
    pol.adam_step(self_norm=True, grad_invalid=word)                   # refused
    torch.cuda.synchronize()
    assert int(pol.step) == 2 and torch.equal(pol.h2_scales, stale)
    for a, b in zip(keep, (pol.P, pol.PH, pol.PTH, pol.exp_avg, pol.exp_avg_sq)):
        assert torch.equal(a, b)
    want = [h2_weight_scale(m) for m in _layer_max(pol.P)]
    assert all(w != float(s) for w, s in zip(want, stale[H2_W0:H2_W0 + 4].cpu()))     # (the test bites)
    word.zero_()
    pol.adam_step(self_norm=True, grad_invalid=word)                   # the same gradient, applied this time
    torch.cuda.synchronize()
    assert int(pol.step) == 3
    got = [float(s) for s in pol.h2_scales[H2_W0:H2_W0 + 4].cpu()]
    assert got == want, (got, want)
    _assert_planes_follow(pol, got)


@pytest.mark.parametrize("classes,k", [("dz", 4), ("dz", 6), ("dz", 8), ("dz", 10), ("dz", 11), ("act", 8)])
def test_h2_scales_lagging_high_meet_the_fp64_bar_or_are_refused(classes, k):
    """Scales 2^k too large for the data: the lag that follows a class maximum falling k binades between two launches (measured on
    real updates: up to ~8 for a gradient class).  Frozen table, the four gradient (dz4 .. dz1) or activation (x, h1 .. h3) scales
    times 2^-k.  Every chain tensor and every dW / db block against float64: within 2e-5, the suite's bar, while the classes stay
    within 6 binades of their windows; within 4e-5 2^(k - 8) for the 7 .. 10 binades the step still accepts; a launch with a class
    maximum under the floor (10 binades under the gradient window, csrc/fs_h2.inc H2_CLASS_FLOOR) is refused (sticky word, gradient marked
    invalid).  Errors printed beside bf16x3's and f32's (profiles/h2_lagging_scales.txt)."""
    from fly_bproject_amd.policy import ERR_SLOT, H2_CLASS_FLOOR, H2_INV, untile
    n = 4099
    net, ref, pol, batch = _setup(n, 13, gemm="f16x2")
    want = _fp64_chain(ref, *batch)
    pol.h2_freeze = True
    c0 = 4 if classes == "dz" else 0
    with torch.no_grad():
        pol.h2_scales[c0:c0 + 4] *= 2.0 ** -k
        pol.h2_scales[H2_INV + c0:H2_INV + c0 + 4] *= 2.0 ** k
    errs, gerrs = {}, {}
    pol.minibatch_grad(*batch, 0.2, dump=True)
    torch.cuda.synchronize()
    refused = (int(pol.h2_overflow), float(pol.G[ERR_SLOT]))
    low = min(float(pol.h2_scales[32 + c]) for c in range(c0, c0 + 4))       # this launch's smallest class maximum (|scaled value|)
    c = _chain(pol, n)
    errs["f16x2"], gerrs["f16x2"] = _errs(c, want), _grad_errs(pol.G, batch[0], c)
    pol.h2_overflow.zero_()
    pol.step_gemm = "bf16x3"
    pol.minibatch_grad(*batch, 0.2, dump=True)
    torch.cuda.synchronize()
    c = _chain(pol, n)
    errs["bf16x3"], gerrs["bf16x3"] = _errs(c, want), _grad_errs(pol.G, batch[0], c)
    pol.gemm = "f32"
    pol.minibatch_grad(*batch, 0.2)
    torch.cuda.synchronize()
    errs["f32"] = _errs({kk: untile((pol.saves if kk in pol.saves else pol.dz)[kk], n, w) for kk, w in WIDTH.items()}, want)
    print("\nscales of the %s classes 2^%d too large (smallest class maximum %.3g of |scaled value|; fp16x2 launch %s): "
          "max |got - fp64| / max |fp64|" % (classes, k, low, "REFUSED" if refused[0] else "accepted"))
    for arith in errs:
        print("  %-6s chain %s" % (arith, " ".join("%s %.2e" % (kk, e) for kk, e in errs[arith].items())))
        if arith in gerrs:
            print("  %-6s grad  %s" % (arith, " ".join("%s %.2e" % (kk, e) for kk, e in gerrs[arith].items())))
    assert (low < H2_CLASS_FLOOR) == (classes == "dz" and k > 10), low
    if low < H2_CLASS_FLOOR:
        assert refused == (1, 1.0), refused
        return
    assert refused == (0, 0.0), refused
    bar = 2e-5 if classes == "act" or k <= 6 else 4e-5 * 2.0 ** (k - 8)       # (the activation window sits 5 binades higher)
    for kk in WIDTH:
        assert errs["f16x2"][kk] <= bar, (kk, errs["f16x2"][kk], bar)
    for kk, e in gerrs["f16x2"].items():
        assert e <= bar, (kk, e, bar)


def _grad_errs(G, x, c):
    """dW = dZ^T A and db = colsum(dZ) of the launch against float64 on the chain values it dumped, per block (as
    tests/test_fused_h2_gpu.py::test_h2_gradient_against_fp64_and_bf16x3)."""
    a = [x.double(), c["h1"].double(), c["h2"].double(), c["h3"].double()]
    dz = [c["dz1"].double(), c["dz2"].double(), c["dz3"].double(), c["dz4"].double()]
    views = [(G[:256 * 80].view(256, 80)[:, :73], G[20480:20736]), (G[20736:53504].view(128, 256), G[53504:53632]),
             (G[53632:70016].view(128, 128), G[70016:70144]), (G[70144:74240].view(32, 128), G[74240:74272])]
    out = {}
    for l, ((W, b), A, Z) in enumerate(zip(views, a, dz)):
        W64, b64 = Z.T @ A, Z.sum(0)
        out["dW%d" % (l + 1)] = float((W.double() - W64).abs().max()) / (float(W64.abs().max()) + 1e-30)
        out["db%d" % (l + 1)] = float((b.double() - b64).abs().max()) / (float(b64.abs().max()) + 1e-30)
    return out


@pytest.mark.parametrize("where", ["x_nan", "adv_nan", "x_inf"])
def test_h2_nan_or_inf_in_the_data_refuses_the_step(where):
    """One quiet NaN in one element of x, a NaN in one row's advantage (it reaches the gradient classes only), or an inf in x; every
    other value finite.  The launch sets the sticky word and marks its gradient invalid, the step counter stays, and mlp_adam_step
    leaves weights, moments and both plane buffers bit for bit as they were."""
    from fly_bproject_amd.policy import ERR_SLOT
    n = 4099
    net, ref, pol, batch = _setup(n, 19, gemm="f16x2")
    pol.minibatch_grad(*batch, 0.2, fuse_norm=True)                    # one ordinary step
    pol.adam_step(norm_ready=True)
    torch.cuda.synchronize()
    assert int(pol.step) == 1 and int(pol.h2_overflow) == 0
    keep = [t.clone() for t in (pol.P, pol.exp_avg, pol.exp_avg_sq, pol.PH, pol.PTH, pol.PB, pol.PTB)]
    x, action, old_logp, adv, target, var = [t.clone() for t in batch]
    if where == "x_nan":
        x[1234, 17] = float("nan")
    elif where == "adv_nan":
        adv[2345] = float("nan")
    else:
        x[1234, 17] = float("inf")
    pol.minibatch_grad(x, action, old_logp, adv, target, var, 0.2, fuse_norm=True)
    pol.adam_step(norm_ready=True)
    torch.cuda.synchronize()
    assert int(pol.h2_overflow) == 1 and float(pol.G[ERR_SLOT]) == 1.0 and int(pol.step) == 1
    for name, a, b in zip(("P", "m", "v", "PH", "PTH", "PB", "PTB"), keep,
                          (pol.P, pol.exp_avg, pol.exp_avg_sq, pol.PH, pol.PTH, pol.PB, pol.PTB)):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("where", ["obs_nan", "obs_inf"])
def test_dqn_h2_nan_or_inf_in_the_data_sets_the_overflow_word(where):
    """The DQN update's fp16x2 launch: a NaN or an inf in one element of one chunk's observations sets its overflow word -- DQN.update
    counts one refused fp16x2 update (formed again in bf16x3).  (A NaN reward does not reach a class: the Huber derivative's clamp
    turns it into -1 in both arithmetics.)"""
    from tests.test_dqn import _bare_dqn
    torch.manual_seed(6)
    chunks = _batch(2, 4096, 9)
    d = _bare_dqn(rows=4096, fused=True, gemm="f16x2")
    _perturb_target(d)
    st = _state(d)
    d.update(chunks)
    torch.cuda.synchronize()
    assert d.h2_calibrated and d.h2_overflows == 0
    _restore(d, st)
    obs = chunks[1][0].clone()
    obs[777, 5] = float("nan") if where == "obs_nan" else float("inf")
    bad = [chunks[0], (obs,) + tuple(chunks[1][1:])]
    d.update(bad)
    torch.cuda.synchronize()
    assert d.h2_overflows == 1 and int(d.packed.h2_overflow) == 0
