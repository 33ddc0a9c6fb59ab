"""GPU (-m gpu): the optimizer launches `mlp_adam_step` (all three launch forms) and `dqn_adam_soft_update`, driven DIRECTLY from
constructed states, against float64 torch-equivalent Adam (tests/adam_ref.py) on every buffer they write.

Every bound is counted from the kernel source (csrc/mlp_adam.inc, csrc/dqn_mfma.hip: `-ffp-contract=off`, every operation rounds
once); none is fitted to what the kernels give.  The derivations are in tests/adam_ref.py (per element) and below (the norm).

Norm (assertion 2): all summands are squares, so the relative error of the sum is at most (roundings on the longest path) * 2^-24,
and the square root halves it and adds one.  Longest paths, from the source:
  two launches  (mlp_adam_norm_kernel + apply):  g = G * grad_scale [1; * mask exact] -> g * g [the square doubles g's: 2, + 1]
                -> wave tree __shfl_down 32..1 [6] -> 16 wave sums added serially from 0 [15: 0 + x is exact] -> partial;
                apply: <= 1 partial per thread [0 + x exact] -> wave tree [6] -> 16 wave sums [15] -> * part_scale (1.0f) [0]
                = 45 on the sum  ->  K_n = 45 / 2 + 1 = 23.5
  self_norm     (apply sums the gradient itself): a = g.x * grad_scale * k.x [1] -> a * a [2 + 1] -> (a*a + b*b) + (c*c + d*d) [2]
                -> t += over ceil(18568 / 1024) = 19 trips [18: the first adds to 0] -> wave tree [6] -> 16 wave sums [15]
                = 44  ->  K_n = 23
  norm_ready    (partials from the gradient reduction, of the UNSCALED gradient): a = g.x * mk.x [exact] -> a * a [1] ->
                (a*a + b*b) + (c*c + d*d) [2] -> wave tree [6] -> partial; apply: 291 partials, <= 1 per thread -> wave tree [6]
                -> 16 wave sums [15] -> * part_scale = grad_scale * grad_scale [1 on the host, 1 for the product]
                = 32  ->  K_n = 17
plus what gradual underflow of the squares can add (69 587 * 2^-150 absolute on the sum; nothing at these norms)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_NORM = {"two_launch": 23.5, "self_norm0": 23.0, "self_norm1": 23.0, "norm_ready": 17.0}
BAR_S = 2e-5                    # the bar the suite holds every MLP tensor to (tests/test_ppo_gpu.py, tests/test_fused_h2_gpu.py)
LR, BETAS, EPS, MAX_NORM = 1e-3, (0.9, 0.999), 1e-8, 1.0
CANARY16, CANARY32 = 0x5AC3, -7

FORMS = ("two_launch", "self_norm0", "self_norm1", "norm_ready")
PLANES = ("f32", "bf16x3", "f16x2")
STEPS = (0, 1, 2, 9, 74, 999, 99999)
SCALES = (1.0, 0.5, 0.125)
REGIMES = (0.0, 1e-8, 0.5, 0.999, 1.001, 2.0, 1e3)


def _cases():
    """Every launch form with every clip regime and with every arithmetic; every step count and grad_scale occurs.  (Step count 0
    never meets the norms 0 and 1e-8: with m = v = 0 and no gradient to speak of nothing moves, and there is no step size to
    measure.)"""
    out = []
    for fi, form in enumerate(FORMS):
        for ri, regime in enumerate(REGIMES):
            out.append((form, PLANES[(ri + fi) % 3], STEPS[(ri + 3 * fi + 2) % 7], SCALES[(ri + fi) % 3], regime))
    for axis, k in ((PLANES, 1), (STEPS, 2), (SCALES, 3), (REGIMES, 4)):
        assert {c[k] for c in out} == set(axis)
    assert {(c[0], c[1]) for c in out} == {(f, p) for f in FORMS for p in PLANES}
    assert {(c[0], c[4]) for c in out} == {(f, r) for f in FORMS for r in REGIMES}
    return out


# ---- the constructed state ---------------------------------------------------------------------------------------------------------
CLASS_OF_SLOT = ("bulk",) * 8 + ("g0", "zero", "tiny20", "tiny25", "cancel3", "cancel6", "epsdom", "bulk")      # by i % 16
LIVE_CLASSES = ("bulk", "g0", "zero", "tiny20", "tiny25", "cancel3", "cancel6", "epsdom")


def _classes(mask, packed):
    """Class name of every packed element: the pattern above over i % 16 (every region boundary is a multiple of 64 and every
    row length one of 16, so each class falls into every Adam block of 1024, every weight layer and every bias region);
    `masked` wherever grad_mask == 0 -- those sit where the layout has its padding (W1's columns 73..79, the unused parts of
    W4 and b4), not in every block: W2, W3 and their biases have none."""
    cls = np.array([CLASS_OF_SLOT[i % 16] for i in range(packed)], dtype=object)
    cls[mask == 0] = "masked"
    return cls


def _build_state(mask, regions, steps, gs, regime, seed, err_slot, P0, coef_of=None):
    """fp32 (P, G, m, v) and the class map.  `regime` = the float64 norm of the masked, scaled gradient (None: leave G's scale)."""
    n = mask.size
    rng = np.random.default_rng(seed)
    cls = _classes(mask, n)
    is_ = lambda c: cls == c       # noqa: E731
    sign = rng.choice([-1.0, 1.0], n)
    a = 10.0 ** rng.uniform(-12.0, 0.0, n)                      # bulk: |g| log-uniform over 12 decades
    hist = max(steps, 1)
    h1 = np.where(is_("bulk"), 1.0 - 0.9 ** steps, 1.0 - 0.9 ** hist)       # (bulk at step 0: m = v = 0, as a fresh optimizer has them)
    h2 = np.where(is_("bulk"), 1.0 - 0.999 ** steps, 1.0 - 0.999 ** hist)
    G = sign * a * rng.uniform(0.5, 1.5, n)
    m = a * rng.uniform(-0.7, 0.7, n) * h1                      # moments consistent with a history of such gradients
    v = a * a * rng.uniform(0.6, 1.4, n) * h2
    c3, c6 = is_("cancel3"), is_("cancel6")
    canc = c3 | c6
    G[canc] = (sign * 10.0 ** rng.uniform(-6.0, -1.0, n))[canc]
    v[canc] = (G * G * h2)[canc]
    ed = is_("epsdom")                                          # sqrt(v') / sqrt(bc2) of the order of eps: 1e-9 .. 1e-7
    r = 10.0 ** rng.uniform(-9.0, -7.0, n)
    bc2s = math.sqrt(1.0 - 0.999 ** (steps + 1))
    G[ed] = (sign * r * 0.3)[ed]
    m[ed] = (r * rng.uniform(-0.5, 0.5, n))[ed]
    v[ed] = ((r * bc2s) ** 2)[ed]
    G[is_("g0") | is_("zero")] = 0.0
    m[is_("zero")] = 0.0
    v[is_("zero")] = 0.0
    scaled = is_("bulk") | canc | ed
    if regime is not None:
        base = math.sqrt(float(np.sum((G * gs * mask)[scaled] ** 2)))
        G[scaled] *= regime / base
    for name, val in (("tiny20", 1e-20), ("tiny25", 1e-25)):    # g * g subnormal / zero in fp32, v = 0
        k = is_(name)
        G[k] = (sign * (0.0 if regime == 0.0 else val))[k]
        m[k] = 0.0
        v[k] = 0.0
    mk = is_("masked")                                          # the junk a GEMM leaves in padding: finite, up to 1e6
    G[mk] = (sign * 10.0 ** rng.uniform(-3.0, 6.0, n))[mk]
    G[err_slot] = 0.0                                           # the invalid-gradient mark stays 0
    m[mk] = (rng.uniform(-1e-3, 1e-3, n))[mk]
    v[mk] = (rng.uniform(1e-8, 1e-6, n))[mk]
    P = P0.astype(np.float64).copy()
    P[mk] = (rng.uniform(-0.05, 0.05, n))[mk]                   # (so that "P' == P bit for bit" is not 0 == 0)
    G32 = G.astype(np.float32)
    # cancellation in m': beta1 m = -(1 - beta1) g (1 + delta), g the CLIPPED gradient of the fp32 G the kernel will read
    g64 = G32.astype(np.float64) * gs * mask
    norm = math.sqrt(float(np.sum(g64 * g64)))
    coef = min(1.0, MAX_NORM / (norm + 1e-6)) if coef_of is None else coef_of
    m[c3] = (-(0.1 / 0.9) * g64 * coef * (1.0 + 1e-3))[c3]
    m[c6] = (-(0.1 / 0.9) * g64 * coef * (1.0 + 1e-6))[c6]
    for name in LIVE_CLASSES:       # each class is there after masking: in every region, and in every Adam block (1024 elements)
        k = is_(name)               # that has parameters at all (one lies wholly in the unused rows of the last layer)
        assert all(k[b * 1024:(b + 1) * 1024].any() for b in range((n + 1023) // 1024) if mask[b * 1024:(b + 1) * 1024].any()), name
        assert all(k[lo:hi].any() for lo, hi in regions), name
    assert mk.any() and G[mk].max() > 1e5
    return P.astype(np.float32), G32, m.astype(np.float32), v.astype(np.float32), cls


# ---- one step's numerical assertions (2 - 5) ---------------------------------------------------------------------------------------
def _check_numbers(tag, form, inp, out, steps, gs, cls, k_norm, figures, lr=LR, clip=True, echo=True):
    """inp / out: fp32 numpy P, G, m, v (+ out["norm"]) exactly as in device memory before / after the launch."""
    hp = R.hyper(lr, BETAS, EPS)
    mask = inp["mask"].astype(np.float64)
    P, G, m, v = (inp[k].astype(np.float64) for k in ("P", "G", "m", "v"))
    if clip:
        P2, m2, v2, norm, coef = R.clip_adam(P, G, m, v, steps, mask, lr, BETAS, EPS, MAX_NORM, gs)
        # 2. the norm
        if norm == 0.0:
            assert out["norm"] == 0.0
            nerr = 0.0
        else:
            nerr = abs(float(out["norm"]) - norm) / norm / R.U
            bound = k_norm + 69587 * 2.0 ** -150 / (2 * norm * norm) / R.U
            assert nerr <= bound, (tag, "norm", nerr, bound)
        assert abs(norm + 1e-6 - MAX_NORM) >= 1e-4 * MAX_NORM, "the clip branch must not be ambiguous"
        clipped = coef < 1.0
        e_c = R.coef_error(norm, clipped, k_norm)
        g = G * gs * mask * coef
    else:
        P2, _, m2, v2 = R.dqn_adam_soft(P, P, G, m, v, steps, mask, lr, BETAS, EPS, 0.0)
        norm, nerr, clipped, e_c = float("nan"), 0.0, False, -R.UG      # g = G * mask: no rounding at all
        g = G * mask
    upd = P - P2
    live = mask == 1
    e_m, e_v = R.moment_bounds(g, m, v, e_c, hp)
    w = R.update_weight(v2, steps, hp)
    dP = P - out["P"].astype(np.float64)
    # 3. the uniform step-size factor, over the bulk class and the g = 0 class (the elements adam_ref.step_size_factor admits)
    pool = live & ((cls == "bulk") | (cls == "g0"))
    s, sel, share = R.step_size_factor(dP[pool], upd[pool], w[pool], lr, g[pool], v2[pool], hp)
    cnt = int(sel.sum())
    assert cnt >= 1000, (tag, cnt)
    assert abs(s - 1.0) <= BAR_S, (tag, "step-size factor", s - 1.0)
    # 4. element by element, s divided out
    e_p, w = R.param_bound(P, m2, v2, upd, e_m, e_v, steps, hp, s)
    e_p = e_p + R.factor_uncertainty(e_p[pool], upd[pool], sel, share, hp) * np.abs(upd)
    r_m = np.abs(out["m"] - m2) / e_m
    r_v = np.abs(out["v"] - v2) / e_v
    r_p = np.abs(out["P"] - (P - upd * (1.0 + (s - 1.0) * w))) / e_p
    worst = {}
    for name, r in (("m", r_m), ("v", r_v), ("P", r_p)):
        k = int(np.argmax(np.where(live, r, 0.0)))
        worst[name] = float(r[k])
        assert r[k] <= 1.0, (tag, name, "element", k, cls[k], "error / bound", float(r[k]))
    if clip and not clipped and float(np.float32(gs)) == gs:
        # coef == 1 EXACTLY: then m' is fl(fl(b1f m) + fl(w1f fl(G gs))) to the bit (checked where nothing underflows)
        f = np.float32
        t1, t2 = f(0.9) * inp["m"], (f(1) - f(0.9)) * (inp["G"] * f(gs))
        em = t1 + t2
        tiny = float(np.finfo(f).tiny)
        ok = live & np.all([(np.abs(x) >= tiny) | (x == 0) for x in (t1, t2, em, inp["G"] * f(gs))], axis=0)
        assert ok.sum() > 0.9 * live.sum()
        assert np.array_equal(em[ok].view(np.int32), out["m"][ok].view(np.int32)), (tag, "coef must be exactly 1 when not clipped")
    # zero class: nothing moves, bit for bit
    z = live & (cls == "zero")
    if z.any():
        assert np.array_equal(out["P"][z].view(np.int32), inp["P"][z].view(np.int32)) and not out["m"][z].any() and not out["v"][z].any()
    # 5. masked elements: P' bit-equal, the moments decay by one rounded product (and fp32(beta) for beta)
    dead = ~live
    assert np.array_equal(out["P"][dead].view(np.int32), inp["P"][dead].view(np.int32)), (tag, "masked P moved")
    assert np.all(np.abs(out["m"][dead] - 0.9 * m[dead]) <= np.abs(m[dead]) * (hp["db1"] + R.UG * 0.9) + R.SUB), (tag, "masked m")
    assert np.all(np.abs(out["v"][dead] - 0.999 * v[dead]) <= v[dead] * (hp["db2"] + R.UG * 0.999) + R.SUB), (tag, "masked v")
    line = ("%-44s K_n %4.1f norm err %6.2f u  clipped %d  s-1 %+.3e (n=%d)  worst err/bound m' %.3f v' %.3f P' %.3f"
            % (tag, k_norm, nerr, clipped, s - 1.0, cnt, worst["m"], worst["v"], worst["P"]))
    if echo:
        print(line)
    figures.append(line)
    return {"s": s, "e_m": e_m, "e_v": e_v, "e_p": e_p, "upd": upd, "live": live, "worst": worst, "clipped": clipped}


# ---- the copies and the fp16x2 table (6, 7) ----------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _ppo_offsets():
    from fly_bproject_amd import policy as Pm
    return (Pm.OFF_W1, Pm.OFF_W2, Pm.OFF_W3, Pm.OFF_W4)


def _check_copies(tag, pol, before, planes, rescale_ok=False):
    """PF, PT (and the planes that are live) == derived(P' the kernel left), bit for bit; buffers that are not passed wholly
    unchanged; words no index map addresses unchanged (the maps are onto: there are none, which is asserted, so the whole-buffer
    comparison leaves no word unchecked)."""
    from fly_bproject_amd import policy as Pm
    wsc = pol.h2_scales[Pm.H2_W0:Pm.H2_W0 + 4].clone() if planes == "f16x2" else None
    d = R.derived(pol.P, pol, wsc, _ppo_offsets())
    live = {"F": pol.PF, "T": pol.PT}
    if planes != "f32":
        live.update({"FB": pol.PB, "TB": pol.PTB})
    if planes == "f16x2":
        live.update({"FH": pol.PH, "TH": pol.PTH})
    for name, buf in live.items():
        dst, val = d[name]
        free = R.unaddressed(dst, buf.numel(), buf.device)
        assert torch.equal(_bits(buf)[free], _bits(before[name])[free]), (tag, name, "an unaddressed word changed")
        assert dst.numel() + free.numel() == buf.numel()
        assert torch.equal(_bits(buf)[dst], _bits(val)), (tag, name, "copy != derived(P')")
    for name, buf in (("FB", pol.PB), ("TB", pol.PTB), ("FH", pol.PH), ("TH", pol.PTH)):
        if name not in live:
            assert torch.equal(buf, before[name]), (tag, name, "a buffer that is not passed changed")


def _check_table(tag, pol, before_tab, steps_after, planes, expect_rescale=False, P_before=None):
    from fly_bproject_amd import policy as Pm
    tab = pol.h2_scales
    if planes != "f16x2":
        assert torch.equal(_bits(tab), _bits(before_tab)), (tag, "the table is not passed")
        return
    par = steps_after & 1
    lo = Pm.H2_WMAX + par * Pm.H2_WMAX_SLOTS
    written = torch.zeros(tab.numel(), dtype=torch.bool, device=tab.device)
    written[Pm.H2_SINCE + par] = True
    written[lo:lo + Pm.H2_WMAX_SLOTS] = True
    since_other = float(before_tab[Pm.H2_SINCE + (par ^ 1)])
    if expect_rescale:
        written[Pm.H2_W0:Pm.H2_W0 + 4] = True
        written[Pm.H2_INV + Pm.H2_W0:Pm.H2_INV + Pm.H2_W0 + 4] = True
        assert float(tab[Pm.H2_SINCE + par]) == 1.0
        offs = list(_ppo_offsets())
        ends = (Pm.OFF_B1, Pm.OFF_B2, Pm.OFF_B3, Pm.OFF_B4)
        for l in range(4):      # a rescale derives the scale from the weights as they stood BEFORE the step
            want = Pm.h2_weight_scale(float(P_before[offs[l]:ends[l]].abs().max()))
            assert float(tab[Pm.H2_W0 + l]) == want and float(tab[Pm.H2_INV + Pm.H2_W0 + l]) == 1.0 / want, (tag, "rescale", l)
    else:
        assert float(tab[Pm.H2_SINCE + par]) == since_other + 1.0, (tag, "H2_SINCE")
    assert torch.equal(_bits(tab)[~written], _bits(before_tab)[~written]), (tag, "a table word outside the written parity changed")
    # the written parity's maxima: per 64 packed elements max |P'_hip| for weight groups, 0 for bias groups
    Pp = torch.zeros(Pm.H2_WMAX_SLOTS * 64, device=tab.device)
    Pp[:Pm.PACKED] = pol.P.abs()
    want = Pp.view(-1, 64).max(dim=1).values
    o = torch.arange(Pm.H2_WMAX_SLOTS, device=tab.device) * 64
    is_w = (o < Pm.OFF_B1) | ((o >= Pm.OFF_W2) & (o < Pm.OFF_B2)) | ((o >= Pm.OFF_W3) & (o < Pm.OFF_B3)) | ((o >= Pm.OFF_W4) & (o < Pm.OFF_B4))
    want = torch.where(is_w, want, torch.zeros_like(want))
    assert torch.equal(_bits(tab[lo:lo + Pm.H2_WMAX_SLOTS].contiguous()), _bits(want)), (tag, "H2_WMAX")


def _snapshot(pol):
    return {"F": pol.PF.clone(), "T": pol.PT.clone(), "FB": pol.PB.clone(), "TB": pol.PTB.clone(), "FH": pol.PH.clone(),
            "TH": pol.PTH.clone(), "tab": pol.h2_scales.clone(), "P": pol.P.clone()}


def _plant_canaries(pol, planes):
    """Buffers the launch is not given carry a canary pattern in every word (words of a live buffer that no map addresses would
    too: there are none)."""
    if planes == "f32":
        pol.PB.fill_(CANARY16)
        pol.PTB.fill_(CANARY16)
    if planes != "f16x2":
        pol.PH.fill_(CANARY16)
        pol.PTH.fill_(CANARY16)


def _regions():
    from fly_bproject_amd import policy as Pm
    return ((Pm.OFF_W1, Pm.OFF_B1), (Pm.OFF_B1, Pm.OFF_W2), (Pm.OFF_W2, Pm.OFF_B2), (Pm.OFF_B2, Pm.OFF_W3), (Pm.OFF_W3, Pm.OFF_B3),
            (Pm.OFF_B3, Pm.OFF_W4), (Pm.OFF_W4, Pm.OFF_B4), (Pm.OFF_B4, Pm.PACKED))


def _policy(planes, lr=LR, rows=32, seed=11):
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(seed)
    pol = PackedPolicy(Net(73, 18).to(DEV), DEV)
    pol.init_training(rows, lr=lr, betas=BETAS, eps=EPS, max_norm=MAX_NORM)
    pol.gemm = planes
    assert pol.h2_live() == (planes == "f16x2") and pol._planes_live() == (planes != "f32")
    return pol


def _np(t):
    return t.detach().cpu().numpy().copy()


def _put(dst, a):
    dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dst.device))


def _set_step_words(pol, form, steps):
    """-> (index of the word the launch reads, index of the word that must hold steps + 1 afterwards)."""
    read = 1 if form == "self_norm1" else 0
    pol._step_idx = read
    pol._step2[read] = steps
    pol._step2[read ^ 1] = CANARY32
    return read, (read ^ 1) if form.startswith("self_norm") else read


def _launch(pol, form, gs):
    if form.startswith("self_norm"):
        pol.adam_step(grad_scale=gs, self_norm=True)
    elif form == "norm_ready":
        pol.adam_step(grad_scale=gs, norm_ready=True)
    else:
        pol.adam_step(grad_scale=gs)
    torch.cuda.synchronize()


def _real_gradient(pol, planes, steps, gs, regime, seed):
    """norm_ready: G and the norm partials come from one real minibatch_grad(fuse_norm=True) on the network's own weights; the
    gradient is linear in 1 / global_rows, which steers its norm to the regime (0: 1 / inf)."""
    from tests.test_mlp_train_gpu import _setup
    n = 4099
    _, _, src, batch = _setup(n, seed, gemm="f32")       # (only for the batch: x, action, old_logp, adv, target, var)
    x, action, old_logp, adv, target, var = batch
    del src
    mask = _np(pol.grad_mask)

    def grad(rows, fuse):
        if planes == "f16x2":
            pol.calibrate_h2(x, action, old_logp, adv, target, var, 0.2, global_rows=rows)
        pol.minibatch_grad(x, action, old_logp, adv, target, var, 0.2, global_rows=rows, fuse_norm=fuse)
        torch.cuda.synchronize()
        g = _np(pol.G).astype(np.float64) * gs * mask
        return math.sqrt(float(np.sum(g * g)))
    rows = float("inf")
    if regime != 0.0:
        rows = n * grad(float(n), False) / regime
    return lambda: grad(rows, True)


@pytest.fixture(scope="module")
def figures():
    lines = []
    yield lines
    print("\n==== adam step against float64: figures of this run ====")
    for ln in lines:
        print(ln)


@pytest.mark.parametrize("form,planes,steps,gs,regime", _cases())
def test_one_launch_from_a_constructed_state(form, planes, steps, gs, regime, figures):
    from fly_bproject_amd import policy as Pm
    tag = "%s/%s/t=%d/gs=%g/norm=%g" % (form, planes, steps, gs, regime)
    pol = _policy(planes, rows=4128 if form == "norm_ready" else 32)
    mask = _np(pol.grad_mask)
    seed = 1000 + 100 * FORMS.index(form) + 10 * STEPS.index(steps) + REGIMES.index(regime)
    P, G, m, v, cls = _build_state(mask, _regions(), steps, gs, None if form == "norm_ready" else regime, seed, Pm.ERR_SLOT, _np(pol.P))
    read, wrote = _set_step_words(pol, form, steps)
    if form == "norm_ready":
        _put(pol.exp_avg, m)
        _put(pol.exp_avg_sq, v)
        fire = _real_gradient(pol, planes, steps, gs, regime, seed)
        _set_step_words(pol, form, steps)
        pol.refresh()
        _plant_canaries(pol, planes)
        fire()                                  # leaves G, the partials, and advances the step word
        assert int(pol._step2[read]) == steps + 1, "the gradient launch was refused"
        cls = np.where(mask == 1, "bulk", "masked").astype(object)     # (the element classes are those of a constructed G)
    else:
        _put(pol.P, P)
        _put(pol.exp_avg, m)
        _put(pol.exp_avg_sq, v)
        _put(pol.G, G)
        pol.refresh()
        _plant_canaries(pol, planes)
    inp = {"P": _np(pol.P), "G": _np(pol.G), "m": _np(pol.exp_avg), "v": _np(pol.exp_avg_sq), "mask": mask}
    before = _snapshot(pol)
    _launch(pol, form, gs)
    # 1. the step words
    assert int(pol._step2[wrote]) == steps + 1, (tag, "step word")
    assert int(pol._step2[wrote ^ 1]) == (steps if form.startswith("self_norm") else CANARY32), (tag, "the other step word")
    out = {"P": _np(pol.P), "m": _np(pol.exp_avg), "v": _np(pol.exp_avg_sq), "norm": float(pol._norm_ws[0])}
    _check_numbers(tag, form, inp, out, steps, gs, cls, K_NORM[form], figures)
    _check_copies(tag, pol, before, planes)
    _check_table(tag, pol, before["tab"], steps + 1, planes)


# ---- (b) a trajectory ---------------------------------------------------------------------------------------------------------------
TRAJ_STEPS = 260


@pytest.mark.parametrize("form", ["self_norm", "two_launch"])
def test_trajectory_of_260_steps_on_prescribed_gradients(form, figures):
    """Resynchronised (the reference restarts every step from the kernel's own state: assertions 1 - 7 at every step) and
    free-running (float64 from the common start on the same gradients: the end state within the summed per-step bounds plus the
    accumulated step-size bias).  lr = 1e-3 -> rescale period 64: the applied steps 64, 128, 192, 256 (counting from 0)
    rescale, and one weight per layer walks from 2^-3 - 20 lr across 2^-3, so the first rescale must change every scale."""
    from fly_bproject_amd import policy as Pm
    pol = _policy("f16x2")
    mask = _np(pol.grad_mask)
    n = mask.size
    rng = np.random.default_rng(77)
    P0 = _np(pol.P) * 0.5                       # every |w| < 2^-4: the walkers are their layers' maxima
    offs = _ppo_offsets()
    walkers = np.array([o + 3 for o in offs])   # row 0, column 3 of each weight matrix: unmasked
    assert np.all(mask[walkers] == 1)
    P0[walkers] = 2.0 ** -3 - 20 * LR
    assert np.max(np.abs(np.delete(P0, walkers))) < 2.0 ** -4
    _put(pol.P, P0)
    pol.refresh()
    hp = R.hyper(LR, BETAS, EPS)
    scales0 = _np(pol.h2_scales[Pm.H2_W0:Pm.H2_W0 + 4])
    assert list(scales0) == [2.0 ** 15] * 4
    free = {"P": P0.astype(np.float64), "m": np.zeros(n), "v": np.zeros(n)}
    acc = {"P": np.zeros(n), "m": np.zeros(n), "v": np.zeros(n)}
    cls = np.where(mask == 1, "bulk", "masked").astype(object)
    clipped, rescales, changed, worst_s = [], [], [], 0.0
    quiet = []
    pol._step2[0] = 0
    pol._step2[1] = 0
    for t in range(TRAJ_STEPS):
        scale = 10.0 ** (-2.6 + 1.3 * math.sin(0.37 * t) + 0.2 * rng.standard_normal())      # the norm swings around max_norm
        G = (rng.standard_normal(n) * scale)
        G[walkers] = -50.0 * scale              # constant sign: the walkers climb by about lr per step
        G[Pm.ERR_SLOT] = 0.0
        _put(pol.G, G.astype(np.float32))
        inp = {"P": _np(pol.P), "G": _np(pol.G), "m": _np(pol.exp_avg), "v": _np(pol.exp_avg_sq), "mask": mask}
        before = _snapshot(pol)
        idx = pol._step_idx
        par = (t + 1) & 1
        since = float(before["tab"][Pm.H2_SINCE + (par ^ 1)])
        is_rescale = since >= 64
        if form == "self_norm":
            pol.adam_step(self_norm=True)
        else:
            pol.adam_step()
        torch.cuda.synchronize()
        tag = "traj/%s/t=%d" % (form, t)
        if form == "self_norm":
            assert pol._step_idx == idx ^ 1 and int(pol._step2[idx ^ 1]) == t + 1 and int(pol._step2[idx]) == t, tag
        else:
            assert int(pol._step2[0]) == t + 1 and int(pol._step2[1]) == 0, tag
        out = {"P": _np(pol.P), "m": _np(pol.exp_avg), "v": _np(pol.exp_avg_sq), "norm": float(pol._norm_ws[0])}
        res = _check_numbers(tag, "self_norm0" if form == "self_norm" else form, inp, out, t, 1.0, cls,
                             K_NORM["self_norm0" if form == "self_norm" else form], quiet, echo=False)
        _check_copies(tag, pol, before, "f16x2")
        _check_table(tag, pol, before["tab"], t + 1, "f16x2", expect_rescale=is_rescale, P_before=before["P"])
        if is_rescale:
            rescales.append(t)
        if not torch.equal(pol.h2_scales[:40], before["tab"][:40]):
            changed.append(t)
        clipped.append(res["clipped"])
        worst_s = max(worst_s, abs(res["s"] - 1.0))
        for k, e in (("P", res["e_p"]), ("m", res["e_m"]), ("v", res["e_v"])):
            acc[k] += np.where(res["live"], e, 0.0)
        acc["P"] += abs(res["s"] - 1.0) * np.abs(res["upd"])
        free["P"], free["m"], free["v"], _, _ = R.clip_adam(free["P"], inp["G"], free["m"], free["v"], t, mask, LR, BETAS, EPS, MAX_NORM, 1.0)
    assert rescales == [64, 128, 192, 256], rescales
    assert set(changed) <= set(rescales) and 64 in changed, (changed, "the crossing must change a published scale")
    assert list(_np(pol.h2_scales[Pm.H2_W0:Pm.H2_W0 + 4])) != list(scales0)
    assert any(clipped) and not all(clipped)
    live = mask == 1
    ratios = {}
    for k, got in (("P", _np(pol.P)), ("m", _np(pol.exp_avg)), ("v", _np(pol.exp_avg_sq))):
        r = np.abs(got - free[k])[live] / acc[k][live]
        ratios[k] = float(r.max())
    line = ("trajectory %-10s 260 steps: clipped on %d, worst |s-1| %.3e; resynchronised worst err/bound (last lines of the run); "
            "free-running end state err / summed bound: m %.3f v %.3f P %.3f"
            % (form, sum(clipped), worst_s, ratios["m"], ratios["v"], ratios["P"]))
    print(line)
    figures.append(line)
    figures.extend(quiet[:3] + quiet[63:66] + quiet[-2:])
    for k in ratios:
        assert ratios[k] <= 1.0, (k, ratios[k])


# ---- (c) dqn_adam_soft_update -------------------------------------------------------------------------------------------------------
DQN_LR, TAU = 3e-4, 0.995


def _dqn_call(d, guard=None):
    from fly_bproject_amd import _lib
    pk = d.packed
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(d._lib.dqn_adam_soft_update(p(pk.P), p(pk.PF), p(pk.PT), p(pk.P_tgt), p(pk.PF_tgt), p(pk.idx_f), p(pk.idx_t),
                                           p(pk.G), p(pk.grad_mask), p(pk.exp_avg), p(pk.exp_avg_sq), p(pk.step),
                                           C.c_float(DQN_LR), C.c_float(0.9), C.c_float(0.999), C.c_float(EPS), C.c_float(TAU),
                                           *pk.plane_args(), p(guard) if guard is not None else None, _lib.stream_ptr()),
               "dqn_adam_soft_update")
    torch.cuda.synchronize()


def _dqn_buffers(pk):
    return {"P": pk.P, "P_tgt": pk.P_tgt, "m": pk.exp_avg, "v": pk.exp_avg_sq, "PF": pk.PF, "PT": pk.PT, "PF_tgt": pk.PF_tgt,
            "QB": pk.QB, "QTB": pk.QTB, "QB_tgt": pk.QB_tgt, "step": pk.step}


def check_dqn_adam_soft(tag, pk, inp, tgt_in, steps, cls, figures):
    """What ONE applied `dqn_adam_soft_update` must have left in `pk` (the packed pair, or any object with its buffers and index maps
    as the launch left them), given `inp` (fp32 numpy P, G, m, v, mask in front of the launch), `tgt_in` (float64 P_tgt in front of it)
    and the step count in front of it: the step word, P' / m' / v' element by element within their counted bounds (_check_numbers),
    P_tgt' within its own, every fragment copy and bf16x3 plane bit-equal to its derivation from the masters the launch left.
    Shared by the constructed states below and the training loop's own updates (tests/test_dqn_loop_gpu.py)."""
    assert int(pk.step) == steps + 1
    out = {"P": _np(pk.P), "m": _np(pk.exp_avg), "v": _np(pk.exp_avg_sq)}
    _check_numbers(tag, "dqn", inp, out, steps, 1.0, cls, 0.0, figures, lr=DQN_LR, clip=False)
    # P_tgt' = fl(fl(P_tgt tauf) + fl(P' w)), tauf = fp32(tau), w = 1.0f - tauf (exact: Sterbenz), against float64 on the P' the
    # kernel left: two products and a sum, and |tauf - tau| on both coefficients
    p2 = out["P"].astype(np.float64)
    dtau = abs(float(np.float32(TAU)) - TAU)
    want = TAU * tgt_in + (1.0 - TAU) * p2
    bound = np.abs(tgt_in) * (dtau + R.UG * TAU) + np.abs(p2) * (dtau + R.UG * (1 - TAU)) + R.UG * (TAU * np.abs(tgt_in) + (1 - TAU) * np.abs(p2))
    got = _np(pk.P_tgt).astype(np.float64)
    err = np.abs(got - want)
    # (bound == 0 only where both masters are 0 -- the layout's padding in a training loop: there the target must be 0 exactly)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    far = np.abs(p2 - tgt_in) > 1e-2
    # (the measured mixing weight is a figure, not an assertion: a young training loop has no element this far from its target)
    line = "%-44s P_tgt' worst err/bound %.3f" % (tag, float(r.max()))
    if far.any():
        mix = float(np.median((got - tgt_in)[far] / (p2 - tgt_in)[far])) / (1.0 - TAU)
        line += "; measured (1 - tau) / 0.005 - 1 = %+.3e (fp32(0.995): %+.3e)" % (mix - 1.0, (1.0 - float(np.float32(TAU))) / (1.0 - TAU) - 1.0)
    print(line)
    figures.append(line)
    assert r.max() <= 1.0, (tag, "P_tgt", float(r.max()))
    # masked elements of the target follow the same formula (P' == P there); the copies, from what the kernel left
    for master, names in ((pk.P, {"F": pk.PF, "T": pk.PT, "FB": pk.QB, "TB": pk.QTB}), (pk.P_tgt, {"F": pk.PF_tgt, "FB": pk.QB_tgt})):
        dd = R.derived(master, pk)
        for name, buf in names.items():
            dst, val = dd[name]
            assert R.unaddressed(dst, buf.numel(), buf.device).numel() == 0     # onto: no word is left unchecked
            assert torch.equal(_bits(buf)[dst], _bits(val)), (tag, name, "copy != derived")


@pytest.mark.parametrize("steps", [0, 1, 9, 999])
def test_dqn_adam_soft_update_against_float64(steps, figures):
    from fly_bproject_amd import dqn as Dm
    from tests.test_dqn import _bare_dqn
    torch.manual_seed(5)
    d = _bare_dqn()
    pk = d.packed
    mask = _np(pk.grad_mask)
    regions = ((Dm.OFF_W1, Dm.OFF_B1), (Dm.OFF_B1, Dm.OFF_W2), (Dm.OFF_W2, Dm.OFF_B2), (Dm.OFF_B2, Dm.OFF_W3), (Dm.OFF_W3, Dm.OFF_B3),
               (Dm.OFF_B3, Dm.PACKED))
    # no clipping: coef = 1, the gradient is what it is (norm about 1: the regime the PPO cases call 0.999 .. 1.001)
    P, G, m, v, cls = _build_state(mask, regions, steps, 1.0, 1.0, 300 + steps, 76, _np(pk.P), coef_of=1.0)
    rng = np.random.default_rng(steps)
    _put(pk.P, P)
    _put(pk.P_tgt, (P.astype(np.float64) + rng.uniform(-0.02, 0.02, P.size)).astype(np.float32))
    _put(pk.exp_avg, m)
    _put(pk.exp_avg_sq, v)
    _put(pk.G, G)
    pk.step.fill_(steps)
    pk.refresh()
    tag = "dqn/t=%d" % steps
    # a refused launch (grad_invalid != 0) leaves every buffer and the step word bit-identical
    before = {k: t.clone() for k, t in _dqn_buffers(pk).items()}
    _dqn_call(d, guard=torch.ones(1, dtype=torch.int32, device=DEV))
    for k, t in _dqn_buffers(pk).items():
        assert torch.equal(_bits(t), _bits(before[k])), (tag, k, "a refused step wrote")
    inp = {"P": _np(pk.P), "G": _np(pk.G), "m": _np(pk.exp_avg), "v": _np(pk.exp_avg_sq), "mask": mask}
    tgt_in = _np(pk.P_tgt).astype(np.float64)
    _dqn_call(d, guard=torch.zeros(1, dtype=torch.int32, device=DEV))
    check_dqn_adam_soft(tag, pk, inp, tgt_in, steps, cls, figures)
