"""GPU (-m gpu): the PPO optimizer step's fp16x2 arithmetic (csrc/mlp_fused_h2.inc) against float64 on minibatches the training loop
itself produced -- heavy-tailed gradients, x maxima near 150 (or clipped to +-5 under --normalize_obs), scales lagging behind the
data -- where every other float64 test of the step runs on light-tailed synthetic rows (tests/test_mlp_train_gpu.py::_setup).

Six PPO updates at 8192 envs (seed 0) run with `PackedPolicy.minibatch_grad` wrapped: every live fp16x2 launch (fuse_norm, not
suspended: the calibration launches pass fuse_norm=False) leaves its arguments, the policy state in front of it and the gradient it
made.  Three are kept: the first and the last minibatch of the third epoch of the last update, and the minibatch of all updates whose
rows' ||dz4|| (float64) has the largest max / median.  Each is replayed from its state:
  0. under the loop's own scales, frozen: the gradient is bit for bit the loop's (the capture is faithful);
  1. the chain and every dW / db block against float64 (the bars of tests/test_fused_h2_gpu.py: 2e-5, and the chain within 2x the
     fp32-MFMA chain's error + 2e-7) under scales calibrated to the minibatch and under the loop's scales -- a class more than 6
     binades under its window is held to the lagging-scale bar of tests/test_h2_edges_gpu.py instead, 4e-5 2^(k - 8);
  2. (the heavy-tailed one) the BULK: calibrated on the whole minibatch, so that its outliers set the gradient scales, then launched
     on the rows outside the top 1 % by ||dz4|| (normalised by the whole minibatch's row count, as in the loop) and held to float64
     relative to ITS OWN maxima: the contract fs_h2.inc states for a class k binades under its window, or the refusal under the floor.
Rows at PPO's ratio-clip boundary take either branch of the surrogate in any fp32 arithmetic; each is compared with the branch it
took (_refs, _pick).  The dW / db blocks of the heavy-tailed minibatch under calibrated scales miss the 2e-5 bar (up to 1.0e-4: the
gradient classes' second fp16 term has a fixed absolute quantum, csrc/fs_h2.inc): the main test holds them to a ceiling of 2e-4, a
strict xfail holds them to 2e-5 until the arithmetic is fixed.
The tables the test prints are profiles/h2_real_minibatches.txt."""
import contextlib
import io
import math

import pytest
import torch

from tests.test_fused_h2_gpu import _errs, _fp64_chain
from tests.test_fused_step_gpu import WIDTH, _chain
from tests.test_h2_edges_gpu import _grad_errs, _restore_snapshot, _snapshot

pytestmark = pytest.mark.gpu

ITERS = 6
CLASSES = ("x", "h1", "h2", "h3", "dz4", "dz3", "dz2", "dz1")
GRADS = ("dW1", "db1", "dW2", "db2", "dW3", "db3", "dW4", "db4")


class _Weights:
    """The `ref` of _fp64_chain: the network's weights as they were in front of a launch."""

    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return self.sd


def _capture(normalize_obs):
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import PPO
    from tests.hip_helpers import make_args
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(8192, seed=0, normalize_obs=normalize_obs))
    pol = agent.policy
    assert pol.h2_live() and pol.fused_step
    per_update = agent.epoch * (agent.chuck_number - 1)
    first, last = 2 * (agent.chuck_number - 1), 3 * (agent.chuck_number - 1) - 1      # the third epoch's first and last minibatch
    kept, heavy = {}, {"ratio": 0.0}
    seen = {"launches": 0, "refused": 0}
    orig = PackedPolicy.minibatch_grad

    def patched(self, *a, **kw):
        if not (self is pol and kw.get("fuse_norm") and not self.h2_suspended):
            return orig(self, *a, **kw)
        update, j = agent.optim_step // per_update, seen["launches"] - (agent.optim_step // per_update) * per_update
        seen["launches"] += 1
        args = [t.clone() for t in a[:6]]
        rec = {"update": update, "step": j, "per_epoch": agent.chuck_number - 1, "args": args, "clip": a[6], "snap": _snapshot(self),
               "sd": {k: v.detach().clone() for k, v in agent.net.state_dict().items()}}
        r = orig(self, *a, **kw)
        rec["G"] = self.G.clone()
        rec["refused"] = int(self.h2_overflow.item())
        seen["refused"] += rec["refused"]
        rec["want"] = _fp64_chain(_Weights(rec["sd"]), *args, clip=rec["clip"])
        norm = rec["want"]["dz4"].norm(dim=1)
        rec["ratio"] = float(norm.max() / norm.median())
        if update == ITERS - 1 and j in (first, last):
            kept["first" if j == first else "last"] = rec
        if rec["ratio"] > heavy["ratio"]:
            if "rec" in heavy:
                heavy["rec"].pop("want")                            # (float64 chains are only kept for the heaviest so far)
            heavy.update(ratio=rec["ratio"], rec=rec)
        else:
            del rec["want"]
        return r

    PackedPolicy.minibatch_grad = patched
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(ITERS):
                for _ in range(agent.rollout_size):
                    agent.run()
        torch.cuda.synchronize()
    finally:
        PackedPolicy.minibatch_grad = orig
    assert seen["launches"] == ITERS * per_update and seen["refused"] == 0 and pol.h2_overflows == 0, seen
    kept["heavy"] = heavy["rec"]
    return agent, kept


def _rows(rec, keep):
    """The launch's arguments, or those of the rows `keep` only (the action variance is per column)."""
    a = rec["args"]
    return a if keep is None else [t[keep].contiguous() for t in a[:5]] + [a[5]]


def _launch(pol, rec, dump, keep=None):
    """The captured launch again (keep: on those rows only, normalised by the whole minibatch's row count as before)."""
    pol.minibatch_grad(*_rows(rec, keep), rec["clip"], global_rows=rec["args"][0].shape[0], dump=dump)
    torch.cuda.synchronize()


HEAVY_CEILING = 2e-4   # heavy-tailed minibatch, calibrated scales, dW / db: see the test
CLIP_DELTA = 1e-4      # a row whose float64 ratio is within 1e-4 (relative) of 1 +- clip may take either side of PPO's clip


def _refs(rec, keep=None):
    """float64 references of the launch (of the rows `keep`, normalised by the whole minibatch's row count as the launch is): the
    chain, and for the rows at PPO's ratio-clip boundary the chain of the OTHER branch.  There the surrogate's gradient is either
    the unclipped one or zero, and which one an fp32 launch takes is decided by the last bits of its log-probability, in any
    arithmetic (bf16x3 and fp32 too): each such row is then compared with the branch it took (_pick), as the DQN tests take out the
    LeakyReLU pairs the kernel flipped.  A row's chain below dz4 depends on that row's dz4 only."""
    sd = _Weights(rec["sd"])
    x, action, old_logp, adv, target, var = _rows(rec, keep)
    clip = rec["clip"]
    base = _fp64_chain(sd, x, action, old_logp, adv, target, var, clip=clip)
    mu = base["out"][:, :18]
    L = var.double().sqrt()
    logp = -0.5 * (18 * 1.8378770664093453 + (((action.double() - mu) / L) ** 2).sum(-1)) - L.log().sum()
    ratio = (logp - old_logp.double()).exp()
    amb = ((ratio / (1 + clip) - 1).abs() <= CLIP_DELTA) | ((ratio / (1 - clip) - 1).abs() <= CLIP_DELTA)
    idx = torch.nonzero(amb).squeeze(1)
    adv0 = adv.clone()
    adv0[idx] = 0.0
    cands = [base, _fp64_chain(sd, x, action, old_logp, adv0, target, var, clip=clip),     # the clipped side: no policy gradient
             _fp64_chain(sd, x, action, old_logp, adv, target, var, clip=1e30)]            # the unclipped side
    f = x.shape[0] / rec["args"][0].shape[0]
    for r in cands:
        for c in ("dz4", "dz3", "dz2", "dz1"):
            r[c] *= f
    return {"cands": [{k: r[k][idx] for k in WIDTH} for r in cands], "base": base, "idx": idx}


def _pick(got, refs):
    """The reference for the chain `got`: refs' chain, each clip-boundary row taken from the branch whose dz4 is nearest got's."""
    idx = refs["idx"]
    if idx.numel() == 0:
        return refs["base"]
    g = got["dz4"][idx].double()
    best = torch.stack([(g - r["dz4"]).abs().amax(1) for r in refs["cands"]]).argmin(0)
    out = {}
    for k in WIDTH:
        t = refs["base"][k].clone()
        t[idx] = torch.stack([r[k] for r in refs["cands"]])[best, torch.arange(idx.numel(), device=idx.device)]
        out[k] = t
    return out


def _lag(pol):
    """Per class: how many binades this launch's maximum of |scaled value| sits under its window (ceil; <= 0 inside it), and the
    smallest maximum."""
    from fly_bproject_amd.policy import H2_TARGET_EXP_ACT, H2_TARGET_EXP_GRAD
    m = [float(v) for v in pol.h2_scales[32:40].cpu()]
    return [math.ceil((H2_TARGET_EXP_ACT if c < 4 else H2_TARGET_EXP_GRAD) - math.log2(v)) if v > 0 else 0 for c, v in enumerate(m)], min(v for v in m if v > 0)


def _bar(k):
    """The contract for a launch whose worst class sits k binades under its window (csrc/fs_h2.inc; the lagging-scale test)."""
    return 2e-5 if k <= 6 else 4e-5 * 2.0 ** (k - 8)


def _three_arithmetics(pol, rec, refs, keep=None, calibrate=False):
    """Replays from the captured state: fp16x2 (scales calibrated to these rows, or the loop's), bf16x3, the fp32-MFMA chain.  Returns
    {arith: (chain errors, gradient errors or None)}, the fp16x2 launch's per-class lag, smallest maximum and refusal."""
    from fly_bproject_amd.policy import ERR_SLOT, untile
    x = _rows(rec, keep)[0]
    n = x.shape[0]
    out = {}
    _restore_snapshot(pol, rec["snap"])
    if calibrate:
        pol.calibrate_h2(*rec["args"], rec["clip"])
    pol.h2_freeze = True
    _launch(pol, rec, True, keep)
    refused = (int(pol.h2_overflow), float(pol.G[ERR_SLOT]))
    lag, low = _lag(pol)
    c = _chain(pol, n)
    out["f16x2"] = (_errs(c, _pick(c, refs)), _grad_errs(pol.G, x, c))
    pol.h2_overflow.zero_()
    _restore_snapshot(pol, rec["snap"])
    pol.step_gemm = "bf16x3"
    _launch(pol, rec, True, keep)
    c = _chain(pol, n)
    out["bf16x3"] = (_errs(c, _pick(c, refs)), _grad_errs(pol.G, x, c))
    pol.gemm = "f32"
    _launch(pol, rec, False, keep)
    c = {k: untile((pol.saves if k in pol.saves else pol.dz)[k], n, w) for k, w in WIDTH.items()}
    out["f32"] = (_errs(c, _pick(c, refs)), None)
    pol.gemm = "f16x2"
    _restore_snapshot(pol, rec["snap"])
    return out, lag, low, refused


def _table(title, rows):
    print(title)
    print("  %-22s %s | %s" % ("", " ".join("%8s" % k for k in WIDTH), " ".join("%8s" % k for k in GRADS)))
    for label, (chain, grad) in rows:
        print("  %-22s %s | %s" % (label, " ".join("%8.2e" % chain[k] for k in WIDTH),
                                   " ".join("%8.2e" % grad[k] for k in GRADS) if grad else ""))


_RESULTS = {}


def _run(normalize_obs):
    """Capture (once per setting, shared by the tests below), replay, print the tables; the figures the tests assert on."""
    if normalize_obs in _RESULTS:
        return _RESULTS[normalize_obs]
    from fly_bproject_amd.policy import ERR_SLOT
    agent, kept = _capture(normalize_obs)
    pol = agent.policy
    m = pol.grad_mask > 0
    res = {"ratio": kept["heavy"]["ratio"]}
    print("\n==== normalize_obs=%s: %d updates at 8192 envs, seed 0; errors are max |got - fp64| / max |fp64| per tensor (the chain "
          "against float64 end to end, dW / db against float64 on the chain the launch dumped); k = binades under the window"
          % (normalize_obs, ITERS))
    for name in ("first", "last", "heavy"):
        rec = kept[name]
        rec.pop("want", None)
        refs = _refs(rec)
        want = refs["base"]
        n = rec["args"][0].shape[0]
        # 0. faithful capture: the loop's own launch again, bit for bit
        _restore_snapshot(pol, rec["snap"])
        pol.h2_freeze = True
        x, action, old_logp, adv, target, var = rec["args"]
        pol.minibatch_grad(x, action, old_logp, adv, target, var, rec["clip"], fuse_norm=True)
        torch.cuda.synchronize()
        faithful = bool(torch.equal(pol.G[m], rec["G"][m]))
        # 1. calibrated scales and the loop's scales
        cal, lag_c, _, ref_c = _three_arithmetics(pol, rec, refs, calibrate=True)
        loop, lag_l, _, ref_l = _three_arithmetics(pol, rec, refs)
        _table("\n-- %s: update %d, step %d (epoch %d, minibatch %d), %d rows, max|x| %.3g, max/median ||dz4|| %.3g; k calibrated %d, "
               "k loop %d; %d rows at the ratio-clip boundary" % (name, rec["update"], rec["step"], rec["step"] // rec["per_epoch"] + 1,
                                                                 rec["step"] % rec["per_epoch"] + 1, n, float(x.abs().max()), rec["ratio"],
                                                                 max(lag_c), max(lag_l), refs["idx"].numel()),
               [("f16x2 calibrated", cal["f16x2"]), ("f16x2 loop scales", loop["f16x2"]), ("bf16x3", cal["bf16x3"]),
                ("f32 (3 launches)", cal["f32"])])
        res[name] = dict(faithful=faithful, cal=cal, loop=loop, lag_c=lag_c, lag_l=lag_l, ref_c=ref_c, ref_l=ref_l)
        if name != "heavy":
            continue
        # 2. the bulk under scales its outliers set
        rows = want["dz4"].norm(dim=1)
        top = torch.topk(rows, max(1, n // 100)).indices
        keep = torch.ones(n, dtype=torch.bool, device=x.device)
        keep[top] = False
        keep = torch.nonzero(keep).squeeze(1)
        refs_b = _refs(rec, keep)
        want_b = refs_b["base"]
        k64 = {c: math.log2(float(want[c].abs().max()) / float(want_b[c].abs().max())) for c in ("dz4", "dz3", "dz2", "dz1")}
        _restore_snapshot(pol, rec["snap"])
        pol.calibrate_h2(*rec["args"], rec["clip"])                 # the whole minibatch sets the scales ...
        pol.h2_freeze = True
        _launch(pol, rec, True, keep)                              # ... the bulk runs under them
        refused = (int(pol.h2_overflow), float(pol.G[ERR_SLOT]))
        lag_b, low_b = _lag(pol)
        c = _chain(pol, keep.numel())
        bulk = {"f16x2": (_errs(c, _pick(c, refs_b)), _grad_errs(pol.G, x[keep], c))}
        pol.h2_overflow.zero_()
        others, _, _, _ = _three_arithmetics(pol, rec, refs_b, keep=keep)
        _table("-- heavy, bulk: the rows outside the top %d by ||dz4||, scales calibrated on all rows; binades between the "
               "full minibatch's and the bulk's maximum (float64) %s; k of the launch per class %s; %d rows at the ratio-clip "
               "boundary%s" % (top.numel(), " ".join("%s %.1f" % kv for kv in k64.items()),
                               " ".join("%s %d" % kv for kv in zip(CLASSES, lag_b)), refs_b["idx"].numel(), "; REFUSED" if refused[0] else ""),
               [("f16x2 (outliers' scales)", bulk["f16x2"]), ("bf16x3", others["bf16x3"]), ("f32 (3 launches)", others["f32"])])
        res["bulk"] = dict(errs=bulk["f16x2"], lag=lag_b, low=low_b, refused=refused)
    agent.exit()
    _RESULTS[normalize_obs] = res
    return res


@pytest.mark.parametrize("normalize_obs", [False, True])
def test_h2_step_on_minibatches_of_the_training_loop_against_float64(normalize_obs):
    """Checks 0 .. 2 of the module docstring on the three captured minibatches.  The dW / db blocks of the heavy-tailed one under
    calibrated scales are held to HEAVY_CEILING here and to the suite's 2e-5 in the strict xfail below.  The heavy-tailed minibatch
    must have a max / median ||dz4|| of 2^8 or more (otherwise this is not the heavy tail the step's gradient window was chosen for)."""
    from fly_bproject_amd.policy import H2_CLASS_FLOOR
    res = _run(normalize_obs)
    assert res["ratio"] >= 2.0 ** 8, res["ratio"]
    for name in ("first", "last", "heavy"):
        r = res[name]
        assert r["faithful"], name
        assert r["ref_c"] == (0, 0.0) and r["ref_l"] == (0, 0.0), (name, r["ref_c"], r["ref_l"])
        assert max(r["lag_c"]) <= 1, (name, r["lag_c"])
        cal, loop = r["cal"], r["loop"]
        for k in WIDTH:
            assert cal["f16x2"][0][k] <= 2e-5 and cal["f16x2"][0][k] <= 2.0 * cal["f32"][0][k] + 2e-7, (name, "calibrated", k, cal)
        for kk, e in cal["f16x2"][1].items():
            # the heavy-tailed minibatch's dW / db miss the suite's bar (the strict xfail below holds it there); they are held to
            # the ceiling of what the fixed-quantum second term costs on it, twice the 1.0e-4 measured (profiles/h2_real_minibatches.txt)
            assert e <= (2e-5 if name != "heavy" else HEAVY_CEILING), (name, "calibrated", kk, e)
        kl = max(r["lag_l"])
        for k in WIDTH:
            assert loop["f16x2"][0][k] <= _bar(kl), (name, "loop", k, loop["f16x2"][0][k], kl)
            if kl <= 6:
                assert loop["f16x2"][0][k] <= 2.0 * loop["f32"][0][k] + 2e-7, (name, "loop", k, loop)
        for kk, e in loop["f16x2"][1].items():
            assert e <= _bar(kl), (name, "loop", kk, e, kl)
    b = res["bulk"]
    if b["low"] < H2_CLASS_FLOOR:
        assert b["refused"] == (1, 1.0), b["refused"]
        return
    assert b["refused"] == (0, 0.0), b["refused"]
    kb = max(b["lag"])
    for k in WIDTH:
        assert b["errs"][0][k] <= _bar(kb), ("bulk", k, b["errs"][0][k], kb)
    for kk, e in b["errs"][1].items():
        assert e <= _bar(kb), ("bulk", kk, e, kb)


@pytest.mark.xfail(strict=True, reason="known gap: the gradient classes' second fp16 term has a fixed absolute quantum (2^-24 of the "
                   "scaled value), so when a few rows carry a class maximum 10^4 .. 10^5 x the median the remaining rows keep ~13 bits "
                   "and dW3 / db3 / dW4 / db4 come out 3e-5 .. 1e-4 off float64 (csrc/fs_h2.inc, profiles/h2_real_minibatches.txt)")
@pytest.mark.parametrize("normalize_obs", [False, True])
def test_h2_heavy_minibatch_gradient_under_calibrated_scales_against_float64(normalize_obs):
    """Check 1's dW / db bar (2e-5 of each block's largest entry, float64 on the dumped chain) on the heavy-tailed minibatch under
    scales calibrated to it: the suite's bar, which the fp16x2 step does not meet there yet -- strict: the day it does, this fails
    and the mark must go."""
    res = _run(normalize_obs)
    for kk, e in res["heavy"]["cal"]["f16x2"][1].items():
        assert e <= 2e-5, (kk, e)
