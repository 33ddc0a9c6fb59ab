"""The seeded optimizer sequences behind tests/test_adam_round_trips_gpu.py and its golden file (not a test module).

    FLYHIP_LIB=<a build of the REFERENCE commit> python -m tests.adam_round_trips_seq tests/golden/adam_round_trips.json

writes, for every launch of the sequences, a SHA-256 of every buffer the launch may write; the test runs the same sequences on the
library under test and compares.  The sequences drive `mlp_adam_step` through everything its load order could get wrong -- the
three launch forms (norm_ready on real gradients of 33 and 64 rows, two-launch, self_norm in both step-word parities with
grad_scale 0.5), the three plane sets, norms on both sides of max_norm, refused steps (the mark in G, the grad_invalid word),
step words set from outside, lr and betas changed between launches, rescale steps (one right behind a refused step) -- and the
two slab reductions through fuse_norm launches at both row counts, with the sticky overflow word / the tile error word set.

Every input comes from numpy generators and a CPU-initialised network: the same on every machine."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import torch

DEV = "cuda:0"
LR, BETAS, EPS, MAX_NORM = 1e-3, (0.9, 0.999), 1e-8, 1.0
MAIN_STEPS = 150
SHORT_STEPS = 14
STEP_BUFFERS = ("P", "PF", "PT", "PB", "PTB", "PH", "PTH", "exp_avg", "exp_avg_sq", "_step2", "norm", "h2_scales")
GRAD_BUFFERS = ("G", "partials", "_step2", "h2_overflow", "h2_scales")


def compiler_string():
    """What `hipcc --version` prints (the golden digests hold for the code this compiler generates)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        return subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError) as e:
        return "unavailable: %r" % (e,)


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _buffers(pol):
    return {"P": pol.P, "PF": pol.PF, "PT": pol.PT, "PB": pol.PB, "PTB": pol.PTB, "PH": pol.PH, "PTH": pol.PTH,
            "exp_avg": pol.exp_avg, "exp_avg_sq": pol.exp_avg_sq, "_step2": pol._step2, "norm": pol._norm_ws[:1],
            "h2_scales": pol.h2_scales}


def _step_digest(pol):
    torch.cuda.synchronize()
    return {k: _sha(t) for k, t in _buffers(pol).items()}


def _grad_digest(pol):
    torch.cuda.synchronize()
    return {"G": _sha(pol.G), "partials": _sha(pol._norm_ws[1:292]), "_step2": _sha(pol._step2), "h2_overflow": _sha(pol.h2_overflow),
            "h2_scales": _sha(pol.h2_scales)}


def _elu(a):
    return np.where(a > 0, a, np.expm1(np.minimum(a, 0.0)))


def _batch(sd, n, seed):
    """(x, action, old_logp, adv, target, var) of n rows as tests/test_mlp_train_gpu._setup makes them, but from numpy in float64."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 73))
    h = _elu(x @ sd["shared_net.0.weight"].T + sd["shared_net.0.bias"])
    h = _elu(h @ sd["shared_net.2.weight"].T + sd["shared_net.2.bias"])
    h = _elu(h @ sd["to_mean.0.weight"].T + sd["to_mean.0.bias"])
    mu = _elu(h @ sd["to_mean.2.weight"].T + sd["to_mean.2.bias"])
    var = 0.15
    action = np.clip(mu + 0.4 * rng.standard_normal((n, 18)), -1.0, 1.0)
    logp = -0.5 * (18 * math.log(2 * math.pi) + np.sum((action - mu) ** 2, axis=1) / var) - 18 * math.log(math.sqrt(var))
    old_logp = logp + 0.3 * rng.standard_normal(n)
    adv = rng.standard_normal(n)
    target = rng.standard_normal(n) * 1.5
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)     # noqa: E731
    return dev(x), dev(action), dev(old_logp), dev(adv), dev(target), torch.full((18,), var, device=DEV)


def _policy(planes, seed):
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(seed)
    net = Net(73, 18)
    sd = {k: v.detach().double().numpy().copy() for k, v in net.state_dict().items()}
    pol = PackedPolicy(net.to(DEV), DEV)
    pol.init_training(64, lr=LR, betas=BETAS, eps=EPS, max_norm=MAX_NORM)
    pol.gemm = planes
    assert pol.h2_live() == (planes == "f16x2") and pol._planes_live() == (planes != "f32")
    return pol, sd


def _assert_untouched(pol, before, tag, step_copy=None):
    """A refused launch stored nothing.  step_copy = (read, written): the self_norm form hands the count on to the other step word."""
    torch.cuda.synchronize()
    for k, t in _buffers(pol).items():
        if k == "_step2" and step_copy is not None:
            r, w = step_copy
            assert int(t[w]) == int(before[k][r]) and int(t[r]) == int(before[k][r]), (tag, "step words of a refused self_norm launch")
            continue
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, before[k].view(torch.int32)
                           if t.dtype == torch.float32 else before[k]), (tag, k, "a refused step wrote")


def run_sequence(planes, steps, seed):
    """-> {"records": [[label, {buffer: sha256}], ...], "facts": {...}}: one record per launch (gradient launches of the norm_ready
    steps included)."""
    from fly_bproject_amd import policy as Pm
    pol, sd = _policy(planes, seed)
    rng = np.random.default_rng(seed + 1)
    batches = {33: _batch(sd, 33, seed + 2), 64: _batch(sd, 64, seed + 3)}
    records = []
    facts = {"clipped": 0, "unclipped": 0, "rescales": 0, "refused": 0, "rescale_behind_refusal": 0, "parities": set(), "forms": set()}
    state = {"refusal_before_rescale_done": False, "expect_rescale": False}
    main = planes == "f16x2" and steps >= MAIN_STEPS

    def put_g(scale):
        g = (rng.standard_normal(Pm.PACKED) * scale).astype(np.float32)
        g[Pm.ERR_SLOT] = 0.0
        pol.G.copy_(torch.from_numpy(g).to(DEV))

    def rescale_due():      # every form applies its step as count + 1, and that step reads the rescale counter the other parity holds
        return planes == "f16x2" and float(pol.h2_scales[Pm.H2_SINCE + (int(pol.step) & 1)]) >= 64.0

    def applied(label, form, due):
        torch.cuda.synchronize()
        records.append([label, _step_digest(pol)])
        facts["forms"].add(form)
        norm = float(pol._norm_ws[0])
        facts["clipped" if norm + 1e-6 > MAX_NORM else "unclipped"] += 1
        if due:
            assert float(pol.h2_scales[Pm.H2_SINCE + (int(pol.step) & 1)]) == 1.0, (label, "a rescale was due")
            facts["rescales"] += 1
            if state["expect_rescale"]:
                facts["rescale_behind_refusal"] += 1
        assert due or not state["expect_rescale"], (label, "the applied step behind the refused one must rescale")
        state["expect_rescale"] = False

    def refuse_by_mark(label):
        put_g(1e-3)
        pol.G[Pm.ERR_SLOT] = 1.0
        before = {k: t.clone() for k, t in _buffers(pol).items()}
        pol.adam_step()
        _assert_untouched(pol, before, label)
        records.append([label, _step_digest(pol)])
        facts["refused"] += 1

    for t in range(steps):
        tag = "%s/%d" % (planes, t)
        if main and not state["refusal_before_rescale_done"] and rescale_due():
            refuse_by_mark(tag + "/refused-before-rescale")
            state["refusal_before_rescale_done"] = True
            state["expect_rescale"] = True
        if main and t == 20:
            refuse_by_mark(tag + "/refused-mark")
        if main and t == 21:                        # the grad_invalid word, self_norm form: the count moves to the other word, nothing else
            put_g(1e-3)
            word = torch.ones(1, dtype=torch.int32, device=DEV)
            before = {k: x.clone() for k, x in _buffers(pol).items()}
            r = pol._step_idx
            pol.adam_step(grad_scale=0.5, self_norm=True, grad_invalid=word)
            _assert_untouched(pol, before, tag, step_copy=(r, r ^ 1))
            records.append([tag + "/refused-invalid-self_norm", _step_digest(pol)])
            facts["refused"] += 1
        if main and t == 22:                        # the grad_invalid word, norm_ready form, behind a real gradient launch
            b = batches[33]
            pol.calibrate_h2(*b, 0.2)
            pol.minibatch_grad(*b, 0.2, fuse_norm=True)
            word = torch.full((1,), 7, dtype=torch.int32, device=DEV)
            before = {k: x.clone() for k, x in _buffers(pol).items()}
            pol.adam_step(norm_ready=True, grad_invalid=word)
            _assert_untouched(pol, before, tag)
            records.append([tag + "/refused-invalid-norm_ready", _step_digest(pol)])
            facts["refused"] += 1
            pol._step2[pol._step_idx] -= 1          # (the gradient launch had advanced the count for a step that was not applied)
        if main and t in (30, 31, 32):              # the step words set from outside
            pol._step2[pol._step_idx] = {30: 9, 31: 99999, 32: 2}[t]
        if main and t == 40:
            pol.lr, pol.betas = 3e-4, (0.8, 0.99)
        if main and t == 45:
            pol.lr, pol.betas = LR, BETAS
        kind = t % 10
        words = pol._step2.clone()
        due = rescale_due()
        if kind in (0, 1, 6):                       # norm_ready on a real gradient: 33 rows (one whole and one ragged tile) or 64
            n = 64 if kind == 1 else 33
            b = batches[n]
            rows = n / 64.0 if kind == 6 else None  # (the gradient is linear in 1 / global_rows: kind 6 is 64 times kind 0's)
            if planes == "f16x2":
                pol.calibrate_h2(*b, 0.2, global_rows=rows)
            pol.minibatch_grad(*b, 0.2, global_rows=rows, fuse_norm=True)
            records.append([tag + "/grad%d" % n, _grad_digest(pol)])
            assert int(pol.step) == int(words[pol._step_idx]) + 1, (tag, "the gradient launch was refused")
            pol.adam_step(norm_ready=True)
            applied(tag + "/norm_ready%d" % n, "norm_ready", due)
        elif kind in (4, 5):                        # self_norm, twice in a row: both parities of the step words
            put_g(1e-2 if kind == 4 else 4e-3)
            facts["parities"].add(pol._step_idx)
            pol.adam_step(grad_scale=0.5, self_norm=True)
            applied(tag + "/self_norm", "self_norm", due)
        else:
            put_g(1e-2 if kind in (3, 8) else 1e-3)
            pol.adam_step(grad_scale=1.0 if kind != 9 else 0.25)
            applied(tag + "/two_launch", "two_launch", due)
    # the reductions' refusing branch: the sticky overflow word (fp16x2) / the tile error word (the three-launch path) set
    b = batches[64]
    if planes == "f16x2":
        pol.calibrate_h2(*b, 0.2)
        pol.h2_overflow.fill_(1)
        pol.minibatch_grad(*b, 0.2, fuse_norm=True)
        records.append([planes + "/grad64-sticky-overflow", _grad_digest(pol)])
        assert float(pol.G[Pm.ERR_SLOT]) == 1.0
        pol.h2_overflow.zero_()
    elif planes == "f32":
        pol.tile_wait_error.fill_(1)
        pol.minibatch_grad(*b, 0.2, fuse_norm=True)
        records.append([planes + "/grad64-tile-error", _grad_digest(pol)])
        assert float(pol.G[Pm.ERR_SLOT]) == 1.0
        pol.tile_wait_error.zero_()
    facts["parities"] = sorted(facts["parities"])
    facts["forms"] = sorted(facts["forms"])
    facts = {k: (int(v) if isinstance(v, (bool, np.integer)) else v) for k, v in facts.items()}
    return {"records": records, "facts": facts}


def check_facts(planes, facts):
    """The sequence went where it was meant to go (holds for the reference and for the library under test alike)."""
    assert facts["forms"] == ["norm_ready", "self_norm", "two_launch"] and facts["parities"] == [0, 1], facts
    assert facts["clipped"] >= 3 and facts["unclipped"] >= 3, facts
    if planes == "f16x2":
        assert facts["rescales"] >= 2 and facts["refused"] == 4 and facts["rescale_behind_refusal"] == 1, facts


SEQUENCES = (("f16x2", MAIN_STEPS, 101), ("bf16x3", SHORT_STEPS, 202), ("f32", SHORT_STEPS, 303))


def run_all():
    out = {}
    for planes, steps, seed in SEQUENCES:
        r = run_sequence(planes, steps, seed)
        check_facts(planes, r["facts"])
        out[planes] = r
    return out


def main(path):
    from fly_bproject_amd import _lib
    first, second = run_all(), run_all()
    assert first == second, "two runs of the sequences in one process disagree"
    doc = {"what": "SHA-256 of every buffer mlp_adam_step / the fuse_norm gradient launch may write, after every launch of "
                   "tests/adam_round_trips_seq.py's sequences, from a build of the reference commit",
           "compiler": compiler_string(), "library": os.path.basename(_lib.LIB_PATH), "sequences": first}
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    for planes, r in first.items():
        print(planes, len(r["records"]), "records", r["facts"])


if __name__ == "__main__":
    main(sys.argv[1])
