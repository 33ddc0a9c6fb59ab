"""GPU (-m gpu): three data-parallel optimizer steps ON THE KERNELS -- two ranks on cuda:0, each with its half of the batch, issuing
`PPO._optimizer_step` (the gradient launch on the local rows, the exchange of the packed gradient, the `self_norm` clip + Adam launch
with grad_scale = 1 / world) -- against the float64 single-process step on the whole batch (tests/dist_step_ref.py, pinned on the
CPU by tests/test_dist_step_ref_cpu.py).

The other two-rank tests assert that the replicas are finite and equal to each other, which a wrong `grad_scale`, a wrong per-rank
`inv_b`, a clip on the wrong norm or an all-reduced gradient that is not the global batch's would all satisfy.  Here every one of
them is a visible error: a missing or doubled scale is a factor of 2 in the norm and in the gradient.

One `mp.spawn` per exchange ("collective": `dist.all_reduce` over gloo, RCCL refuses two ranks on one device; "p2p":
`P2PAllReduce` with `fail_slot` and the err word as `PPO` wires them); the workers loop over the arithmetics and sizes inside it.
The same three steps also run single-process on the whole 2 n rows (`minibatch_grad` + plain `adam_step()`): the control the
figures of profiles/dp_step_vs_float64.txt are read against (`-s` prints them)."""
import datetime
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from tests import dist_step_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GEMMS = ("f32", "bf16x3", "f16x2")
SIZES = (33, 2049)          # rows per rank: two tiles with ONE row in the second; 65 tiles with a ragged last one
EXCHANGES = ("collective", "p2p")
SAVED = ("G", "grad_norm", "P", "exp_avg", "exp_avg_sq")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _policy(n, rows, gemm):
    """The problem's initial weights packed for the kernels, with room for `rows` rows."""
    from fly_bproject_amd.policy import PackedPolicy
    sd, _ = R.problem(n)
    net = R.make_net(sd, torch.float32).to(DEV)
    pol = PackedPolicy(net, DEV)
    pol.init_training(max(rows, 32))
    pol.gemm = gemm
    return pol


def _snapshot(pol):
    torch.cuda.synchronize()
    d = {k: getattr(pol, k).detach().cpu().clone() for k in SAVED}
    d["step"] = int(pol.step)
    return d


def _dp_case(rank, n, gemm, p2p):
    """Rank `rank`'s three steps of one case, through the method `_update_hip.run` calls for every minibatch."""
    from fly_bproject_amd.ppo import PPO
    _, batch = R.problem(n)
    x, action, old_logp, adv, target, var = (t.to(DEV).contiguous() for t in R.rank_rows(batch, rank, n))
    pol = _policy(n, n, gemm)
    if gemm == "f16x2":                     # each rank calibrates on its own rows, as _update_hip does
        pol.calibrate_h2(x, action, old_logp, adv, target, var, R.CLIP)
    agent = PPO.__new__(PPO)
    agent.policy, agent._p2p, agent.world_size, agent.clip, agent._action_var = pol, p2p, 2, R.CLIP, var
    steps = []
    for it in range(R.STEPS):
        agent._optimizer_step(x, action, old_logp, R.step_advantage(adv, it).contiguous(), target, True)
        steps.append(_snapshot(pol))
    return steps


def _worker(rank, world, port, out_dir, exchange):
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    from fly_bproject_amd.dist import P2PAllReduce
    from fly_bproject_amd.policy import ERR_SLOT, PACKED
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    p2p = P2PAllReduce(PACKED, DEV, fail_slot=ERR_SLOT) if exchange == "p2p" else None
    out = {"%s/%d" % (gemm, n): _dp_case(rank, n, gemm, p2p) for gemm in GEMMS for n in SIZES}
    if p2p is not None:
        assert p2p.check()
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    if p2p is not None:
        p2p.close()
    dist.destroy_process_group()


_RUNS, _CONTROL, _INDEX = {}, {}, {}


def _dp_runs(exchange, tmp_path_factory):
    """Both ranks' saved steps of every case under `exchange`: ONE spawn, shared by the cases.  After a spawn that did not finish
    nothing of this module goes to the device again: every later case fails with the first one's message."""
    if "failed" in _RUNS:
        pytest.fail(_RUNS["failed"])
    if exchange not in _RUNS:
        out_dir = tmp_path_factory.mktemp("dp_step_" + exchange)
        try:
            mp.spawn(_worker, args=(2, _free_port(), str(out_dir), exchange), nprocs=2, join=True)
            _RUNS[exchange] = [torch.load(out_dir / ("rank%d.pt" % r), weights_only=True) for r in range(2)]
        except BaseException as e:
            _RUNS["failed"] = "the two ranks of %r did not finish: %r" % (exchange, e)
            raise
    return _RUNS[exchange]


def _control(gemm, n):
    """The same three steps in ONE process on the whole 2 n rows: minibatch_grad + a plain adam_step()."""
    if (gemm, n) not in _CONTROL:
        _, batch = R.problem(n)
        x, action, old_logp, adv, target, var = (t.to(DEV).contiguous() for t in batch)
        pol = _policy(n, 2 * n, gemm)
        if gemm == "f16x2":
            pol.calibrate_h2(x, action, old_logp, adv, target, var, R.CLIP)
        steps = []
        for it in range(R.STEPS):
            pol.minibatch_grad(x, action, old_logp, R.step_advantage(adv, it).contiguous(), target, var, R.CLIP)
            pol.adam_step()
            steps.append(_snapshot(pol))
        _CONTROL[(gemm, n)] = steps
    return _CONTROL[(gemm, n)]


def _views():
    """name -> int64 index of the parameter's elements in a packed buffer (the layout tables alone: no kernel runs on the CPU)."""
    if not _INDEX:
        from fly_bproject_amd.policy import PACKED, PackedPolicy
        from fly_bproject_amd.ppo import Net
        pol = PackedPolicy(Net(73, 18), "cpu")
        for name, view in pol.views.items():
            _INDEX[name] = torch.arange(PACKED).as_strided(view.shape, view.stride(), view.storage_offset())
    return _INDEX


def _figures(steps, ref, grad_factor):
    """One run (a rank's or the control's) against the float64 reference.  Returns (figures, misses): the figures of the profile
    file and the list of every bar of the project that the run misses ("tight" ones apart: the caller judges those against the control)."""
    fig = {"grad": 0.0, "grad_at": "", "norm": 0.0, "tight": 1.0, "tight_at": "", "elem": 0.0, "elem_bar": 0.0, "m": 0.0, "v": 0.0}
    misses = []
    for it, (s, want) in enumerate(zip(steps, ref)):
        rel = abs(float(s["grad_norm"]) - want["norm"]) / want["norm"]
        fig["norm"] = max(fig["norm"], rel)
        if rel > 2e-4:
            misses.append("step %d: grad_norm %.7g against %.7g (%.2e > 2e-4)" % (it, float(s["grad_norm"]), want["norm"], rel))
        for name, idx in _views().items():
            g64 = want["grads"][name]
            scale = float(g64.abs().max()) + 1e-12
            err = float((grad_factor * s["G"][idx].double() - g64).abs().max())
            if err / scale > fig["grad"]:
                fig["grad"], fig["grad_at"] = err / scale, "%s, step %d" % (name, it)
            if err > 2e-4 * scale + 1e-9:
                misses.append("step %d: gradient of %s off by %.3e of its scale %.3e" % (it, name, err / scale, scale))
            if it == 0:
                # from zero moments: m = (1 - beta1) c g, v = (1 - beta2) (c g)^2 with c the clip coefficient -- the gradient bar plus
                # the norm bar, once for m and twice for v
                for key, short, bar in (("exp_avg", "m", 4e-4), ("exp_avg_sq", "v", 8e-4)):
                    m64 = want[key][name]
                    mscale = float(m64.abs().max())
                    merr = float((s[key][idx].double() - m64).abs().max())
                    fig[short] = max(fig[short], merr / (mscale + 1e-300))
                    if merr > bar * mscale:
                        misses.append("step 0: %s of %s off by %.3e of its scale" % (key, name, merr / mscale))
            q = want["params"][name]
            perr = (s["P"][idx].double() - q).abs()
            tight = float((perr <= 2e-6 + 2e-4 * q.abs()).double().mean())
            if tight < fig["tight"]:
                fig["tight"], fig["tight_at"] = tight, "%s, step %d" % (name, it)
            s.setdefault("tight", {})[name] = tight
            if float(perr.max()) / (1.05e-3 * (it + 1)) > fig["elem_bar"]:
                fig["elem"], fig["elem_bar"] = float(perr.max()), float(perr.max()) / (1.05e-3 * (it + 1))
            if float(perr.max()) > 1.05e-3 * (it + 1):
                misses.append("step %d: an element of %s is %.3e off (bar %.3e)" % (it, name, float(perr.max()), 1.05e-3 * (it + 1)))
    return fig, misses


def _line(tag, fig):
    return ("%-36s grad %.2e (%s)  norm %.2e  m %.2e  v %.2e  tight %.5f (%s)  largest element error %.2e (%.2f of its bar)"
            % (tag, fig["grad"], fig["grad_at"], fig["norm"], fig["m"], fig["v"], fig["tight"], fig["tight_at"], fig["elem"], fig["elem_bar"]))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("exchange", EXCHANGES)
def test_two_rank_steps_match_the_float64_step_on_the_whole_batch(tmp_path_factory, exchange, gemm, n):
    """Per case: the replicas are bit-identical and count the steps; 0.5 G (through `pol.views`) is the float64 gradient of the
    WHOLE batch within 2e-4 of each tensor's scale (the bar of test_minibatch_gradient_matches_autograd, against a stricter
    reference); `grad_norm` is the float64 pre-clip norm at rtol 2e-4; the moments after step 0 (linear and quadratic in the clipped
    gradient) are within 4e-4 / 8e-4 of their scale; after every step >= 99.9 % of every tensor's elements lie within 2e-6 +
    2e-4 |q| and every element within 1.05e-3 (it + 1) (the bar of test_adam_clip_step_matches_torch: Adam's first steps move a
    weight by ~lr sign(g), so an element whose gradient is at rounding level may land anywhere in that range).

    The 99.9 % fraction had only been measured against fp32 torch.  Where the single-process control misses it against float64
    too, that is a finding about the bar, not about the data-parallel composition: the assertion there is that the two ranks' fraction
    is no lower than the control's minus 5e-4 (profiles/dp_step_vs_float64.txt holds both sets of figures)."""
    ranks = _dp_runs(exchange, tmp_path_factory)
    key = "%s/%d" % (gemm, n)
    a, b = ranks[0][key], ranks[1][key]
    for it in range(R.STEPS):
        for k in SAVED:
            assert torch.equal(a[it][k], b[it][k]), (it, k)             # replicas in lock step, bit for bit
        assert a[it]["step"] == b[it]["step"] == it + 1                   # no step refused, both parities of the counter
    ref = R.reference(n)
    fig, misses = _figures(a, ref, 0.5)
    ctl = _control(gemm, n)
    cfig, cmisses = _figures(ctl, ref, 1.0)
    print()
    print(_line("%s %s n=%d  two ranks" % (exchange, gemm, n), fig))
    print(_line("%s %s n=%d  one process" % (exchange, gemm, n), cfig))
    for m in cmisses:
        print("    one process misses: " + m)
    assert not misses, misses
    for it in range(R.STEPS):
        for name, tight in a[it]["tight"].items():
            c = ctl[it]["tight"][name]
            if c >= 0.999:
                assert tight >= 0.999, (it, name, tight)
            else:
                assert tight >= c - 5e-4, (it, name, tight, c)
