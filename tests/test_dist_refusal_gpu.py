"""GPU (-m gpu): the fp16x2 optimizer step's refusal path ACROSS RANKS, on the kernels -- two ranks of `PPO` on cuda:0 (gloo
transport: RCCL refuses two ranks on one device), one whole update of 75 steps with something going wrong on ONE rank in the middle.

  * An overflow on one rank: that rank's launch marks `G[ERR_SLOT]`, the mark rides the all-reduce, every rank's `mlp_adam_step`
    refuses that step and every later one, every rank finds the step counter equally short and redoes the refused steps on bf16x3 --
    and the update ends bit for bit where an update ends that runs steps 0 .. 39 in fp16x2 and 40 .. 74 in bf16x3 by construction.
    (tests/test_dist_cpu.py covers the layout of the mark, tests/test_fused_h2_gpu.py the mechanism on one rank.)
  * A `calibrate_h2` that does not settle on one rank: the ranks decide together, every rank runs the update on bf16x3 and none
    raises (before, the failing rank raised alone and its peers waited in the update's first all-reduce).

No fault is forced: an fp16 overflow sets a word on the device and the step is refused.  Every process group has an explicit
timeout, so a rank left alone in a collective fails with an error instead of waiting."""
import contextlib
import datetime
import io
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("P", "exp_avg", "exp_avg_sq", "PB")
KNOCK_STEP = 40


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    return dist


def _make_agent(rank, exchange, dp_mode):
    from fly_bproject_amd.dist import broadcast_policy
    from fly_bproject_amd.ppo import PPO
    from tests.hip_helpers import make_args
    torch.manual_seed(0)
    agent = PPO(make_args(2048, rank=rank, world_size=2, seed=0, dp_mode=dp_mode, dp_allreduce=exchange))
    agent.policy.gemm = "f16x2"
    broadcast_policy(agent)
    assert agent.policy.h2_live()
    return agent


def _iteration(agent):
    for _ in range(agent.rollout_size):
        agent.run()
    torch.cuda.synchronize()


def _record(agent):
    pol = agent.policy
    d = {k: getattr(pol, k).detach().cpu().clone() for k in STATE}
    d.update(optim_step=agent.optim_step, step=int(pol.step), h2_overflows=pol.h2_overflows, h2_calibrated=bool(pol.h2_calibrated),
             h2_calibration_failures=pol.h2_calibration_failures, h2_suspended=bool(pol.h2_suspended),
             finite=all(bool(torch.isfinite(getattr(pol, k)).all()) for k in STATE[:3]))
    return d


@contextlib.contextmanager
def _count_calibrations(count):
    """While active, count["ok"] counts the `calibrate_h2` calls that settled."""
    from fly_bproject_amd.policy import PackedPolicy
    orig = PackedPolicy.calibrate_h2

    def counted(self, *a, **kw):
        k = orig(self, *a, **kw)
        count["ok"] = count.get("ok", 0) + 1
        return k

    PackedPolicy.calibrate_h2 = counted
    try:
        yield
    finally:
        PackedPolicy.calibrate_h2 = orig


@contextlib.contextmanager
def _gradient_launch_hook(plan):
    """While active, `PackedPolicy.minibatch_grad` acts on `plan` just before the gradient launch of optimizer step `plan["at"]` of
    the update that began at `plan["base"]` issued steps -- once, and only on a launch in fp16x2.  The data-parallel launches pass
    fuse_norm=False as the calibration launches do, so the moment is picked by `steps_issued`, never by `fuse_norm`.
    "knock": class 2's scale times 2^20 (its inverse times 2^-20) -- an overflow from any calibrated table (a calibrated class sits
    within a binade of its window, whose exponent is far above -4), and within reach of calibrate_h2's back-off of 2^-8 per launch.
    "suspend": h2_suspended becomes a truthy marker the redo path never clears: bf16x3 from here on BY CONSTRUCTION."""
    from fly_bproject_amd.policy import H2_INV, PackedPolicy
    orig = PackedPolicy.minibatch_grad

    def patched(self, *a, **kw):
        if plan.get("what") and not self.h2_suspended and self.steps_issued - plan["base"] == plan["at"]:
            if plan["what"] == "knock":
                self.h2_scales[2] *= 2.0 ** 20
                self.h2_scales[H2_INV + 2] *= 2.0 ** -20
            else:
                self.h2_suspended = "by construction"
            plan["what"] = None
            plan["hits"] = plan.get("hits", 0) + 1
        return orig(self, *a, **kw)

    PackedPolicy.minibatch_grad = patched
    try:
        yield
    finally:
        PackedPolicy.minibatch_grad = orig


def _overflow_worker(rank, world, port, out_dir, exchange, dp_mode, knocked):
    dist = _init(rank, world, port)
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for mode in ("overflow", "mixed"):
            agent = _make_agent(rank, exchange, dp_mode)
            if mode == "overflow":
                what = "knock" if rank == knocked else None
            else:       # param_average: the peer never sees the refusal, so only the knocked rank leaves fp16x2
                what = "suspend" if (dp_mode == "grad_allreduce" or rank == knocked) else None
            plan = {"what": what, "at": KNOCK_STEP, "base": agent.policy.steps_issued}
            with _gradient_launch_hook(plan):
                _iteration(agent)
            assert plan.get("hits", 0) == (1 if what else 0)
            if exchange == "p2p":
                assert agent._p2p is not None and agent._p2p.check()
            out[mode] = _record(agent)
            if mode == "overflow":
                count = {}
                with _count_calibrations(count):
                    _iteration(agent)       # a second whole update: both ranks calibrate again, from the tables the first left
                if exchange == "p2p":
                    assert agent._p2p.check()
                out["second"] = _record(agent)
                out["second"]["calibrations"] = count.get("ok", 0)
            agent.exit()
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("exchange,dp_mode,knocked", [("rccl", "grad_allreduce", 1), ("p2p", "grad_allreduce", 0),
                                                      ("rccl", "param_average", 1)])
def test_an_overflow_on_one_rank_is_refused_and_redone_by_all(tmp_path, exchange, dp_mode, knocked):
    """Just before the gradient launch of step 40 of the first update, ONE rank's scale table is knocked out of range.  With
    grad_allreduce both ranks refuse steps 40 .. 74, count one overflow, redo on bf16x3 and lose their calibration; with
    param_average only the knocked rank does.  Either way the update ends, on both ranks, bit for bit where the "mixed" update ends
    (steps 0 .. 39 in fp16x2, 40 .. 74 in bf16x3 by construction, no refusal).  A second update calibrates again on both ranks and
    stays in lock step (not comparable with the mixed run bit for bit: its scales are newly measured there and lagged here)."""
    mp.spawn(_overflow_worker, args=(2, _free_port(), str(tmp_path), exchange, dp_mode, knocked), nprocs=2, join=True)
    r = [torch.load(tmp_path / ("rank%d.pt" % k), weights_only=True) for k in range(2)]
    for k in range(2):
        sees = dp_mode == "grad_allreduce" or k == knocked
        for mode in ("overflow", "mixed"):
            assert r[k][mode]["optim_step"] == 75 and r[k][mode]["step"] == 75, (k, mode)
            assert not r[k][mode]["h2_suspended"] and r[k][mode]["h2_calibration_failures"] == 0
        assert r[k]["overflow"]["h2_overflows"] == (1 if sees else 0), k
        assert r[k]["mixed"]["h2_overflows"] == 0, k
        if dp_mode == "grad_allreduce":
            assert not r[k]["overflow"]["h2_calibrated"], k
    for mode in ("overflow", "mixed"):
        for key in STATE:
            assert torch.equal(r[0][mode][key], r[1][mode][key]), (mode, key)                 # the replicas
    for key in STATE:
        assert torch.equal(r[0]["overflow"][key], r[0]["mixed"][key]), key                    # the redo == by construction
        assert not torch.equal(r[0]["overflow"][key], torch.zeros_like(r[0]["overflow"][key])), key
    for k in range(2):
        s = r[k]["second"]
        assert s["calibrations"] == 1 and s["finite"], k                # calibrated again, from the knocked / lagged table
        if dp_mode == "grad_allreduce":     # (param_average rebuilds the copies after every exchange, which drops the calibration)
            assert s["h2_calibrated"], k
        assert s["h2_overflows"] == r[k]["overflow"]["h2_overflows"], k
        assert s["optim_step"] == 150 and s["step"] == 150, k
    for key in STATE:
        assert torch.equal(r[0]["second"][key], r[1]["second"][key]), key


def _calibration_worker(rank, world, port, out_dir):
    dist = _init(rank, world, port)
    from fly_bproject_amd.policy import PackedPolicy
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        # "failed": rank 0's first calibration fails as a real one does -- calibrate_h2 itself, out of launches
        agent = _make_agent(rank, "rccl", "grad_allreduce")
        orig, calls = PackedPolicy.calibrate_h2, {"n": 0}

        def failing(self, *a, **kw):
            calls["n"] += 1
            if rank == 0 and calls["n"] == 1:
                kw["max_launches"] = 0
            return orig(self, *a, **kw)

        PackedPolicy.calibrate_h2 = failing
        try:
            _iteration(agent)
            out["failed"] = _record(agent)
            _iteration(agent)
            out["second"] = _record(agent)
        finally:
            PackedPolicy.calibrate_h2 = orig
        assert calls["n"] == 2              # every rank attempted both calibrations: the decision to exchange a verdict is alike
        agent.exit()
        # "suspended": both ranks on bf16x3 from step 0 by construction
        agent = _make_agent(rank, "rccl", "grad_allreduce")
        plan = {"what": "suspend", "at": 0, "base": agent.policy.steps_issued}
        with _gradient_launch_hook(plan):
            _iteration(agent)
        assert plan.get("hits", 0) == 1
        out["suspended"] = _record(agent)
        agent.exit()
    torch.save(out, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_a_calibration_failure_on_one_rank_is_decided_by_all(tmp_path):
    """Rank 0's first `calibrate_h2` does not settle.  Both ranks finish the 75 steps, count one calibration failure and no
    overflow, and end bit for bit where two ranks end that are suspended from step 0 by construction; the next update calibrates
    on both and stays in lock step.  (Without the ranks' common verdict rank 0 raises alone and rank 1 is left in the update's first
    all-reduce until the process group's timeout.)"""
    mp.spawn(_calibration_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / ("rank%d.pt" % k), weights_only=True) for k in range(2)]
    for k in range(2):
        f = r[k]["failed"]
        assert f["optim_step"] == 75 and f["step"] == 75, k
        assert f["h2_calibration_failures"] == 1 and f["h2_overflows"] == 0, k
        assert not f["h2_calibrated"] and not f["h2_suspended"], k
        assert r[k]["suspended"]["h2_calibration_failures"] == 0 and r[k]["suspended"]["step"] == 75, k
        s = r[k]["second"]
        assert s["h2_calibrated"] and s["finite"] and s["step"] == 150, k
        assert s["h2_calibration_failures"] == 1 and s["h2_overflows"] == 0, k
    for key in STATE:
        assert torch.equal(r[0]["failed"][key], r[1]["failed"][key]), key
        assert torch.equal(r[0]["failed"][key], r[0]["suspended"][key]), key
        assert torch.equal(r[0]["second"][key], r[1]["second"][key]), key
