"""GPU (-m gpu): PPO with minibatch="shuffled" -- the gather kernel behind the seam `PPO._gather_minibatch` against a torch
index_select over the reference's indices, the two update backends against each other, which rows an update visits, the mode
beside the other opt-in modes, the untouched reference mode, and two data-parallel ranks on one GPU."""
import contextlib
import io
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import minibatch_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096                                                    # mini_chunk_size 10, rollout 160 steps, 40960-row minibatches


def make_agent(n=N, gemm=None, **kw):
    from fly_bproject_amd.ppo import PPO
    from tests.hip_helpers import make_args
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(n, **kw))
    if gemm:
        agent.policy.gemm = gemm
    return agent


def one_update(agent):
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(agent.rollout_size):
            agent.run()
        agent.flush_log()
    torch.cuda.synchronize()
    return agent


def capture_indices(agent):
    """Wrap the seam: the source rows of every staged minibatch, by (epoch key, first position)."""
    seen = {}
    rows = agent.mini_chunk_size * int(agent.args.num_envs)
    agent._mb_index = torch.full((rows,), -1, dtype=torch.int32, device=agent.device)
    inner = agent._gather_minibatch

    def seam(epoch_key, first, rows, *data):
        out = inner(epoch_key, first, rows, *data)
        got = agent._mb_index.cpu().numpy().astype(np.int64)
        assert (epoch_key, first) not in seen or np.array_equal(seen[(epoch_key, first)], got)    # a restaged step: the same rows
        seen[(epoch_key, first)] = got
        return out

    agent._gather_minibatch = seam
    return seen


def state(agent):
    pol = agent.policy
    return {"P": pol.P.clone(), "m": pol.exp_avg.clone(), "v": pol.exp_avg_sq.clone(), "optim_step": agent.optim_step,
            "h2_overflows": pol.h2_overflows, "seed": agent._mb_seed, "rows": agent.mini_chunk_size * int(agent.args.num_envs),
            "R": agent.rollout_size * int(agent.args.num_envs), "epochs": agent.epoch}


@pytest.fixture(scope="module")
def kernel_run():
    """One rollout and one update through the gather kernel, with the staged indices captured: shared by the tests below."""
    agent = make_agent(minibatch="shuffled")
    seen = capture_indices(agent)
    one_update(agent)
    out = state(agent)
    out["seen"] = seen
    agent.exit()
    return out


def test_kernel_seam_equals_torch_seam(kernel_run):
    """The same agent with `_gather_minibatch` replaced by torch.index_select over tests/minibatch_ref.perm_index: the packed
    parameters and both Adam moments are bit-identical after one update (default arithmetic: the fp16x2 step and its
    calibration on the staged first minibatch included), 75 steps, no overflow."""
    agent = make_agent(minibatch="shuffled")
    seed, R = agent._mb_seed, agent.rollout_size * N

    def seam(epoch_key, first, rows, obs, action, old_log_prob, target, advantage):
        idx = torch.from_numpy(M.perm_index(R, seed, epoch_key, np.arange(first, first + rows))).to(agent.device)
        return (obs.reshape(R, 73).index_select(0, idx), action.reshape(R, 18).index_select(0, idx),
                old_log_prob.reshape(R).index_select(0, idx), target.reshape(R, 1).index_select(0, idx),
                advantage.reshape(R, 1).index_select(0, idx))

    agent._gather_minibatch = seam
    one_update(agent)
    got = state(agent)
    agent.exit()
    assert got["optim_step"] == kernel_run["optim_step"] == 75
    assert got["h2_overflows"] == kernel_run["h2_overflows"] == 0
    for k in ("P", "m", "v"):
        assert torch.equal(got[k].view(torch.int32), kernel_run[k].view(torch.int32)), k


def test_every_epoch_visits_fifteen_sixteenths_of_all_rows(kernel_run):
    seen, rows, R, seed = kernel_run["seen"], kernel_run["rows"], kernel_run["R"], kernel_run["seed"]
    assert R == 16 * rows
    assert sorted(seen) == [(e, w * rows) for e in range(kernel_run["epochs"]) for w in range(15)]     # update 0: keys 0..4
    visited = []
    for e in range(kernel_run["epochs"]):
        idx = np.concatenate([seen[(e, w * rows)] for w in range(15)])
        assert idx.min() >= 0 and idx.max() < R
        assert np.unique(idx).size == 15 * rows                         # disjoint windows: 15/16 of the rows, each once
        assert (idx >= 15 * rows).sum() > 0.9 * 15 / 16 * rows          # rows of the 16th time chunk train too (expected 15/16 of it)
        visited.append(idx)
    assert np.array_equal(seen[(3, 7 * rows)], M.perm_index(R, seed, 3, np.arange(7 * rows, 8 * rows)))
    for a in range(len(visited)):
        for b in range(a):
            assert (visited[a] == visited[b]).mean() < 0.01             # epochs differ


def test_hip_and_torch_updates_agree_in_shuffled_mode():
    """tests/test_mlp_train_gpu.py::test_ppo_hip_and_torch_updates_agree with minibatch='shuffled': its setup (gemm f32) and its
    bars (apart <= 0.3 x moved per tensor, <= 0.2 x moved in function space)."""
    outs, init, fn = {}, None, {}
    for backend in ("hip", "torch"):
        agent = make_agent(gemm="f32", update_backend=backend, minibatch="shuffled")
        init = {k: v.clone() for k, v in agent.net.state_dict().items()}
        with torch.no_grad():
            probe = torch.randn(512, 73, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
            fn["init"] = torch.cat([agent.net.pi(probe), agent.net.v(probe)], dim=1)
        one_update(agent)
        with torch.no_grad():
            fn[backend] = torch.cat([agent.net.pi(probe), agent.net.v(probe)], dim=1)
        assert agent.optim_step == 75
        outs[backend] = {k: v.clone() for k, v in agent.net.state_dict().items()}
        agent.exit()
    for k in outs["hip"]:
        moved = float((outs["torch"][k] - init[k]).norm())
        apart = float((outs["hip"][k] - outs["torch"][k]).norm())
        assert moved > 0 and apart <= 0.3 * moved, (k, apart, moved)
    moved = float((fn["torch"] - fn["init"]).norm())
    apart = float((fn["hip"] - fn["torch"]).norm())
    assert apart <= 0.2 * moved, (apart, moved)


@pytest.mark.parametrize("persistent", [True, False])
def test_shuffled_mode_beside_the_other_modes(persistent):
    agent = make_agent(minibatch="shuffled", normalize_obs=True, normalize_value=True, gae="episodic",
                       persistent_rollout=persistent)
    assert agent.persistent_rollout == persistent
    seen = capture_indices(agent)
    one_update(agent)
    assert agent.optim_step == 75 and len(seen) == 75
    assert bool(torch.isfinite(agent.policy.P).all())
    assert agent._mb_update == 1
    agent.exit()


def test_reference_mode_is_untouched():
    outs = []
    for kw in (dict(minibatch="reference"), dict()):
        agent = make_agent(**kw)
        assert agent.minibatch == "reference" and agent._mb_stage is None and agent._mb_index is None
        assert not hasattr(agent, "_mb_seed") and not hasattr(agent, "_mb_update")
        mc = agent.mini_chunk_size
        assert agent._minibatches() == [(j - mc, j) for _ in range(5) for j in range(mc, agent.rollout_size, mc)]
        one_update(agent)
        assert agent.optim_step == 75
        outs.append(agent.policy.P.clone())
        agent.exit()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


# ---- two data-parallel ranks on ONE GPU (gloo transport, as tests/test_obs_norm_dist_gpu.py)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    from fly_bproject_amd.dist import broadcast_policy
    from fly_bproject_amd.ppo import PPO
    from tests.hip_helpers import make_args
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.manual_seed(10 + rank)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(2048, rank=rank, world_size=world, seed=0, dp_mode="grad_allreduce", minibatch="shuffled"))
        broadcast_policy(agent)
        seen = capture_indices(agent)
        for _ in range(agent.rollout_size):
            agent.run()
    torch.cuda.synchronize()
    assert agent.optim_step == 75
    rows = agent.mini_chunk_size * 2048
    torch.save({"P": agent.policy.P.cpu(), "seed": agent._mb_seed, "idx": torch.from_numpy(seen[(0, 0)]),
                "want": torch.from_numpy(M.perm_index(16 * rows, M.rank_seed(0, rank), 0, np.arange(rows)))},
               os.path.join(out_dir, "r%d.pt" % rank))
    agent.exit()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_shuffle_differently_and_stay_in_step(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a = torch.load(tmp_path / "r0.pt", weights_only=True)
    b = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert torch.equal(a["P"].view(torch.int32), b["P"].view(torch.int32))
    assert a["seed"] == M.rank_seed(0, 0) and b["seed"] == M.rank_seed(0, 1)
    assert torch.equal(a["idx"], a["want"]) and torch.equal(b["idx"], b["want"])
    assert float((a["idx"] == b["idx"]).float().mean()) < 0.01
