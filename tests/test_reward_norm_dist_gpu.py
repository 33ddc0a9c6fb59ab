"""GPU (-m gpu): reward scaling on two data-parallel ranks on ONE MI355X (gloo transport, the harness of
tests/test_episode_stats_dist_gpu.py).  Every rank gathers both ranks' sets and merges them in rank order: after an iteration
both ranks hold bit-identical S_r and table, equal to one ppo_value_norm_merge of the two ranks' sets in rank order and to the
reference's moments of both ranks' returns; the carries are each rank's own."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import reward_norm_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, REPO)
    import contextlib
    import io
    import torch.distributed as dist
    from fly_bproject_amd.dist import broadcast_policy
    from fly_bproject_amd.ppo import PPO
    from tests.hip_helpers import make_args
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.manual_seed(10 + rank)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(N, rank=rank, world_size=world, seed=0, normalize_reward=True))
        broadcast_policy(agent)
        for _ in range(agent.rollout_size):
            agent.run()
        agent.flush_log()
    torch.cuda.synchronize()
    assert agent.optim_step == 75
    torch.save({"sets": agent._rnorm_sets.cpu(), "gathered": agent._keep_rnorm_sets.cpu(), "stats": agent._rnorm_stats.cpu(),
                "table": agent._rnorm_table.cpu(), "carry": agent._rnorm_carry.cpu(), "reward": agent.all_reward.cpu(),
                "reset": agent._reset_rows.cpu(), "T": agent.rollout_size},
               os.path.join(out_dir, "r%d.pt" % rank))
    agent.exit()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_statistics_of_both_ranks_returns(tmp_path):
    from fly_bproject_amd import _lib
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(tmp_path / "r0.pt", weights_only=True)
    b = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["table"], b["table"])
    assert not torch.equal(a["sets"], b["sets"]) and not torch.equal(a["reward"], b["reward"])       # different rollouts
    assert not torch.equal(a["carry"], b["carry"])                                                    # the carries are per rank
    both = torch.cat([a["sets"], b["sets"]])                                                          # rank order
    assert torch.equal(a["gathered"], both) and torch.equal(b["gathered"], both)
    T = a["T"]
    assert float(a["stats"][0]) == 2 * T * N
    # one merge of the two ranks' sets in rank order, here
    dev = "cuda:0"
    init = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
    sets, out, tab = both.to(dev), torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(4, device=dev)
    _lib.api().ppo_value_norm_merge(init, sets, sets.shape[0], out, tab, None)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), a["stats"]) and torch.equal(tab.cpu(), a["table"])
    # and the reference on both ranks' own rows
    G = []
    for r in (a, b):
        w = R.walk(r["reward"].numpy()[..., 0], r["reset"].numpy(), 0.99)
        G.append(w.G)
        assert np.array_equal(r["carry"].numpy().view(np.uint64), w.carry.view(np.uint64))
    c, mu, var = R.moments(np.concatenate(G))
    got = a["stats"].numpy()
    assert got[0] == c
    np.testing.assert_allclose(got[1], mu, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(got[2], var, rtol=1e-10, atol=0)
    assert np.array_equal(a["table"].numpy().view(np.uint32), R.table(tuple(got)).view(np.uint32))
