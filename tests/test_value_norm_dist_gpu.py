"""GPU (-m gpu): value normalisation with two data-parallel ranks on ONE MI355X (gloo transport, as
tests/test_obs_norm_dist_gpu.py).  Every rank gathers all ranks' target moments and merges them in rank order, so after every
update the running statistics and the table are bit-identical on both ranks and equal the float64 moments of both ranks' raw
targets."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import value_norm_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    targets = []
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(2048, rank=rank, world_size=world, seed=0, normalize_value=True))
        if rank == 0:
            agent._value_stats[1] = 0.25                    # rank 0's statistics must reach rank 1 with the policy
            agent._value_table[0] = 0.25
        broadcast_policy(agent)
        start = (agent._value_stats.clone(), agent._value_table.clone())
        agent._value_stats[1] = 0.0                          # then start both from the initial S_v
        agent._value_table[0] = 0.0
        for _ in range(2):
            for _ in range(agent.rollout_size):
                agent.run()
            targets.append(agent._target.cpu())              # the raw targets of the rollout just trained on
    torch.cuda.synchronize()
    assert agent.optim_step == 150
    torch.save({"P": agent.policy.P.cpu(), "S": agent._value_stats.cpu(), "table": agent._value_table.cpu(),
                "targets": torch.stack(targets), "start": (start[0].cpu(), start[1].cpu()), "T": agent.rollout_size},
               os.path.join(out_dir, "r%d.pt" % rank))
    agent.exit()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_share_value_statistics(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a = torch.load(tmp_path / "r0.pt", weights_only=True)
    b = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert torch.equal(a["start"][0], b["start"][0]) and torch.equal(a["start"][1], b["start"][1])    # broadcast_policy
    assert float(b["start"][0][1]) == 0.25 and float(b["start"][1][0]) == 0.25
    assert torch.equal(a["S"], b["S"]) and torch.equal(a["table"], b["table"]) and torch.equal(a["P"], b["P"])
    assert not torch.equal(a["targets"], b["targets"])                              # different rollouts
    S = a["S"].numpy()
    assert S[0] == 2 * a["T"] * 2048 * 2
    want = R.moments(np.concatenate([a["targets"].numpy().reshape(-1), b["targets"].numpy().reshape(-1)]))
    print("two ranks: S_v %r, float64 moments %r" % (tuple(S), want))
    assert S[0] == want[0]
    np.testing.assert_allclose(S[1], want[1], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(S[2], want[2], rtol=1e-10, atol=0)
    np.testing.assert_array_equal(a["table"].numpy(), R.table(tuple(S)))
