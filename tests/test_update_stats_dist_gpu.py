"""GPU (-m gpu): the update diagnostics on two data-parallel ranks on ONE MI355X (gloo transport, the harness of
tests/test_episode_stats_dist_gpu.py).  Every rank gathers both ranks' sets and merges them in rank order: after an update both
ranks hold bit-identical last, window and total, equal to the reference's merge of the two ranks' own sets in rank order."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import update_stats_ref as R

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
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        agent = PPO(make_args(N, rank=rank, world_size=world, seed=0, update_stats=True))
        broadcast_policy(agent)
        for _ in range(agent.rollout_size):
            agent.run()
        agent.flush_log()
    torch.cuda.synchronize()
    assert agent.optim_step == 75
    torch.save({"sets": agent._us_sets.cpu(), "gathered": agent._keep_us_sets.cpu(), "last": agent._us_last.cpu(),
                "window": agent._us_window.cpu(), "total": agent._us_total.cpu(), "acts": agent.all_acts.cpu(),
                "T": agent.rollout_size, "lines": [ln for ln in out.getvalue().splitlines() if ln.startswith("Steps:")]},
               os.path.join(out_dir, "r%d.pt" % rank))
    agent.exit()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_sets_of_both_ranks_rows(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(tmp_path / "r0.pt", weights_only=True)
    b = torch.load(tmp_path / "r1.pt", weights_only=True)
    for k in ("last", "window", "total"):
        assert a[k].dtype == torch.float64 and torch.equal(a[k], b[k]), k
    assert not torch.equal(a["sets"], b["sets"]) and not torch.equal(a["acts"], b["acts"])            # different rollouts
    both = torch.cat([a["sets"], b["sets"]])                                                          # rank order
    assert torch.equal(a["gathered"], both) and torch.equal(b["gathered"], both)
    last, want = a["last"].numpy(), R.merge_all(both.numpy())
    plain = [k for k in range(R.SET) if k not in (R.TMEAN, R.TM2, R.EMEAN, R.EM2)]
    assert np.array_equal(last[plain].view(np.uint64), want[plain].view(np.uint64))
    np.testing.assert_allclose(last[[R.TMEAN, R.EMEAN]], want[[R.TMEAN, R.EMEAN]], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(last[[R.TM2, R.EM2]], want[[R.TM2, R.EM2]], rtol=1e-10, atol=0)
    rows = 2 * a["T"] * N
    assert last[R.ROWS] == rows and a["total"][R.ROWS] == rows and a["window"][R.ROWS] == rows and last[R.NONFINITE] == 0
    assert last[R.K3] > 0 and last[R.RMIN] < last[R.RMAX]
    # only rank 0 prints; one rollout's lines all come before its update
    assert a["lines"] and all(ln.endswith(" | KL n/a") for ln in a["lines"]) and b["lines"] == []
