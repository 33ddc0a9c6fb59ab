"""GPU (-m gpu): episode statistics on two data-parallel ranks on ONE MI355X (gloo transport, the harness of
tests/test_lambda_returns_dist_gpu.py).  Every rank gathers both ranks' sets and merges them in rank order: after a rollout both
ranks hold bit-identical window and total, equal to the reference's merge of the two ranks' own sets and to the reference's
set of both ranks' episodes."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import episode_stats_ref as R

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
        agent = PPO(make_args(N, rank=rank, world_size=world, seed=0, episode_stats=True))
        broadcast_policy(agent)
        for _ in range(agent.rollout_size):
            agent.run()
        agent.flush_log()
    torch.cuda.synchronize()
    assert agent.optim_step == 75
    torch.save({"sets": agent._ep_sets.cpu(), "gathered": agent._keep_ep_sets.cpu(), "total": agent._ep_total.cpu(),
                "window": agent._ep_window.cpu(), "reward": agent.all_reward.cpu(), "reset": agent._reset_rows.cpu(),
                "progress": agent._progress_rows.cpu(), "mel": int(agent.env.max_episode_length), "T": agent.rollout_size},
               os.path.join(out_dir, "r%d.pt" % rank))
    agent.exit()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_total_of_both_ranks_episodes(tmp_path):
    from tests.test_episode_stats_gpu import INTS, _check_set
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(tmp_path / "r0.pt", weights_only=True)
    b = torch.load(tmp_path / "r1.pt", weights_only=True)
    assert torch.equal(a["total"], b["total"]) and torch.equal(a["window"], b["window"])
    assert not torch.equal(a["sets"], b["sets"]) and not torch.equal(a["reward"], b["reward"])       # different rollouts
    both = torch.cat([a["sets"], b["sets"]])                                                          # rank order
    assert torch.equal(a["gathered"], both) and torch.equal(b["gathered"], both)
    total = a["total"].numpy()
    # the reference's merge of the two ranks' sets
    want = R.pool(both.numpy())
    exact = INTS + [R.ROWS, R.RMIN, R.RMAX]
    assert np.array_equal(total[exact], want[exact]) and total[R.ROWS] == 2 * a["T"] * N
    n, big = want[R.N_], max(abs(want[R.RMIN]), abs(want[R.RMAX]))
    assert n > 100
    assert abs(total[R.MEAN] - want[R.MEAN]) <= 8 * n * R.U * big
    assert abs(total[R.M2] - want[R.M2]) <= 8 * n * R.U * (want[R.M2] + n * want[R.MEAN] ** 2)
    # and the reference's set of both ranks' episodes, from their own rows
    episodes = []
    for r in (a, b):
        w = R.walk(r["reward"].numpy()[..., 0], r["reset"].numpy(), r["progress"].numpy(), r["mel"])
        episodes += w.episodes
    _check_set(total, R.Walk(episodes, None, None, None, None, None), 2 * a["T"] * N, "two ranks")
