"""GPU (-m gpu): the make_data chain on two data-parallel ranks on ONE MI355X (gloo transport, the harness of
tests/test_reward_norm_dist_gpu.py): 2048 envs per rank (T = 320), every opt-in, two iterations.  Each worker captures its own
make_data / update() (tests/make_data_capture.py) and saves it; the parent runs ONE Chain(world_size=2) on both ranks' rows
and holds each rank to it as tests/test_make_data_chain_gpu.py does.  Beyond that: the statistics and tables are bit-identical
on the two ranks, and the advantages are normalised by the moments of all 2 T N rows."""
import os
import pickle
import signal
import socket
import sys
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import make_data_capture as K
from tests.test_make_data_chain_gpu import ALL

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, ITERATIONS = 2048, 320, 2
WORKER_LIMIT = 240                    # seconds: a worker that is still running then is killed by its own alarm


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    signal.alarm(WORKER_LIMIT)
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    from tests import make_data_capture as cap
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    info, its = cap.run_agent(N, ITERATIONS, world=world, rank=rank, world_size=world, seed=0, **ALL)
    with open(os.path.join(out_dir, "r%d.pkl" % rank), "wb") as f:
        pickle.dump((info, its), f, protocol=4)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_against_one_chain(tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + WORKER_LIMIT + 20
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a worker outlived its time limit")
    ranks = []
    for r in range(2):
        with open(tmp_path / ("r%d.pkl" % r), "rb") as f:
            ranks.append(pickle.load(f))
    infos, its = [r[0] for r in ranks], [r[1] for r in ranks]
    for r, info in enumerate(infos):
        assert (info["T"], info["N"], info["options"]["world_size"]) == (T, N, 2)
        K.check_coverage(info, its[r])
    assert infos[0]["mb_seed"] != infos[1]["mb_seed"]
    # bit-identical statistics and tables on the two ranks, from different rollouts
    for k in range(ITERATIONS):
        a, b = its[0][k], its[1][k]
        assert not np.array_equal(a["raw"]["reward"], b["raw"]["reward"])
        for name in ("S_r_next", "rnorm_table_next", "S_v_next", "value_table_next"):
            assert K.same(a["scratch"][name], b["scratch"][name]), (k, name)
        for name in ("S_r", "rnorm_table", "S_v", "value_table", "S_obs", "obs_table"):
            assert K.same(a["after"][name], b["after"][name]), (k, name)
        assert not K.same(a["after"]["carry"], b["after"]["carry"])                    # the carries are per rank
        # the advantages are normalised by the moments of all 2 T N rows: together they have mean 0 and std 1, apart they do not
        both = np.concatenate([x["returned"][4].reshape(-1).astype(np.float64) for x in (a, b)])
        assert abs(both.mean()) < 1e-5 and abs(both.std(ddof=1) - 1.0) < 1e-5
        assert K.same(a["scratch"]["adv_totals"], b["scratch"]["adv_totals"])
    # one chain over both ranks' rows
    kw = dict(minibatch_seeds=[i["mb_seed"] for i in infos], minibatch_rows=infos[0]["mb_rows"])
    c64, c32 = K.chain_pair(infos[0], **kw)
    outs64, outs32, states = [], [], []
    for k in range(ITERATIONS):
        raws = [its[r][k]["raw"] for r in range(2)]
        outs64.append(c64.step(raws))
        outs32.append(c32.step(raws))
        c64.commit()
        c32.commit()
        states.append(c64.state())
    peers = [[its[0][k], its[1][k]] for k in range(ITERATIONS)]
    for r in range(2):
        worst = K.check_rank(infos[r], its[r], [o[r] for o in outs64], [o[r] for o in outs32], states, peers, r)
        print("make_data chain, rank %d of 2: worst error / bar per output: %s"
              % (r, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
        assert max(worst.values()) <= 1.0
