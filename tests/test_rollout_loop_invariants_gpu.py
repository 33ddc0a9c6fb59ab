"""The one-launch rollout (ppo_rollout_all) fetches FlyConfig once per launch, stores the env's state tensors only after a tile's
last step and carries the episode accumulators in registers.  Everything a launch leaves behind must still be, bit for bit, what T
launches of ppo_rollout_step leave: the rollout rows, the env's state tensors and the five episode accumulators.

Each case clones one warmed-up env state into two envs, gives both the same weights, noise and variance, runs the one launch on the
first and the T per-step launches on the second, and compares with torch.equal.  Every second env starts two steps short of its time
limit and every fourth-plus-one with its reset flag set, so that resets fire inside the rollout (from carried registers) and the
finished-episode sums move."""
import ctypes as C

import pytest
import torch

from fly_bproject_amd import _lib
from tests.hip_helpers import make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VAR_MIN = 0.01
EPISODE = ("episode_return_buf", "episode_length_buf", "finished_return_sum", "finished_length_sum", "finished_count")
ROWS = ("obs", "act", "logp", "v", "reward", "reset", "progress")


def _policy(seed=3):
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(seed)
    pol = PackedPolicy(Net(73, 18).to(DEV), DEV)
    pol.gemm = "bf16x3"                     # whole tiles then take rollout_all_fs_kernel, ragged ones rollout_all_kernel<true>
    return pol


def _rings(rows, n):
    f = dict(dtype=torch.float32, device=DEV)
    return {"obs": torch.zeros(rows + 1, n, 73, **f), "act": torch.zeros(rows, n, 18, **f), "logp": torch.zeros(rows, n, **f),
            "v": torch.zeros(rows + 1, n, **f), "reward": torch.zeros(rows, n, **f),
            "reset": torch.zeros(rows, n, dtype=torch.long, device=DEV), "progress": torch.zeros(rows, n, dtype=torch.long, device=DEV)}


class Pair:
    """envs[0] runs ppo_rollout_all, envs[1] the per-step launches, from one cloned state."""

    def __init__(self, n, norm=False, dr=False, episodes=True):
        self.n, self.episodes = n, episodes
        self.pol = _policy()
        self.envs = [make_env(n), make_env(n)]
        if dr:
            from tests.test_domain_rand_gpu import WIDE
            for env in self.envs:
                env.set_randomization(WIDE, seed=17)
        if norm:
            g = torch.Generator().manual_seed(11)
            self.table = torch.cat([0.2 * torch.randn(73, generator=g), 0.5 + 1.5 * torch.rand(73, generator=g), torch.tensor([2.0])]).to(DEV)
            torch.cuda.synchronize()
            for env in self.envs:
                _lib.api().fly_set_obs_norm(env._handle, self.table)
        a, b = self.envs
        g = torch.Generator().manual_seed(7)
        a.step((0.3 * torch.randn(n, 18, generator=g)).clamp(-1, 1).to(DEV))       # every env resets, then one step of physics
        a.progress_buf[0::2] = a.max_episode_length - 2                            # the time limit ends these at the rollout's step 0
        a.reset_buf[1::4] = 1                                                      # and these reset at its step 0
        a.episode_return_buf.copy_(torch.rand(n, generator=g).to(DEV) * 5 - 2)     # accumulators that are not zero: a load that
        a.episode_length_buf.copy_(torch.randint(1, 50, (n,), generator=g).float().to(DEV))   # is missing shows
        a.finished_return_sum.copy_(torch.rand(n, generator=g).to(DEV) * 40)
        a.finished_length_sum.copy_(torch.randint(0, 900, (n,), generator=g).float().to(DEV))
        a.finished_count.copy_(torch.randint(0, 9, (n,), generator=g).float().to(DEV))
        for k in a._STATE_TENSORS:
            getattr(b, k).copy_(getattr(a, k))
        if dr:
            b._dr_table.copy_(a._dr_table)
        self.obs0 = a.obs_buf.clone()
        if not episodes:
            for env in self.envs:
                bufs = env._bufs
                bufs.ep_return = bufs.ep_length = bufs.done_return = bufs.done_length = bufs.done_count = None
        self.before = {k: getattr(a, k).clone() for k in EPISODE}
        torch.cuda.synchronize()

    def run(self, T, launches=1, var_decay=1e-3):
        n, pol, api = self.n, self.pol, _lib.api()
        rows = T * launches
        g = torch.Generator().manual_seed(9)
        eps = torch.randn(rows, n, 18, generator=g).to(DEV)
        var = torch.linspace(VAR_MIN + 2 * 1e-3, 0.2, 18).to(DEV)
        one, steps = _rings(rows, n), _rings(rows, n)
        for r in (one, steps):
            r["obs"][0].copy_(self.obs0)
        env = self.envs[0]
        for k in range(launches):                 # var_decay is 0 when launches > 1: `var` is then row 0's variance of every launch
            lo = k * T
            if k > 0:                             # the current flags are the last row the previous launch wrote
                env._bufs.reset, env._bufs.progress = one["reset"][lo - 1].data_ptr(), one["progress"][lo - 1].data_ptr()
            api.ppo_rollout_all(env._handle, C.byref(env._bufs), pol.P, pol.PF, one["obs"][lo:], eps[lo:], var, var_decay, VAR_MIN,
                                one["act"][lo:], one["logp"][lo:], one["v"][lo:], one["reward"][lo:], T, None, pol.infer_pb_ptr(),
                                one["reset"][lo:], one["progress"][lo:], _lib.stream_ptr())
        env = self.envs[1]
        for t in range(rows):
            env.bind_obs(steps["obs"][t + 1])
            env.bind_reward(steps["reward"][t])
            api.ppo_rollout_step(env._handle, C.byref(env._bufs), pol.P, pol.PF, steps["obs"][t], eps[t], var, t, var_decay, VAR_MIN,
                                 steps["act"][t], steps["logp"][t], steps["v"][t], pol.infer_pb_ptr(), None, _lib.stream_ptr())
            steps["reset"][t].copy_(env.reset_buf)
            steps["progress"][t].copy_(env.progress_buf)
        torch.cuda.synchronize()
        return one, steps

    def compare(self, one, steps, rows):
        a, b = self.envs
        for k in ROWS:
            upto = rows + 1 if k == "obs" else rows           # v_ring's row T belongs to the critic pass
            assert torch.equal(one[k][:upto], steps[k][:upto]), k
        for k in a._STATE_TENSORS:
            if k in ("reset_buf", "progress_buf"):            # with flag rows the one launch only reads the env's own flags
                assert torch.equal(one[k[:-4]][rows - 1], getattr(b, k)), k
            else:
                assert torch.equal(getattr(a, k), getattr(b, k)), k
        if a.randomized:
            assert torch.equal(a._dr_table, b._dr_table)
        assert torch.isfinite(one["obs"]).all() and torch.isfinite(one["reward"]).all()
        # the case did what it is for: episodes ended inside the rollout, and (with the statistics on) the sums moved
        assert int(steps["reset"].sum()) > 0
        moved = not torch.equal(b.finished_count, self.before["finished_count"])
        assert moved == self.episodes
        if not self.episodes:
            for k in EPISODE:
                assert torch.equal(getattr(a, k), self.before[k]) and torch.equal(getattr(b, k), self.before[k]), k

    def close(self):
        for env in self.envs:
            env.exit()


def _check(n, T, launches=1, **kw):
    pair = Pair(n, **kw)
    try:
        one, steps = pair.run(T, launches, var_decay=1e-3 if launches == 1 else 0.0)
        pair.compare(one, steps, T * launches)
    finally:
        pair.close()


@pytest.mark.parametrize("n,T", [(64, 4), (64, 1), (300, 3)])
def test_one_launch_leaves_what_the_per_step_launches_leave(n, T):
    """64 envs: two whole tiles, the fused-style kernel; T = 1: the first step is the last, so it stores the state; 300 envs:
    a ragged last tile, so rollout_all_kernel."""
    _check(n, T)


def test_more_tiles_than_compute_units():
    """8224 envs = 257 tiles: on 256 CUs the smallest shape whose workgroup 0 walks a second tile (the MULTI instantiation), which
    must store the first tile's state before it loads the second's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if 8224 // 32 <= cus:
        pytest.skip("%d CUs: 257 tiles are one per workgroup here" % cus)
    _check(8224, 2)


def test_normalising_and_randomising_instantiations():
    _check(64, 3, norm=True, dr=True)


def test_second_launch_starts_from_what_the_first_stored():
    """Two launches back to back against 2T per-step launches: a final store the first launch left out would start the second
    from stale state, accumulators included."""
    _check(64, 3, launches=2)


def test_episode_pointers_null():
    """ep_return == NULL keeps meaning "off": nothing is read or written through the five pointers."""
    _check(64, 3, episodes=False)
