"""GPU (-m gpu): running observation normalisation (PPO normalize_obs) -- the statistics pass and merge against float64
numpy, the normalised copy against torch bit for bit, every rollout form bit for bit, the policy seeing normalised inputs,
the timing of the merges, the update against the torch backend, and trainer.py end to end with a checkpoint."""
import contextlib
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import obs_norm_ref as R
from tests.hip_helpers import make_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return C.c_void_p(t.data_ptr())


class _Stats:
    """S, the table and the moment sets on the device, driven through the C ABI."""

    def __init__(self, clip=5.0):
        from fly_bproject_amd import _lib
        from fly_bproject_amd.ppo import obs_norm_table
        self.lib, self._lib, self.clip = _lib.load(), _lib, clip
        self.stats = torch.zeros(147, dtype=torch.float64, device=DEV)
        self.stats[74:] = 1.0
        self.table = obs_norm_table(self.stats, clip).to(DEV)
        self.sets = torch.zeros((_lib.OBS_NORM_SETS, 147), dtype=torch.float64, device=DEV)

    def pass_(self, ring, count_from):
        rows = ring.numel() // 73
        out = torch.empty_like(ring)
        self._lib.check(self.lib.ppo_obs_norm_pass(_p(ring), rows, count_from, _p(self.table), _p(out), _p(self.sets), None),
                        "ppo_obs_norm_pass")
        return out

    def merge(self, sets=None):
        sets = self.sets if sets is None else sets
        self._lib.check(self.lib.ppo_obs_norm_merge(_p(self.stats), _p(self.table), _p(sets), sets.shape[0], self.clip, None),
                        "ppo_obs_norm_merge")

    def host(self):
        s = self.stats.cpu().numpy()
        return s[0], s[1:74], s[74:]


def _assert_stats(got, want):
    c, mu, var = got
    wc, wmu, wvar = want
    assert c == wc
    np.testing.assert_allclose(mu, wmu, rtol=1e-10, atol=1e-12)
    zero = wvar == 0
    np.testing.assert_allclose(var[~zero], wvar[~zero], rtol=1e-10, atol=0)
    assert np.all(np.abs(var[zero]) <= 1e-12)


@pytest.mark.parametrize("n", [300, 8192, 16384])
def test_pass_and_merge_statistics(n):
    """From the initial S, one pass over rows 1..T plus one merge equals the float64 moments of those rows (1e-10 relative,
    1e-12 absolute where the variance is 0), on columns of mean 1e3 / std 1e-2, constant, 0/1; two rollouts merged one after
    the other equal one merge of both; two runs are bit-identical; the table is the float64 one rounded once."""
    T = 12
    x = R.hard_ring(2 * T + 1, n, seed=n)
    a, b = x[:T + 1], x[T:]                                  # b's row 0 is a's row T (the ring's carry)
    runs = []
    for _ in range(2):
        st = _Stats()
        st.pass_(torch.from_numpy(a).to(DEV), n)
        st.merge()
        first = st.host()
        st.pass_(torch.from_numpy(b).to(DEV), n)
        st.merge()
        torch.cuda.synchronize()
        runs.append((first, st.host(), st.table.cpu().numpy()))
    _assert_stats(runs[0][0], R.moments(a[1:]))
    _assert_stats(runs[0][1], R.moments(x[1:]))
    for u, v in zip(runs[0][:2], runs[1][:2]):
        for p, q in zip(u, v):
            assert np.array_equal(p, q)
    S = runs[0][1]
    np.testing.assert_array_equal(runs[0][2], R.table(S, 5.0))
    # one merge of the concatenation (the pass counts rows >= count_from of whatever it is given)
    st = _Stats()
    st.pass_(torch.from_numpy(np.concatenate([a, b[1:]])).to(DEV), n)
    st.merge()
    _assert_stats(st.host(), R.moments(x[1:]))
    np.testing.assert_allclose(st.host()[1], S[1], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(st.host()[2], S[2], rtol=1e-10, atol=1e-12)


def test_normalised_copy_is_torch_bit_for_bit():
    """The pass's copy == ((x - m) * r).clamp(-clip, clip) in torch for every row (row 0 included), with a NaN row that stays
    NaN and values far beyond the clip; the raw ring is untouched."""
    from fly_bproject_amd.ppo import normalize_obs_ref
    n, T = 1000, 5
    x = torch.from_numpy(R.hard_ring(T, n, seed=1)).to(DEV)
    st = _Stats(clip=3.0)
    st.pass_(x, n)
    st.merge()                                               # a non-trivial table
    x[2, 7] = float("nan")
    x[3, 9, :] = 1e30
    x[3, 10, :] = -1e30
    x[4, 11, :] = float("inf")
    raw = x.clone()
    y = st.pass_(x, n)
    torch.cuda.synchronize()
    assert torch.equal(x, raw) or torch.equal(torch.nan_to_num(x), torch.nan_to_num(raw))
    want = normalize_obs_ref(x, st.table)
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and torch.isnan(y[2, 7]).all()
    assert torch.equal(torch.nan_to_num(y), torch.nan_to_num(want))
    assert (y[3, 9] == 3.0).all() and (y[3, 10] == -3.0).all() and (y[4, 11] == 3.0).all()
    assert float(y.abs().nan_to_num().max()) <= 3.0


def _run(agent, steps):
    for _ in range(steps):
        agent.run()


@pytest.mark.parametrize("n,fs", [(4096, None), (8192, None), (16384, None), (300, None), (4096, "0"), (8192, "0")])
def test_every_rollout_form_bit_for_bit(n, fs, monkeypatch):
    """tests/test_ppo_gpu.py's one-launch-per-rollout test with normalize_obs: persistent and per-step launches agree bit for
    bit on the ring, actions, log-probs, values, rewards, flags, action_var, parameters and S, over two iterations with their
    updates and merges."""
    from fly_bproject_amd.ppo import PPO
    if fs is not None:
        monkeypatch.setenv("FLY_ROLLOUT_FS", fs)
    res = {}
    for persistent in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(n, persistent_rollout=persistent, normalize_obs=True))
            assert agent.persistent_rollout == persistent
            T = agent.rollout_size
            iters = 2 if T <= 160 else 1
            extra = 37 if T > 37 else T // 2
            flags = []
            for i in range(iters * T + extra):
                agent.run()
                if i >= iters * T:
                    flags.append((agent.env.reset_buf.clone(), agent.env.progress_buf.clone()))
            agent.flush_log()
        torch.cuda.synchronize()
        assert agent.optim_step == 75 * iters
        assert float(agent.obs_count) == iters * T * n
        res[persistent] = (agent._obs_ring[:extra + 1].clone(), agent.all_acts[:extra].clone(), agent.all_reward[:extra].clone(),
                           agent.all_log_prob[:extra].clone(), agent._v_ring[:extra].clone(), float(agent.action_var[0]),
                           agent.policy.P.clone(), agent.policy.exp_avg_sq.clone(), agent.all_advantage.clone(),
                           torch.stack([f[0] for f in flags]), torch.stack([f[1] for f in flags]),
                           agent._obs_stats.clone(), agent._obs_table.clone())
        agent.exit()
    for i, (a, b) in enumerate(zip(res[False], res[True])):
        if torch.is_tensor(a):
            assert torch.equal(a, b), i
        else:
            assert a == b, (i, a, b)


def _two_iterations(**kw):
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096, normalize_obs=True, **kw))
        _run(agent, 2 * agent.rollout_size)
        agent.flush_log()
    torch.cuda.synchronize()
    out = [agent._obs_ring.clone(), agent.all_acts.clone(), agent.all_log_prob.clone(), agent._v_ring.clone(),
           agent.all_reward.clone(), agent.policy.P.clone(), agent._obs_stats.clone(), float(agent.action_var[0])]
    return agent, out


def test_graph_replay_equals_eager():
    _, eager = _two_iterations(persistent_rollout=False)
    agent, graph = _two_iterations(graph=True)
    assert agent.use_graph and agent._graphs
    agent.exit()
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b), i


def test_recording_leaves_normalised_training_unchanged(tmp_path):
    a0, plain = _two_iterations()
    a0.exit()
    agent, rec = _two_iterations(record=True, record_dir_name=str(tmp_path / "f"), time_steps_per_recorded_frame=40)
    poses = agent.env.recorder.poses[:agent.rollout_size].clone()
    agent.generate_video()
    agent.exit()
    for i, (a, b) in enumerate(zip(plain, rec)):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b), i
    assert torch.isfinite(poses).all()


def test_policy_sees_normalised_inputs():
    """Value row t of the rollout == the critic forward (same arithmetic) of normalize(ring[t]; S_k), != that of the raw row;
    make_data's obs == the normalised rows 0..T-1 (bit for bit against torch)."""
    from fly_bproject_amd.ppo import PPO, normalize_obs_ref
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096, normalize_obs=True))
        T = agent.rollout_size
        _run(agent, T)                                       # iteration 1: S_1 is merged after its update
        _run(agent, T - 1)                                   # rollout 2 under S_1 (one launch: all T rows written), no update yet
    torch.cuda.synchronize()
    table = agent._obs_table.clone()
    with torch.no_grad():
        obs = agent.make_data()[0]
        want = normalize_obs_ref(agent._obs_ring[:T], table)
        assert torch.equal(obs, want)
        v_norm = agent.net.v(want[:T - 1].reshape(-1, 73)).view(T - 1, -1)
        v_raw = agent.net.v(agent._obs_ring[:T - 1].reshape(-1, 73)).view(T - 1, -1)
    v_roll = agent._v_ring[:T - 1].view(T - 1, -1)
    torch.testing.assert_close(v_roll, v_norm, rtol=2e-6, atol=2e-6)
    assert not torch.allclose(v_roll, v_raw, rtol=1e-3, atol=1e-3)
    assert float(agent.obs_count) == T * 4096
    agent.exit()


def test_statistics_follow_the_rollouts_and_testing_never_merges(tmp_path):
    """After iteration k, S == the float64 moments of rows 1..T of rollouts 1..k; in --testing S stays as loaded."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    rows = []
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096, normalize_obs=True, save=True, save_path=str(tmp_path / "ck_"), save_freq=75))
        T = agent.rollout_size
        assert float(agent.obs_count) == 0 and torch.equal(agent.obs_var, torch.ones(73, dtype=torch.float64, device=DEV))
        for k in range(3):
            _run(agent, T - 1)
            torch.cuda.synchronize()
            # the last step of the rollout is issued by the next run() (its update follows); the rows are final once it is
            agent.run()
            torch.cuda.synchronize()
            rows.append(agent._obs_ring[1:].cpu().numpy().copy())
            want = R.moments(np.concatenate(rows))
            _assert_stats((float(agent.obs_count), agent.obs_mean.cpu().numpy(), agent.obs_var.cpu().numpy()), want)
        agent.flush_log()
    saved = (agent.obs_mean, agent.obs_var, agent.obs_count)
    agent.exit()
    sd = torch.load(str(tmp_path / "ck_225.pth"), weights_only=True)
    assert sd["obs_rms.mean"].dtype == torch.float64 and sd["obs_rms.var"].shape == (73,) and sd["obs_rms.count"].dim() == 0
    with contextlib.redirect_stdout(io.StringIO()):
        t = PPO(make_args(4096, normalize_obs=True, load=True, load_path=str(tmp_path / "ck_225.pth"), testing=True))
        for got, want in zip((t.obs_mean, t.obs_var, t.obs_count), saved):
            assert torch.equal(got, want)
        table = t._obs_table.clone()
        _run(t, 2 * t.rollout_size + 3)
    torch.cuda.synchronize()
    assert torch.equal(t.obs_count, saved[2]) and torch.equal(t.obs_mean, saved[0]) and torch.equal(t._obs_table, table)
    t.exit()
    with pytest.raises(ValueError, match="--normalize_obs"):
        with contextlib.redirect_stdout(io.StringIO()):
            PPO(make_args(4096, load=True, load_path=str(tmp_path / "ck_225.pth"), testing=True))


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "f32"])
def test_update_agrees_with_torch_backend(gemm):
    """One update with normalisation on, through the HIP kernels in each arithmetic, against update_backend="torch" on the same
    normalised rollout: the bound of tests/test_mlp_train_gpu.py::test_ppo_hip_and_torch_updates_agree."""
    from fly_bproject_amd.ppo import PPO
    outs, init, fn, refused = {}, None, {}, 0
    for backend in ("hip", "torch"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(4096, update_backend=backend, normalize_obs=True))
            agent.policy.gemm = gemm
            init = {k: v.clone() for k, v in agent.net.state_dict().items()}
            with torch.no_grad():
                probe = torch.randn(512, 73, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
                fn["init"] = torch.cat([agent.net.pi(probe), agent.net.v(probe)], dim=1)
            _run(agent, agent.rollout_size)
            with torch.no_grad():
                fn[backend] = torch.cat([agent.net.pi(probe), agent.net.v(probe)], dim=1)
        assert agent.optim_step == 75
        if backend == "hip":
            refused = agent.policy.h2_overflows
        outs[backend] = {k: v.clone() for k, v in agent.net.state_dict().items()}
        outs[backend + "_S"] = agent._obs_stats.clone()
        agent.exit()
    print("gemm %s: updates with a refused fp16x2 step: %d" % (gemm, refused))
    assert torch.equal(outs["hip_S"], outs["torch_S"])              # same rollout, same statistics
    for k in init:
        moved = float((outs["torch"][k] - init[k]).norm())
        apart = float((outs["hip"][k] - outs["torch"][k]).norm())
        assert moved > 0 and apart <= 0.3 * moved, (k, apart, moved)
    moved = float((fn["torch"] - fn["init"]).norm())
    apart = float((fn["hip"] - fn["torch"]).norm())
    assert apart <= 0.2 * moved, (apart, moved)


def test_two_launch_step_refuses_normalisation(monkeypatch):
    from fly_bproject_amd import _lib
    from fly_bproject_amd.ppo import PPO
    monkeypatch.setenv("FLY_FUSE_ROLLOUT_STEP", "0")
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096, normalize_obs=True, persistent_rollout=False))
        with pytest.raises(_lib.FlyHipError, match="normalise"):
            agent.run()
    agent.exit()


def test_trainer_end_to_end(tmp_path):
    """trainer.py --normalize_obs trains and saves; --testing --load_path runs from the checkpoint, statistics and all."""
    ck = str(tmp_path / "ck_")
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "trainer.py"), "--num_envs", "4096", "--headless", "True",
                        "--normalize_obs", "--max_steps", "330", "--save_path", ck, "--save_freq", "75"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Steps: 0300" in r.stdout and "Training" in r.stdout
    sd = torch.load(ck + "150.pth", weights_only=True)
    assert float(sd["obs_rms.count"]) == 2 * 160 * 4096
    r = subprocess.run([sys.executable, os.path.join(REPO, "trainer.py"), "--num_envs", "4096", "--headless", "True",
                        "--normalize_obs", "--testing", "True", "--max_steps", "210", "--load_path", ck + "150.pth"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert "Steps: 0200" in r.stdout and "Training" not in lines and not any("holds no observation statistics" in ln for ln in lines)
