"""GPU (-m gpu): running value normalisation (PPO normalize_value) -- the GAE pass with denormalisation against today's kernel
(identity table, bit for bit) and against the float32 reference, its moments and the merge against float64 numpy, the apply
against torch bit for bit, the make_data / update flow in PPO (scratch, commit, checkpoint), the flag-off path, the update
against the torch backend, and trainer.py end to end."""
import contextlib
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import value_norm_ref as R
from tests.hip_helpers import cuda, make_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = (0.0, 0.0, 1.0 - 1e-5)           # var + 1e-5 = 1 to an ulp: m = 0, s = r = 1.0f


def _p(t):
    return C.c_void_p(t.data_ptr())


class _VN:
    """The three entry points through the C ABI, with the sets, the scratch statistics and the scratch table on the device."""

    def __init__(self, S=R.initial()):
        from fly_bproject_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.stats = torch.tensor(S, dtype=torch.float64, device=DEV)
        self.table = cuda(R.table(S))
        self.sets = torch.full((_lib.VALUE_NORM_SETS, 3), -7.0, dtype=torch.float64, device=DEV)
        self.stats_out = torch.zeros(3, dtype=torch.float64, device=DEV)
        self.table_out = torch.full((4,), -7.0, device=DEV)

    def gae(self, r, v, vn, d, mode, guards=None):
        """-> (target, adv).  With `guards` = three sentinel-guarded buffers for the targets, the advantages and the sets
        (objects with .ptr and .get(), as tests/test_gae_episodic_gpu.py's Guarded) the launch writes into those: -> (target,
        adv, sets [k][3]), the guards checked on the way, and the sets copied to self.sets for merge()."""
        T, N = r.shape
        dr, dv, dvn, dd = cuda(r), cuda(v), cuda(vn), cuda(d)
        if guards is not None:
            tgt, adv, sets = guards
            self._lib.check(self.lib.ppo_td_gae_vnorm(_p(dr), _p(dv), _p(dvn), _p(dd), _p(self.table), 0.99, 0.95, T, N, tgt.ptr,
                                                      adv.ptr, sets.ptr, mode, None), "ppo_td_gae_vnorm")
            out = tgt.get().reshape(T, N), adv.get().reshape(T, N), sets.get().reshape(-1, 3)
            self.sets.copy_(cuda(out[2]))
            return out
        tgt, adv = torch.empty(T, N, device=DEV), torch.empty(T, N, device=DEV)
        self._lib.check(self.lib.ppo_td_gae_vnorm(_p(dr), _p(dv), _p(dvn), _p(dd), _p(self.table), 0.99, 0.95, T, N, _p(tgt),
                                                  _p(adv), _p(self.sets), mode, None), "ppo_td_gae_vnorm")
        torch.cuda.synchronize()
        return tgt.cpu().numpy(), adv.cpu().numpy()

    def gae_plain(self, r, v, vn, d, mode):
        T, N = r.shape
        dr, dv, dvn, dd = cuda(r), cuda(v), cuda(vn), cuda(d)
        tgt, adv = torch.empty(T, N, device=DEV), torch.empty(T, N, device=DEV)
        self._lib.check(self.lib.ppo_td_gae(_p(dr), _p(dv), _p(dvn), _p(dd), 0.99, 0.95, T, N, _p(tgt), _p(adv), mode, None),
                        "ppo_td_gae")
        torch.cuda.synchronize()
        return tgt.cpu().numpy(), adv.cpu().numpy()

    def merge(self, sets=None):
        sets = self.sets if sets is None else sets
        self._lib.check(self.lib.ppo_value_norm_merge(_p(self.stats), _p(sets), sets.shape[0], _p(self.stats_out),
                                                      _p(self.table_out), None), "ppo_value_norm_merge")
        torch.cuda.synchronize()

    def commit(self):
        self.stats.copy_(self.stats_out)
        self.table.copy_(self.table_out)

    def out(self):
        return tuple(float(x) for x in self.stats_out.cpu().numpy())


def _assert_stats(got, want):
    """The bounds tests/test_obs_norm_gpu.py holds its statistics to."""
    (c, mu, var), (wc, wmu, wvar) = got, want
    print("value statistics: count %r (want %r)  mean %.17g (want %.17g)  var %.17g (want %.17g)" % (c, wc, mu, wmu, var, wvar))
    assert c == wc
    np.testing.assert_allclose(mu, wmu, rtol=1e-10, atol=1e-12)
    if wvar == 0:
        assert abs(var) <= 1e-12
    else:
        np.testing.assert_allclose(var, wvar, rtol=1e-10, atol=0)


def _random_case(T, N, mode, seed):
    rng = np.random.default_rng(seed)
    r, v, vn = (rng.normal(0, 1, (T, N)).astype(np.float32) for _ in range(3))
    d = (rng.random((T, N) if mode & 1 else (N,)) < 0.9).astype(np.float32)
    return r, v, vn, d


def test_identity_table_is_exact():
    tab = R.table(IDENTITY)
    assert tab[0] == 0.0 and tab[1] == np.float32(1.0) and tab[2] == np.float32(1.0) and tab[3] == 0.0


@pytest.mark.parametrize("tag", ["a", "b"])
def test_identity_table_reproduces_td_gae_on_the_golden(tag):
    """Under m = 0, s = 1 ppo_td_gae_vnorm is ppo_td_gae bit for bit in every lane = env mode, and in the reference's mode the
    stored target / advantage of tests/golden/g6_gae.npz."""
    g = np.load(os.path.join(REPO, "tests", "golden", "g6_gae.npz"))
    r, v, vn = g[tag + "_reward"][..., 0], g[tag + "_v"][..., 0], g[tag + "_v_next"][..., 0]
    d_row = g[tag + "_done"][..., 0].astype(np.float32)
    T, N = r.shape
    vn_ = _VN(IDENTITY)
    for mode in range(4):
        d = np.ascontiguousarray(np.broadcast_to(d_row, (T, N))) if mode & 1 else d_row
        tg, adv = vn_.gae(r, v, vn, d, mode)
        t0, a0 = vn_.gae_plain(r, v, vn, d, mode)
        assert np.array_equal(tg, t0) and np.array_equal(adv, a0), mode
        if mode == 0:
            assert np.array_equal(tg, g[tag + "_target"][..., 0]) and np.array_equal(adv, g[tag + "_adv"][..., 0])


@pytest.mark.parametrize("N", [300, 8192, 16384])
def test_identity_table_reproduces_td_gae_at_size(N):
    T = 160
    vn_ = _VN(IDENTITY)
    for mode in range(4):
        r, v, vn, d = _random_case(T, N, mode, seed=N + mode)
        tg, adv = vn_.gae(r, v, vn, d, mode)
        t0, a0 = vn_.gae_plain(r, v, vn, d, mode)
        assert np.array_equal(tg, t0) and np.array_equal(adv, a0), mode


@pytest.mark.parametrize("T,N,mode", [(40960, 16, 0), (640, 100, 1), (3, 5, 0)])
def test_identity_table_reproduces_the_scan_form(T, N, mode):
    """The scan form is the same code path as ppo_td_gae's with an exact denormalisation: bit for bit."""
    vn_ = _VN(IDENTITY)
    r, v, vn, d = _random_case(T, N, mode, seed=T + N)
    tg, adv = vn_.gae(r, v, vn, d, mode | 4)
    t0, a0 = vn_.gae_plain(r, v, vn, d, mode | 4)
    assert np.array_equal(tg, t0) and np.array_equal(adv, a0)
    assert vn_.lib.ppo_td_gae_vnorm(_p(vn_.table), _p(vn_.table), _p(vn_.table), _p(vn_.table), _p(vn_.table), 0.99, 0.95, 1, 1,
                                    _p(vn_.table_out), _p(vn_.table_out), _p(vn_.sets), 4 | 2, None) == -1   # as ppo_td_gae


@pytest.mark.parametrize("T,N", [(160, 300), (80, 8192), (40, 16384), (7, 130)])
def test_nontrivial_table_against_the_float32_reference(T, N):
    """Critic outputs of unit scale under a table of mean 37.5 / std ~ 211: targets and advantages equal the float32 reference
    (the same separately rounded ops in the same order) bit for bit, in the four lane = env modes."""
    S = (1000.0, 37.5, 44444.0)
    vn_ = _VN(S)
    for mode in range(4):
        r, v, vn, d = _random_case(T, N, mode, seed=7 * N + mode)
        r = (r * 20).astype(np.float32)
        tg, adv = vn_.gae(r, v, vn, d, mode)
        t2, a2 = R.td_gae(r, v, vn, d, R.table(S), mode=mode)
        assert np.array_equal(tg, t2) and np.array_equal(adv, a2), mode


def test_nontrivial_table_scan_form():
    """The scan form under a non-trivial table against the sequential float32 reference at 1e-5, N = 16, T = 40 960.  The
    table (m = 0.25, var = 0.6) keeps targets and advantages at the unit scale that bound was stated for (ppo_kernels.hip); only
    the 63 chunk carries are re-associated, and a carry decays by (gamma lambda)^640 across a chunk."""
    T, N = 40960, 16
    S = (1000.0, 0.25, 0.6)
    vn_ = _VN(S)
    for mode in (0, 1):
        r, v, vn, d = _random_case(T, N, mode, seed=11 + mode)
        tg, adv = vn_.gae(r, v, vn, d, mode | 4)
        t2, a2 = R.td_gae(r, v, vn, d, R.table(S), mode=mode)
        print("scan mode %d: max |adv - ref| %.3g, max |adv| %.3g" % (mode, np.abs(adv - a2).max(), np.abs(a2).max()))
        assert np.array_equal(tg, t2)                        # the targets are elementwise: bit for bit
        np.testing.assert_allclose(adv, a2, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("N", [300, 8192, 16384])
def test_moments_and_merge_against_float64(kind, N):
    """v_next = 0 and m = 0, so the TD target is the reward exactly: (a) mean 1e3 / std 1e-2, (b) constant 0.37, (c) mean -3e4 /
    std 50.  One pass + one merge from the initial S_v equals the float64 moments; two rollouts merged one after the other equal
    one merge of both; two runs are bit-identical; stats_in is not written; the table is the float64 one rounded once."""
    T = 80
    x = R.hard_rewards(kind, 2 * T, N, seed=N)
    a, b = x[:T], x[T:]
    zeros, ones = np.zeros((T, N), np.float32), np.ones(N, np.float32)

    def two_rollouts():
        st = _VN()
        tg, _ = st.gae(a, zeros, zeros, ones, 0)
        assert np.array_equal(tg, a)
        before = st.stats.clone()
        st.merge()
        assert torch.equal(st.stats, before)                 # the merge reads stats_in, it never writes it
        first = (st.out(), st.table_out.cpu().numpy(), st.sets.clone())
        st.stats.copy_(st.stats_out)                         # commit the statistics; the table stays at m = 0, so tg = reward again
        tg, _ = st.gae(b, zeros, zeros, ones, 0)
        assert np.array_equal(tg, b)
        st.merge()
        return first + (st.out(), st.table_out.cpu().numpy(), st.sets.clone())

    run1, run2 = two_rollouts(), two_rollouts()
    for u, w in zip(run1, run2):                             # two runs: bit-identical
        assert torch.equal(u, w) if torch.is_tensor(u) else np.array_equal(u, w)
    S1, tab1, sets_a, S2, tab2, sets_b = run1
    _assert_stats(S1, R.moments(a))
    _assert_stats(S2, R.moments(x))
    np.testing.assert_array_equal(tab1, R.table(S1))
    np.testing.assert_array_equal(tab2, R.table(S2))
    # one merge of both rollouts' sets (2 x 256, as a data-parallel caller passes them)
    one = _VN()
    one.merge(torch.cat([sets_a, sets_b]))
    _assert_stats(one.out(), R.moments(x))
    np.testing.assert_allclose(one.out()[1], S2[1], rtol=1e-10, atol=1e-12)
    if R.moments(x)[2] > 0:
        np.testing.assert_allclose(one.out()[2], S2[2], rtol=1e-10, atol=0)
    # sets over nothing have count 0: N envs fill ceil(N / 64) workgroups
    cnt = sets_a[:, 0].cpu().numpy()
    assert cnt.sum() == T * N and (cnt[(N + 63) // 64:] == 0).all()
    # all sets empty: statistics and table of stats_in pass through
    emp = _VN((5.0, 2.0, 3.0))
    emp.merge(torch.zeros((4, 3), dtype=torch.float64, device=DEV))
    assert emp.out() == (5.0, 2.0, 3.0)
    np.testing.assert_array_equal(emp.table_out.cpu().numpy(), R.table((5.0, 2.0, 3.0)))


def test_scan_form_moments():
    T, N = 4096, 16
    x = R.hard_rewards("a", T, N, seed=5)
    zeros = np.zeros((T, N), np.float32)
    st = _VN()
    tg, _ = st.gae(x, zeros, zeros, np.ones(N, np.float32), 4)
    assert np.array_equal(tg, x)
    st.merge()
    _assert_stats(st.out(), R.moments(x))


@pytest.mark.parametrize("n", [655360, 1001, 7])
def test_apply_is_torch_bit_for_bit(n):
    st = _VN((10.0, 123.456, 789.0))
    x = torch.randn(n + 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) * 300
    x[0], x[n // 2], x[n - 1] = float("nan"), float("inf"), -1e30
    for off in (0, 1):                                       # 16-byte aligned and not
        tg = x[off:off + n]
        raw = tg.clone()
        out = torch.full((n + 8,), -7.0, device=DEV)
        st._lib.check(st.lib.ppo_value_norm_apply(_p(tg), n, _p(st.table), _p(out[4:]), None), "ppo_value_norm_apply")
        torch.cuda.synchronize()
        want = (tg - st.table[0]) * st.table[2]
        got = out[4:4 + n]
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
        assert torch.equal(torch.nan_to_num(tg), torch.nan_to_num(raw))            # the raw buffer is untouched
        assert (out[:4] == -7.0).all() and (out[4 + n:] == -7.0).all()              # and nothing beyond n is written


def _run(agent, steps):
    for _ in range(steps):
        agent.run()


def _stats_of(agent):
    return float(agent.value_count), float(agent.value_mean), float(agent.value_var)


@pytest.mark.parametrize("n,persistent", [(4096, True), (4096, False), (8192, True), (8192, False)])
def test_make_data_and_update_in_ppo(n, persistent):
    """One iteration: make_data is idempotent and commits nothing; update() commits exactly the moments of the raw targets; the
    targets handed to the update are the raw ones under the scratch table; the advantages are the float32 reference's from the
    value ring, the rewards and the table that was committed when make_data ran."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    seen = {}
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(n, persistent_rollout=persistent, normalize_value=True))
        assert agent.persistent_rollout == persistent
        T = agent.rollout_size
        agent._value_stats.copy_(torch.tensor([1000.0, 3.0, 50.0], dtype=torch.float64))      # a committed table that is not
        agent._value_table.copy_(cuda(R.table((1000.0, 3.0, 50.0))))                          # the identity
        real_update = agent.update

        def checked_update():
            first = [t.clone() for t in agent.make_data()]
            second = [t.clone() for t in agent.make_data()]
            for a, b in zip(first, second):
                assert torch.equal(a, b)
            assert _stats_of(agent) == (1000.0, 3.0, 50.0)                         # make_data never commits
            seen["table"] = agent._value_table.cpu().numpy().copy()
            seen["targets"] = first[3]
            real_update()

        agent.update = checked_update
        _run(agent, T)
        agent.flush_log()
    torch.cuda.synchronize()
    assert agent.optim_step == 75
    raw = agent._target.cpu().numpy()[..., 0]
    want = R.merge((1000.0, 3.0, 50.0), raw)
    _assert_stats(_stats_of(agent), want)
    assert float(agent.value_count) == 1000.0 + T * n
    np.testing.assert_array_equal(agent._value_table.cpu().numpy(), R.table(_stats_of(agent)))
    # the targets the update saw: raw ones under the scratch table (= the committed one now)
    np.testing.assert_array_equal(agent._target_norm.cpu().numpy()[..., 0], R.normalize(raw, agent._value_table.cpu().numpy()))
    assert torch.equal(seen["targets"], agent._target_norm)
    # advantages and raw targets: the float32 reference on the value ring under the table committed at make_data time
    v = agent._v_ring.cpu().numpy()[..., 0]
    done = agent.all_done.to(torch.float32).cpu().numpy().reshape(-1)
    t2, a2 = R.td_gae(agent.all_reward.cpu().numpy()[..., 0], v[:T], v[1:], done, seen["table"], mode=0)
    assert np.array_equal(raw, t2) and np.array_equal(agent.all_advantage.cpu().numpy()[..., 0], a2)
    # denormalize_value is that map
    x = torch.randn(100, device=DEV)
    np.testing.assert_array_equal(agent.denormalize_value(x).cpu().numpy(),
                                  R.denormalize(x.cpu().numpy(), agent._value_table.cpu().numpy()))
    agent.exit()


def test_first_update_commits_the_batch_moments():
    """From the initial S_v (0 | 0 | 1): after update(), count == T N and mean / var are the float64 moments of the raw targets."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096, normalize_value=True))
        T = agent.rollout_size
        assert _stats_of(agent) == (0.0, 0.0, 1.0)
        _run(agent, T - 1)
        torch.cuda.synchronize()
        assert float(agent.value_count) == 0
        agent.run()
        agent.flush_log()
    torch.cuda.synchronize()
    assert float(agent.value_count) == T * 4096
    _assert_stats(_stats_of(agent), R.moments(agent._target.cpu().numpy()))
    agent.exit()


def test_checkpoint_and_testing(tmp_path):
    """Save -> load -> continue: the statistics come back bit-equal and go on counting; --testing over three rollouts leaves
    them untouched; the file does not load without the flag."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096, normalize_value=True, save=True, save_path=str(tmp_path / "ck_"), save_freq=75))
        T = agent.rollout_size
        _run(agent, T)
        agent.flush_log()
    saved = agent._value_stats.clone()
    agent.exit()
    path = str(tmp_path / "ck_75.pth")
    sd = torch.load(path, weights_only=True)
    assert sd["value_rms.mean"].dtype == torch.float64 and float(sd["value_rms.count"]) == T * 4096
    assert not any(k.startswith("obs_rms.") for k in sd)
    with contextlib.redirect_stdout(io.StringIO()):
        t = PPO(make_args(4096, normalize_value=True, load=True, load_path=path, testing=True))
        assert torch.equal(t._value_stats, saved)
        table = t._value_table.clone()
        np.testing.assert_array_equal(table.cpu().numpy(), R.table(tuple(saved.cpu().numpy())))
        _run(t, 3 * T + 3)
    torch.cuda.synchronize()
    assert torch.equal(t._value_stats, saved) and torch.equal(t._value_table, table)
    t.exit()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        c = PPO(make_args(4096, normalize_value=True, load=True, load_path=path))
        assert torch.equal(c._value_stats, saved)
        _run(c, T)
        c.flush_log()
    torch.cuda.synchronize()
    assert float(c.value_count) == 2 * T * 4096 and "holds no value statistics" not in buf.getvalue()
    c.exit()
    with pytest.raises(ValueError, match="--normalize_value"):
        with contextlib.redirect_stdout(io.StringIO()):
            PPO(make_args(4096, load=True, load_path=path, testing=True))
    # a checkpoint without the statistics under the flag: one printed line, initial S_v
    plain = {k: v for k, v in sd.items() if not k.startswith("value_rms.")}
    torch.save(plain, str(tmp_path / "plain.pth"))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        p = PPO(make_args(4096, normalize_value=True, load=True, load_path=str(tmp_path / "plain.pth"), testing=True))
    assert _stats_of(p) == (0.0, 0.0, 1.0)
    assert sum("holds no value statistics" in ln for ln in buf.getvalue().splitlines()) == 1
    p.exit()


def test_flag_off_is_todays_path(tmp_path, monkeypatch):
    """normalize_value=False never reaches the new entry points, allocates none of the new buffers and saves no value_rms.*."""
    from fly_bproject_amd import _lib
    from fly_bproject_amd.ppo import PPO

    def refuse(*a):
        raise AssertionError("a value-normalisation entry point was called with the flag off")

    lib = _lib.load()
    for name in ("ppo_td_gae_vnorm", "ppo_value_norm_merge", "ppo_value_norm_apply"):
        monkeypatch.setattr(lib, name, refuse)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096, save=True, save_path=str(tmp_path / "ck_"), save_freq=75))
        _run(agent, agent.rollout_size)
        agent.flush_log()
    assert agent.optim_step == 75 and agent.normalize_value is False
    assert agent.value_mean is None and agent.value_var is None and agent.value_count is None
    for name in ("_value_stats", "_value_table", "_value_sets", "_target_norm", "_value_stats_next", "_value_table_next"):
        assert not hasattr(agent, name), name
    x = torch.randn(4, device=DEV)
    assert agent.denormalize_value(x) is x
    assert agent.make_data()[3] is agent._target
    agent.exit()
    sd = torch.load(str(tmp_path / "ck_75.pth"), weights_only=True)
    assert not any(k.startswith("value_rms.") for k in sd)


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "f32"])
def test_update_agrees_with_torch_backend(gemm):
    """One update with value normalisation on, through the HIP kernels in each arithmetic, against update_backend="torch" on
    the same rollout: the construction and bounds of tests/test_obs_norm_gpu.py::test_update_agrees_with_torch_backend."""
    from fly_bproject_amd.ppo import PPO
    outs, init, fn, refused = {}, None, {}, 0
    for backend in ("hip", "torch"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(4096, update_backend=backend, normalize_value=True))
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
        outs[backend + "_S"] = agent._value_stats.clone()
        agent.exit()
    print("gemm %s: h2_overflows (updates with a refused fp16x2 step) with normalize_value: %d" % (gemm, refused))
    assert torch.equal(outs["hip_S"], outs["torch_S"])              # same rollout, same statistics
    assert float(outs["hip_S"][0]) == 160 * 4096
    for k in init:
        moved = float((outs["torch"][k] - init[k]).norm())
        apart = float((outs["hip"][k] - outs["torch"][k]).norm())
        print("  %-20s moved %.4g apart %.4g" % (k, moved, apart))
        assert moved > 0 and apart <= 0.3 * moved, (k, apart, moved)
    moved = float((fn["torch"] - fn["init"]).norm())
    apart = float((fn["hip"] - fn["torch"]).norm())
    print("  probe outputs: moved %.4g apart %.4g" % (moved, apart))
    assert apart <= 0.2 * moved, (apart, moved)


def test_trainer_end_to_end(tmp_path):
    """trainer.py --normalize_value trains two rollouts and saves; the checkpoint holds the three keys."""
    ck = str(tmp_path / "ck_")
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "trainer.py"), "--num_envs", "4096", "--headless", "True",
                        "--normalize_value", "--max_steps", "330", "--save_path", ck, "--save_freq", "75"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Steps: 0300" in r.stdout and "Training" in r.stdout
    sd = torch.load(ck + "150.pth", weights_only=True)
    assert float(sd["value_rms.count"]) == 2 * 160 * 4096
    assert sd["value_rms.mean"].dtype == torch.float64 and float(sd["value_rms.var"]) > 0
