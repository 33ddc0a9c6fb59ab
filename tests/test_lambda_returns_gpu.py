"""GPU (-m gpu): lambda-return critic targets (PPO lambda_returns) -- the kernel against the float32
reference bit for bit (vector path, scalar path, tails, a second grid-stride sweep, NaN / inf), its moment sets against float64
numpy, the make_data flow in PPO for both estimators with and without value normalisation, the flag-off path against today's
TD target, one update against the torch backend, and trainer.main end to end."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests import value_norm_ref as VN
from tests import value_target_ref as R
from tests.hip_helpers import cuda, make_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 262144 + 5]
TABLE = VN.table((1000.0, 37.5, 44444.0))            # mean 37.5, std ~ 211


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _lib():
    from fly_bproject_amd import _lib as L
    return L, L.load()


def _launch(adv, v, tab, out, sets):
    L, lib = _lib()
    L.check(lib.ppo_lambda_targets(_p(adv), _p(v), _p(tab), adv.numel(), _p(out), _p(sets), None), "ppo_lambda_targets")
    torch.cuda.synchronize()


def _inputs(n, seed):
    """Advantages of unit scale around 1e3 (moments that break naive sums) and critic outputs of unit scale."""
    rng = np.random.default_rng(seed)
    adv = (1e3 + rng.standard_normal(n)).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    return adv, v


def _new_sets():
    L, _ = _lib()
    return torch.full((L.VALUE_NORM_SETS, L.VALUE_NORM_SET), -7.0, dtype=torch.float64, device=DEV)


@pytest.fixture(scope="module")
def cases():
    """One launch per (n, table) with moment sets: (adv, v, reference targets, kernel targets, kernel sets), shared."""
    out = {}
    for n in SIZES:
        for tab in (None, TABLE):
            adv, v = _inputs(n, n)
            got, sets = torch.full((n + 8,), -7.0, device=DEV), _new_sets()
            _launch(cuda(adv), cuda(v), None if tab is None else cuda(tab), got[4:4 + n], sets)
            out[n, tab is not None] = (adv, v, R.lambda_targets(adv, v, tab), got.cpu().numpy(), sets.cpu().numpy())
    return out


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_targets_equal_the_float32_reference(cases, n, with_table):
    _, _, want, got, _ = cases[n, with_table]
    assert np.array_equal(got[4:4 + n], want)
    assert (got[:4] == -7.0).all() and (got[4 + n:] == -7.0).all()               # nothing outside [0, n) is written


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_moment_sets_equal_float64(cases, n, with_table):
    """The sets combined in order against the float64 moments of the reference targets, at the bounds
    tests/test_value_norm_gpu.py holds this set format to."""
    _, _, want, _, sets = cases[n, with_table]
    cnt, mean, m2 = R.combine(sets)
    wn, wmean, wm2 = R.moments(want)
    print("n %d table %s: count %r mean %.17g (want %.17g) M2 %.17g (want %.17g)" % (n, with_table, cnt, mean, wmean, m2, wm2))
    assert cnt == wn == n and sets[:, 0].sum() == n
    assert (sets[:, 0] >= 0).all() and (sets[:, 2] >= 0).all()
    np.testing.assert_allclose(mean, wmean, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(m2, wm2, rtol=1e-10, atol=0)
    if n == 1:
        assert sets[0, 0] == 1 and (sets[1:, 0] == 0).all()                       # sets over nothing have count 0


def test_scalar_path_is_the_vector_path(cases):
    """All three pointers one element off a 16-byte boundary: the scalar path, same results and same moments to the bounds."""
    for n in (5, 1023, 262144 + 5):
        adv, v, want, _, sets_vec = cases[n, True]
        a, x = cuda(np.concatenate([[0], adv]).astype(np.float32)), cuda(np.concatenate([[0], v]).astype(np.float32))
        got, sets = torch.full((n + 9,), -7.0, device=DEV), _new_sets()
        assert a[1:].data_ptr() % 16 == 4 and x[1:].data_ptr() % 16 == 4 and got[5:].data_ptr() % 16 == 4
        _launch(a[1:], x[1:], cuda(TABLE), got[5:5 + n], sets)
        g = got.cpu().numpy()
        assert np.array_equal(g[5:5 + n], want) and (g[:5] == -7.0).all() and (g[5 + n:] == -7.0).all()
        cnt, mean, m2 = R.combine(sets.cpu().numpy())
        wn, wmean, wm2 = R.moments(want)
        assert cnt == wn
        np.testing.assert_allclose(mean, wmean, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(m2, wm2, rtol=1e-10, atol=0)
    # one misaligned pointer is enough to leave the vector path
    adv, v, want, _, _ = cases[1023, False]
    x = cuda(np.concatenate([[0], v]).astype(np.float32))
    got = torch.empty(1023, device=DEV)
    _launch(cuda(adv), x[1:], None, got, None)
    assert np.array_equal(got.cpu().numpy(), want)


def test_nan_and_infinities_pass_through():
    n = 1030
    adv, v = _inputs(n, 7)
    adv[[0, 5, 1029]] = np.nan, np.inf, -np.inf
    v[[3, 5, 600, 1028]] = np.nan, -np.inf, np.inf, -0.0
    adv[1028] = -0.0
    for tab in (None, TABLE):
        want = R.lambda_targets(adv, v, tab)
        assert np.isnan(want[[0, 3, 5]]).all() and want[600] == np.inf and want[1029] == -np.inf
        got = torch.empty(n, device=DEV)
        _launch(cuda(adv), cuda(v), None if tab is None else cuda(tab), got, None)
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert np.array_equal(g[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))     # signs of zero too
    assert np.signbit(R.lambda_targets(adv, v, None)[1028])                      # -0 + -0: no table, no "+ 0" on the way


def test_sets_are_deterministic_optional_and_empty_at_zero():
    n = 100003
    adv, v = _inputs(n, 11)
    a, x, t = cuda(adv), cuda(v), cuda(TABLE)
    out1, out2, s1, s2 = torch.empty(n, device=DEV), torch.empty(n, device=DEV), _new_sets(), _new_sets()
    _launch(a, x, t, out1, s1)
    _launch(a, x, t, out2, s2)
    assert torch.equal(s1, s2) and torch.equal(out1, out2)                        # two launches: bit-identical
    # sets = NULL writes no set (and the same targets)
    out3 = torch.empty(n, device=DEV)
    _launch(a, x, t, out3, None)
    assert torch.equal(out3, out1)
    # n == 0 is a no-op that still writes empty sets
    s0, keep = _new_sets(), out1.clone()
    L, lib = _lib()
    L.check(lib.ppo_lambda_targets(_p(a), _p(x), _p(t), 0, _p(out1), _p(s0), None), "ppo_lambda_targets")
    torch.cuda.synchronize()
    assert (s0 == 0).all() and torch.equal(out1, keep)


# ---- in PPO --------------------------------------------------------------------------------------------------------------------
COMMITTED = (1000.0, 3.0, 50.0)


def _rollout_with_make_data(n, persistent, seen, **kw):
    """One rollout of a new agent; update() is replaced by two make_data calls on the finished rollout, the second with
    normalize_advantage switched on, and clones of everything they leave go into `seen` (no optimizer step).  The ring and the
    value rows are as make_data saw them only inside the update: run() moves row T of the ring to row 0 right after it."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(n, persistent_rollout=persistent, **kw))
        assert agent.persistent_rollout == persistent
        if agent.normalize_value:
            agent._value_stats.copy_(torch.tensor(COMMITTED, dtype=torch.float64))      # a committed table that is not the identity
            agent._value_table.copy_(cuda(VN.table(COMMITTED)))
        names = ("_target", "all_advantage", "_v_ring") + (("_target_norm", "_value_stats", "_value_table", "_value_stats_next",
                                                             "_value_table_next") if agent.normalize_value else ())

        def recording_update():
            seen["data"] = [t.clone() for t in agent.make_data()]
            seen.update({k: getattr(agent, k).clone() for k in names})
            agent.normalize_advantage = True
            seen["data_adv_norm"] = [t.clone() for t in agent.make_data()]
            seen.update({k + "_adv_norm": getattr(agent, k).clone() for k in names})
            agent.normalize_advantage = False

        agent.update = recording_update
        for _ in range(agent.rollout_size):
            agent.run()
        agent.flush_log()
    torch.cuda.synchronize()
    return agent


def _td_target(agent):
    """Today's TD target by a direct ppo_td_gae call on the agent's own rewards, values and done mask (reference estimator)."""
    L, lib = _lib()
    T, n = agent.rollout_size, int(agent.args.num_envs)
    done = agent.all_done.to(torch.float32).contiguous()
    tg, adv = torch.empty(T, n, 1, device=DEV), torch.empty(T, n, 1, device=DEV)
    L.check(lib.ppo_td_gae(_p(agent.all_reward), _p(agent._v_ring[:T]), _p(agent._v_ring[1:]), _p(done), C.c_float(agent.gamma),
                           C.c_float(agent.lmbda), T, n, _p(tg), _p(adv), 0, None), "ppo_td_gae")
    torch.cuda.synchronize()
    return tg, adv


@pytest.mark.parametrize("normalize_value", [False, True], ids=["plain", "vnorm"])
@pytest.mark.parametrize("gae", ["reference", "episodic"])
@pytest.mark.parametrize("n,persistent", [(4096, True), (4096, False), (8192, True), (8192, False)])
def test_make_data_in_ppo(n, persistent, gae, normalize_value):
    """_target is the reference applied to the agent's own raw advantages and critic outputs, bit for bit; with value
    normalisation the scratch statistics and table are those of the lambda targets and _target_norm is their normalisation under
    the scratch table; nothing committed moves; normalize_advantage changes the advantages and not the targets."""
    seen = {}
    agent = _rollout_with_make_data(n, persistent, seen, gae=gae, normalize_value=normalize_value, lambda_returns=True)
    assert agent.lambda_returns is True
    T = agent.rollout_size
    adv = seen["all_advantage"].cpu().numpy()[..., 0]                             # raw: read before any normalisation
    v = seen["_v_ring"].cpu().numpy()[:T, :, 0]
    tab = seen["_value_table"].cpu().numpy() if normalize_value else None
    want = R.lambda_targets(adv, v, tab)
    raw = seen["_target"].cpu().numpy()[..., 0]
    vd = VN.denormalize(v, tab) if normalize_value else v
    assert np.array_equal(raw, want)
    assert np.abs(adv).max() > 0 and not np.array_equal(raw, vd)
    assert torch.equal(seen["data"][4], seen["all_advantage"])
    if gae == "episodic":
        stale = torch.cat([agent._ended_prev.reshape(1, -1), agent._reset_rows[:-1]]).cpu().numpy() != 0
        assert stale.any() and (adv[stale] == 0).all() and np.array_equal(raw[stale], vd[stale])
    if normalize_value:
        assert tuple(seen["_value_stats"].cpu().numpy()) == COMMITTED             # make_data never commits
        np.testing.assert_array_equal(tab, VN.table(COMMITTED))
        got = tuple(float(x) for x in seen["_value_stats_next"].cpu().numpy())
        wc, wmean, wvar = VN.merge(COMMITTED, raw)
        print("scratch statistics %r, float64 merge of the lambda targets %r" % (got, (wc, wmean, wvar)))
        assert got[0] == wc == COMMITTED[0] + T * n
        np.testing.assert_allclose(got[1], wmean, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(got[2], wvar, rtol=1e-10, atol=0)
        table_next = seen["_value_table_next"].cpu().numpy()
        np.testing.assert_array_equal(table_next, VN.table(got))
        np.testing.assert_array_equal(seen["_target_norm"].cpu().numpy()[..., 0], VN.normalize(raw, table_next))
        assert torch.equal(seen["data"][3], seen["_target_norm"])
    else:
        assert torch.equal(seen["data"][3], seen["_target"])
    # the same rollout with normalize_advantage on: other advantages (mean 0, std 1 to the noise of a float32 reduction), and
    # everything about the targets bit for bit as before
    normed = seen["all_advantage_adv_norm"]
    assert not torch.equal(normed, seen["all_advantage"]) and torch.equal(seen["data_adv_norm"][4], normed)
    assert abs(float(normed.double().mean())) < 1e-3 and abs(float(normed.double().std()) - 1) < 1e-3
    for k in seen:
        if k.endswith("_adv_norm") and k not in ("all_advantage_adv_norm", "data_adv_norm"):
            assert torch.equal(seen[k], seen[k[:-len("_adv_norm")]]), k
    assert torch.equal(seen["data_adv_norm"][3], seen["data"][3])
    agent.exit()


def test_flag_off_is_todays_td_target(monkeypatch):
    """Without the flag the new entry point is never reached and _target is ppo_td_gae's target on the same inputs."""
    L, lib = _lib()

    def refuse(*a):
        raise AssertionError("ppo_lambda_targets was called with the flag off")

    monkeypatch.setattr(lib, "ppo_lambda_targets", refuse)
    seen = {}
    agent = _rollout_with_make_data(4096, True, seen)
    assert agent.lambda_returns is False
    tg, adv = _td_target(agent)
    assert torch.equal(seen["data"][3], tg) and torch.equal(seen["_target"], tg) and torch.equal(seen["all_advantage"], adv)
    agent.exit()
    # and with the flag on, the same rollout has other targets and the same advantages
    monkeypatch.undo()
    seen_on = {}
    on = _rollout_with_make_data(4096, True, seen_on, lambda_returns=True)
    assert torch.equal(seen_on["all_advantage"], adv) and not torch.equal(seen_on["_target"], tg)
    on.exit()


def test_update_agrees_with_torch_backend():
    """One update on lambda targets with value normalisation on, through the HIP kernels against update_backend="torch" on the
    same rollout: the construction and bounds of tests/test_value_norm_gpu.py::test_update_agrees_with_torch_backend."""
    from fly_bproject_amd.ppo import PPO
    outs, init, fn = {}, None, {}
    for backend in ("hip", "torch"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(4096, update_backend=backend, normalize_value=True, lambda_returns=True))
            init = {k: v.clone() for k, v in agent.net.state_dict().items()}
            with torch.no_grad():
                probe = torch.randn(512, 73, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
                fn["init"] = torch.cat([agent.net.pi(probe), agent.net.v(probe)], dim=1)
            for _ in range(agent.rollout_size):
                agent.run()
            with torch.no_grad():
                fn[backend] = torch.cat([agent.net.pi(probe), agent.net.v(probe)], dim=1)
        assert agent.optim_step == 75
        outs[backend] = {k: v.clone() for k, v in agent.net.state_dict().items()}
        outs[backend + "_S"] = agent._value_stats.clone()
        outs[backend + "_target"] = agent._target.clone()
        agent.exit()
    assert torch.equal(outs["hip_S"], outs["torch_S"]) and torch.equal(outs["hip_target"], outs["torch_target"])
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


def test_trainer_end_to_end(capsys):
    """trainer.main --lambda_returns over one rollout and its update."""
    import trainer
    policy = trainer.main(["--num_envs", "4096", "--headless", "True", "--lambda_returns", "--max_steps", "160"])
    out = capsys.readouterr().out
    assert "rollout_size:  160" in out and "Training" in out
    assert policy.lambda_returns is True and policy.optim_step == 75 and policy.run_step == 160
    assert torch.isfinite(policy._target).all() and torch.isfinite(policy.policy.P).all()
