"""GPU (-m gpu): running reward scaling in the agent (PPO normalize_reward), 4096 envs (T = 160): make_data's
pass against the reference on the agent's own rows, its idempotency and the commit in update(), the two rollout forms, the
composition with the other opt-in estimators, the flag-off path, and trainer.py end to end."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import reward_norm_ref as R
from tests.hip_helpers import make_args

pytestmark = pytest.mark.gpu
N, T = 4096, 160
INITIAL = (0.0, 0.0, 1.0)
STATE = ("_rnorm_stats", "_rnorm_table", "_rnorm_carry")


def _agent(**kw):
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        return PPO(make_args(N, **kw))


def _rollout(agent, first=0):
    """run() from step `first` to the end of the rollout (with its update): -> the stdout."""
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        for _ in range(first, agent.rollout_size):
            agent.run()
        agent.flush_log()
    torch.cuda.synchronize()
    return out.getvalue()


def _rows(agent):
    return agent.all_reward.cpu().numpy()[..., 0].copy(), agent._reset_rows.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_stats(got, want):
    (c, mu, var), (wc, wmu, wvar) = got, want
    print("statistics: count %r (want %r)  mean %.17g (want %.17g)  var %.17g (want %.17g)" % (c, wc, mu, wmu, var, wvar))
    assert c == wc
    np.testing.assert_allclose(mu, wmu, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(var, wvar, rtol=1e-10, atol=0)


@pytest.fixture(scope="module")
def runs():
    """The flag-on agent: its first rollout on the device before any update (run() once: the one-launch rollout), what two
    make_data() calls return there, then two whole iterations; and a flag-off agent's first iteration on the same seed."""
    from fly_bproject_amd import _lib
    got = {}
    agent = _agent(normalize_reward=True)
    assert agent.persistent_rollout and agent.rollout_size == T and agent.reward_clip == 10.0
    head = io.StringIO()
    with contextlib.redirect_stdout(head):
        agent.run()
    torch.cuda.synchronize()
    before = {k: getattr(agent, k).clone() for k in STATE}
    have = agent._v_have                                            # (make_data ends the reuse of the rollout's critic outputs:
    first = [x.clone() for x in agent.make_data()]                  # put back below, so that the run goes on as any other)
    second = [x.clone() for x in agent.make_data()]
    agent._v_have = have
    torch.cuda.synchronize()
    got["idempotent"] = all(torch.equal(a, b) for a, b in zip(first, second))
    got["committed_untouched"] = all(torch.equal(before[k], getattr(agent, k)) for k in STATE)
    # the unchanged GAE entry point, called here on the agent's scaled buffer and the critic outputs it kept
    values, done_f = agent._keep
    tgt, adv = torch.empty_like(agent._target), torch.empty_like(agent.all_advantage)
    _lib.api().ppo_td_gae(agent._rnorm_scaled, values[:T], values[1:], done_f, agent.gamma, agent.lmbda, T, N, tgt, adv, 0,
                         _lib.stream_ptr())
    torch.cuda.synchronize()
    got["gae"] = (torch.equal(adv, agent.all_advantage), torch.equal(tgt, agent._target), torch.equal(first[4], adv))
    got["rows1"] = _rows(agent)
    got["scaled"] = agent._rnorm_scaled.cpu().numpy()[..., 0].copy()
    got["next"] = {k: getattr(agent, "_rnorm_" + k).cpu().numpy().copy() for k in ("stats_next", "table_next", "carry_next")}
    got["stdout1"] = head.getvalue() + _rollout(agent, first=1)
    got["after1"] = {k: getattr(agent, k).cpu().numpy().copy() for k in STATE}
    got["public1"] = (float(agent.reward_var), float(agent.reward_count), float(agent.reward_scale))
    _rollout(agent)
    got["rows2"] = _rows(agent)
    got["after2"] = {k: getattr(agent, k).cpu().numpy().copy() for k in STATE}
    got["count2"] = float(agent.reward_count)
    agent.exit()
    off = _agent()
    got["off_stdout1"] = _rollout(off)
    got["off_reward1"] = _rows(off)[0]
    off.exit()
    return got


def test_make_data_is_idempotent_and_reads_the_scaled_buffer(runs):
    assert runs["idempotent"] and runs["committed_untouched"]
    assert runs["gae"] == (True, True, True)                       # advantages and targets: the GAE entry point on the scaled buffer


def test_the_scaled_buffer_is_the_reference_on_the_agents_own_rows(runs):
    reward, reset = runs["rows1"]
    assert (reset != 0).any()
    w = R.walk(reward, reset, 0.99)
    nxt = runs["next"]
    assert np.array_equal(_bits(nxt["carry_next"]), _bits(w.carry))                     # lane = env form: bit for bit
    _assert_stats(tuple(nxt["stats_next"]), R.merge(INITIAL, w.G))
    assert np.array_equal(nxt["table_next"].view(np.uint32), R.table(tuple(nxt["stats_next"])).view(np.uint32))
    want = R.scale(reward, nxt["table_next"][2], 10.0)
    assert np.array_equal(runs["scaled"].view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(runs["scaled"], reward)                                    # (it does scale)


def test_raw_rewards_and_the_score_line_are_the_flag_off_runs(runs):
    assert np.array_equal(runs["rows1"][0].view(np.uint32), runs["off_reward1"].view(np.uint32))
    lines = [ln for ln in runs["stdout1"].splitlines() if ln.startswith("Steps:")]
    assert len(lines) == 2 and lines == [ln for ln in runs["off_stdout1"].splitlines() if ln.startswith("Steps:")]
    assert runs["stdout1"] == runs["off_stdout1"]                                        # nothing else is printed either


def test_update_commits_and_the_carries_run_on(runs):
    nxt, a1, a2 = runs["next"], runs["after1"], runs["after2"]
    assert np.array_equal(_bits(a1["_rnorm_stats"]), _bits(nxt["stats_next"]))
    assert np.array_equal(a1["_rnorm_table"].view(np.uint32), nxt["table_next"].view(np.uint32))
    assert np.array_equal(_bits(a1["_rnorm_carry"]), _bits(nxt["carry_next"]))
    var, count, scale = runs["public1"]
    assert (var, count) == (a1["_rnorm_stats"][2], float(T * N)) and np.float32(scale) == a1["_rnorm_table"][2]
    assert runs["count2"] == 2.0 * T * N == a2["_rnorm_stats"][0]
    w1 = R.walk(*runs["rows1"], 0.99)
    w2 = R.walk(*runs["rows2"], 0.99, w1.carry)
    assert np.array_equal(_bits(a2["_rnorm_carry"]), _bits(w2.carry))
    _assert_stats(tuple(a2["_rnorm_stats"]), R.moments(np.concatenate((w1.G, w2.G))))


def test_both_rollout_forms_give_the_same_statistics_and_carries(runs):
    agent = _agent(normalize_reward=True, persistent_rollout=False)
    assert not agent.persistent_rollout
    _rollout(agent)
    _rollout(agent)
    for k in STATE:
        got = getattr(agent, k).cpu().numpy()
        assert got.tobytes() == runs["after2"][k].tobytes(), k
    assert np.array_equal(agent._reset_rows.cpu().numpy(), runs["rows2"][1])
    agent.exit()


def test_composes_with_the_other_estimators():
    """--gae episodic --normalize_value --lambda_returns: one iteration, everything finite, and the value statistics are those
    of the targets the critic saw -- lambda-returns of SCALED rewards, so of unit scale where the raw ones are not."""
    agent = _agent(normalize_reward=True, gae="episodic", normalize_value=True, lambda_returns=True)
    _rollout(agent)
    for t in (agent.policy.P, agent.all_advantage, agent._target, agent._target_norm, agent._rnorm_scaled, agent._value_stats,
              agent._rnorm_stats):
        assert torch.isfinite(t).all()
    tg = agent._target.cpu().numpy().astype(np.float64)
    _assert_stats(tuple(agent._value_stats.cpu().numpy()), R.moments(tg))
    assert float(agent.reward_count) == T * N == float(agent.value_count)
    scaled, raw = agent._rnorm_scaled.cpu().numpy(), agent.all_reward.cpu().numpy()
    assert np.abs(scaled).max() <= 10.0 and np.array_equal(scaled, R.scale(raw, float(agent.reward_scale), 10.0))
    agent.exit()


def test_flag_off_allocates_launches_and_saves_nothing(monkeypatch, tmp_path):
    from fly_bproject_amd import _lib
    api, calls = _lib.ext(), []
    for name in ("ppo_reward_returns", "ppo_reward_scale"):
        monkeypatch.setattr(api, name, lambda *a, _n=name: calls.append(_n))
    path = str(tmp_path / "off_")
    agent = _agent(save=True, save_state=True, save_path=path)
    text = _rollout(agent)
    assert agent.optim_step == 75 and calls == []
    assert not any("_rnorm_" in k for k in vars(agent))     # no allocation
    assert agent.reward_var is None and agent.reward_count is None and agent.reward_scale is None
    assert "normalize_reward" not in text
    with contextlib.redirect_stdout(io.StringIO()):
        agent.save("x")
    sd = torch.load(path + "x.pth", weights_only=True)
    assert not any(k.startswith("reward_rms") for k in sd)
    state = torch.load(agent.training_state_path(path + "x.pth", 0), weights_only=True)
    assert "reward_norm" not in state["agent"] and state["meta_ext"] == {"lambda_returns": False}
    assert "normalize_reward" not in state["meta"] and "reward_clip" not in state["meta"]
    agent.exit()


def test_weights_file_carries_the_statistics(tmp_path, capsys):
    """Flag on: reward_rms.* go into the weights file, load back into the committed statistics, refuse to load without the
    flag; a file without them under the flag says so and starts from 0 | 0 | 1."""
    from fly_bproject_amd.ppo import PPO
    path = str(tmp_path / "on_")
    agent = _agent(normalize_reward=True, save=True, save_path=path)
    _rollout(agent)
    with contextlib.redirect_stdout(io.StringIO()):
        agent.save("x")
    stats = agent._rnorm_stats.cpu().numpy().copy()
    agent.exit()
    sd = torch.load(path + "x.pth", weights_only=True)
    assert [float(sd["reward_rms." + k]) for k in ("count", "mean", "var")] == stats.tolist() and stats[0] == T * N
    capsys.readouterr()
    loaded = PPO(make_args(N, normalize_reward=True, load=True, load_path=path + "x.pth"))
    assert loaded._rnorm_stats.cpu().numpy().tobytes() == stats.tobytes()
    assert np.array_equal(loaded._rnorm_table.cpu().numpy(), R.table(tuple(stats)))
    assert "holds no return statistics" not in capsys.readouterr().out
    loaded.exit()
    with pytest.raises(ValueError, match="run with --normalize_reward"):
        PPO(make_args(N, load=True, load_path=path + "x.pth"))
    torch.save({k: v for k, v in sd.items() if not k.startswith("reward_rms")}, path + "plain.pth")
    plain = PPO(make_args(N, normalize_reward=True, load=True, load_path=path + "plain.pth"))
    assert "normalize_reward: %s holds no return statistics (reward_rms.*); starting from mean 0, var 1" % (path + "plain.pth") \
        in capsys.readouterr().out
    assert plain._rnorm_stats.tolist() == [0.0, 0.0, 1.0]
    plain.exit()


def test_trainer_end_to_end_and_in_testing(monkeypatch, capsys):
    import trainer
    from fly_bproject_amd import _lib
    policy = trainer.main(["--num_envs", "4096", "--headless", "True", "--normalize_reward", "--max_steps", "320"])
    capsys.readouterr()
    assert policy.optim_step == 150 and policy.run_step == 320 and float(policy.reward_count) == 2 * T * N
    assert 0 < float(policy.reward_scale) and torch.isfinite(policy.policy.P).all()
    # --testing True has no update: nothing is launched
    api, calls = _lib.ext(), []
    for name in ("ppo_reward_returns", "ppo_reward_scale"):
        monkeypatch.setattr(api, name, lambda *a, _n=name: calls.append(_n))
    policy = trainer.main(["--num_envs", "4096", "--headless", "True", "--normalize_reward", "--reward_clip", "5", "--max_steps", "320",
                           "--testing", "True"])
    assert policy.optim_step == 0 and calls == [] and float(policy.reward_count) == 0.0 and policy.reward_clip == 5.0
