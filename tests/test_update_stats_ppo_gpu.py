"""GPU (-m gpu): the update diagnostics in the agent (PPO update_stats), 2048 envs (T = 320, 655 360 rows):
`last` against the reference applied to the agent's own tensors and the probe's own mu and v, under the defaults, with every
opt-in on together and with the torch update backend; the probe's forward against net.pi / net.v; the score line's suffix, its
window and the blocking log route; the flag-off path; and weights, Adam moments and rollout tensors bit-identical with the flag
on and off."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

from tests import update_stats_ref as R
from tests.hip_helpers import make_args
from tests.test_resume_gpu import _differences, _snapshot
from tests.test_update_stats_gpu import _check_against_reference

pytestmark = pytest.mark.gpu
N = 2048
T = 320
SUFFIX = re.compile(r" \| KL (?:n/a|(\S+) \| Clip (\S+)% \| EV (\S+) \| Loss (\S+)(?: \| Nonfinite (\d+))?)$")
ALL_OPT_INS = dict(normalize_obs=True, normalize_value=True, normalize_reward=True, lambda_returns=True, gae="episodic",
                   minibatch="shuffled", normalize_advantage=True)


def _run(iterations, **kw):
    """A new agent under seed 0, `iterations` rollouts with their updates.  Per iteration: the snapshot tests/test_resume_gpu.py
    compares runs in, stdout, and with the flag on what the probe read and wrote."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(N, **kw))
    assert agent.rollout_size == T
    seen = []
    for _ in range(iterations):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            for _ in range(T):
                agent.run()
            agent.flush_log()
        s = {"snapshot": _snapshot(agent), "stdout": out.getvalue(), "public": agent.update_stats()}
        if agent.update_stats() is not None:
            obs = agent._obs_norm_ring[:T] if agent.normalize_obs else agent.all_obs
            target = agent._target_norm if agent.normalize_value else agent._target
            with torch.no_grad():                                      # (the packed policy's forward, as make_data calls it)
                pi, net_v = agent.net.pi(obs).clone(), agent.net.v(obs).clone()
            s.update(target=target.clone(), mu=agent._us_mu.clone(), v=agent._us_v.clone(), pi=pi, net_v=net_v,
                     var=agent._action_var.clone(),
                     **{k: getattr(agent, "_us_" + k).cpu().numpy().copy() for k in ("last", "window", "total", "sets")})
        seen.append(s)
    return agent, seen


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, iterations, kw in (("default", 3, {}), ("all", 2, ALL_OPT_INS), ("torch", 2, dict(update_backend="torch")),
                                 ("blocking", 2, dict(async_log=False))):
        agent, seen = _run(iterations, update_stats=True, **kw)
        out[name] = seen
        agent.exit()
    return out


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name", ["default", "all", "torch"])
def test_last_is_the_reference_on_the_agents_own_tensors(runs, name):
    s = runs[name][1]                                                  # after two iterations
    snap = s["snapshot"]
    mu, v = _np(s["mu"]).reshape(-1, 18), _np(s["v"]).reshape(-1)
    assert mu.shape[0] == T * N == v.shape[0]
    acts, logp, adv = _np(snap["all_acts"]).reshape(-1, 18), _np(snap["all_log_prob"]).reshape(-1), _np(snap["all_advantage"]).reshape(-1)
    target = _np(s["target"]).reshape(-1)
    t = R.row_terms(mu, acts, logp, adv, v, target, _np(s["var"]), 0.2)
    want = R.set_from_terms(t, adv, v, target)
    with np.errstate(invalid="ignore"):
        near = int((t.finite & ((np.abs(t.ratio - t.lo) <= t.rb) | (np.abs(t.ratio - t.hi) <= t.rb))).sum())
    print("update_stats in the agent (%s): %d of %d rows within their margin of a clip edge" % (name, near, T * N))
    assert near < T * N // 100                                         # few: the margin is rounding
    _check_against_reference(s["last"], t, want, "agent, " + name, near=near)
    assert s["last"][R.ROWS] == T * N and s["last"][R.NONFINITE] == 0
    # the sets the launch left fold to `last`, and `total` holds both updates
    assert np.array_equal(R.merge_all(s["sets"])[list(R.EXACT)], s["last"][list(R.EXACT)])
    assert s["total"][R.ROWS] == 2 * T * N
    pub = s["public"]["last"]
    assert pub["approx_kl"] > 0 and pub["ratio_min"] < pub["ratio_max"] and pub["rows"] == T * N and pub["nonfinite"] == 0
    assert pub["approx_kl"] == s["last"][R.K3] / (T * N) and pub["clip_fraction"] == s["last"][R.CLIPPED] / (T * N)
    assert pub["explained_variance"] == 1.0 - s["last"][R.EM2] / s["last"][R.TM2] and pub["explained_variance"] < 1
    assert pub["loss"] == s["last"][R.POL] / (T * N) + s["last"][R.HUB] / (T * N)
    if name == "all":
        assert abs(pub["target_mean"]) < 1.0 and 0.2 < pub["target_std"] < 5.0       # normalised targets: the units of _target_norm


@pytest.mark.parametrize("name", ["default", "all", "torch"])
def test_the_probes_forward_is_the_networks(runs, name):
    """mu and v of the probe against net.pi(obs) and net.v(obs) of the updated network, bit for bit.  Row 0 of the raw ring is
    the next rollout's first observation by then (ring[0] <- ring[T] at the rollout boundary), so the comparison starts at row 1
    where the update read the raw ring."""
    s = runs[name][1]
    lo = 0 if name == "all" else 1
    assert torch.equal(s["mu"][lo:], s["pi"][lo:]) and torch.equal(s["v"][lo:], s["net_v"][lo:])
    assert s["mu"].shape == (T, N, 18) and s["v"].shape == (T, N, 1)


def _score(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("Steps:")]
    found = [SUFFIX.search(ln) for ln in lines]
    assert lines and all(found), lines
    return lines, found


def test_score_line_suffix_window_and_the_blocking_route(runs):
    from fly_bproject_amd import ppo
    seen = runs["default"]
    lines, found = _score(seen[0]["stdout"])
    assert len(lines) == 4 and all(m.group(0) == " | KL n/a" for m in found)          # steps 0 .. 300: before the first update
    for k in (1, 2):
        lines, found = _score(seen[k]["stdout"])
        # the first line behind update k carries it, alone in its window: the text is the suffix of that update's `last`
        assert found[0].group(0) == ppo.update_stats_suffix(seen[k - 1]["last"].tolist()) != " | KL n/a"
        assert float(found[0].group(1)) > 0 and found[0].group(5) is None
        assert all(m.group(0) == " | KL n/a" for m in found[1:]) and len(found) >= 3   # the window was reset behind the line
        # at the end of iteration k the window holds that iteration's update alone
        assert np.array_equal(seen[k]["window"], seen[k]["last"]) and seen[k]["public"]["window"] == seen[k]["public"]["last"]
    assert seen[2]["total"][R.ROWS] == 3 * T * N
    # async_log=False reads the window with a blocking copy: the same text, line for line
    for k in (0, 1):
        assert runs["blocking"][k]["stdout"] == seen[k]["stdout"]
        assert np.array_equal(runs["blocking"][k]["total"], seen[k]["total"])


def test_the_feature_observes_and_does_not_steer(runs, monkeypatch, tmp_path):
    """Three iterations under the same seed with the flag off: weights, Adam moments, rollout tensors, h2_overflows and
    optim_step bit for bit those of the run with the flag on.  With the flag off the two entry points are never called,
    nothing is allocated, stdout has no suffix and a saved state holds no block."""
    from fly_bproject_amd import _lib

    def refuse(*a):
        raise AssertionError("an update-statistics entry point was called with the flag off")

    us = _lib.update_stats_api()
    monkeypatch.setattr(us, "ppo_update_stats", refuse)
    monkeypatch.setattr(us, "ppo_update_stats_merge", refuse)
    agent, off = _run(3)
    on = runs["default"]
    for k in range(3):
        assert _differences(on[k]["snapshot"], off[k]["snapshot"]) == [], k
        assert on[k]["snapshot"]["optim_step"] == 75 * (k + 1) and "h2_overflows" in on[k]["snapshot"]
        strip = [SUFFIX.sub("", ln) for ln in on[k]["stdout"].splitlines()]
        assert strip == off[k]["stdout"].splitlines() and " | KL" not in off[k]["stdout"]
        assert off[k]["public"] is None
    assert agent.update_stats() is None and not any(k.startswith("_us_") for k in vars(agent))
    path = str(tmp_path / "off.state.pth")
    agent.save_training_state(path)
    state = torch.load(path, weights_only=True)
    assert "update_stats" not in state["agent"] and "update_stats" not in state["meta"] and "update_stats" not in state["meta_ext"]
    agent.exit()


def test_trainer_end_to_end_and_in_testing(capsys):
    import trainer
    policy = trainer.main(["--num_envs", "4096", "--headless", "True", "--update_stats", "--max_steps", "320"])
    out = capsys.readouterr().out
    assert policy.optim_step == 150 and policy.run_step == 320
    assert " | KL n/a\n" in out and re.search(r" \| KL \d+\.\d{5} \| Clip \d+\.\d% \| EV \S+ \| Loss \S+\n", out)
    assert policy.update_stats()["total"]["rows"] == 2 * 160 * 4096
    policy = trainer.main(["--num_envs", "4096", "--headless", "True", "--update_stats", "--max_steps", "320", "--testing", "True"])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("Steps:")]
    assert policy.optim_step == 0 and lines and all(ln.endswith(" | KL n/a") for ln in lines)
    assert policy.update_stats()["total"]["rows"] == 0
