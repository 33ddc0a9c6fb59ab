"""GPU (-m gpu): exact resume (--save_state / --resume_path).  A run that is saved, stopped and resumed by a new
agent leaves bit for bit what the uninterrupted run leaves: every comparison here is torch.equal, or string equality for the
score lines.  Each continuation case is run A = 2 rollouts + updates, save, 2 more; run B = a new PPO that resumes from A's save
and makes 2 -- so the 150 + 150 optimizer steps cross a weight-rescale step of the fp16x2 planes (period 64) on both sides of
the save, value statistics are committed, observation statistics merged and the epoch keys advanced."""
import contextlib
import io
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPT_IN = dict(normalize_obs=True, normalize_value=True, normalize_advantage=True, gae="episodic", minibatch="shuffled",
              action_noise="ar1", randomize=True)
# name -> (num_envs, options, how A saves: "periodic" = run()'s own save at optim_step 150, "direct" = save() between two run()s)
CASES = {
    "a_defaults_8192": (8192, {}, "periodic"),                                      # T = 80, one launch per rollout, fp16x2 step
    "b_300_bf16x3": (300, dict(gemm="bf16x3"), "direct"),                           # T = 2176, a ragged last tile of 12 envs
    "c_all_opt_in_4096": (4096, OPT_IN, "periodic"),                                # T = 160, one launch per rollout
    "d_all_opt_in_4096_stepwise": (4096, dict(OPT_IN, persistent_rollout=False), "direct"),
}


def make_args(n, **kw):
    from tests.hip_helpers import make_args as make
    return make(n, **kw)


def _make(n, seed_net, **kw):
    """A PPO set up as trainer.main sets it up (the --gemm selection after the constructor)."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(seed_net)                             # the initial weights come from torch's global generator
    agent = PPO(make_args(n, **kw))
    if kw.get("gemm"):
        agent.policy.gemm = kw["gemm"]
    return agent


def _rollouts(agent, k):
    for _ in range(k * agent.rollout_size):
        agent.run()
    agent.flush_log()


def _score_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("Steps:")]


def _snapshot(agent):
    """Device clones of everything the continuation is compared in."""
    torch.cuda.synchronize()
    pol, env = agent.policy, agent.env
    s = {"P": pol.P, "exp_avg": pol.exp_avg, "exp_avg_sq": pol.exp_avg_sq, "step": pol.step, "h2_scales": pol.h2_scales,
         "action_var": agent.action_var, "all_obs": agent.all_obs, "all_acts": agent.all_acts, "all_log_prob": agent.all_log_prob,
         "all_reward": agent.all_reward, "all_advantage": agent.all_advantage, "target": agent._target,
         "root": env.root_tensor, "dof_states": env.dof_states, "potentials": env.potentials, "reset_buf": env.reset_buf,
         "progress_buf": env.progress_buf, "episode_return_buf": env.episode_return_buf,
         "episode_length_buf": env.episode_length_buf, "finished_return_sum": env.finished_return_sum,
         "finished_length_sum": env.finished_length_sum, "finished_count": env.finished_count}
    if agent.normalize_obs:
        s.update(obs_stats=agent._obs_stats, obs_table=agent._obs_table)
    if agent.normalize_value:
        s.update(value_stats=agent._value_stats, value_table=agent._value_table, value_stats_next=agent._value_stats_next,
                 value_table_next=agent._value_table_next, target_norm=agent._target_norm)
    if env.randomized:
        s["dr_table"] = env._dr_table
    s = {k: v.detach().clone() for k, v in s.items()}
    s.update(h2_overflows=pol.h2_overflows, h2_calibrated=pol.h2_calibrated, steps_issued=pol.steps_issued,
             optim_step=agent.optim_step, run_step=agent.run_step)
    return s


def _differences(a, b):
    assert list(a) == list(b)
    return [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]


def _same_state(a, b, where=""):
    """Names of the entries in which two loaded state dicts differ."""
    out = []
    assert list(a) == list(b), (where, list(a), list(b))
    for k in a:
        if isinstance(a[k], dict):
            out += _same_state(a[k], b[k], where + k + ".")
        elif torch.is_tensor(a[k]):
            if not (a[k].dtype == b[k].dtype and torch.equal(a[k], b[k])):
                out.append(where + k)
        elif a[k] != b[k]:
            out.append(where + k)
    return out


def _run_a(tmp, n, kw, how):
    """The uninterrupted run: 2 rollouts, save, 1 rollout (snapshot), 1 rollout (snapshot).  save_freq 150: run() saves by itself
    at optim_step 150 and 300; with how == "direct" the periodic saves are off and save() is called between two run() calls."""
    periodic = how == "periodic"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        agent = _make(n, 0, save=True, save_state=True, save_path=os.path.join(tmp, "a_"), save_freq=150 if periodic else 10 ** 9,
                      **kw)
        _rollouts(agent, 2)
        if not periodic:
            agent.save("150")
    weights = os.path.join(tmp, "a_150.pth")
    assert agent.optim_step == 150 and agent.run_step == 2 * agent.rollout_size
    assert os.path.isfile(weights) and os.path.isfile(agent.training_state_path(weights, 0))
    at_save = _snapshot(agent)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        _rollouts(agent, 1)
        after_3 = _snapshot(agent)
        _rollouts(agent, 1)
        if not periodic:
            agent.save("300")
    res = {"weights": weights, "at_save": at_save, "after_3": after_3, "after_4": _snapshot(agent),
           "lines": _score_lines(out.getvalue()), "dir": tmp, "T": agent.rollout_size}
    agent.exit()
    return res


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """Run A of case (a): shared by the continuation, the control, the refusals and off-is-off."""
    n, kw, how = CASES["a_defaults_8192"]
    return _run_a(str(tmp_path_factory.mktemp("resume_a")), n, kw, how)


@pytest.mark.parametrize("case", list(CASES))
def test_continuation_is_bit_exact(case, run_a, tmp_path):
    n, kw, how = CASES[case]
    a = run_a if case == "a_defaults_8192" else _run_a(str(tmp_path), n, kw, how)
    assert a["T"] == {8192: 80, 300: 2176, 4096: 160}[n]
    assert len(a["lines"]) >= 2                             # A printed score lines after its save point
    if kw.get("randomize"):
        # enough early falls: envs redrew their constants on both sides of the save
        draws = [s["dr_table"][:, 6].view(torch.int32).sum().item() for s in (a["at_save"], a["after_4"])]
        assert draws[0] > n and draws[1] > draws[0], draws
    periodic = how == "periodic"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b = _make(n, 12345, resume=True, resume_path=a["weights"], save=True, save_state=True,      # other initial weights
                  save_path=os.path.join(str(tmp_path), "b_"), save_freq=150 if periodic else 10 ** 9, **kw)
        b.load_training_state()
        assert _differences(a["at_save"], _snapshot(b)) == ["all_obs", "all_acts", "all_log_prob", "all_reward", "all_advantage",
                                                             "target"] + (["target_norm"] if b.normalize_value else [])
        _rollouts(b, 2)
        if not periodic:
            b.save("300")
    got = _snapshot(b)
    assert got["optim_step"] == 300 and got["run_step"] == 4 * a["T"] and int(got["step"]) == 300
    assert _differences(a["after_4"], got) == []
    assert _score_lines(out.getvalue()) == a["lines"]
    # and the state the two runs saved at optim_step 300 is the same file content, entry by entry
    sa = torch.load(b.training_state_path(os.path.join(a["dir"], "a_300.pth"), 0), weights_only=True)
    sb = torch.load(b.training_state_path(os.path.join(str(tmp_path), "b_300.pth"), 0), weights_only=True)
    assert _same_state(sa, sb) == []
    b.exit()


def test_weights_only_continuation_differs(run_a):
    """The control: from the same save, `load` (the weights alone) is a different run -- the comparison can tell."""
    with contextlib.redirect_stdout(io.StringIO()):
        c = _make(8192, 12345, load=True, load_path=run_a["weights"])
        assert torch.equal(c.policy.P, run_a["at_save"]["P"])
        first_var = c.action_var.clone()
        _rollouts(c, 1)
    assert torch.equal(first_var, torch.full_like(first_var, 0.2))
    assert float(run_a["at_save"]["action_var"][0]) < 0.2 - 1e-4        # A's had decayed over 160 steps
    assert c.optim_step == 75
    assert not torch.equal(c.policy.P, run_a["after_3"]["P"])
    c.exit()


def test_inside_a_rollout_only_the_weights_are_saved(tmp_path):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        agent = _make(8192, 0, save=True, save_state=True, save_path=str(tmp_path / "w_"), save_freq=10 ** 9)
        for _ in range(agent.rollout_size + 7):
            agent.run()
        agent.save("end")
    assert sorted(os.listdir(tmp_path)) == ["w_end.pth"]
    said = [ln for ln in out.getvalue().splitlines() if ln.startswith("save_state:")]
    assert len(said) == 1 and "step 7 of 80" in said[0] and "no training state" in said[0] and "last periodic save" in said[0]
    with pytest.raises(ValueError, match="rollout boundary"):
        agent.save_training_state(str(tmp_path / "x.state.r0.pth"))
    assert sorted(os.listdir(tmp_path)) == ["w_end.pth"]
    agent.exit()


@pytest.mark.parametrize("field,change", [("num_envs", dict(num_envs=4096)), ("gae", dict(gae="episodic"))])
def test_a_state_of_other_options_is_refused_before_anything_is_built(run_a, field, change):
    from fly_bproject_amd.ppo import PPO
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    kw = dict(num_envs=8192, resume=True, resume_path=run_a["weights"])
    kw.update(change)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match=r" %s is " % field):
            PPO(make_args(kw.pop("num_envs"), **kw))
    assert torch.cuda.memory_allocated() == before          # no env, no ring was built


def test_resume_excludes_load_and_needs_its_state_file(run_a, tmp_path):
    from fly_bproject_amd.ppo import PPO
    with pytest.raises(ValueError, match="exclude"):
        PPO(make_args(8192, resume=True, resume_path=run_a["weights"], load=True, load_path=run_a["weights"]))
    with pytest.raises(ValueError, match="testing"):
        PPO(make_args(8192, resume=True, resume_path=run_a["weights"], testing=True))
    lone = str(tmp_path / "lone.pth")
    torch.save(torch.load(run_a["weights"], weights_only=True), lone)
    with pytest.raises(FileNotFoundError, match="lone.state.r0.pth"):
        PPO(make_args(8192, resume=True, resume_path=lone))


def test_off_is_off(run_a, tmp_path):
    """Without save_state a saving run writes the weights files and nothing else; with it, the weights file is the same file."""
    with contextlib.redirect_stdout(io.StringIO()):
        agent = _make(8192, 0, save=True, save_path=str(tmp_path / "o_"), save_freq=150)
        _rollouts(agent, 2)
        agent.save()
    assert sorted(os.listdir(tmp_path)) == ["o_.pth", "o_150.pth"]
    off = torch.load(tmp_path / "o_150.pth", weights_only=True)
    on = torch.load(run_a["weights"], weights_only=True)
    assert list(off) == list(on) == ["shared_net.0.weight", "shared_net.0.bias", "shared_net.2.weight", "shared_net.2.bias",
                                     "to_mean.0.weight", "to_mean.0.bias", "to_mean.2.weight", "to_mean.2.bias",
                                     "to_value.0.weight", "to_value.0.bias", "to_value.2.weight", "to_value.2.bias"]
    assert all(torch.equal(off[k], on[k]) for k in off)
    assert sorted(os.listdir(run_a["dir"])) == ["a_150.pth", "a_150.state.r0.pth", "a_300.pth", "a_300.state.r0.pth"]
    agent.exit()


# ---- two ranks on one GPU over gloo --------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_worker(rank, world, port, out_dir, resume):
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    from fly_bproject_amd.dist import broadcast_policy
    from fly_bproject_amd.ppo import PPO
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.manual_seed((99 if resume else 10) + rank)
    weights = os.path.join(out_dir, "d_75.pth")
    res = {}
    with contextlib.redirect_stdout(io.StringIO()):
        kw = dict(rank=rank, world_size=world, seed=0, dp_mode="grad_allreduce", dp_allreduce="rccl")
        if resume:
            agent = PPO(make_args(2048, resume=True, resume_path=weights, **kw))
            broadcast_policy(agent)
            if rank == 1:
                try:
                    agent.load_training_state(agent.training_state_path(weights, 0))
                    res["other_rank"] = "accepted"
                except ValueError as e:
                    res["other_rank"] = str(e)
            agent.load_training_state()
            updates = 1
        else:
            agent = PPO(make_args(2048, save=True, save_state=True, save_path=os.path.join(out_dir, "d_"), save_freq=75, **kw))
            broadcast_policy(agent)
            updates = 2                                     # run() saves by itself after the first (optim_step 75), on every rank
        for _ in range(updates * agent.rollout_size):
            agent.run()
    torch.cuda.synchronize()
    assert agent.optim_step == 150 and agent.run_step == 2 * agent.rollout_size
    pol = agent.policy
    res.update(P=pol.P.cpu(), exp_avg=pol.exp_avg.cpu(), exp_avg_sq=pol.exp_avg_sq.cpu(), step=pol.step.cpu(),
               acts=agent.all_acts[0, :8].cpu())
    torch.save(res, os.path.join(out_dir, "%s%d.pt" % ("resumed" if resume else "full", rank)))
    agent.exit()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_resume(tmp_path):
    out = str(tmp_path)
    mp.spawn(_dist_worker, args=(2, _free_port(), out, False), nprocs=2, join=True)
    assert sorted(f for f in os.listdir(out) if f.startswith("d_75")) == ["d_75.pth", "d_75.state.r0.pth", "d_75.state.r1.pth"]
    mp.spawn(_dist_worker, args=(2, _free_port(), out, True), nprocs=2, join=True)
    full = [torch.load(os.path.join(out, "full%d.pt" % r), weights_only=True) for r in range(2)]
    resumed = [torch.load(os.path.join(out, "resumed%d.pt" % r), weights_only=True) for r in range(2)]
    for k in ("P", "exp_avg", "exp_avg_sq", "step"):
        assert torch.equal(resumed[0][k], resumed[1][k]), k                 # the resumed pair in lock step
        assert torch.equal(resumed[0][k], full[0][k]) and torch.equal(full[0][k], full[1][k]), k   # and where the uninterrupted pair is
    for r in range(2):
        assert torch.equal(resumed[r]["acts"], full[r]["acts"]), r         # each rank continued ITS rollouts
    assert not torch.equal(resumed[0]["acts"], resumed[1]["acts"])
    assert " rank is 0 in the state file and 1 in this run" in resumed[1]["other_rank"]
