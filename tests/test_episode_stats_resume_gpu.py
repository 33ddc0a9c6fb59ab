"""GPU (-m gpu): exact resume of an --episode_stats run, after tests/test_lambda_returns_resume_gpu.py:
run A = 1 rollout + update, save at the rollout boundary, 1 more; run B = a new PPO that resumes from A's save and makes 1.  B's
carries, window and total are bit for bit A's, and so are its score lines.  A state file without the block resumes with the
lengths of the open episodes taken from the env and says so; with the flag off a block is ignored."""
import contextlib
import io
import os

import pytest
import torch

from tests.test_resume_gpu import _differences, _make, _rollouts, _score_lines, _snapshot

pytestmark = pytest.mark.gpu
EP = ("carry_ret", "carry_len", "window", "total")
SAID = "episode_stats: the training state holds no episode statistics"


def _ep(agent):
    torch.cuda.synchronize()
    return {k: getattr(agent, "_ep_" + k).clone() for k in EP}


def test_resume_continues_the_episode_statistics_bit_for_bit(tmp_path):
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a_dir)
    os.makedirs(b_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        a = _make(4096, 0, save=True, save_state=True, save_path=os.path.join(a_dir, "a_"), save_freq=75, episode_stats=True)
        _rollouts(a, 1)                                     # run() saves by itself at optim_step 75
    weights = os.path.join(a_dir, "a_75.pth")
    state_path = a.training_state_path(weights, 0)
    state = torch.load(state_path, weights_only=True)
    assert sorted(state["agent"]["episode_stats"]) == sorted(EP)
    assert "episode_stats" not in state["meta"] and state["meta_ext"] == {"lambda_returns": False}
    at_save = _ep(a)
    for k in EP:
        assert torch.equal(state["agent"]["episode_stats"][k], at_save[k].cpu()), k
    assert float(at_save["window"][0]) > 0 and int(at_save["carry_len"].max()) > 0      # open and closed episodes at the save
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        _rollouts(a, 1)
    after, after_ep, lines = _snapshot(a), _ep(a), _score_lines(out.getvalue())
    a.exit()
    assert any(" | Return " in ln for ln in lines)

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b = _make(4096, 12345, resume=True, resume_path=weights, save=True, save_state=True, save_path=os.path.join(b_dir, "b_"),
                  save_freq=75, episode_stats=True)
        b.load_training_state()
        restored = _ep(b)
        for k in EP:
            assert torch.equal(restored[k], at_save[k]), k
        _rollouts(b, 1)
    assert SAID not in out.getvalue()
    got, got_ep = _snapshot(b), _ep(b)
    assert _differences(after, got) == []
    for k in EP:
        assert got_ep[k].dtype == after_ep[k].dtype and torch.equal(got_ep[k], after_ep[k]), k
    assert _score_lines(out.getvalue()) == lines
    b.exit()

    # the flag off: the block is ignored, and the run is the one without statistics
    with contextlib.redirect_stdout(io.StringIO()):
        c = _make(4096, 12345, resume=True, resume_path=weights)
        c.load_training_state()
        _rollouts(c, 1)
    assert c.episode_stats() is None and _differences(after, _snapshot(c)) == []
    c.exit()


def test_a_state_without_the_block_resumes_with_the_envs_lengths(tmp_path):
    with contextlib.redirect_stdout(io.StringIO()):
        a = _make(4096, 0, save=True, save_state=True, save_path=str(tmp_path / "a_"), save_freq=75)
        _rollouts(a, 1)
    weights = str(tmp_path / "a_75.pth")
    state = torch.load(a.training_state_path(weights, 0), weights_only=True)
    assert "episode_stats" not in state["agent"]
    a.exit()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b = _make(4096, 12345, resume=True, resume_path=weights, episode_stats=True)
        b.load_training_state()
    assert out.getvalue().count(SAID) == 1 and "partial" in out.getvalue()
    torch.cuda.synchronize()
    # carry_len is env.progress_buf -- except where the env's end flag is up: that episode is closed, the env resets its count
    # in the step to come, and the kernel's carry behind an end is 0
    progress, pending = b.env.progress_buf, b.env.reset_buf != 0
    assert torch.equal(b._ep_carry_len[~pending], progress[~pending]) and not b._ep_carry_len[pending].any()
    assert int(pending.sum()) > 0 and int(b._ep_carry_len.max()) > 0 and (progress[pending] > 0).all()
    assert not b._ep_carry_ret.any() and b.episode_stats()["total"]["episodes"] == 0
    # and from there every closed episode's length is the env's own count again
    with contextlib.redirect_stdout(io.StringIO()):
        _rollouts(b, 1)
    torch.cuda.synchronize()
    reset, progress = b._reset_rows.cpu(), b._progress_rows.cpu()
    ends = reset != 0
    total = b.episode_stats()["total"]
    assert total["episodes"] == int(ends.sum()) > 0
    assert float(b._ep_total[5]) == int(progress[ends].sum())          # len_sum
    assert (total["length_min"], total["length_max"]) == (int(progress[ends].min()), int(progress[ends].max()))
    b.exit()
