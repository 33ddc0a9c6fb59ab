"""GPU (-m gpu): exact resume of an --update_stats run, after tests/test_episode_stats_resume_gpu.py:
run A = 2 rollouts + updates, save at the rollout boundary, 1 more; run B = a new PPO that resumes from A's save and makes 1.
B's last, window and total are bit for bit A's, and so are its score lines.  A state file without the block resumes with empty
sets and says so; with the flag off a block is ignored."""
import contextlib
import io
import os

import pytest
import torch

from tests.test_resume_gpu import _differences, _make, _rollouts, _score_lines, _snapshot

pytestmark = pytest.mark.gpu
US = ("last", "window", "total")
SAID = "update_stats: the training state holds no update statistics"


def _us(agent):
    torch.cuda.synchronize()
    return {k: getattr(agent, "_us_" + k).clone() for k in US}


def test_resume_continues_the_update_statistics_bit_for_bit(tmp_path):
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a_dir)
    os.makedirs(b_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        a = _make(4096, 0, save=True, save_state=True, save_path=os.path.join(a_dir, "a_"), save_freq=150, update_stats=True)
        _rollouts(a, 2)                                     # run() saves by itself at optim_step 150
    weights = os.path.join(a_dir, "a_150.pth")
    state = torch.load(a.training_state_path(weights, 0), weights_only=True)
    assert sorted(state["agent"]["update_stats"]) == sorted(US) and state["format"] == 1
    assert "update_stats" not in state["meta"] and state["meta_ext"] == {"lambda_returns": False}
    at_save = _us(a)
    for k in US:
        assert torch.equal(state["agent"]["update_stats"][k], at_save[k].cpu()), k
    rows = 160 * 4096
    # T = 160: the lines of steps 200 and 300 emptied the window, so at the save it holds update 2 alone; total holds both
    assert float(at_save["total"][0]) == 2 * rows and float(at_save["window"][0]) == rows == float(at_save["last"][0])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        _rollouts(a, 1)
    after, after_us, lines = _snapshot(a), _us(a), _score_lines(out.getvalue())
    a.exit()
    assert len(lines) == 1 and " | Clip " in lines[0]                 # step 400 carries update 2, from the SAVED window

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b = _make(4096, 12345, resume=True, resume_path=weights, save=True, save_state=True, save_path=os.path.join(b_dir, "b_"),
                  save_freq=150, update_stats=True)
        b.load_training_state()
        restored = _us(b)
        for k in US:
            assert torch.equal(restored[k], at_save[k]), k
        _rollouts(b, 1)
    assert SAID not in out.getvalue()
    got, got_us = _snapshot(b), _us(b)
    assert _differences(after, got) == []
    for k in US:
        assert got_us[k].dtype == after_us[k].dtype and torch.equal(got_us[k], after_us[k]), k
    assert float(got_us["total"][0]) == 3 * rows
    assert _score_lines(out.getvalue()) == lines
    b.exit()

    # the flag off: the block is ignored, and the run is the one without statistics
    with contextlib.redirect_stdout(io.StringIO()):
        c = _make(4096, 12345, resume=True, resume_path=weights)
        c.load_training_state()
        _rollouts(c, 1)
    assert c.update_stats() is None and _differences(after, _snapshot(c)) == []
    c.exit()


def test_a_state_without_the_block_resumes_with_empty_sets(tmp_path):
    from fly_bproject_amd import ppo
    with contextlib.redirect_stdout(io.StringIO()):
        a = _make(4096, 0, save=True, save_state=True, save_path=str(tmp_path / "a_"), save_freq=75)
        _rollouts(a, 1)
    weights = str(tmp_path / "a_75.pth")
    state = torch.load(a.training_state_path(weights, 0), weights_only=True)
    assert "update_stats" not in state["agent"]
    a.exit()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b = _make(4096, 12345, resume=True, resume_path=weights, update_stats=True)
        b.load_training_state()
    assert out.getvalue().count(SAID) == 1
    for k in US:
        assert torch.equal(_us(b)[k].cpu(), ppo.update_stats_empty()), k
    assert b.update_stats()["total"]["rows"] == 0
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        _rollouts(b, 1)
    assert b.update_stats()["total"]["rows"] == 160 * 4096 and b.optim_step == 150
    lines = _score_lines(out.getvalue())
    assert lines and all(" | KL " in ln for ln in lines)
    b.exit()
