"""GPU (-m gpu): exact resume of a --lambda_returns --normalize_value run, after
tests/test_resume_gpu.py: run A = 1 rollout + update, save at the rollout boundary, 1 more; run B = a new PPO that resumes from
A's save and makes 1.  B's rollout, targets, value statistics and weights are bit for bit A's; the state file carries the
`meta_ext` block, and a run with the other value of the option is refused before anything is built."""
import contextlib
import io
import os

import pytest
import torch

from tests.test_resume_gpu import _differences, _make, _rollouts, _same_state, _score_lines, _snapshot, make_args

pytestmark = pytest.mark.gpu
KW = dict(lambda_returns=True, normalize_value=True)


def test_resume_continues_a_lambda_returns_run_bit_for_bit(tmp_path):
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a_dir)
    os.makedirs(b_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        a = _make(8192, 0, save=True, save_state=True, save_path=os.path.join(a_dir, "a_"), save_freq=75, **KW)
        _rollouts(a, 1)                                     # run() saves by itself at optim_step 75
    weights = os.path.join(a_dir, "a_75.pth")
    state_path = a.training_state_path(weights, 0)
    assert a.optim_step == 75 and os.path.isfile(weights) and os.path.isfile(state_path)
    state = torch.load(state_path, weights_only=True)
    assert state["format"] == 1 and state["meta_ext"] == {"lambda_returns": True} and "lambda_returns" not in state["meta"]
    assert list(state)[:3] == ["format", "meta", "meta_ext"]
    at_save = _snapshot(a)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        _rollouts(a, 1)
    after, lines = _snapshot(a), _score_lines(out.getvalue())
    a.exit()
    assert float(after["value_stats"][0]) == 2 * 80 * 8192 and len(lines) >= 1

    # the other value of the option: refused by the constructor, before anything is built
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    from fly_bproject_amd.ppo import PPO
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match=" lambda_returns is True in the state file and False in this run"):
            PPO(make_args(8192, resume=True, resume_path=weights, normalize_value=True))
    assert torch.cuda.memory_allocated() == before

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        b = _make(8192, 12345, resume=True, resume_path=weights, save=True, save_state=True, save_path=os.path.join(b_dir, "b_"),
                  save_freq=75, **KW)                       # other initial weights
        b.load_training_state()
        assert b.lambda_returns is True
        assert _differences(at_save, _snapshot(b)) == ["all_obs", "all_acts", "all_log_prob", "all_reward", "all_advantage", "target",
                                                        "target_norm"]
        # load_training_state holds the block against the live run once more
        b.args.lambda_returns = False
        with pytest.raises(ValueError, match=" lambda_returns is True in the state file and False in this run"):
            b.load_training_state(state_path)
        b.args.lambda_returns = True
        _rollouts(b, 1)
    got = _snapshot(b)
    assert got["optim_step"] == 150 and got["run_step"] == 160
    assert _differences(after, got) == []                   # rollout, lambda targets, their statistics, weights, Adam: bit for bit
    assert _score_lines(out.getvalue()) == lines
    sa = torch.load(b.training_state_path(os.path.join(a_dir, "a_150.pth"), 0), weights_only=True)
    sb = torch.load(b.training_state_path(os.path.join(b_dir, "b_150.pth"), 0), weights_only=True)
    assert _same_state(sa, sb) == [] and sb["meta_ext"] == {"lambda_returns": True}
    b.exit()


def test_a_state_file_without_the_block_resumes_with_the_option_off(tmp_path):
    """A state written before the option existed (no meta_ext): resumes as today, and is refused under lambda_returns."""
    with contextlib.redirect_stdout(io.StringIO()):
        a = _make(8192, 0, save=True, save_state=True, save_path=str(tmp_path / "a_"), save_freq=75)
        _rollouts(a, 1)
    weights = str(tmp_path / "a_75.pth")
    state_path = a.training_state_path(weights, 0)
    a.exit()
    state = torch.load(state_path, weights_only=True)
    assert state.pop("meta_ext") == {"lambda_returns": False}
    torch.save(state, state_path)
    from fly_bproject_amd.ppo import PPO
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match=" lambda_returns is False in the state file and True in this run"):
            PPO(make_args(8192, resume=True, resume_path=weights, lambda_returns=True))
        b = _make(8192, 12345, resume=True, resume_path=weights)
        b.load_training_state()
    assert b.lambda_returns is False and b.optim_step == 75 and b.run_step == 80
    b.exit()
