"""Exact resume (--save_state / --resume_path), the part that needs no GPU: the strict meta check, the state
file's name, the file format's round trip through the weights-only loader, and trainer.py's flags."""
import types

import pytest
import torch

from fly_bproject_amd import train_state


def _args(**kw):
    d = dict(sim_device="cuda:0", num_envs=8192, testing=False, seed=0, rank=0, world_size=1, variant="bigGrav",
             reward="standing")
    d.update(kw)
    return types.SimpleNamespace(**d)


# every opt-in on: each dependent field (seeds, rho, clip, ranges) then means something and is compared
FULL = dict(gae="episodic", minibatch="shuffled", action_noise="ar1", normalize_obs=True, normalize_value=True,
            normalize_advantage=True, randomize=True, gemm="f16x2", persistent_rollout=True)

# one difference per meta field: (the field the error must name, the resuming run's args)
DIFFERENCES = [
    ("num_envs", dict(num_envs=8191)),                      # same rollout_size (40960 // n == 5): num_envs is what differs
    ("rollout_size", dict(num_envs=4096)),                  # (num_envs differs too: see the test)
    ("variant", dict(variant="lowGrav")),
    ("reward", dict(reward="walking")),
    ("world_size", dict(world_size=2)),
    ("rank", dict(rank=1, minibatch_seed=0 - 0x9E3779B9, dr_seed=(0 - 0x9E3779B9) % (1 << 32))),   # the rank alone: seeds held
    ("gae", dict(gae="reference")),
    ("minibatch", dict(minibatch="reference")),
    ("minibatch_seed", dict(minibatch_seed=5)),
    ("action_noise", dict(action_noise="white")),
    ("noise_rho", dict(noise_rho=0.25)),
    ("normalize_obs", dict(normalize_obs=False)),
    ("obs_clip", dict(obs_clip=4.0)),
    ("normalize_value", dict(normalize_value=False)),
    ("normalize_advantage", dict(normalize_advantage=False)),
    ("randomize", dict(randomize=False)),
    ("dr_ranges", dict(dr_mass=(0.7, 1.3))),
    ("dr_seed", dict(dr_seed=9)),
    ("gemm", dict(gemm="f32")),
    ("step_gemm", dict(gemm="bf16x3")),
    ("persistent_rollout", dict(persistent_rollout=False)),
    ("dp_mode", dict(dp_mode="param_average")),
]


def test_differences_cover_every_meta_field():
    assert [f for f, _ in DIFFERENCES] == list(train_state.META_FIELDS)
    assert sorted(train_state.expected_meta(_args(**FULL))) == sorted(train_state.META_FIELDS)


def test_meta_check_accepts_an_identical_meta(monkeypatch):
    for k in ("FLY_GEMM", "FLY_STEP_GEMM", "FLY_PERSISTENT_ROLLOUT"):
        monkeypatch.delenv(k, raising=False)
    for kw in ({}, FULL):
        meta = train_state.expected_meta(_args(**kw))
        train_state.check_meta(meta, _args(**kw))
        # and after the trip through a file
        import io
        f = io.BytesIO()
        torch.save({"meta": meta}, f)
        f.seek(0)
        train_state.check_meta(torch.load(f, weights_only=True)["meta"], _args(**kw))


@pytest.mark.parametrize("field,change", DIFFERENCES, ids=[f for f, _ in DIFFERENCES])
def test_meta_check_names_the_field_that_differs(monkeypatch, field, change):
    for k in ("FLY_GEMM", "FLY_STEP_GEMM", "FLY_PERSISTENT_ROLLOUT"):
        monkeypatch.delenv(k, raising=False)
    meta = train_state.expected_meta(_args(**FULL))
    run = _args(**dict(FULL, **change))
    if field == "rollout_size":
        meta = dict(meta, num_envs=4096)                    # a file that agrees on num_envs and not on the rollout it implies
    with pytest.raises(ValueError) as e:
        train_state.check_meta(meta, run)
    msg = str(e.value)
    assert (" %s is " % field) in msg, msg
    want = train_state.expected_meta(run)[field]
    assert repr(meta[field]) in msg and repr(want) in msg, msg
    if field not in ("minibatch", "action_noise", "normalize_obs", "randomize", "gemm"):     # (these take dependent fields along)
        train_state.check_meta(dict(meta, **{field: want}), run)        # nothing else differs: with that field taken over it passes


def test_meta_check_refuses_a_missing_field_and_a_missing_block():
    meta = train_state.expected_meta(_args())
    del meta["dp_mode"]
    with pytest.raises(ValueError, match="dp_mode"):
        train_state.check_meta(meta, _args())
    with pytest.raises(ValueError, match="meta"):
        train_state.check_meta(None, _args())


def test_values_of_options_that_are_off_do_not_block_a_resume():
    """noise_rho without ar1, obs_clip without normalize_obs, the seeds and ranges of features that are off: not compared."""
    meta = train_state.expected_meta(_args())
    train_state.check_meta(meta, _args(noise_rho=0.9, obs_clip=2.0, minibatch_seed=3, dr_seed=4, dr_mass=(0.5, 2.0)))


def test_training_state_path():
    from fly_bproject_amd.ppo import PPO
    assert PPO.training_state_path("a/b_300.pth", 1) == "a/b_300.state.r1.pth"
    assert train_state.training_state_path("a/b_300.pth", 0) == "a/b_300.state.r0.pth"
    assert train_state.training_state_path("run_", 3) == "run_.state.r3.pth"


def _hand_made_state():
    return {"format": train_state.FORMAT, "meta": train_state.expected_meta(_args(**FULL)),
            "policy": {"P": torch.arange(6, dtype=torch.float32), "step2": torch.tensor([150, 0], dtype=torch.int32),
                       "PB": torch.arange(4, dtype=torch.int16), "step_idx": 0, "h2_calibrated": True},
            "agent": {"run_step": 160, "generator": torch.arange(16, dtype=torch.uint8),
                      "obs_stats": torch.linspace(0, 1, 7, dtype=torch.float64)},
            "env": {"reset_buf": torch.tensor([0, 1], dtype=torch.long), "render_count": 160}}


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


def test_a_state_dict_round_trips_through_the_weights_only_loader(tmp_path):
    state = _hand_made_state()
    path = str(tmp_path / "s.state.r0.pth")
    torch.save(state, path)
    back = train_state.read_state_file(path)                # torch.load(..., weights_only=True) inside
    assert _same(state, back)
    dst = torch.zeros(6)
    train_state.restore(dst, back["policy"], "policy", "P")
    assert torch.equal(dst, state["policy"]["P"])


def test_unknown_format_missing_file_and_wrong_tensor_are_errors_of_their_own(tmp_path):
    state = _hand_made_state()
    state["format"] = 2
    path = str(tmp_path / "s.pth")
    torch.save(state, path)
    with pytest.raises(ValueError, match="unknown format 2"):
        train_state.read_state_file(path)
    torch.save({"shared_net.0.weight": torch.zeros(2)}, path)       # a weights file is no state file
    with pytest.raises(ValueError, match="no format number"):
        train_state.read_state_file(path)
    with pytest.raises(FileNotFoundError, match="no training state file"):
        train_state.read_state_file(str(tmp_path / "absent.state.r0.pth"))
    blk = _hand_made_state()["policy"]
    with pytest.raises(ValueError, match=r"policy\.P is \(6,\) torch\.float32, this run holds \(5,\) torch\.float32"):
        train_state.restore(torch.zeros(5), blk, "policy", "P")
    with pytest.raises(ValueError, match=r"policy\.P is .*float32, this run holds .*float64"):
        train_state.restore(torch.zeros(6, dtype=torch.float64), blk, "policy", "P")
    with pytest.raises(ValueError, match=r"policy\.exp_avg is missing"):
        train_state.restore(torch.zeros(6), blk, "policy", "exp_avg")
    with pytest.raises(ValueError, match=r"policy\.step_idx is 0, not bool"):
        train_state.value(blk, "policy", "step_idx", bool)


def test_trainer_flags(capsys):
    import trainer
    args = trainer.parse_args([])
    assert args.save_state is False and args.resume is False and args.resume_path is None
    args = trainer.parse_args(["--resume_path", "x.pth"])
    assert args.resume is True and args.resume_path == "x.pth" and args.load is False
    args = trainer.parse_args(["--save_path", "run_", "--save_state"])
    assert args.save_state is True and args.save is True
    for bad in (["--resume_path", "x.pth", "--load_path", "y.pth"], ["--resume_path", "x.pth", "--testing", "True"],
                ["--save_state"]):
        with pytest.raises(SystemExit):
            trainer.parse_args(bad)
    capsys.readouterr()
