"""GPU (-m gpu): recording -- fly_render against its float64 oracle (tests/render_ref.py), the pose record of the persistent
rollout against the per-step state, recording leaving training's bits alone, and trainer.py --record end to end."""
import contextlib
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests.hip_helpers import make_args, make_env
from tests.test_record_cpu import decode_png

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose(params, pos=(0.0, 0.0, 2.0), quat=(0.0, 0.0, 0.0, 1.0), joints=None):
    p = np.zeros(25, np.float32)
    p[0:3], p[3:7] = pos, quat
    p[7:] = params.dof_pose[:] if joints is None else joints
    return p


def _poses(params):
    lo, hi = np.array(params.dof_lo[:]), np.array(params.dof_hi[:])
    s = math.sqrt(0.5)
    yaw = (0.0, 0.0, math.sin(0.35), math.cos(0.35))
    return {
        "rest": _pose(params),
        "rolled_90": _pose(params, quat=(s, 0.0, 0.0, s)),
        "upside_down": _pose(params, pos=(0.0, 0.0, 2.5), quat=(1.0, 0.0, 0.0, 0.0)),
        "legs_at_limits": _pose(params, quat=yaw, joints=np.where(np.arange(18) % 2 == 0, lo, hi)),
        "half_sunk": _pose(params, pos=(0.0, 0.0, 0.1)),
        "x_1000": _pose(params, pos=(1000.0, 3.0, 2.0), quat=yaw),
    }


def _near_boundary(ids):
    """Pixels whose 3x3 neighbourhood in `ids` holds more than one id."""
    h, w = ids.shape
    p = np.pad(ids, 1, mode="edge")
    out = np.zeros((h, w), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= p[dy:dy + h, dx:dx + w] != ids
    return out


@pytest.mark.parametrize("size", [(320, 240), (200, 150)])     # 200 x 150: tiles cut by the image's right and bottom edges
def test_renderer_matches_oracle(size):
    from fly_bproject_amd import record
    w, h = size
    env = make_env(32)
    rc = record.render_config(width=w, height=h)
    poses = _poses(env.params)
    rgba, ids = record.render(env, torch.from_numpy(np.stack(list(poses.values()))).cuda(), rc, with_ids=True)
    torch.cuda.synchronize()
    rgb_all, ids_all = record.rgba_to_rgb(rgba), ids.cpu().numpy()
    assert (rgba.cpu().numpy().view(np.uint8).reshape(len(poses), h, w, 4)[..., 3] == 255).all()
    for i, (name, pose) in enumerate(poses.items()):
        ref_rgb, ref_ids = RR.render(env.params, pose.astype(np.float64), w, h, record.FOV_Y_DEG, record.CAM_OFFSET,
                                     record.LOOK_Z)
        got_rgb, got_ids = rgb_all[i], ids_all[i]
        diff = got_ids != ref_ids
        assert diff.mean() <= 0.002, (name, diff.mean())
        assert not (diff & ~_near_boundary(ref_ids)).any(), (name, np.argwhere(diff & ~_near_boundary(ref_ids))[:5])
        close = (np.abs(got_rgb.astype(int) - ref_rgb.astype(int)) <= 2).all(-1)
        assert close.mean() >= 0.995, (name, close.mean())
        assert (ref_ids >= RR.RID_BODY).sum() > 200, name                 # the fly is in view
    env.exit()


def _state0(env):
    return torch.cat([env.root_tensor[0, :7], env.dof_states.view(-1, 18, 2)[0, :, 0]]).clone()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", ["fs_8192", "fs_multi", "ragged_1000", "no_fs_4096", "graph_4096"])
def test_pose_record_equals_per_step_state(case, tmp_path, monkeypatch):
    """Every row of the persistent rollout's pose record is bit-equal to env 0's root[0, :7] / dof_state[0, :, 0] after the
    same step of a per-step run with the same seed, over two rollouts (an update between them).  graph_4096: the record of
    the per-step path, whose second rollout is replayed from a captured hipGraph."""
    from fly_bproject_amd.ppo import PPO
    n = {"fs_8192": 8192, "fs_multi": 32 * (_cus() + 1), "ragged_1000": 1000, "no_fs_4096": 4096, "graph_4096": 4096}[case]
    if case == "no_fs_4096":
        monkeypatch.setenv("FLY_ROLLOUT_FS", "0")
    graph = case == "graph_4096"
    out = {}
    for persistent in (False, True):        # True: the recording run
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(n, persistent_rollout=persistent and not graph, graph=persistent and graph, record=persistent,
                                  record_dir_name=str(tmp_path / "f"), time_steps_per_recorded_frame=50))
            assert agent.persistent_rollout == (persistent and not graph)
            T = agent.rollout_size
            rows = []
            for i in range(2 * T):
                agent.run()
                if not persistent:
                    rows.append(_state0(agent.env))
                elif i % T == T - 1:
                    rows.append(agent.env.recorder.poses[:T].clone())
            agent.generate_video()
            agent.exit()
        torch.cuda.synchronize()
        out[persistent] = torch.stack(rows) if not persistent else torch.cat(rows)
    assert out[True].shape == (2 * T, 25)
    assert torch.equal(out[True], out[False])
    assert sorted(os.listdir(tmp_path / "f")) == ["frame_%06d.png" % s for s in range(0, 2 * T, 50)]


@pytest.mark.parametrize("case", ["default", "f32", "ragged_1000"])
def test_recording_does_not_perturb_training(case, tmp_path, monkeypatch):
    from fly_bproject_amd.ppo import PPO
    n = 1000 if case == "ragged_1000" else 4096
    if case == "f32":
        monkeypatch.setenv("FLY_GEMM", "f32")
    out = {}
    for rec in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(n, record=rec, record_dir_name=str(tmp_path / "f"), time_steps_per_recorded_frame=4))
            assert agent.persistent_rollout and (agent.env.recorder is not None) == rec
            for _ in range(agent.rollout_size):                 # one rollout and its update
                agent.run()
            agent.flush_log()
            torch.cuda.synchronize()
            assert agent.optim_step == 75
            out[rec] = [agent.all_acts.clone(), agent.all_reward.clone(), agent.all_log_prob.clone(), agent._obs_ring.clone(),
                        agent.policy.P.clone(), agent.env.root_tensor.clone(), agent.env.dof_states.clone()]
            agent.generate_video()
            agent.exit()
    for i, (a, b) in enumerate(zip(out[False], out[True])):
        assert torch.equal(a, b), i
    assert len(os.listdir(tmp_path / "f")) == len(range(0, agent.rollout_size, 4))


def test_fly_step_path_frames(tmp_path):
    """Fly.step (DQN's env step): ten steps, k = 2 -> frames of steps 0, 2, 4, 6, 8, each the render of the state read back
    after that step."""
    from fly_bproject_amd import record
    from tests.hip_helpers import cuda, pose_actions
    env = make_env(64, record=True, record_dir_name=str(tmp_path / "f"), time_steps_per_recorded_frame=2)
    rng = np.random.default_rng(0)
    a0 = pose_actions(env.params, 64)
    states = []
    for _ in range(10):
        env.step(cuda(np.clip(a0 + rng.normal(0, 0.5, a0.shape), -1, 1).astype(np.float32)))
        states.append(_state0(env))
    assert env.render() is not None and env.render().shape == (480, 640, 3)
    env.generate_video()
    files = sorted(os.listdir(tmp_path / "f"))
    assert [f for f in files if f.endswith(".png")] == ["frame_%06d.png" % s for s in range(0, 10, 2)]
    want, _ = record.render(env, torch.stack(states[0::2]))
    want = record.rgba_to_rgb(want)
    for i, s in enumerate(range(0, 10, 2)):
        got = decode_png((tmp_path / "f" / ("frame_%06d.png" % s)).read_bytes())
        np.testing.assert_array_equal(got, want[i])
    env.exit()


def _trainer(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(REPO, "trainer.py")] + args, cwd=REPO, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("Steps:")]


def test_trainer_records_end_to_end(tmp_path):
    base = ["--num_envs", "4096", "--headless", "True", "--max_steps", "167"]
    ck = str(tmp_path / "ck")
    plain = _trainer(base + ["--save_path", ck])
    rec_dir = tmp_path / "rec"
    recorded = _trainer(base + ["--record_dir_name", str(rec_dir), "--time_steps_per_recorded_frame", "3"])
    assert plain and recorded == plain
    pngs = sorted(f for f in os.listdir(rec_dir) if f.endswith(".png"))
    assert pngs == ["frame_%06d.png" % s for s in range(0, 166, 3)]
    imgs = [decode_png((rec_dir / f).read_bytes()) for f in pngs]
    assert all(im.shape == (480, 640, 3) for im in imgs)
    assert any(not np.array_equal(imgs[0], im) for im in imgs[1:])
    for f, im in zip(pngs, imgs):
        c = im[180:300, 260:380].astype(int)
        assert ((c[..., 0] != c[..., 1]) | (c[..., 1] != c[..., 2])).any(), f      # the ground is grey, the fly is not
    # --testing on the checkpoint the first run wrote
    test_dir = tmp_path / "test_rec"
    _trainer(["--num_envs", "4096", "--headless", "True", "--max_steps", "20", "--testing", "True", "--load_path",
              ck + ".pth", "--record_dir_name", str(test_dir), "--time_steps_per_recorded_frame", "3"])
    assert sorted(f for f in os.listdir(test_dir) if f.endswith(".png")) == ["frame_%06d.png" % s for s in range(0, 20, 3)]
