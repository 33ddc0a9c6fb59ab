"""CPU: `bench.py --dump-outputs DIR` -- what it writes, that the sample of wide arrays is fixed, and that the
largest rollout the PPO loop accepts stays inside the size limit."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_rows_is_fixed_sorted_and_aligned():
    import bench
    a = torch.arange(1000 * 3, dtype=torch.float32).view(10, 100, 3)
    b = torch.arange(1000 * 5, dtype=torch.float32).view(10, 100, 5)
    s1, s2 = bench.sample_rows(a, 64), bench.sample_rows(a, 64)
    assert s1.shape == (64, 3) and torch.equal(s1, s2)
    rows = (s1[:, 0] / 3).long()
    assert torch.equal(rows, torch.sort(rows).values) and len(set(rows.tolist())) == 64
    assert torch.equal((bench.sample_rows(b, 64)[:, 0] / 5).long(), rows)          # same rows of another array
    assert torch.equal(bench.sample_rows(a, 5000), a.reshape(-1, 3))                # small arrays whole


def test_dump_outputs_writes_float32_or_float64_and_refuses_oversize(tmp_path):
    import bench
    got = bench.dump_outputs(str(tmp_path / "d"), {"x": torch.ones(4, 2), "i": torch.arange(3), "w": np.zeros(2, np.float64)})
    assert got["arrays"] == 3 and got["bytes"] == 4 * 8 + 3 * 4 + 2 * 8
    assert np.load(tmp_path / "d" / "x.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "d" / "i.npy"), np.arange(3, dtype=np.float32))
    assert np.load(tmp_path / "d" / "w.npy").dtype == np.float64
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": torch.empty(bench.DUMP_LIMIT_BYTES // 4 + 1)})
    assert not (tmp_path / "big").exists()


@pytest.mark.parametrize("n", [8192, 16])
def test_ppo_outputs_of_the_largest_rollout_fit_the_limit(tmp_path, n):
    """T = 16 * (40960 // n) env steps of n envs: T * n is at most 655 360 rows at any accepted num_envs."""
    import bench
    from fly_bproject_amd.ppo import Net
    T = 16 * (40960 // n)
    obs_ring = torch.zeros(T + 1, n, 73)
    agent = types.SimpleNamespace(rollout_size=T, args=types.SimpleNamespace(num_envs=n), net=Net(73, 18),
                                  action_var=torch.full((18,), 0.2), all_reward=torch.zeros(T, n, 1),
                                  all_log_prob=torch.zeros(T, n), _target=torch.zeros(T, n, 1),
                                  all_advantage=torch.zeros(T, n, 1), all_done=torch.ones(n, 1, dtype=torch.long),
                                  all_next_obs=obs_ring[1:], all_acts=torch.zeros(T, n, 18))
    got = bench.dump_outputs(str(tmp_path), bench.ppo_outputs(agent))
    assert got["bytes"] <= bench.DUMP_LIMIT_BYTES
    assert np.load(tmp_path / "next_obs.npy").shape == (bench.DUMP_SAMPLE_ROWS, 73)
    assert np.load(tmp_path / "advantage.npy").shape == (T, n)
    assert np.load(tmp_path / "param.shared_net.0.weight.npy").shape == (256, 73)


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0", "--dry_run"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
