"""The inputs the reward-scaling tests share (tests/test_reward_norm_cpu.py, tests/test_reward_norm_gpu.py): seeded, no GPU."""
import numpy as np

HUGE = np.float32(1e20)
PATTERNS = ("nowhere", "first", "last", "consecutive", "every", "boundaries")


def place(reset, e, pattern, lanes=64):
    """Column e of the reset rows <- one of the hand-placed end patterns; "boundaries" are the last row of a scan chunk and
    the first row of the next (chunks of ceil(T / lanes) rows)."""
    T = reset.shape[0]
    L = -(-T // lanes)
    reset[:, e] = 0
    if pattern == "first":
        reset[0, e] = 1
    elif pattern == "last":
        reset[T - 1, e] = 2
    elif pattern == "consecutive":
        reset[T // 2, e] = 1
        reset[min(T // 2 + 1, T - 1), e] = 1
    elif pattern == "every":
        reset[:, e] = 3
    elif pattern == "boundaries":
        for k in (1, 2, 5):
            if k * L - 1 < T:
                reset[k * L - 1, e] = 1
            if k * L < T and k != 2:
                reset[k * L, e] = 1
    else:
        assert pattern == "nowhere"


def case(T, N, seed, carry=False, nan=False, huge=True, lanes=64):
    """-> (reward f32 [T][N], reset int64 [T][N], carry_in f64 [N]): seeded normals with a few exact zeros and one huge value
    (with `nan` one NaN too, in an env of its own where there are several), Bernoulli(0.05) ends, and the hand-placed end
    patterns on the first columns (rotated by the seed, so N = 1 meets all of them over the seeds)."""
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((T, N)).astype(np.float32)
    flat = reward.reshape(-1)
    flat[rng.integers(0, flat.size, min(3, flat.size))] = 0.0
    if huge and flat.size > 1:
        flat[rng.integers(0, flat.size)] = HUGE * (1 if seed % 2 else -1)
    reset = (rng.random((T, N)) < 0.05).astype(np.int64)
    for k in range(min(N, len(PATTERNS))):
        place(reset, k, PATTERNS[(seed + k) % len(PATTERNS)], lanes)
    if nan:
        reward[rng.integers(0, T), N // 2] = np.nan
    cin = rng.normal(0, 3, N) if carry else np.zeros(N)
    return reward, reset, cin
