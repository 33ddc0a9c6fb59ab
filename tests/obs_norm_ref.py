"""float64 numpy statements of observation normalisation (PPO normalize_obs), for the tests.

S = (count, mean[k], var[k]) with population variance; initial S = (0, 0, 1).  A merge of a batch of rows replaces S by the
statistics of all rows seen so far: from the initial S, the batch's own mean and variance."""
import numpy as np

EPS = 1e-5


def initial(k=73):
    return 0.0, np.zeros(k), np.ones(k)


def moments(rows):
    """(count, mean, population var) of rows [m][k] in float64: a two-pass mean and centred sum of squares."""
    x = np.asarray(rows, dtype=np.float64).reshape(-1, np.shape(rows)[-1])
    mean = x.mean(axis=0)
    return float(x.shape[0]), mean, ((x - mean) ** 2).mean(axis=0)


def merge(S, rows):
    """S after a merge of `rows`: the moments of every row S covers plus these."""
    c, mu, var = S
    nb, mb, vb = moments(rows)
    if nb == 0:
        return S
    n = c + nb
    d = mb - mu
    return n, mu + d * (nb / n), (var * c + vb * nb + d * d * (c * nb / n)) / n


def table(S, clip=5.0):
    """The f32 table [m | r | clip] the kernels read."""
    _, mu, var = S
    return np.concatenate([mu.astype(np.float32), (1.0 / np.sqrt(var + EPS)).astype(np.float32),
                           np.array([clip], np.float32)])


def normalize(x, tab):
    """clamp((x - m) * r, -clip, clip) in fp32, separately rounded, NaN passing through."""
    k = (tab.size - 1) // 2
    x = np.asarray(x, dtype=np.float32)
    y = (x - tab[:k]).astype(np.float32) * tab[k:2 * k]
    clip = np.float32(tab[2 * k])
    with np.errstate(invalid="ignore"):
        return np.where(y < -clip, -clip, np.where(y > clip, clip, y)).astype(np.float32)


def hard_ring(T, n, seed=0, k=73):
    """A raw ring [T + 1][n][k] with the columns that break naive statistics: column 0 mean 1e3 / std 1e-2, column 1 constant,
    columns 2..7 0/1 flags, column 8 mean -3e4 / std 50, the rest standard normal times a per-column scale."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T + 1, n, k)) * np.exp(rng.uniform(-3, 5, k))
    x[..., 0] = 1e3 + 1e-2 * rng.standard_normal((T + 1, n))
    x[..., 1] = 0.37
    x[..., 2:8] = rng.integers(0, 2, (T + 1, n, 6))
    x[..., 8] = -3e4 + 50 * rng.standard_normal((T + 1, n))
    return x.astype(np.float32)
