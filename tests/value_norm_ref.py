"""numpy statements of value normalisation (PPO normalize_value), for the tests.

Statistics in float64: S_v = (count, mean, var) with population variance, initially (0, 0, 1); a merge of a batch of targets
replaces S_v by the statistics of every target seen so far.  The table and the two maps in float32, every op rounded on its
own (numpy float32 arithmetic does that), in the order the kernels use -- so the kernels can be held to them bit for bit."""
import numpy as np

EPS = 1e-5
f32 = np.float32


def initial():
    return 0.0, 0.0, 1.0


def moments(x):
    """(count, mean, population var) of all elements of x in float64: a two-pass mean and centred sum of squares."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    mean = x.mean()
    return float(x.size), float(mean), float(((x - mean) ** 2).mean())


def merge(S, x):
    """S after a merge of the targets x: the moments of everything S covers plus these."""
    c, mu, var = S
    nb, mb, vb = moments(x)
    if nb == 0:
        return S
    n = c + nb
    d = mb - mu
    return n, mu + d * (nb / n), (var * c + vb * nb + d * d * (c * nb / n)) / n


def table(S):
    """The f32 table m | s | r | 0: each entry computed in float64 and rounded once."""
    _, mu, var = S
    sd = np.sqrt(np.float64(var) + EPS)
    return np.array([mu, sd, 1.0 / sd, 0.0], dtype=np.float64).astype(np.float32)


def denormalize(v, tab):
    """v * s + m in fp32, two separately rounded ops."""
    return (np.asarray(v, f32) * f32(tab[1])).astype(f32) + f32(tab[0])


def normalize(tg, tab):
    """(tg - m) * r in fp32, two separately rounded ops, no clamp; NaN passes through."""
    with np.errstate(invalid="ignore"):
        return ((np.asarray(tg, f32) - f32(tab[0])).astype(f32) * f32(tab[2])).astype(f32)


def td_gae(reward, v, v_next, done, tab, gamma=0.99, lam=0.95, mode=0):
    """The lane = env GAE pass in float32 (ppo.py:157-171 with v / v_next denormalised under `tab`): mode bit 0 = done is
    [T][N] instead of [N], bit 1 = the recurrence is masked by done.  Returns (target, advantage), both [T][N], reward units."""
    reward, v, v_next, done = (np.asarray(a, f32) for a in (reward, v, v_next, done))
    T, N = reward.shape
    g = f32(gamma)
    gl = f32(np.float64(g) * np.float64(f32(lam)))          # the entry point takes gamma and lambda as floats
    vd, vdn = denormalize(v, tab), denormalize(v_next, tab)
    d = done if mode & 1 else np.broadcast_to(done.reshape(1, N), (T, N))
    target = reward + ((g * vdn).astype(f32) * d).astype(f32)
    delta = (target - vd).astype(f32)
    adv = np.zeros((T, N), f32)
    a = np.zeros(N, f32)
    for t in range(T - 1, -1, -1):
        carry = (a * d[t]).astype(f32) if mode & 2 else a
        a = ((gl * carry).astype(f32) + delta[t]).astype(f32)
        adv[t] = a
    return target.astype(f32), adv


def hard_rewards(kind, T, n, seed=0):
    """Rewards that break naive statistics (with v_next = 0 and m = 0 the TD target IS the reward): "a" mean 1e3 / std 1e-2,
    "b" constant 0.37, "c" mean -3e4 / std 50."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((T, n))
    return {"a": 1e3 + 1e-2 * z, "b": np.full((T, n), 0.37), "c": -3e4 + 50 * z}[kind].astype(np.float32)
