"""numpy statements of the lambda-return critic target (PPO lambda_returns, csrc/value_target.hip), for the tests.

    target = adv + vd,   vd = v * s + m under a value-normalisation table (m | s | r | 0), or v without one

`lambda_targets` in float32, every op rounded on its own in the kernel's order, so the kernel is held to it bit for bit;
`lambda_targets64` the same in float64; `moments` / `combine` the float64 moments (count, mean, M2) of a batch of targets and
of a stack of moment sets combined in order.  `gae64` is the sequential float64 estimator of ppo.py:157-171 (done per step, the
recurrence unmasked), for the hand-computed cases.  Nothing here is shared with the kernels."""
import numpy as np

f32 = np.float32


def lambda_targets(adv, v, tab=None):
    """float32: (v * s) rounded, (+ m) rounded, (adv +) rounded; without a table v goes in as it is (-0 stays -0)."""
    adv, v = np.asarray(adv, f32), np.asarray(v, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        vd = v if tab is None else ((v * f32(tab[1])).astype(f32) + f32(tab[0])).astype(f32)
        return (adv + vd).astype(f32)


def lambda_targets64(adv, v, tab=None):
    adv, v = np.asarray(adv, np.float64), np.asarray(v, np.float64)
    vd = v if tab is None else v * float(tab[1]) + float(tab[0])
    return adv + vd


def moments(x):
    """(count, mean, M2) of all elements of x in float64: a two-pass mean and centred sum of squares."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size == 0:
        return 0.0, 0.0, 0.0
    mean = x.mean()
    return float(x.size), float(mean), float(((x - mean) ** 2).sum())


def combine(sets):
    """The moment sets [k][3] (count | mean | M2) combined in index order by Chan et al.'s update, empty sets skipped."""
    n, mean, m2 = 0.0, 0.0, 0.0
    for nb, mb, qb in np.asarray(sets, np.float64):
        if not nb > 0:
            continue
        if not n > 0:
            n, mean, m2 = float(nb), float(mb), float(qb)
            continue
        t, d = n + nb, mb - mean
        mean += d * (nb / t)
        m2 += qb + d * d * (n * nb / t)
        n = t
    return n, mean, m2


def gae64(reward, v, v_next, done, gamma, lam):
    """Sequential float64 GAE: delta = r + gamma v' done - v, a_t = gamma lam a_{t+1} + delta_t; all [T][N]."""
    r, v, vn, d = (np.asarray(x, np.float64) for x in (reward, v, v_next, done))
    adv = np.zeros_like(r)
    a = np.zeros(r.shape[1])
    for t in range(r.shape[0] - 1, -1, -1):
        a = gamma * lam * a + (r[t] + gamma * vn[t] * d[t] - v[t])
        adv[t] = a
    return adv
