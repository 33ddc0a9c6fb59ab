"""numpy restatement of per-env physics domain randomisation (include/flyhip.h, fly_set_randomization): lowbias32, the
draw of (seed, e, k, j) and the multiplier rule, in uint32 (wrapping) and float32."""
import numpy as np

NAMES = ("kp", "kd", "effort", "mass", "mu", "gravity")
GOLDEN = np.uint32(0x9E3779B9)


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def uniforms(seed, e, k):
    """u [len(e), 6] float32 in [0, 1) of env indices e (array) at draw counts k (array or scalar)."""
    e = np.asarray(e, dtype=np.uint32)
    k = np.broadcast_to(np.asarray(k, dtype=np.uint32), e.shape)
    with np.errstate(over="ignore"):
        key = lowbias32(np.uint32(int(seed) % (1 << 32)) ^ lowbias32(e))
        ctr = lowbias32(key + k)
        u = np.empty(e.shape + (6,), np.float32)
        for j in range(6):
            h = lowbias32(ctr + GOLDEN * np.uint32(j + 1))
            u[..., j] = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u


def bounds(ranges):
    lo = np.array([ranges.get(n, (1.0, 1.0))[0] for n in NAMES], np.float32)
    hi = np.array([ranges.get(n, (1.0, 1.0))[1] for n in NAMES], np.float32)
    return lo, hi


def multipliers(ranges, seed, e, k):
    """m [len(e), 6] float32: lo + (hi - lo) * u, each op rounded to float32."""
    lo, hi = bounds(ranges)
    u = uniforms(seed, e, k)
    return (lo + ((hi - lo) * u).astype(np.float32)).astype(np.float32)


def env_config(cfg, m):
    """A copy of oracle config `cfg` for ONE env running on multipliers m[6] (num_envs = 1): the fp32 products."""
    c = type(cfg).from_buffer_copy(cfg)
    c.num_envs = 1
    f = np.float32
    c.kp = float(f(cfg.kp) * f(m[0]))
    c.kd = float(f(cfg.kd) * f(m[1]))
    c.effort = float(f(cfg.effort) * f(m[2]))
    c.mass = float(f(cfg.mass) * f(m[3]))
    for i in range(3):
        c.inertia[i] = float(f(cfg.inertia[i]) * f(m[3]))
    c.mu = float(f(cfg.mu) * f(m[4]))
    c.gravity = float(f(cfg.gravity) * f(m[5]))
    return c
