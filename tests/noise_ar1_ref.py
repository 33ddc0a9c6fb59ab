"""Reference of the AR(1) exploration noise (PPO action_noise="ar1"), written from the definition in include/flyhip.h and not
from the kernel: float32 numpy, every operation rounded on its own.

    s        = float32(sqrt(1 - float64(rho32)^2))          rho32 = float32(rho), what the C ABI receives
    y[-1][c] = carry[c]
    y[t][c]  = float32(float32(rho32 * y[t-1][c]) + float32(s * x[t][c]))
    carry'   = y[T-1]
"""
import numpy as np


def scale(rho):
    """s of the definition: formed in float64 from the float32 rho, rounded once."""
    r = float(np.float32(rho))
    return np.float32(np.sqrt(1.0 - r * r))


def ar1(x, carry, rho):
    """x float32 [T, C] (or [T, N, 18]: columns are the trailing axes), carry float32 of one row's shape.  Returns (y, carry'),
    new arrays; the inputs are left as they are."""
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[0]
    rows = x.reshape(T, -1)
    rho32, s = np.float32(rho), scale(rho)
    y = np.empty_like(rows)
    prev = np.asarray(carry, dtype=np.float32).reshape(-1).copy()
    assert prev.shape[0] == rows.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            a = (rho32 * prev).astype(np.float32)
            b = (s * rows[t]).astype(np.float32)
            prev = (a + b).astype(np.float32)
            y[t] = prev
    return y.reshape(x.shape), prev.reshape(np.shape(carry)).copy()


def stats(y, lags=(1, 5)):
    """Pooled moments of y [T, C] over all columns: mean, variance, and the lag-k autocorrelations along time (about zero, the
    process' known mean, in float64)."""
    y = np.asarray(y, dtype=np.float64)
    var = float((y * y).mean())
    return float(y.mean()), float(y.var()), [float((y[k:] * y[:-k]).mean() / var) for k in lags]
