"""Running reward scaling (PPO --normalize_reward) restated in numpy from the definition, not from the kernels.

Per env e, with the carry G[e] (float64, the discounted return of the env's open episode) living across rollouts, rows walked
forward in time, g = float64(float32(gamma)):

    G = fl(fl(g * G) + float64(reward[t][e]))     two separately rounded float64 ops (numpy does not fuse them)
    the moments take G                            every (t, e) counts, the step that performs a reset too
    reset[t][e] != 0:  G = 0

`walk` is that loop, sequential in t (all envs of a row at once: the same two ops per env in the same order, so a kernel that
walks forward is held to it bit for bit).  Beside every G it carries the quantity a bound on ANY re-association is made of:

    M = g * M + |reward[t][e]|     from M = |carry in|, M = 0 behind an end         (|G| <= M at every step)
    S = the largest M since the env's last end (the carry-in's |.| included while no end has come)

The scaled reward is float32: rs = clip(reward * r, -c, +c) with r = float32(1 / sqrt(var + 1e-5)), one rounded multiply.

The bound on a scan's carry (one wave per env, time on 64 lanes; `scan_walk` restates its arithmetic).  u = 2^-53; n steps
since the env's last end, exact return X_n, everything to first order in u (the factor 1.001 below covers the second-order
terms, which are smaller by u / (1 - g) < 2^-40):

  sequential ops   A walk from any start computes G^_t = (g G^_{t-1} (1 + d1) + r_t)(1 + d2), |d| <= u, so its error obeys
                   e_t = g e_{t-1} + (terms of size <= u g |G_{t-1}| + u |G_t| <= 2 u M_t), and |e_n| <= 2 u sum_j g^(n-j) M_j
                   <= 2 u S / (1 - g).  That holds for the sequential reference (2 / (1 - g)) and, chunk by chunk with the
                   chunks' weights g^(steps behind the chunk), for the scan's pass 1 (another 2 / (1 - g)).
  g^len            A chunk's multiplier is g^len by len multiplications: relative error <= len u.  The weight of a reward
                   r_k in the carry is a product of such multipliers with exponents adding to at most n - k, so these errors
                   add up to at most u sum_k (n - k) g^(n-k) |r_k| (the carry-in counting as r_0)
                   = u sum_{j>=1} g^j M_(n-j) <= u S g / (1 - g)   (summation by parts).
                   Term by term len g^len <= 1 / (e ln(1 / g)), which is what the carry-in's own term is held to once more.
  scan levels      Kogge-Stone over 64 lanes has 6 levels.  At a level a lane's b takes one rounded multiply and one rounded
                   add (2 roundings on everything the lane covers), and the multipliers it meets on its way are products of
                   at most 63 chunk multipliers with at most 63 rounded multiplies between them: at most 12 + 63 <= 6 * 13
                   relative roundings on every term of the carry, whose magnitudes add up to at most S.
  the last apply   carry = fl(fl(a * carry_in) + b): 2 more.

  c(g) = 4 / (1 - g) + g / (1 - g) + 1 / (e ln(1 / g)) + 6 * 13 + 2        |scan carry - walk carry| <= 1.001 c(g) u S

An end passes on exactly nothing, so S = 0 (the last row is an end) admits only the exact carry 0.
"""
import collections
import fractions
import math

import numpy as np

EPS = 1e-5
U = 2.0 ** -53                                   # unit roundoff of float64
f32 = np.float32

# G [T][N]: the value the moments take at every row; carry [N]: G behind the last row; mag [T][N]: M beside every G;
# smax [N]: S of the carry
Walk = collections.namedtuple("Walk", "G carry mag smax")


def discount(gamma):
    """The entry point takes gamma as a float: g = (double)(float)gamma."""
    return np.float64(f32(gamma))


def walk(reward, reset, gamma, carry=None):
    """The definition over reward f32 [T][N] and the int64 reset rows; the carry defaults to zero."""
    reward, reset = np.asarray(reward), np.asarray(reset)
    T, N = reward.shape
    assert reward.dtype == np.float32 and reset.shape == (T, N)
    g = discount(gamma)
    r64 = reward.astype(np.float64)
    G = np.zeros(N) if carry is None else np.array(carry, dtype=np.float64)
    M = np.abs(G)
    S = M.copy()
    out, mag = np.empty((T, N)), np.empty((T, N))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            G = g * G                            # rounded
            G = G + r64[t]                       # rounded
            M = g * M + np.abs(r64[t])
            S = np.fmax(S, M)
            out[t], mag[t] = G, M
            ended = reset[t] != 0
            G = np.where(ended, 0.0, G)
            M = np.where(ended, 0.0, M)
            S = np.where(ended, 0.0, S)
    return Walk(out, G, mag, S)


def exact_walk(reward, reset, gamma, carry=None):
    """The same walk in exact rational arithmetic (tiny inputs): -> (G [T][N], carry [N]) of fractions.Fraction."""
    reward, reset = np.asarray(reward), np.asarray(reset)
    T, N = reward.shape
    g = fractions.Fraction(float(discount(gamma)))
    G = [fractions.Fraction(0) if carry is None else fractions.Fraction(float(carry[e])) for e in range(N)]
    out = [[None] * N for _ in range(T)]
    for t in range(T):
        for e in range(N):
            G[e] = g * G[e] + fractions.Fraction(float(reward[t, e]))
            out[t][e] = G[e]
            if reset[t, e] != 0:
                G[e] = fractions.Fraction(0)
    return out, G


def scan_c(gamma):
    """c(g) of the module's derivation."""
    g = float(discount(gamma))
    return 4.0 / (1.0 - g) + g / (1.0 - g) + 1.0 / (math.e * math.log(1.0 / g)) + 6 * 13 + 2


def scan_bound(gamma, smax):
    """|scan carry - walk carry| per env, from the walk's S."""
    return 1.001 * scan_c(gamma) * U * np.asarray(smax, dtype=np.float64)


def chunk_map(reward, reset, g, lo, hi, e):
    """Rows [lo, hi) of env e as the affine map G_out = a * G_in + b: a = g^len without an end, a = 0 and b the return behind
    the last end otherwise; every op rounded on its own."""
    a, b = np.float64(1.0), np.float64(0.0)
    for t in range(lo, hi):
        b = np.float64(g * b) + np.float64(reward[t, e])
        a = np.float64(a * g)
        if reset[t, e] != 0:
            a, b = np.float64(0.0), np.float64(0.0)
    return a, b


def compose(first, then):
    """(a1, b1) then (a2, b2) = (a1 a2, a2 b1 + b2); a2 == 0 passes on exactly nothing."""
    (a1, b1), (a2, b2) = first, then
    if a2 == 0.0:
        return a2, b2
    return np.float64(a1 * a2), np.float64(np.float64(a2 * b1) + b2)


def scan_walk(reward, reset, gamma, carry=None, lanes=64):
    """The scan's arithmetic: `lanes` chunks of L = ceil(T / lanes) rows (lanes past T hold the identity), a Kogge-Stone
    inclusive scan of their maps, every chunk walked again from the return that enters it.  -> (G [T][N], carry [N])."""
    reward, reset = np.asarray(reward), np.asarray(reset)
    T, N = reward.shape
    g = discount(gamma)
    L = -(-T // lanes)
    cin = np.zeros(N) if carry is None else np.array(carry, dtype=np.float64)
    G, out = np.empty((T, N)), np.empty(N)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(N):
            lo = [min(l * L, T) for l in range(lanes)]
            hi = [min(x + L, T) for x in lo]
            x = [chunk_map(reward, reset, g, lo[l], hi[l], e) for l in range(lanes)]
            o = 1
            while o < lanes:
                x = [compose(x[l - o], x[l]) if l >= o else x[l] for l in range(lanes)]
                o <<= 1

            def apply(m):
                return np.float64(np.float64(m[0] * cin[e]) + m[1]) if m[0] != 0.0 else m[1]

            for l in range(lanes):
                cur = apply(x[l - 1]) if l else cin[e]
                for t in range(lo[l], hi[l]):
                    cur = np.float64(g * cur) + np.float64(reward[t, e])
                    G[t, e] = cur
                    if reset[t, e] != 0:
                        cur = np.float64(0.0)
            out[e] = apply(x[lanes - 1])
    return G, out


def moments(x):
    """(count, mean, population var) of all elements of x in float64: a two-pass mean and centred sum of squares."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    mean = x.mean()
    return float(x.size), float(mean), float(((x - mean) ** 2).mean())


def merge(S, x):
    """S_r = (count, mean, var) after the returns x are folded in: the moments of everything S covers plus these."""
    c, mu, var = S
    nb, mb, vb = moments(x)
    n = c + nb
    d = mb - mu
    return n, mu + d * (nb / n), (var * c + vb * nb + d * d * (c * nb / n)) / n


def table(S):
    """The f32 table m | s | r | 0 of S_r: each entry computed in float64 and rounded once."""
    _, mu, var = S
    sd = np.sqrt(np.float64(var) + EPS)
    return np.array([mu, sd, 1.0 / sd, 0.0], dtype=np.float64).astype(f32)


def scale(reward, r, clip):
    """clip(reward * r, -clip, +clip) in float32: one rounded multiply, NaN passes through."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip((np.asarray(reward, f32) * f32(r)).astype(f32), -f32(clip), f32(clip)).astype(f32)
