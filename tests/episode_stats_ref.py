"""Episode statistics (PPO --episode_stats) restated in numpy from the definitions, not from the kernels.

Per env e, with the carries carry_ret (float64) and carry_len (int64) living across rollouts, rows walked forward in time:

    carry_ret += float64(reward[t][e]);  carry_len += 1
    reset[t][e] != 0:  an episode closes with return carry_ret, length carry_len,
                       timeout = progress[t][e] >= max_episode_length - 1;  carry_ret = 0, carry_len = 0

Every step counts, the one that performs the reset too.  `walk` is that loop, sequential in t (all envs of a row at once: the
same float64 additions per env in the same order).  Beside the sequentially rounded return every episode carries the correctly
rounded one (math.fsum over the carry-in and its rewards), the sum of their magnitudes and the number of summands: what a
bound on ANY order of summation is made of.  A set is SET doubles:

    n | ret_mean | ret_M2 | ret_min | ret_max | len_sum | len_min | len_max | timeouts | rows
"""
import collections
import math

import numpy as np

SET = 10
N_, MEAN, M2, RMIN, RMAX, LSUM, LMIN, LMAX, TIMEOUTS, ROWS = range(SET)
U = 2.0 ** -53                                   # unit roundoff of float64

# ret: the sequential float64 sum (the definition, op for op); exact: the correctly rounded sum of the same summands;
# abs_sum: the sum of their magnitudes; terms: how many there are (the steps, plus one for a non-zero carry-in)
Episode = collections.namedtuple("Episode", "env t ret exact length timeout abs_sum terms")
Walk = collections.namedtuple("Walk", "episodes carry_ret carry_len carry_exact carry_abs carry_terms")


def walk(reward, reset, progress, max_episode_length, carry_ret=None, carry_len=None):
    """The definitions over reward f32 [T][N] and the int64 flag rows; carries default to zero.  Returns a Walk: the closed
    episodes ordered by (t, env) and, per env, the carries out with their correctly rounded value, magnitude sum and summand
    count."""
    reward, reset, progress = np.asarray(reward), np.asarray(reset), np.asarray(progress)
    T, N = reward.shape
    assert reward.dtype == np.float32 and reset.shape == progress.shape == (T, N)
    r64 = reward.astype(np.float64)
    cr = np.zeros(N) if carry_ret is None else np.array(carry_ret, dtype=np.float64)
    cl = np.zeros(N, np.int64) if carry_len is None else np.array(carry_len, dtype=np.int64)
    cin = cr.copy()                              # the carry-in, while it is still inside the env's open episode
    start = np.zeros(N, np.int64)                # the first row of the env's open episode inside this walk
    limit = int(max_episode_length) - 1
    episodes = []

    def summands(e, stop):
        seg = r64[start[e]:stop, e].tolist()
        return ([float(cin[e])] if cin[e] != 0 or math.isnan(cin[e]) else []) + seg

    for t in range(T):
        cr = cr + r64[t]
        cl = cl + 1
        for e in np.flatnonzero(reset[t] != 0):
            x = summands(e, t + 1)
            episodes.append(Episode(int(e), t, float(cr[e]), math.fsum(x) if np.isfinite(x).all() else float("nan"), int(cl[e]),
                                    bool(progress[t, e] >= limit), math.fsum(abs(v) for v in x), len(x)))
            cr[e], cl[e], cin[e], start[e] = 0.0, 0, 0.0, t + 1
    exact, mags, terms = np.zeros(N), np.zeros(N), np.zeros(N, np.int64)
    for e in range(N):
        x = summands(e, T)
        exact[e] = math.fsum(x) if np.isfinite(x).all() else float("nan")
        mags[e], terms[e] = math.fsum(abs(v) for v in x), len(x)
    return Walk(episodes, cr, cl, exact, mags, terms)


def empty_set(rows=0):
    return np.array([0.0, 0.0, 0.0, np.inf, -np.inf, 0.0, np.inf, 0.0, 0.0, float(rows)])


def set_of(episodes, rows, key="exact"):
    """The set of `episodes` over `rows` walked rows: mean and M2 by math.fsum, so to one rounding each."""
    s = empty_set(rows)
    n = len(episodes)
    if n == 0:
        return s
    ret = [getattr(ep, key) for ep in episodes]
    lens = [ep.length for ep in episodes]
    mean = math.fsum(ret) / n
    s[:ROWS] = (n, mean, math.fsum((x - mean) ** 2 for x in ret), min(ret), max(ret), sum(lens), min(lens), max(lens),
                sum(ep.timeout for ep in episodes))
    return s


def pool(sets):
    """The pooled set of several sets (their order does not matter here): counts, sums and extremes exactly, the mean as the
    count-weighted mean and M2 = sum M2_i + sum n_i (mean_i - mean)^2, both by math.fsum."""
    sets = np.asarray(sets, dtype=np.float64).reshape(-1, SET)
    out = empty_set(sets[:, ROWS].sum())
    full = sets[sets[:, N_] > 0]
    n = full[:, N_].sum()
    if n == 0:
        return out
    mean = math.fsum(full[:, N_] * full[:, MEAN]) / n
    out[:ROWS] = (n, mean, math.fsum(full[:, M2]) + math.fsum(full[:, N_] * (full[:, MEAN] - mean) ** 2), full[:, RMIN].min(),
                  full[:, RMAX].max(), full[:, LSUM].sum(), full[:, LMIN].min(), full[:, LMAX].max(), full[:, TIMEOUTS].sum())
    return out


def conservation_gap(reward, w, carry_in=None):
    """Per env: |(sum of closed returns) + carry out - carry in - (float64 sum of the env's rewards)|, everything by math.fsum
    over the walk's sequentially rounded values, and the bound the roundings of those values allow: every return and carry is
    a recursive sum, off by at most terms * U * abs_sum."""
    reward = np.asarray(reward)
    T, N = reward.shape
    cin = np.zeros(N) if carry_in is None else np.asarray(carry_in, dtype=np.float64)
    gap, bound = np.zeros(N), np.zeros(N)
    closed = [[] for _ in range(N)]
    for ep in w.episodes:
        closed[ep.env].append(ep)
    for e in range(N):
        total = math.fsum(reward[:, e].astype(np.float64).tolist())
        got = math.fsum([ep.ret for ep in closed[e]] + [float(w.carry_ret[e]), -float(cin[e])])
        gap[e] = abs(got - total)
        bound[e] = U * (sum(ep.terms * ep.abs_sum for ep in closed[e]) + w.carry_terms[e] * w.carry_abs[e])
    return gap, bound


def return_bound(ep_or_terms, abs_sum=None):
    """terms * 2^-53 * sum |summand|: the recursive-summation bound, which holds for every order of adding the summands."""
    if abs_sum is None:
        return ep_or_terms.terms * U * ep_or_terms.abs_sum
    return ep_or_terms * U * abs_sum
