"""float64 references of the rollout's PPO kernels (csrc/ppo_kernels.hip), written from the equations.

Plain numpy float64; nothing here is shared with oracle/ or with the kernels.  Inputs are the float32 arrays the kernels
read, promoted exactly; gamma and gamma * lambda come in as the float32 values the kernels receive (`gamma_gl32`).  Next
to every value the functions return what a test needs to bound a float32 evaluation of the same equations: the magnitudes
of the rounded intermediates, and first-order error bounds built from them with u = 2^-24 (one rounding to nearest).
"""
import numpy as np

U = 2.0 ** -24                    # unit roundoff of float32: |fl(x) - x| <= U |x|
GAE_DONE_PER_STEP, GAE_MASK_RECURRENCE, GAE_SCAN = 1, 2, 4       # include/flyhip.h: PPO_GAE_*


def gamma_gl32(gamma=0.99, lam=0.95):
    """(gamma, gamma * lambda) as the kernels see them: both arguments rounded to float32 at the ABI, their product taken in
    float64 and rounded once."""
    g, l = np.float32(gamma), np.float32(lam)
    return g, np.float32(float(g) * float(l))


# ------------------------------------------------------------------------------------------------ sampling and log-prob
def sample_logprob64(mu, var, eps):
    """a = mu + sqrt(var) eps;  log N(a; mu, diag var) = -1/2 (k log 2 pi + sum ((a - mu) / sqrt(var))^2) - 1/2 sum log var.
    mu, eps [n][k]; var [k].  Returns (a, clip(a, -1, 1), logp)."""
    mu, var, eps = (np.asarray(x, np.float64) for x in (mu, var, eps))
    L = np.sqrt(var)
    a = mu + L * eps
    x = (a - mu) / L
    k = mu.shape[1]
    logp = -0.5 * (k * np.log(2.0 * np.pi) + np.sum(x ** 2, axis=1)) - 0.5 * np.sum(np.log(var))
    return a, np.clip(a, -1.0, 1.0), logp


def logprob_cancellation64(mu, var, eps):
    """What rounding a to float32 costs the log-prob, per row.  A float32 evaluation recovers x = (a - mu) / L from the ROUNDED
    a: a carries up to 2^-24 |a| (and the subtraction sees operands of size |mu| + |a|), divided by L, and enters the
    Mahalanobis sum as 2 |x| dx:   sum_j |x_j| 2^-23 (|mu_j| + |a_j|) / L_j."""
    mu, var, eps = (np.asarray(x, np.float64) for x in (mu, var, eps))
    L = np.sqrt(var)
    a = mu + L * eps
    return np.sum(np.abs(eps) * 2.0 ** -23 * (np.abs(mu) + np.abs(a)) / L, axis=1)


def sample_action32(mu, var, eps):
    """The action as a float32 evaluation of a = mu + L eps must round it: L = fl(sqrt(var)), fl(mu + fl(L eps)), clipped.
    Elementwise, so numpy float32 is the specification."""
    mu, var, eps = (np.asarray(x, np.float32) for x in (mu, var, eps))
    L = np.sqrt(var.astype(np.float64)).astype(np.float32)
    return np.clip(mu + L * eps, np.float32(-1), np.float32(1)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- TD target and GAE
class Gae:
    """target, adv [T][N] in float64; gv = |gamma v'| (for the target's bound); B [T][N] the summed magnitudes of the six
    rounded intermediates of a step; bound [T][N] = u sum_{s >= t} (prod of the carry factors between) B_s; delta [T][N]."""


def td_gae64(reward, v, v_next, done, gamma32, gl32, mode=0):
    """tg_t = r_t + gamma v'_t d_t;  delta_t = tg_t - v_t;  A_t = gl c_t A_{t+1} + delta_t with A_T = 0, where d is done [N]
    broadcast over t (mode 0), or done [T][N] (mode & 1), and c_t = d_t with mode & 2 (the recurrence stops at episode ends),
    else 1.  A float32 evaluation rounds gamma v', (.) d, (.) + r, (.) - v, gl (c A), (.) + delta: six intermediates per step,
    each off by at most u times its magnitude; an error made at step s reaches step t < s through the factors gl c."""
    r, v, vn = (np.asarray(x, np.float64) for x in (reward, v, v_next))
    T, N = r.shape
    g, gl = float(gamma32), float(gl32)
    d = np.asarray(done, np.float64)
    d = d.reshape(T, N) if mode & GAE_DONE_PER_STEP else np.broadcast_to(d.reshape(1, N), (T, N))
    out = Gae()
    gv = g * vn
    gvd = gv * d
    out.target = r + gvd
    out.delta = out.target - v
    out.gv = np.abs(gv)
    out.adv, out.B, out.bound = np.empty((T, N)), np.empty((T, N)), np.empty((T, N))
    a, e = np.zeros(N), np.zeros(N)
    for t in range(T - 1, -1, -1):
        c = d[t] if mode & GAE_MASK_RECURRENCE else 1.0
        glc = gl * (a * c)
        a = glc + out.delta[t]
        out.B[t] = np.abs(gv[t]) + np.abs(gvd[t]) + np.abs(out.target[t]) + np.abs(out.delta[t]) + np.abs(glc) + np.abs(a)
        e = gl * c * e + U * out.B[t]
        out.adv[t], out.bound[t] = a, e
    return out


def target_bound64(g):
    """Two roundings between the float32 target and float64: gamma v' and the sum (the product with d in {0, 1} is exact)."""
    return 2.0 ** -23 * (g.gv + np.abs(g.target))


def scan_chunks(T, lanes=64):
    """The scan form's split of the time axis: `lanes` chunks of ceil(T / lanes) steps counted from the END of the rollout;
    [(t_lo, t_hi)] latest first, chunks past the data dropped."""
    L = -(-T // lanes)
    out = []
    for c in range(lanes):
        t_hi = T - c * L
        if t_hi <= 0:
            break
        out.append((max(t_hi - L, 0), t_hi))
    return out


def scan_carry_bound64(delta, gl32, lanes=64, stages=6):
    """What evaluating the GAE as a scan over `lanes` chunks adds to the sequential bound, [T][N] (modes without
    GAE_MASK_RECURRENCE).  The scan runs every chunk j from a zero carry (S_j, its value at the chunk's first step t_lo_j),
    combines S_j by A_c = sum_{j < c} gl^(t_lo_j - t_hi_c) S_j in a log-depth tree, and reruns chunk c from the carry A_c.
    Against the sequential loop the carry differs by
      * the roundings of the zero-carry pass: u (|gl s| + |s'|) per step, propagated to the chunk's first step;
      * `stages` tree levels of one multiply-add each, two roundings per level: 2 u stages sum_j gl^dist_j |S_j|;
      * the multipliers gl^dist_j, built by repeated rounded multiplication: at most dist_j + stages roundings each;
    and the error of the carry reaches step t of chunk c as gl^(t_hi_c - t).  All from float64 chunk values."""
    delta = np.asarray(delta, np.float64)
    T, N = delta.shape
    gl = float(gl32)
    chunks = scan_chunks(T, lanes)
    S, eS = [], []
    for t_lo, t_hi in chunks:
        s, e = np.zeros(N), np.zeros(N)
        for t in range(t_hi - 1, t_lo - 1, -1):
            sp = gl * s
            s = sp + delta[t]
            e = gl * e + U * (np.abs(sp) + np.abs(s))
        S.append(s)
        eS.append(e)
    extra = np.zeros((T, N))
    for c in range(1, len(chunks)):
        t_lo, t_hi = chunks[c]
        tree, mult, first = np.zeros(N), np.zeros(N), np.zeros(N)
        for j in range(c):
            dist = chunks[j][0] - t_hi
            w = gl ** dist
            tree += w * np.abs(S[j])
            mult += (dist + stages) * w * np.abs(S[j])
            first += w * eS[j]
        term = first + U * (2 * stages * tree + mult)
        for t in range(t_lo, t_hi):
            extra[t] = gl ** (t_hi - t) * term
    return extra


# ---------------------------------------------------------------------------------------------- advantage normalisation
def adv_normalise64(a, eps=1e-8):
    """(a - mean) / (std + eps), std with ddof = 1 (torch.std).  Returns (normalised, sum, mean, std)."""
    a = np.asarray(a, np.float64)
    mean, std = a.mean(), a.std(ddof=1)
    return (a - mean) / (std + eps), a.sum(), mean, std


# ------------------------------------------------------------------------------------------------------------ bookkeeping
def bookkeeping64(reward_rows, score0, scale, var0, decay, var_min):
    """score += mean(row) * scale for every row of reward_rows [rows][n], in float64 from the float32 inputs;
    var <- max(var_min, var - decay) once per row (skipped when decay <= 0) in numpy float32: elementwise, so bit-exact.
    Returns (score, tol, var): tol is what a float32 tree reduction in 1024 lanes may be off by, per row added
        (n / 1024 + 16) u sum|r| / n |scale|  (n / 1024 sequential adds per lane, then 6 + 4 + 1 tree levels and the
        division and the product, rounded up to 16)  +  2 u |score| (the term's product and the running sum)."""
    rows = np.asarray(reward_rows, np.float64)
    n = rows.shape[1]
    score, tol = float(np.float32(score0)), 0.0
    sc = float(np.float32(scale))
    var = np.array(var0, np.float32, copy=True)
    dec, vmin = np.float32(decay), np.float32(var_min)
    for row in rows:
        score += row.mean() * sc
        tol += (n / 1024 + 16) * U * np.abs(row).sum() / n * abs(sc) + 2 * U * abs(score)
        if dec > 0:
            var = np.maximum(vmin, (var - dec).astype(np.float32))
    return score, tol, var
