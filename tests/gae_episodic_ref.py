"""References of the episode-aware advantage estimate (PPO gae="episodic", csrc/gae_episodic.hip), written from its definition.

Per row (t, e), from the int64 flag rows the rollout writes and the flags the env carried into it:
    ended   = reset[t][e] != 0
    timeout = ended and progress[t][e] >= max_episode_length - 1
    stale   = (reset[t-1][e] if t > 0 else ended_prev[e]) != 0
    boot = 0 if ended and not timeout else 1;  cont = 0 if ended else 1
    not stale:  tg = r + (gamma v') boot;  delta = tg - v;  a = gl (a_next cont) + delta
    stale:      tg = v;  a = 0
with v, v' replaced by v s + m under a value table (m, s).

  episodic64   sequential float64, with the first-order rounding bounds of a float32 evaluation (tests/rollout_ref.py's model:
               u = 2^-24 per rounded intermediate, errors carried through the factors gl cont) and the targets' moments
  episodic32   the same in numpy float32, every op rounded on its own, in the kernels' order: the lane = env form bit for bit
  scan_carry_bound64_masked   rollout_ref.scan_carry_bound64 restated for per-step multipliers gl live_t in {0, gl}
Nothing here is shared with the kernels; rollout_ref is imported, not edited."""
import numpy as np

from tests import rollout_ref as R

U = R.U
f32 = np.float32


def flags_of(reset, progress, ended_prev, max_episode_length):
    """(ended, timeout, stale), bool [T][N]."""
    reset, progress = np.asarray(reset), np.asarray(progress)
    ended = reset != 0
    timeout = ended & (progress >= max_episode_length - 1)
    stale = np.concatenate([(np.asarray(ended_prev) != 0).reshape(1, -1), ended[:-1]], axis=0)
    return ended, timeout, stale


class Episodic:
    """target, adv, delta [T][N] float64 (delta is 0 on stale rows: the recurrence's additive term); live [T][N] bool: the step
    hands its carry on (neither ended nor stale); target_err, bound [T][N]: first-order bounds of a float32 evaluation;
    moments = (count, mean, population var) of the targets."""


def episodic64(reward, v, v_next, reset, progress, ended_prev, max_episode_length, gamma32, gl32, table=None):
    r, v, vn = (np.asarray(x, np.float64) for x in (reward, v, v_next))
    T, N = r.shape
    g, gl = float(gamma32), float(gl32)
    ended, timeout, stale = flags_of(reset, progress, ended_prev, max_episode_length)
    boot = np.where(ended & ~timeout, 0.0, 1.0)
    cont = np.where(ended, 0.0, 1.0)
    if table is None:
        vd, vnd, ev, evn = v, vn, np.zeros((T, N)), np.zeros((T, N))
    else:
        m, s = float(table[0]), float(table[1])
        vd, vnd = v * s + m, vn * s + m
        ev, evn = U * (np.abs(v * s) + np.abs(vd)), U * (np.abs(vn * s) + np.abs(vnd))     # product and sum, rounded
    gv = g * vnd
    gvb = gv * boot
    t_live = r + gvb
    d_live = t_live - vd
    out = Episodic()
    out.target = np.where(stale, vd, t_live)
    # gamma v' and the sum are rounded (the product with boot in {0, 1} is exact); the denormalisation's error comes through
    out.target_err = np.where(stale, ev, U * (np.abs(gv) + np.abs(t_live)) + g * boot * evn)
    out.delta = np.where(stale, 0.0, d_live)
    out.live = ~(ended | stale)
    out.adv, out.bound = np.empty((T, N)), np.empty((T, N))
    a, e = np.zeros(N), np.zeros(N)
    for t in range(T - 1, -1, -1):
        glc = gl * (a * cont[t])
        al = glc + d_live[t]
        B = np.abs(gv[t]) + np.abs(gvb[t]) + np.abs(t_live[t]) + np.abs(d_live[t]) + np.abs(glc) + np.abs(al)
        el = gl * cont[t] * e + U * B + g * boot[t] * evn[t] + ev[t]
        a = np.where(stale[t], 0.0, al)
        e = np.where(stale[t], 0.0, el)
        out.adv[t], out.bound[t] = a, e
    flat = out.target.reshape(-1)
    mean = flat.mean()
    out.moments = (float(flat.size), float(mean), float(((flat - mean) ** 2).mean()))
    return out


def episodic32(reward, v, v_next, reset, progress, ended_prev, max_episode_length, table=None, gamma=0.99, lam=0.95):
    """(target, advantage) float32 [T][N]: the lane = env kernel's ops in its order."""
    r, v, vn = (np.asarray(x, f32) for x in (reward, v, v_next))
    T, N = r.shape
    g = f32(gamma)
    gl = f32(np.float64(g) * np.float64(f32(lam)))
    ended, timeout, stale = flags_of(reset, progress, ended_prev, max_episode_length)
    boot = np.where(ended & ~timeout, f32(0), f32(1)).astype(f32)
    cont = np.where(ended, f32(0), f32(1)).astype(f32)
    if table is not None:
        m, s = f32(table[0]), f32(table[1])
        v, vn = ((v * s).astype(f32) + m).astype(f32), ((vn * s).astype(f32) + m).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t_live = (r + ((g * vn).astype(f32) * boot).astype(f32)).astype(f32)
        delta = (t_live - v).astype(f32)
        adv = np.zeros((T, N), f32)
        a = np.zeros(N, f32)
        for t in range(T - 1, -1, -1):
            al = ((gl * (a * cont[t]).astype(f32)).astype(f32) + delta[t]).astype(f32)
            a = np.where(stale[t], f32(0), al).astype(f32)
            adv[t] = a
    return np.where(stale, v, t_live).astype(f32), adv


def scan_carry_bound64_masked(delta, live, gl32, lanes=64, stages=6):
    """rollout_ref.scan_carry_bound64 for the recurrence a_t = (gl live_t) a_{t+1} + delta_t: what evaluating it as a scan over
    `lanes` chunks adds to the sequential bound, [T][N].  The same three terms in the same order; every power gl^k over a run
    of steps becomes the product of the run's multipliers -- gl^k when all k steps are live, exactly 0 otherwise (the kernel's
    chunk multiplier is then an exact 0 and passes on neither a carry nor an error).  With live all True this IS
    scan_carry_bound64, value for value."""
    delta = np.asarray(delta, np.float64)
    live = np.asarray(live, bool)
    T, N = delta.shape
    gl = float(gl32)
    dead = np.concatenate([np.zeros((1, N)), np.cumsum(~live, axis=0)], axis=0)      # dead[t] = non-live steps in [0, t)

    def run(lo, hi):
        """1 where every step of [lo, hi) is live, else 0."""
        return (dead[hi] - dead[lo] == 0).astype(np.float64)

    chunks = R.scan_chunks(T, lanes)
    S, eS = [], []
    for t_lo, t_hi in chunks:
        s, e = np.zeros(N), np.zeros(N)
        for t in range(t_hi - 1, t_lo - 1, -1):
            mt = gl * live[t]
            sp = mt * s
            s = sp + delta[t]
            e = mt * e + U * (np.abs(sp) + np.abs(s))
        S.append(s)
        eS.append(e)
    extra = np.zeros((T, N))
    for c in range(1, len(chunks)):
        t_lo, t_hi = chunks[c]
        tree, mult, first = np.zeros(N), np.zeros(N), np.zeros(N)
        for j in range(c):
            dist = chunks[j][0] - t_hi
            w = gl ** dist * run(t_hi, chunks[j][0])
            tree += w * np.abs(S[j])
            mult += (dist + stages) * w * np.abs(S[j])
            first += w * eS[j]
        term = first + U * (2 * stages * tree + mult)
        for t in range(t_lo, t_hi):
            extra[t] = gl ** (t_hi - t) * run(t, t_hi) * term
    return extra
