"""TEST INFRASTRUCTURE: plain-numpy restatement of the env's two packs, tables that land on every hard branch of
them, and one-decision mutants of the restatement.  Shares no code with oracle/ (and must not import it).

  obs_ref     fly.py:771-805 with compute_heading_and_up, compute_rot, get_euler_xyz, unscale   (kernel K4)
  reward_ref  fly.py:413-443, :685-768, both reward_modes                                       (kernel K5)

Both evaluate in float64 on the fp32 inputs.  The DECIDING quantities are the exception: each is one or two correctly
rounded fp32 operations in the reference program, so they are formed in np.float32, every operation rounded: z,
ori = fl(fl(qz qz) + fl(qw qw)), the per-body contact sums fl(fl(fx + fy) + fz), the abdomen sum added in body order
from 0, fl(hi 0.9f) and fl(lo 0.9f), heading_proj (read from the obs row) and progress.  Constants the reference
program holds in fp32 (2 pi, pi/2, 0.8, 1e-9, dt, the config) enter as the float64 value of that fp32 number.

`cfg` is any object with the config's attribute names (oracle.params.OrcConfig and the product's FlyConfig both do).

Mutants: `mutant=` changes ONE decision.  A table pins a decision when the mutant's output leaves the unmutated
one's by more than the test's bound on some row.  EQUIVALENT_MUTANTS lists the mutants that no table can tell from
the unmutated program, with the reason; the CPU test holds them to be output-identical AT the decision point.
"""
import numpy as np

F = np.float32
NDOF, NOBS, NLEG, NABD, NCON = 18, 73, 6, 5, 11
EXACT_COLS = [0] + list(range(48, 66)) + list(range(67, 73))
ANGLE_COLS = (7, 8, 9, 66)
TWO_PI32 = float(F(2.0 * np.pi))       # `% (2 * np.pi)` on an fp32 tensor: the scalar is held in fp32
HALF_PI32 = float(F(np.pi / 2.0))      # copysign(np.pi / 2.0, sinp) builds an fp32 tensor
U32 = 2.0 ** -24

REWARD_MUTANTS = (
    "z_lo_le", "z_hi_ge", "up14_ge", "up21_le", "ori98_ge", "ori50_le", "abd_ge", "abd_ne", "abd_onesum",
    "touch_ge", "touch_ne", "lim_hi_ge", "lim_lo_le", "lim_hi_only", "heading_ge", "prog0_keep", "prog_gt", "prog_max")
OBS_MUTANTS = (
    "sinp_gt", "pitch_asin_clip", "pitch_asin_noclip", "nrm_le", "nrm_noclamp", "pymod_nowrap", "pymod_le", "walk_y",
    "touch_ge", "touch_ne")
EQUIVALENT_MUTANTS = {
    # the reward is continuous across this threshold: at heading_proj == fp32(0.8) the other arm is
    # heading_weight * 0.8f / 0.8f == heading_weight exactly
    "heading_ge": "both arms give heading_weight at heading_proj == 0.8f",
    # at |sinp| == 1 the other arm is asin(+-1) == +-pi/2 (to 4e-8: the fp32 constant); beyond 1 clip() makes it so
    "sinp_gt": "asin(+-1) is +-pi/2, the value of the branch",
    "pitch_asin_clip": "asin(clip(sinp)) is +-pi/2 wherever the branch is taken",
    # x / clamp(nrm, min=1e-9): at nrm == 1e-9 both arms divide by 1e-9
    "nrm_le": "both arms divide by 1e-9 at nrm == 1e-9",
}


def _cfg_vec(cfg, name, n=None):
    v = getattr(cfg, name)
    return np.array(v[:] if n is None else v[:n], dtype=F)


def body_sums32(contact):
    """[n, 11, 3] fp32 -> [n, 11] fp32: fl(fl(fx + fy) + fz), fly.py:744, :756, :797 (`.sum(1)` over three components)."""
    c = np.asarray(contact, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return (c[..., 0] + c[..., 1]) + c[..., 2]


def abdomen_sum32(contact, onesum=False):
    c = np.asarray(contact, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if onesum:                                     # mutant: the 15 components as one running sum
            flat = c[:, :NABD].reshape(c.shape[0], NABD * 3)
            s = np.zeros(c.shape[0], F)
            for k in range(NABD * 3):
                s = s + flat[:, k]
            return s
        b = body_sums32(c)
        s = np.zeros(c.shape[0], F)
        for k in range(NABD):                          # body order from 0
            s = s + b[:, k]
        return s


def ori32(root):
    q = np.asarray(root, F)
    return q[:, 5] * q[:, 5] + q[:, 6] * q[:, 6]      # fly.py:728, two fp32 products and one fp32 add


def _touching(contact, mutant):
    s = body_sums32(contact)[:, NABD:]
    with np.errstate(invalid="ignore"):
        if mutant == "touch_ge":
            return s >= 0
        if mutant == "touch_ne":
            return s != 0
        return s > 0


# ---- K5 -----------------------------------------------------------------------------------------------------------
def reward_ref(cfg, obs, targets, root, contact, pot, prev_pot, progress, reset, reward_mode=None, add_progress=0,
               mutant=None):
    """fly.py:413-443, :685-768.  Returns a dict: reward (float64), reset, progress (int64), dead, mag (the sum of the
    absolute values of the reward's elementary terms) and the deciding quantities (for the coverage conditions)."""
    assert mutant is None or mutant in REWARD_MUTANTS, mutant
    mode = int(cfg.reward_mode) if reward_mode is None else int(reward_mode)
    obs32 = np.asarray(obs, F)
    n = obs32.shape[0]
    hi, lo = _cfg_vec(cfg, "dof_hi"), _cfg_vec(cfg, "dof_lo")
    uw, hw = float(F(cfg.up_weight)), float(F(cfg.heading_weight))
    acs, ecs = float(F(cfg.actions_cost_scale)), float(F(cfg.energy_cost_scale))
    jal, death = float(F(cfg.joints_at_limit_cost_scale)), float(F(cfg.death_cost))
    th, thup = F(cfg.termination_height), F(cfg.termination_height_up)
    progress = np.asarray(progress, np.int64).copy()
    if add_progress:
        progress = progress + 1                                            # fly.py:678
    if mutant != "prog0_keep":
        progress[progress == 0] = 1                                        # :415-416
    z = obs32[:, 0]
    hp = obs32[:, 11]
    act = np.asarray(targets, F).astype(np.float64)
    oact32 = obs32[:, 48:66]
    oact = oact32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        hp_over = (hp >= F(0.8)) if mutant == "heading_ge" else (hp > F(0.8))
        heading_r = np.where(hp_over, hw, hw * hp.astype(np.float64) / float(F(0.8)))      # :715-716
        up_add = (z >= F(1.4)) if mutant == "up14_ge" else (z > F(1.4))                    # :719-721
        up_sub = (z <= F(2.1)) if mutant == "up21_le" else (z < F(2.1))
        up_r = np.where(up_add, uw, 0.0) - np.where(up_sub, uw, 0.0)
        ori = ori32(root)
        orient_r = np.where((ori >= F(0.98)) if mutant == "ori98_ge" else (ori > F(0.98)), uw, 0.0)      # :728
        hi9 = hi * F(0.9)
        lo9 = lo if mutant == "lim_hi_only" else lo * F(0.9)
        over = (oact32 >= hi9) if mutant == "lim_hi_ge" else (oact32 > hi9)                # :736-737
        under = (oact32 <= lo9) if mutant == "lim_lo_le" else (oact32 < lo9)
        lim = over.sum(1) + under.sum(1)
        touching = _touching(contact, mutant).sum(1)                                       # :744
        abd = abdomen_sum32(contact, onesum=(mutant == "abd_onesum"))                      # :756
        d_lo = (z <= th) if mutant == "z_lo_le" else (z < th)
        d_hi = (z >= thup) if mutant == "z_hi_ge" else (z > thup)
        d_ori = (ori <= F(0.5)) if mutant == "ori50_le" else (ori < F(0.5))
        d_abd = (abd >= 0) if mutant == "abd_ge" else ((abd != 0) if mutant == "abd_ne" else (abd > 0))
    acost_t = act * act                                                    # :732
    elec_t = np.abs(act - oact)                                            # :733
    acost, elec = acost_t.sum(1), elec_t.sum(1)
    progress_r = np.asarray(pot, F).astype(np.float64) - np.asarray(prev_pot, F).astype(np.float64)      # :741
    leg_r = touching * float(F(0.1))
    if mode == 0:                                                          # :750
        summands = [np.full(n, 0.5), up_r * orient_r, -ecs * elec, -lim * jal, leg_r]
        mag = ecs * elec
    else:                                                                  # :747-748
        summands = [progress_r * 2.0, np.full(n, 0.5), up_r * orient_r, heading_r, -acs * acost, -ecs * elec, -lim * jal]
        mag = ecs * elec + acs * acost
    total = np.zeros(n)
    for s in summands:
        total = total + s
        mag = mag + np.abs(s)
    dead = d_lo | d_hi | d_ori | d_abd                                     # :753-756
    total = np.where(dead, death, total)
    lim_prog = int(cfg.max_episode_length) - (0 if mutant == "prog_max" else 1)
    timeout = (progress > lim_prog) if mutant == "prog_gt" else (progress >= lim_prog)      # :761
    rs = np.asarray(reset, np.int64).copy()
    rs[dead | timeout] = 1                                                 # :759-766
    return dict(reward=total, reset=rs, progress=progress, dead=dead, mag=mag, d_lo=d_lo, d_hi=d_hi, d_ori=d_ori,
                d_abd=d_abd, timeout=timeout, lim=lim, touching=touching, ori=ori, abd=abd, up_r=up_r)


def reward_bound(mag):
    """16 * 2^-24 * mag: 16 = the fp32 roundings on the longest path from an input to `total` in the kernel and in the
    oracle alike (one product or difference, the in-lane adds, the cross-lane levels, one scale product, up to six
    adds of `total`); a wrong branch moves the reward by 0.1 (leg_reward) to 2.5 (death_cost)."""
    return 16.0 * U32 * mag


# ---- K4 -----------------------------------------------------------------------------------------------------------
def _quat_mul(a, b):
    x1, y1, z1, w1 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    x2, y2, z2, w2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    w = qq - ww + (z1 - y1) * (y2 - z2)
    x = qq - xx + (x1 + w1) * (x2 + w2)
    y = qq - yy + (w1 - x1) * (y2 + z2)
    z = qq - zz + (z1 + y1) * (w2 - x2)
    return np.stack([x, y, z, w], axis=-1)


def _quat_rotate(q, v, sign):
    qw = q[:, 3:4]
    qv = q[:, :3]
    a = v * (2.0 * qw ** 2 - 1.0)
    b = np.cross(qv, v) * qw * 2.0
    c = qv * (qv * v).sum(-1, keepdims=True) * 2.0
    return a + sign * b + c


def _py_mod(a, b, mutant):
    m = np.fmod(a, b)
    if mutant == "pymod_nowrap":
        return m
    neg = (m <= 0.0) if mutant == "pymod_le" else ((m != 0.0) & (m < 0.0))
    return np.where(neg, m + b, m)


def obs_ref(cfg, root, dof_pos, dof_vel, targets, contact, pot, mutant=None):
    """fly.py:771-805.  Returns a dict: obs [n, 73], pot, prev_pot, up_vec, heading_vec (float64) and the deciding
    quantities sinp and nrm in float64 and as the fp32 program forms them (sinp32, nrm32), for the coverage conditions."""
    assert mutant is None or mutant in OBS_MUTANTS, mutant
    r32 = np.asarray(root, F)
    r = r32.astype(np.float64)
    n = r.shape[0]
    tgt = _cfg_vec(cfg, "target").astype(np.float64)
    dt = float(F(cfg.dt))
    hi, lo = _cfg_vec(cfg, "dof_hi").astype(np.float64), _cfg_vec(cfg, "dof_lo").astype(np.float64)
    tt = np.stack([tgt[0] - r[:, 0], tgt[1] - r[:, 1], np.zeros(n)], axis=-1)          # :783-784
    prev_pot = np.asarray(pot, F).astype(np.float64).copy()                            # :786
    nrm = np.sqrt((tt * tt).sum(-1))
    new_pot = -nrm / dt                                                                # :787
    eps = float(F(1e-9))
    with np.errstate(invalid="ignore", divide="ignore"):
        if mutant == "nrm_noclamp":
            dn = nrm
        else:
            dn = np.where((nrm <= eps) if mutant == "nrm_le" else (nrm < eps), eps, nrm)   # normalize()
        td = tt / dn[:, None]
    inv_start = np.tile(np.array([-0.0, -0.0, -0.0, 1.0]), (n, 1))                     # fly.py:129, :217
    tq = _quat_mul(r[:, 3:7], inv_start)
    up = _quat_rotate(tq, np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)), 1.0)
    hd = _quat_rotate(tq, np.tile(np.array([1.0, 0.0, 0.0]), (n, 1)), 1.0)
    up_proj = up[:, 2]
    heading_proj = (hd * td).sum(-1)
    vl = _quat_rotate(tq, r[:, 7:10], -1.0)
    wl = _quat_rotate(tq, r[:, 10:13], -1.0)
    x, y, z, w = tq[:, 0], tq[:, 1], tq[:, 2], tq[:, 3]                                # get_euler_xyz
    roll = np.arctan2(2.0 * (w * x + y * z), w * w - x * x - y * y + z * z)
    sinp = 2.0 * (w * y - z * x)
    with np.errstate(invalid="ignore"):
        if mutant == "pitch_asin_noclip":
            pitch = np.arcsin(sinp)
        elif mutant == "pitch_asin_clip":
            pitch = np.arcsin(np.clip(sinp, -1.0, 1.0))
        else:
            gimbal = (np.abs(sinp) > 1.0) if mutant == "sinp_gt" else (np.abs(sinp) >= 1.0)
            pitch = np.where(gimbal, HALF_PI32 * np.sign(sinp), np.arcsin(np.clip(sinp, -1.0, 1.0)))
    yaw = np.arctan2(2.0 * (w * z + x * y), w * w + x * x - y * y - z * z)
    roll, pitch, yaw = (_py_mod(a, TWO_PI32, mutant) for a in (roll, pitch, yaw))
    if mutant == "walk_y":
        walk = np.arctan2(tgt[1] - r[:, 1], tgt[0] - r[:, 0])
    else:
        walk = np.arctan2(tgt[2] - r[:, 2], tgt[0] - r[:, 0])                          # compute_rot: z, the reference's quirk
    ang = walk - yaw
    obs = np.zeros((n, NOBS))
    obs[:, 0] = r[:, 2]
    obs[:, 1:4], obs[:, 4:7] = vl, wl
    obs[:, 7], obs[:, 8], obs[:, 9], obs[:, 10], obs[:, 11] = yaw, roll, ang, up_proj, heading_proj
    p = np.asarray(dof_pos, F).astype(np.float64)
    obs[:, 12:30] = (2.0 * p - hi - lo) / (hi - lo)                                    # unscale
    obs[:, 30:48] = np.asarray(dof_vel, F).astype(np.float64) * float(F(cfg.dof_vel_scale))
    obs[:, 48:66] = np.asarray(targets, F).astype(np.float64)
    obs[:, 66] = pitch
    obs[:, 67:73] = _touching(contact, mutant).astype(np.float64)                      # :797
    # the same two deciding quantities as the fp32 program forms them
    t0, t1 = F(cfg.target[0]) - r32[:, 0], F(cfg.target[1]) - r32[:, 1]
    nrm32 = np.sqrt((t0 * t0 + t1 * t1) + F(0.0) * F(0.0))
    sinp32 = F(2.0) * (r32[:, 6] * r32[:, 4] - r32[:, 5] * r32[:, 3])
    return dict(obs=obs, pot=new_pot, prev_pot=prev_pot, up_vec=up, heading_vec=hd, sinp=sinp, nrm=nrm, sinp32=sinp32,
                nrm32=nrm32)


# ---- the float64 bound on an observation row ----------------------------------------------------------------------
def circ(d):
    return np.abs((d + np.pi) % (2.0 * np.pi) - np.pi)


def obs_bound(o32, r64):
    """Per element: first = 3e-6 (1 + |ref64|), second = 4 |oracle32 - ref64| (angles on the circle).  The second term is
    for the poses where fp32 itself is ill-conditioned (yaw and roll at gimbal lock, asin next to +-1, body-frame
    velocities that cancel from 1e4); the share of elements where it exceeds the first is capped by the tests."""
    d = np.abs(np.asarray(o32, np.float64) - r64)
    for col in ANGLE_COLS:
        d[:, col] = circ(np.asarray(o32, np.float64)[:, col] - r64[:, col])
    first = 3e-6 * (1.0 + np.abs(r64))
    second = 4.0 * d
    return first, second


def angle_err(got, ref, slack):
    """|got - ref| for the angle columns: the plain difference, and the distance on the circle only where `ref` lies
    within `slack` of the wrap point (0 == 2 pi), where rounding may land either side of it.  Column 9 = walk - yaw
    inherits yaw's wrap.  So a kernel that forgets to wrap is NOT excused by the circle.  got, ref: [n, 73]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    near = {}
    for col in (7, 8, 66):
        near[col] = np.minimum(np.abs(ref[:, col]), np.abs(TWO_PI32 - ref[:, col])) <= slack[:, col]
    near[9] = near[7] | (np.minimum(np.abs(ref[:, 7]), np.abs(TWO_PI32 - ref[:, 7])) <= slack[:, 9])
    for col in ANGLE_COLS:
        err[:, col] = np.where(near[col], circ(got[:, col] - ref[:, col]), err[:, col])
    return err


def obs_err_f64(got, o32, r64):
    """(err, bound, relaxed): `got` against float64 under the bound above; relaxed = second term > first."""
    first, second = obs_bound(o32, r64)
    bound = first + second
    return angle_err(got, r64, bound), bound, second > first


# ---- tables ---------------------------------------------------------------------------------------------------------
def _ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def ori_pairs(thr):
    """(qz, qw) with fl(fl(qz qz) + fl(qw qw)) exactly fp32(thr), one ulp below and one ulp above: qz in {0.5, 0.5 +- 1 ulp},
    qw scanned +-40 ulps around sqrt(thr - 0.25).  (A single non-zero component cannot reach either threshold exactly.)"""
    t = F(thr)
    want = [np.nextafter(t, F(-np.inf)), t, np.nextafter(t, F(np.inf))]
    found = {}
    qw0 = F(np.sqrt(float(t) - 0.25))
    for dz in (0, -1, 1):
        qz = _ulps(0.5, dz)
        for dw in range(-40, 41):
            qw = _ulps(qw0, dw)
            o = F(F(qz * qz) + F(qw * qw))
            for k, wv in enumerate(want):
                if o == wv and k not in found:
                    found[k] = (qz, qw)
    assert len(found) == 3, (thr, found)
    out = [found[k] for k in range(3)]
    for (qz, qw), wv in zip(out, want):
        assert F(F(qz * qz) + F(qw * qw)) == wv
    return out


# abdomen contact of body 2 (all other abdomen bodies zero unless stated): (components, expected dead)
ABDOMEN_CASES = (
    ((0.0, 0.0, 0.0), False),
    ((1.0, -1.0, 0.0), False),              # cancels to 0
    ((1e-45, 0.0, 0.0), True),              # subnormal, > 0
    ((-1.0, 0.5, 0.25), False),             # negative
    ((3.0, -2.0, -1.0), False),
    ((-0.0, 0.0, 0.0), False),
    ((1e-3, -1e-3, 1e-10), True),
    ((np.nan, 0.0, 0.0), False),            # NaN compares false
    # body 1 = (1, 0, 0), body 2 = (-1, 0, 1e-10): per-body sums 1 and -1 cancel; one running sum of the 15 components
    # would end at 1e-10 > 0.  (The one case with a second non-zero abdomen body: it pins the order of summation.)
    ("two_bodies", False),
)
LEG_SPECIALS = ((1.0, -1.0, 0.0), (1e-45, 0.0, 0.0), (-1.0, 0.5, 0.25), (-0.0, 0.0, 0.0), (1e-3, -1e-3, 1e-10))


def _leg_contacts(rng, n):
    c = rng.normal(0.0, 1.0, (n, NLEG, 3)).astype(F)
    c[rng.random((n, NLEG)) < 0.5] = 0.0
    for i in range(n):                                   # cycled: one leg of most rows carries a special triple
        k = i % (len(LEG_SPECIALS) + 2)
        if k < len(LEG_SPECIALS):
            c[i, (i // 7) % NLEG] = np.array(LEG_SPECIALS[k], F)
    return c


def build_reward_table(cfg, seed=0):
    """-> dict of arrays for fly_pack_reward: the product of the z, (qz, qw), abdomen and progress axes, plus the dump's
    0.92 orientation threshold (for reward_terms); limits, heading, leg contacts cycled over the rows."""
    rng = np.random.default_rng(seed)
    zs = []
    for t in (cfg.termination_height, 1.4, 2.1, cfg.termination_height_up):
        zs += [_ulps(t, -1), F(t), _ulps(t, 1)]
    zs += [F(1.7), F(np.inf), F(-np.inf), F(np.nan)]
    quats = ori_pairs(0.5) + ori_pairs(0.98) + [(F(0.0), F(1.0))]
    maxl = int(cfg.max_episode_length)
    progs = [0, 1, maxl - 3, maxl - 2, maxl - 1, maxl + 100]
    rows = [(z, q, a, p) for z in zs for q in quats for a in range(len(ABDOMEN_CASES)) for p in progs]
    for q in ori_pairs(0.92):                            # fly.py:518: the dump's own threshold
        for z in (F(1.7), F(1.4), _ulps(1.4, 1), F(2.1), _ulps(2.1, -1), F(1.0), F(3.0)):
            rows.append((z, q, 0, 5))
    n = len(rows)
    assert n < 8192 and n % 4 != 0 and n % 32 != 0, n
    hi, lo = _cfg_vec(cfg, "dof_hi"), _cfg_vec(cfg, "dof_lo")
    hi9, lo9 = hi * F(0.9), lo * F(0.9)
    obs = rng.normal(0.0, 1.0, (n, NOBS)).astype(F)
    root = rng.normal(0.0, 1.0, (n, 13)).astype(F)
    contact = np.zeros((n, NCON, 3), F)
    contact[:, NABD:] = _leg_contacts(rng, n)
    progress = np.zeros(n, np.int64)
    w = hi - lo
    u = rng.random((n, NDOF)).astype(F)
    oact = (lo + u * w).astype(F)                                              # anywhere in range: many beyond 0.9 of a limit
    inner = (np.arange(n) // 3) % 3 == 0                                        # a third of the rows: clear of both limits
    oact[inner] = (lo + (F(0.3) + F(0.4) * u[inner]) * w).astype(F)
    obs[:, 11] = rng.uniform(-1.0, 1.0, n).astype(F)
    for i, (z, q, a, p) in enumerate(rows):
        obs[i, 0] = z
        root[i, 5], root[i, 6] = q
        case = ABDOMEN_CASES[a][0]
        if isinstance(case, str):
            contact[i, 1] = np.array((1.0, 0.0, 0.0), F)
            contact[i, 2] = np.array((-1.0, 0.0, 1e-10), F)
        else:
            contact[i, 2] = np.array(case, F)
        progress[i] = p
        j, kind = i % NDOF, (i // NDOF) % 5
        if kind == 0:
            oact[i, j] = hi9[j]
        elif kind == 1:
            oact[i, j] = np.nextafter(hi9[j], F(np.inf))
        elif kind == 2:
            oact[i, j] = lo9[j]
        elif kind == 3:
            oact[i, j] = np.nextafter(lo9[j], F(-np.inf))
        hk = (i // 5) % 7
        if hk < 3:
            obs[i, 11] = _ulps(0.8, hk - 1)
    obs[:, 48:66] = oact
    targets = rng.uniform(-1.0, 1.0, (n, NDOF)).astype(F)
    pot = (-6e4 + rng.normal(0.0, 1.0, n)).astype(F)
    prev_pot = (-6e4 + rng.normal(0.0, 1.0, n)).astype(F)
    reset = np.zeros(n, np.int64)
    reset[::397] = 1                                                            # flagged on input: must stay 1
    return dict(n=n, obs=obs, targets=targets, root=root, contact=contact, pot=pot, prev_pot=prev_pot, progress=progress,
                reset=reset, abd_case=np.array([r[2] for r in rows]))


def build_obs_table(cfg, seed=1):
    """-> dict of arrays for fly_pack_obs: quaternions x positions x velocities; joints and leg contacts cycled."""
    rng = np.random.default_rng(seed)
    r = F(np.sqrt(0.5))
    rp, rm = _ulps(r, 1), _ulps(r, -1)
    t = 1e-4
    quats = [
        (0, 0, 0, 1), (0, 0, 0, -1),
        (0, 0, 1, 0), (0, 0, -1, 0), (0, 0, 1, 1e-8), (0, 0, 1, -1e-8),                       # yaw pi
        (0, r, 0, r), (0, -r, 0, r), (0, rp, 0, rp), (0, rm, 0, r), (0, 0.5, 0, 1), (0, -0.5, 0, 1),      # pitch +-pi/2
        (r, 0, 0, r), (-r, 0, 0, r), (1, 0, 0, 0),                                            # roll +-pi/2, pi
        (-t, 0, 0, 1), (0, -t, 0, 1), (0, 0, -t, 1),                                          # wrap to just under 2 pi
        (0.5, 0.5, 0.5, 0.5), (0.5, -0.5, 0.5, -0.5),
        (0, 0, 0, 0),
    ]
    rq = rng.normal(0.0, 1.0, (14, 4))
    quats += [tuple(v / np.linalg.norm(v)) for v in rq]
    quats = np.array(quats, dtype=F)
    tx, ty, tz = (F(v) for v in cfg.target[:])
    pos = np.array([
        (0, 0, 2),
        (tx, ty, 2),                                         # nrm == 0: pot == -0.0
        (_ulps(tx, -1), ty, 2),                              # one ulp short of the target in x
        (tx, ty + F(5e-10), 2),                              # 0 < nrm < 1e-9
        (tx, ty - F(1e-9), 2),                               # nrm == fp32(1e-9): the clamp's own threshold
        (tx + F(250.0), ty + F(3.0), 2),                     # beyond the target
        (F(10.0), F(-4.0), tz + F(1.5)),                     # z above target[2]
        (F(10.0), F(-4.0), tz - F(0.5)),                     # z below target[2]
        (F(-37.25), F(12.5), F(1.3)), (F(512.7), F(-80.1), F(2.6)),
    ], dtype=F)
    sub = F(1e-40)
    vels = np.array([
        (0, 0, 0, 0, 0, 0),
        (1e4, -300, 50, 3, -2, 1), (-1e4, 300, -50, -60, 40, 10),
        (0.7, -1.3, 0.2, 4.0, -2.5, 1.5),
        (sub, -sub, sub, sub, sub, -sub),
    ], dtype=F)
    rows = [(a, b, c) for a in range(len(quats)) for b in range(len(pos)) for c in range(len(vels))]
    n = len(rows)
    assert n % 4 != 0 and n % 32 != 0, n
    root = np.zeros((n, 13), F)
    for i, (a, b, c) in enumerate(rows):
        root[i, 0:3], root[i, 3:7], root[i, 7:13] = pos[b], quats[a], vels[c]
    lo, hi = _cfg_vec(cfg, "dof_lo"), _cfg_vec(cfg, "dof_hi")
    dof_pos = (lo + rng.random((n, NDOF)).astype(F) * (hi - lo)).astype(F)
    dof_pos = np.minimum(np.maximum(dof_pos, lo), hi)
    dof_pos[0::3] = lo
    dof_pos[1::3] = hi
    dof_vel = rng.normal(0.0, 2.0, (n, NDOF)).astype(F)
    targets = (lo + rng.random((n, NDOF)).astype(F) * (hi - lo)).astype(F)
    contact = rng.normal(0.0, 1.0, (n, NCON, 3)).astype(F)
    contact[:, NABD:] = _leg_contacts(rng, n)
    pot = (-6e4 + rng.normal(0.0, 1.0, n)).astype(F)
    return dict(n=n, root=root, dof_pos=dof_pos, dof_vel=dof_vel, targets=targets, contact=contact, pot=pot,
                quat_idx=np.array([r_[0] for r_ in rows]))


def fill_state(s, tab):
    """Copy a table's arrays into an EnvState-shaped object (whatever fields the table has)."""
    for k in ("root", "dof_pos", "dof_vel", "targets", "contact", "pot", "prev_pot", "obs", "progress", "reset"):
        if k in tab:
            getattr(s, k)[:] = tab[k]
    return s
