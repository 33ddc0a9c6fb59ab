"""float64 numpy statement of ONE FlyDyn substep, written from the header comment of oracle/fly_physics.inc (steps 1-3 and the
leg kinematics) and vectorised over envs.  It shares no code with the oracle or the kernel: the tests hold both to it.

`substep(cfg, root, dof_pos, dof_vel, targets)` -> (root', dof_pos', dof_vel', contact [n, 11, 3], branches).

`cfg` is an OrcConfig or a FlyParams (the same field names), or a sequence of n of them (one per env: per-env domain
randomisation); every constant is the fp32 value the kernel reads, taken to float64, and h = float(cfg.dt) / cfg.substeps.

`branches` maps each branch of the substep to a boolean mask, and under "margin" to the signed distance of every element to the
branch's edge (positive = taken), so that a test can count what a set of states reaches and leave out what sits on an edge:

    effort_clamp, vmax_clamp                                   [n, 18]   margins |tau| - effort, |v| - vmax (pre-clamp)
    below_limit_outward / _inward, above_limit_outward / _inward [n, 18] margins "below_limit" = lo - x, "above_limit" = x - hi
    leg_in_ground [n, 6], abd_in_ground [n, 5]                            margins "leg_depth", "abd_depth" = d
    leg_fn_zero, abd_fn_zero (d > 0 and fn clamped at 0)                 margins "leg_fn", "abd_fn" = -(kc d (1 - cdamp u_z))
    leg_friction_capped / _viscous, abd_friction_capped / _viscous       margins "leg_friction", "abd_friction" = cvisc |u_t| - mu fn
    lin_clamp, ang_clamp [n, 3]                                           margins |v| - max_lin_vel, |w_b| - max_ang_vel (pre-clamp)

and "x_pre" [n, 18] holds the joint positions before the limit clamp.

Two test-only arguments: `angle_shift` [n, 18] is added to the leg angles (psi, alpha, gamma of leg l at columns 3l .. 3l+2) before
their sines and cosines are taken; `mutant` names one deliberately wrong term (MUTANTS)."""
import numpy as np

MUTANTS = ("gyro_sign", "no_gyro", "no_rdot", "abdomen_no_torque", "limit_keeps_velocity", "fn_no_damping")
NLEG, NABD, NDOF = 6, 5, 18


def _arr(x):
    return np.array(x[:], dtype=np.float64)


def constants(cfg):
    """The constants of one config as float64 (of the fp32 fields), or of a sequence of n configs stacked env-major."""
    if isinstance(cfg, (list, tuple)):
        each = [constants(c) for c in cfg]
        return {k: np.stack([c[k] for c in each]) for k in each[0]}
    scal = ("kp", "kd", "effort", "vmax", "joint_inertia", "mass", "gravity", "kc", "cdamp", "mu", "cvisc", "lin_damp", "ang_damp",
            "max_lin_vel", "max_ang_vel", "femur_len", "tibia_len", "alpha0", "beta0")
    k = {name: np.float64(getattr(cfg, name)) for name in scal}
    k["h"] = np.float64(float(cfg.dt) / int(cfg.substeps))
    k["inertia"] = _arr(cfg.inertia)
    for name in ("dof_lo", "dof_hi", "dof_pose"):
        k[name] = _arr(getattr(cfg, name)).reshape(NLEG, 3)
    k["leg_attach"] = np.array([list(r) for r in cfg.leg_attach], np.float64)
    k["leg_azimuth"] = _arr(cfg.leg_azimuth)
    k["leg_sigma"] = _arr(cfg.leg_sigma)
    k["abdomen_pts"] = np.array([list(r) for r in cfg.abdomen_pts], np.float64)
    return k


def _c(k, name, extra):
    """constant `name` shaped to broadcast against [n, ...extra dims]: a scalar stays one, a per-env [n] gets `extra` unit axes."""
    v = k[name]
    return v if v.ndim == 0 else v.reshape(v.shape + (1,) * extra)


def rotation(q):
    """[n, 3, 3] rotation matrices of unit quaternions q [n, 4] (x, y, z, w)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def substep(cfg, root, dof_pos, dof_vel, targets, angle_shift=None, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    k = cfg if isinstance(cfg, dict) else constants(cfg)
    root = np.asarray(root, np.float64)
    n = root.shape[0]
    q0 = np.asarray(dof_pos, np.float64).reshape(n, NLEG, 3)
    qd0 = np.asarray(dof_vel, np.float64).reshape(n, NLEG, 3)
    tg = np.asarray(targets, np.float64).reshape(n, NLEG, 3)
    shift = np.zeros((n, NLEG, 3)) if angle_shift is None else np.asarray(angle_shift, np.float64).reshape(n, NLEG, 3)
    h2, h1 = _c(k, "h", 2), _c(k, "h", 1)
    lo, hi, pose = k["dof_lo"], k["dof_hi"], k["dof_pose"]          # [6, 3] or [n, 6, 3]
    br, mg = {}, {}

    # 1. joints
    eff, vmax = _c(k, "effort", 2), _c(k, "vmax", 2)
    tau = _c(k, "kp", 2) * (tg - q0) - _c(k, "kd", 2) * qd0
    mg["effort_clamp"] = np.abs(tau) - eff
    br["effort_clamp"] = np.abs(tau) > eff
    tau = np.clip(tau, -eff, eff)
    v = qd0 + h2 * tau / _c(k, "joint_inertia", 2)
    mg["vmax_clamp"] = np.abs(v) - vmax
    br["vmax_clamp"] = np.abs(v) > vmax
    v = np.clip(v, -vmax, vmax)
    x = q0 + h2 * v
    below, above = x < lo, x > hi
    mg["below_limit"], mg["above_limit"] = lo - x, x - hi
    br["below_limit_outward"], br["below_limit_inward"] = below & (v < 0), below & ~(v < 0)
    br["above_limit_outward"], br["above_limit_inward"] = above & (v > 0), above & ~(v > 0)
    x_pre = x
    x = np.where(below, lo, np.where(above, hi, x))
    if mutant != "limit_keeps_velocity":
        v = np.where(br["below_limit_outward"] | br["above_limit_outward"], 0.0, v)
    q1, qd1 = x, v

    # leg kinematics on the NEW joint state: body-frame tip r_b [n, 6, 3] and its velocity
    sg = k["leg_sigma"]
    psi = k["leg_azimuth"] + sg * (q1[..., 0] - pose[..., 0])
    al = _c(k, "alpha0", 1) + (q1[..., 1] - pose[..., 1])
    gm = al + _c(k, "beta0", 1) + (q1[..., 2] - pose[..., 2])
    psid, ald = sg * qd1[..., 0], qd1[..., 1]
    gmd = ald + qd1[..., 2]
    cp, sp = np.cos(psi + shift[..., 0]), np.sin(psi + shift[..., 0])
    ca, sa = np.cos(al + shift[..., 1]), np.sin(al + shift[..., 1])
    cg, sgm = np.cos(gm + shift[..., 2]), np.sin(gm + shift[..., 2])
    Lf, Lt = _c(k, "femur_len", 1), _c(k, "tibia_len", 1)
    rho, zeta = Lf * ca + Lt * cg, Lf * sa + Lt * sgm
    rhod, zetad = -Lf * sa * ald - Lt * sgm * gmd, Lf * ca * ald + Lt * cg * gmd
    att = k["leg_attach"]
    r_leg = att + np.stack([cp * rho, sp * rho, zeta], axis=-1)
    rd_leg = np.stack([-sp * rho * psid + cp * rhod, cp * rho * psid + sp * rhod, zetad], axis=-1)
    if mutant == "no_rdot":
        rd_leg = np.zeros_like(rd_leg)
    r_abd = np.broadcast_to(k["abdomen_pts"], (n, NABD, 3))
    rb = np.concatenate([r_abd, r_leg], axis=1)                     # contact order: 5 abdomen points, then 6 leg tips
    rd = np.concatenate([np.zeros((n, NABD, 3)), rd_leg], axis=1)

    # 2. contacts
    pos, quat, vel, w = root[:, 0:3], root[:, 3:7], root[:, 7:10], root[:, 10:13]
    R = rotation(quat)
    rw = np.einsum("nij,nkj->nki", R, rb)
    u = vel[:, None, :] + np.cross(w[:, None, :], rw) + np.einsum("nij,nkj->nki", R, rd)
    d = -(pos[:, None, 2] + rw[..., 2])
    inside = d > 0
    kc, cdamp, mu, cvisc = _c(k, "kc", 1), _c(k, "cdamp", 1), _c(k, "mu", 1), _c(k, "cvisc", 1)
    fn_raw = kc * d * (1.0 if mutant == "fn_no_damping" else (1 - cdamp * u[..., 2]))
    fn = np.maximum(fn_raw, 0.0)
    ut = np.sqrt(u[..., 0] ** 2 + u[..., 1] ** 2)
    visc, cap = cvisc * ut, mu * fn
    ft = np.minimum(visc, cap)
    sc = ft / (ut + 1e-9)
    f = np.stack([-sc * u[..., 0], -sc * u[..., 1], fn], axis=-1) * inside[..., None]
    for name, sl in (("abd", slice(0, NABD)), ("leg", slice(NABD, NABD + NLEG))):
        ins = inside[:, sl]
        br[name + "_in_ground"], mg[name + "_depth"] = ins, d[:, sl]
        br[name + "_fn_zero"], mg[name + "_fn"] = ins & (fn_raw[:, sl] < 0), -fn_raw[:, sl]
        br[name + "_friction_capped"] = ins & (visc[:, sl] > cap[:, sl])
        br[name + "_friction_viscous"] = ins & ~(visc[:, sl] > cap[:, sl])
        mg[name + "_friction"] = (visc - cap)[:, sl]
    F = f.sum(axis=1)
    torque_of = f.copy()
    if mutant == "abdomen_no_torque":
        torque_of[:, :NABD] = 0.0
    T = np.cross(rw, torque_of).sum(axis=1)

    # 3. root, semi-implicit Euler
    g = np.zeros((n, 3))
    g[:, 2] = k["gravity"]
    vlim, wlim = _c(k, "max_lin_vel", 1), _c(k, "max_ang_vel", 1)
    v_new = (vel + h1 * (F / _c(k, "mass", 1) + g)) * (1 - h1 * _c(k, "lin_damp", 1))
    mg["lin_clamp"], br["lin_clamp"] = np.abs(v_new) - vlim, np.abs(v_new) > vlim
    v_new = np.clip(v_new, -vlim, vlim)
    I = k["inertia"]
    wb = np.einsum("nji,nj->ni", R, w)
    Tb = np.einsum("nji,nj->ni", R, T)
    gyro = np.cross(wb, I * wb)
    if mutant == "gyro_sign":
        gyro = -gyro
    elif mutant == "no_gyro":
        gyro = np.zeros_like(gyro)
    wb = (wb + h1 * (Tb - gyro) / I) * (1 - h1 * _c(k, "ang_damp", 1))
    mg["ang_clamp"], br["ang_clamp"] = np.abs(wb) - wlim, np.abs(wb) > wlim
    wb = np.clip(wb, -wlim, wlim)
    w_new = np.einsum("nij,nj->ni", R, wb)
    pos_new = pos + h1 * v_new
    qx, qy, qz, qw = quat.T
    wx, wy, wz = w_new.T
    hh = 0.5 * k["h"]
    nq = np.stack([qx + hh * (wx * qw + wy * qz - wz * qy), qy + hh * (-wx * qz + wy * qw + wz * qx),
                   qz + hh * (wx * qy - wy * qx + wz * qw), qw + hh * (-wx * qx - wy * qy - wz * qz)], axis=-1)
    nq /= np.sqrt((nq ** 2).sum(axis=-1, keepdims=True))

    for name in list(br):
        if br[name].ndim == 3:
            br[name] = br[name].reshape(n, NDOF)
    for name in list(mg):
        if mg[name].ndim == 3:
            mg[name] = mg[name].reshape(n, NDOF)
    br["margin"] = mg
    br["x_pre"] = x_pre.reshape(n, NDOF)
    return (np.concatenate([pos_new, nq, v_new, w_new], axis=1), q1.reshape(n, NDOF), qd1.reshape(n, NDOF), f, br)


def steps(cfg, root, dof_pos, dof_vel, targets, count, **kw):
    """`count` substeps in a row (the constants are read once); returns the last substep's outputs and a list of every substep's branches."""
    k = cfg if isinstance(cfg, dict) else constants(cfg)
    hist = []
    contact = None
    for _ in range(count):
        root, dof_pos, dof_vel, contact, br = substep(k, root, dof_pos, dof_vel, targets, **kw)
        hist.append(br)
    return root, dof_pos, dof_vel, contact, hist


# ---- the per-element bound the kernel is held to (tests/test_flydyn_substep_gpu.py; its teeth: tests/test_flydyn_ref_cpu.py) ------
GROUPS = ("position", "quaternion", "v", "omega", "q", "qdot", "force")
K = 4.0            # the suite's own factor (test_fused_step_vs_oracle_resynced)
DELTA = 2e-6       # the trig allowance's angle error: the kernel's hardware sine / cosine document ~1e-6 absolute


def fields(root, dof_pos, dof_vel, contact):
    """The outputs of a substep by field group, float64, each [n, k]."""
    root = np.asarray(root, np.float64)
    n = root.shape[0]
    return {"position": root[:, 0:3], "quaternion": root[:, 3:7], "v": root[:, 7:10], "omega": root[:, 10:13],
            "q": np.asarray(dof_pos, np.float64).reshape(n, NDOF), "qdot": np.asarray(dof_vel, np.float64).reshape(n, NDOF),
            "force": np.asarray(contact, np.float64).reshape(n, 33)}


def excluded(cfg, branches):
    """[n, 18] joints whose float64 pre-clamp position lies within 4 fp32 ulp of a limit: any arithmetic may zero their velocity
    or not, so their VELOCITY is left out (their position stays in).  Nothing else is: every other branch is continuous."""
    k = cfg if isinstance(cfg, dict) else constants(cfg)
    x = branches["x_pre"]
    out = np.zeros(x.shape, bool)
    for lim in (k["dof_lo"], k["dof_hi"]):
        lim = lim.reshape(lim.shape[:-2] + (NDOF,))
        out |= np.abs(x - lim) <= 4.0 * np.spacing(np.abs(lim).astype(np.float32)).astype(np.float64)
    return out


def trig_allowance(cfg, state, ref_fields, delta=DELTA):
    """A = sum_j |ref(angle_shift = delta e_j) - ref| over the 18 leg angles, by field group.  Zero wherever no leg tip is in the ground."""
    k = cfg if isinstance(cfg, dict) else constants(cfg)
    n = state.root.shape[0]
    A = {g: np.zeros_like(ref_fields[g]) for g in GROUPS}
    for j in range(NDOF):
        shift = np.zeros((n, NDOF))
        shift[:, j] = delta
        f = fields(*substep(k, state.root, state.dof_pos, state.dof_vel, state.targets, angle_shift=shift)[:4])
        for g in GROUPS:
            A[g] += np.abs(f[g] - ref_fields[g])
    return A


def bound(ref_fields, f32_fields, A, skip):
    """Per element max(K |f32 oracle - f64|, K M (1 + |f64|)) + A, M = the fp32 oracle's largest scaled miss over the family and the
    field group (skipped elements apart).  `skip`: {group: mask} of the excluded elements.  Returns ({group: bound}, {group: M})."""
    out, Ms = {}, {}
    for g in GROUPS:
        miss = np.abs(f32_fields[g] - ref_fields[g])
        keep = ~skip[g] if g in skip else np.ones(miss.shape, bool)
        Ms[g] = float((miss / (1.0 + np.abs(ref_fields[g])))[keep].max())
        out[g] = np.maximum(K * miss, K * Ms[g] * (1.0 + np.abs(ref_fields[g]))) + A[g]
    return out, Ms


def worst_ratio(got_fields, ref_fields, bnd, skip):
    """{group: (largest scaled miss, largest |got - ref| / bound)} over the elements not skipped; a zero bound admits only a zero miss."""
    res = {}
    for g in GROUPS:
        miss = np.abs(got_fields[g] - ref_fields[g])
        keep = ~skip[g] if g in skip else np.ones(miss.shape, bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(miss == 0.0, 0.0, miss / bnd[g])
        res[g] = (float((miss / (1.0 + np.abs(ref_fields[g])))[keep].max()), float(ratio[keep].max()))
    return res
