"""Seeded numpy generators of the state families that drive ONE FlyDyn substep through every branch of the integrator
(tests/flydyn_ref.py lists them).  A family is fp32 arrays root [n, 13], dof_pos / dof_vel / targets [n, 18]: what the kernel reads.

n = 257: eight workgroups of 32 envs plus a ragged one, whose tail lanes shadow env n - 1."""
import types

import numpy as np

N = 257
VARIANTS = ("bigGrav", "lowGrav")
FAMILIES = ("tumbling", "joint_limits", "free_drive", "belly")

LIMIT_BRANCHES = ("below_limit_outward", "below_limit_inward", "above_limit_outward", "above_limit_inward")
# the branches each family promises to reach (tests/test_flydyn_ref_cpu.py holds it to at least 8 elements of each); lowGrav's effort
# is 1e10, so its effort clamp cannot occur and is promised absent
PROMISED = {
    "tumbling": ("effort_clamp", "vmax_clamp", "lin_clamp", "ang_clamp", "leg_in_ground", "abd_in_ground", "leg_fn_zero", "abd_fn_zero",
                 "leg_friction_capped", "leg_friction_viscous", "abd_friction_capped", "abd_friction_viscous"),
    "joint_limits": LIMIT_BRANCHES + ("vmax_clamp",),
    "free_drive": (),
    "belly": ("abd_in_ground", "abd_fn_zero", "abd_friction_capped", "abd_friction_viscous",
              "leg_in_ground", "leg_fn_zero", "leg_friction_capped", "leg_friction_viscous"),
}
# ... and what a family promises NOT to reach: free_drive is the unsaturated drive in free flight
ABSENT = {
    "free_drive": ("effort_clamp", "vmax_clamp", "leg_in_ground", "abd_in_ground", "lin_clamp", "ang_clamp") + LIMIT_BRANCHES,
}


def one_substep_config(cfg):
    """A copy of `cfg` (OrcConfig or FlyParams) that runs ONE substep of the same length: dt = fp32(dt / substeps), the
    quotient the kernel forms, and substeps = 1."""
    c = type(cfg).from_buffer_copy(cfg)
    c.dt = float(np.float32(cfg.dt) / np.float32(cfg.substeps))
    c.substeps = 1
    return c


def _f32(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]


def _family(root, q, qd, tg):
    root, q, qd, tg = _f32(root, q, qd, tg)
    return types.SimpleNamespace(n=root.shape[0], root=root, dof_pos=q, dof_vel=qd, targets=tg)


def _tables(cfg):
    f = lambda a: np.array(a[:], np.float32).astype(np.float64)
    return f(cfg.dof_lo), f(cfg.dof_hi), f(cfg.dof_pose)


def _pick(rng, n, scales):
    return np.asarray(scales, np.float64)[rng.integers(0, len(scales), n)][:, None]


def _quat_rpy(roll, pitch, yaw):
    """(x, y, z, w) of R = Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], axis=1)


def tumbling(cfg, n=N, seed=101):
    """Any orientation, near the ground, up to speeds and spins past both root clamps; joints anywhere inside their limits."""
    rng = np.random.default_rng(seed)
    lo, hi, _ = _tables(cfg)
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(-5, 5, (n, 2))
    root[:, 2] = rng.uniform(0.2, 2.5, n)
    q = rng.normal(size=(n, 4))
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:10] = rng.normal(size=(n, 3)) * _pick(rng, n, (1.0, 30.0, 700.0))
    root[:, 10:13] = rng.normal(size=(n, 3)) * _pick(rng, n, (1.0, 10.0, 60.0))
    return _family(root, rng.uniform(lo, hi, (n, 18)), rng.uniform(-1, 1, (n, 18)), rng.uniform(lo, hi, (n, 18)))


def joint_limits(cfg, n=N, seed=102):
    """Upright at height 2; every joint within two substeps' travel (2 h vmax) of one of its limits, on either side of it, one
    eighth exactly on it; speeds of both signs; targets around the limit, clipped to the range."""
    rng = np.random.default_rng(seed)
    lo, hi, _ = _tables(cfg)
    h = float(cfg.dt) / cfg.substeps
    reach = 2.0 * h * float(cfg.vmax)
    root = np.zeros((n, 13))
    root[:, 2] = 2.0
    root[:, 6] = 1.0
    lim = np.where(rng.random((n, 18)) < 0.5, lo, hi)
    q = lim + rng.uniform(-reach, reach, (n, 18))
    q = np.where(rng.random((n, 18)) < 0.125, lim, q)
    tg = np.clip(lim + rng.normal(0, 0.05, (n, 18)), lo, hi)
    return _family(root, q, rng.uniform(-1, 1, (n, 18)), tg)


def free_drive(cfg, n=N, seed=103):
    """Far above the plane, tilted and spinning; joints near the pose; targets solved for so that the drive stays unsaturated:
    |tau| < effort and the new |v| <= 0.9 vmax."""
    rng = np.random.default_rng(seed)
    lo, hi, pose = _tables(cfg)
    h = float(cfg.dt) / cfg.substeps
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(-5, 5, (n, 2))
    root[:, 2] = rng.uniform(40, 60, n)
    root[:, 3:7] = _quat_rpy(rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-np.pi, np.pi, n))
    root[:, 7:10] = rng.normal(0, 3, (n, 3))
    root[:, 10:13] = rng.normal(0, 3, (n, 3))
    q = np.clip(pose + rng.normal(0, 0.1, (n, 18)), lo + 0.05, hi - 0.05)
    qd = rng.uniform(-0.3, 0.3, (n, 18))
    v_new = rng.uniform(-0.9, 0.9, (n, 18)) * float(cfg.vmax)
    tau = (v_new - qd) * float(cfg.joint_inertia) / h
    assert np.abs(tau).max() < 0.5 * float(cfg.effort)
    tg = q + (tau + float(cfg.kd) * qd) / float(cfg.kp)
    return _family(root, q, qd, tg)


def belly(cfg, n=N, seed=104):
    """Roll and pitch within 0.6 rad, any yaw, heights 0 .. 0.9: the abdomen points are in the ground with a lever arm, sliding
    slowly (viscous friction), fast (capped) and leaving fast enough for fn to clamp at 0."""
    rng = np.random.default_rng(seed)
    lo, hi, pose = _tables(cfg)
    root = np.zeros((n, 13))
    root[:, 0:2] = rng.uniform(-5, 5, (n, 2))
    root[:, 2] = rng.uniform(0.0, 0.9, n)
    root[:, 3:7] = _quat_rpy(rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(-np.pi, np.pi, n))
    root[:, 7:10] = rng.normal(size=(n, 3)) * _pick(rng, n, (0.2, 5.0, 40.0))
    root[:, 10:13] = rng.normal(0, 3, (n, 3))
    q = np.clip(pose + rng.normal(0, 0.3, (n, 18)), lo, hi)
    tg = np.clip(pose + rng.normal(0, 0.3, (n, 18)), lo, hi)
    return _family(root, q, rng.uniform(-1, 1, (n, 18)), tg)


def make(name, cfg, n=N):
    return {"tumbling": tumbling, "joint_limits": joint_limits, "free_drive": free_drive, "belly": belly}[name](cfg, n)
