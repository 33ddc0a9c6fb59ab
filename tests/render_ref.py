"""Float64 numpy statement of the recording renderer (fly_render, csrc/fly_render.hip): the same scene, the same constants
(FLY_R_* in include/flyhip.h, restated here), the same primitive order and hit rules.  The test oracle for the renderer.

`render(params, pose, width, height, fov_y_deg, cam_offset, look_z)` -> (rgb uint8 [H, W, 3], ids uint8 [H, W]).
`pose`: 25 floats, root position, quaternion xyzw, 18 joint angles (DoF order).  `params`: a FlyParams (FlyConfig fields).
"""
import math

import numpy as np

THORAX_AXES = (0.60, 0.40, 0.35)
HEAD_CENTER = (0.75, 0.0, 0.05)
HEAD_RADIUS = 0.28
ABDOMEN_SPHERE = 0.24
ABDOMEN_LINK = 0.18
LEG_RADIUS = 0.06
CHECKER = 1.0
LIGHT = (0.3, 0.2, 1.0)
AMBIENT = 0.35
SHADOW_BIAS = 1e-3
SKY_RGB = (0.62, 0.76, 0.92)
GROUND_RGB_A = (0.58, 0.58, 0.58)
GROUND_RGB_B = (0.42, 0.42, 0.42)
BODY_RGB = (0.45, 0.30, 0.15)
ABDOMEN_RGB = (0.70, 0.52, 0.22)
LEG_RGB = (0.22, 0.16, 0.10)
RID_SKY, RID_GROUND, RID_BODY, RID_ABDOMEN, RID_LEG0 = 0, 1, 2, 3, 4


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def leg_points(params, pose, leg):
    """Body-frame attach, knee and tip of leg `leg` (the physics' kinematics, oracle/fly_physics.inc)."""
    q = np.asarray(pose[7 + 3 * leg: 10 + 3 * leg], np.float64)
    p0 = [params.dof_pose[3 * leg + i] for i in range(3)]
    psi = params.leg_azimuth[leg] + params.leg_sigma[leg] * (q[0] - p0[0])
    al = params.alpha0 + (q[1] - p0[1])
    gm = al + params.beta0 + (q[2] - p0[2])
    lf, lt = params.femur_len, params.tibia_len
    att = np.array(params.leg_attach[leg][:], np.float64)
    knee = att + np.array([math.cos(psi) * lf * math.cos(al), math.sin(psi) * lf * math.cos(al), lf * math.sin(al)])
    rho, zeta = lf * math.cos(al) + lt * math.cos(gm), lf * math.sin(al) + lt * math.sin(gm)
    tip = att + np.array([math.cos(psi) * rho, math.sin(psi) * rho, zeta])
    return att, knee, tip


def camera(pose, width, height, fov_y_deg, cam_offset, look_z):
    """(camera position, forward, right, up) for the root at pose[0:3]."""
    cam = np.array([pose[0] + cam_offset[0], pose[1] + cam_offset[1], cam_offset[2]], np.float64)
    fw = np.array([-cam_offset[0], -cam_offset[1], look_z - cam_offset[2]], np.float64)
    fw /= np.linalg.norm(fw)
    rt = np.cross(fw, [0.0, 0.0, 1.0])
    rt /= np.linalg.norm(rt)
    return cam, fw, rt, np.cross(rt, fw)


def project(point, pose, width, height, fov_y_deg, cam_offset, look_z):
    """Continuous pixel coordinates (column, row; pixel centres at +0.5) of a world point."""
    cam, fw, rt, up = camera(pose, width, height, fov_y_deg, cam_offset, look_z)
    v = np.asarray(point, np.float64) - cam
    th = math.tan(math.radians(fov_y_deg) / 2)
    sx, sy = v @ rt / (v @ fw), v @ up / (v @ fw)
    return (sx / (th * width / height) + 1) * width / 2, (1 - sy / th) * height / 2


def scene(params, pose, cam):
    """Primitives in camera-relative coordinates, in the renderer's order."""
    R = quat_matrix(pose[3:7])
    rel = np.asarray(pose[0:3], np.float64) - cam
    w = lambda b: rel + R @ np.asarray(b, np.float64)
    sph = [(w(HEAD_CENTER), HEAD_RADIUS, RID_BODY)]
    ab = [w(params.abdomen_pts[k][:]) for k in range(5)]
    sph += [(a, ABDOMEN_SPHERE, RID_ABDOMEN) for a in ab]
    cap = []
    for leg in range(6):
        att, knee, tip = leg_points(params, pose, leg)
        cap.append((w(att), w(knee), LEG_RADIUS, RID_LEG0 + leg))
        cap.append((w(knee), w(tip), LEG_RADIUS, RID_LEG0 + leg))
    cap += [(ab[k], ab[k + 1], ABDOMEN_LINK, RID_ABDOMEN) for k in range(4)]
    return R, rel, sph, cap


def _dot(a, b):
    return (a * b).sum(-1)


def hit_sphere(o, d, c, r):
    oc = o - c
    b = _dot(oc, d)
    h = b * b - (_dot(oc, oc) - r * r)
    with np.errstate(invalid="ignore"):
        return np.where(h < 0, -1.0, -b - np.sqrt(np.maximum(h, 0)))


def hit_capsule(o, d, a, b, r):
    ba, oa = b - a, o - a
    baba, bard, baoa, rdoa, oaoa = _dot(ba, ba), _dot(d, ba), _dot(oa, ba), _dot(d, oa), _dot(oa, oa)
    qa = baba - bard * bard
    qb = baba * rdoa - baoa * bard
    qc = baba * oaoa - baoa * baoa - r * r * baba
    h = qb * qb - qa * qc
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (-qb - np.sqrt(np.maximum(h, 0))) / qa
        y = baoa + t * bard
        body = (h >= 0) & (y > 0) & (y < baba)
        oc = np.where((y <= 0)[..., None], oa, o - b)
        cb = _dot(d, oc)
        hc = cb * cb - (_dot(oc, oc) - r * r)
        tc = np.where(hc > 0, -cb - np.sqrt(np.maximum(hc, 0)), -1.0)
    return np.where(h < 0, -1.0, np.where(body, t, tc))


def hit_ellipsoid(o, d, R, c, inv):
    ob, db = (o - c) @ R * inv, d @ R * inv          # R^T v, row vectors
    a, b, cc = _dot(db, db), _dot(ob, db), _dot(ob, ob) - 1
    h = b * b - a * cc
    with np.errstate(invalid="ignore"):
        return np.where(h < 0, -1.0, (-b - np.sqrt(np.maximum(h, 0))) / a)


def render(params, pose, width=640, height=480, fov_y_deg=40.0, cam_offset=(-5.0, -7.0, 4.0), look_z=1.5):
    pose = np.asarray(pose, np.float64)
    cam, fw, rt, up = camera(pose, width, height, fov_y_deg, cam_offset, look_z)
    R, ec, sph, cap = scene(params, pose, cam)
    inv = 1.0 / np.array(THORAX_AXES)
    th = math.tan(math.radians(fov_y_deg) / 2)
    px, py = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    sx = (2 * px / width - 1) * th * (width / height)
    sy = (1 - 2 * py / height) * th
    d = fw + sx[..., None] * rt + sy[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.zeros_like(d)

    best = np.full(d.shape[:-1], 3.0e38)
    kind = np.zeros(d.shape[:-1], np.int64)
    idx = np.zeros(d.shape[:-1], np.int64)
    ids = np.zeros(d.shape[:-1], np.uint8)

    def take(t, k, i, cls):
        m = (t > 0) & (t < best)
        best[m], kind[m], idx[m], ids[m] = t[m], k, i, cls

    with np.errstate(divide="ignore", invalid="ignore"):
        take(-cam[2] / d[..., 2], 1, 0, RID_GROUND)
    take(hit_ellipsoid(o, d, R, ec, inv), 2, 0, RID_BODY)
    for i, (c, r, cls) in enumerate(sph):
        take(hit_sphere(o, d, c, r), 3, i, cls)
    for i, (a, b, r, cls) in enumerate(cap):
        take(hit_capsule(o, d, a, b, r), 4, i, cls)

    p = d * np.where(kind > 0, best, 0)[..., None]
    n = np.zeros_like(d)
    base = np.zeros_like(d)
    g = kind == 1
    n[g] = [0.0, 0.0, 1.0 if cam[2] >= 0 else -1.0]
    par = (np.floor((cam[0] + p[..., 0]) / CHECKER) + np.floor((cam[1] + p[..., 1]) / CHECKER)).astype(np.int64) & 1
    base[g & (par == 0)] = GROUND_RGB_A
    base[g & (par == 1)] = GROUND_RGB_B
    m = kind == 2
    pb = (p - ec) @ R * inv * inv
    n[m] = (pb @ R.T)[m]
    for i, (c, r, cls) in enumerate(sph):
        m = (kind == 3) & (idx == i)
        n[m] = (p - c)[m]
    for i, (a, b, r, cls) in enumerate(cap):
        m = (kind == 4) & (idx == i)
        ba, pa = b - a, p - a
        baba = ba @ ba
        hh = np.clip(pa @ ba / baba, 0, 1) if baba > 0 else np.zeros(pa.shape[:-1])
        n[m] = (pa - hh[..., None] * ba)[m]
    obj = kind >= 2
    with np.errstate(invalid="ignore"):
        n[obj] /= np.linalg.norm(n[obj], axis=-1, keepdims=True)
    base[obj & (ids == RID_BODY)] = BODY_RGB
    base[obj & (ids == RID_ABDOMEN)] = ABDOMEN_RGB
    base[obj & (ids >= RID_LEG0)] = LEG_RGB

    L = np.array(LIGHT) / np.linalg.norm(LIGHT)
    ndl = np.maximum(n @ L, 0.0)
    lit = (kind > 0) & (ndl > 0)
    so = (p + n * SHADOW_BIAS)[lit]
    sd = np.broadcast_to(L, so.shape)
    occ = hit_ellipsoid(so, sd, R, ec, inv) > 0
    for c, r, _ in sph:
        occ |= hit_sphere(so, sd, c, r) > 0
    for a, b, r, _ in cap:
        occ |= hit_capsule(so, sd, a, b, r) > 0
    v = ndl[lit]
    v[occ] = 0.0
    ndl[lit] = v
    rgb = base * (AMBIENT + (1 - AMBIENT) * ndl)[..., None]
    rgb[kind == 0] = SKY_RGB
    q = np.floor(np.clip(rgb, 0, 1) * 255 + 0.5).astype(np.uint8)
    return q, ids
