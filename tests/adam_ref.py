"""Float64 reference of the optimizer steps (`mlp_adam_step`, `dqn_adam_soft_update`) and the forward-error bounds the GPU tests
hold the kernels to.  Plain numpy / torch: nothing here is shared with the kernels.

The reference is torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (defaults: no weight decay, no amsgrad) evaluated in float64
with the Python-double hyperparameters the reference program passes to torch, NOT their fp32 roundings -- tests/test_adam_ref_cpu.py
pins it to torch itself."""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32 (round to nearest)
UG = U / (1.0 - 64.0 * U)       # n U / (1 - n U) <= n UG for n <= 64: makes a first-order sum of <= 64 roundings a rigorous bound
SUB = 2.0 ** -149               # gradual underflow: absolute error of one fp32 operation whose result is subnormal
POW_ULP = 16.0                  # accuracy the OpenCL specification (which the device math library implements) requires of pow()


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def adam(P, g, m, v, step, mask, lr, betas, eps):
    """torch.optim.Adam's single-tensor step number `step + 1` on the already clipped / masked gradient `g` (float64).
    Returns P', m', v' and the update P - P' = mask * lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps)."""
    b1, b2 = float(betas[0]), float(betas[1])
    t = int(step) + 1
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    denom = np.sqrt(v2) / np.sqrt(bc2) + float(eps)
    upd = mask * ((float(lr) / bc1) * (m2 / denom))
    return P - upd, m2, v2, upd


def clip_adam(P, G, m, v, step, mask, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, grad_scale=1.0):
    """-> P', m', v', norm, coef.  g = G grad_scale mask; norm = ||g||_2; coef = min(1, max_norm / (norm + 1e-6)); Adam on coef g.
    Masked elements: P unchanged, m and v decay only."""
    P, G, m, v, mask = _f64(P), _f64(G), _f64(m), _f64(v), _f64(mask)
    g = G * float(grad_scale) * mask
    norm = float(np.sqrt(np.sum(g * g)))
    coef = min(1.0, float(max_norm) / (norm + 1e-6))
    P2, m2, v2, _ = adam(P, g * coef, m, v, step, mask, lr, betas, eps)
    return P2, m2, v2, norm, coef


def dqn_adam_soft(P, P_tgt, G, m, v, step, mask, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, tau=0.995):
    """-> P', P_tgt', m', v'.  Adam without clipping on G mask, then P_tgt' = tau P_tgt + (1 - tau) P'."""
    P, P_tgt, G, m, v, mask = _f64(P), _f64(P_tgt), _f64(G), _f64(m), _f64(v), _f64(mask)
    P2, m2, v2, _ = adam(P, G * mask, m, v, step, mask, lr, betas, eps)
    return P2, float(tau) * P_tgt + (1.0 - float(tau)) * P2, m2, v2


# ---- the derived copies ------------------------------------------------------------------------------------------------------------
def _h2_pos(k):
    """fp16x2 plane position of a bf16x3 term-0 position: the same layout with 1024-word blocks instead of 1536."""
    return (k // 1536) * 1024 + k % 1536


def derived(P, pol, wscales=None, layer_offsets=None):
    """What every copy of the packed weights `P` (a torch tensor on pol's device: the P' THE KERNEL LEFT) must hold, bit for bit:
    {"F": (dst, values), "T": ..., "FB": ..., "TB": ..., and with `wscales` (the four published layer scales) "FH", "TH"} -- the
    gather through idx_f / idx_t, split_bf16x3 through idx_fb / idx_tb (terms 512 and 1024 words on) and split_f16x2 under the
    layer's scale (terms 512 words apart).  `dst` are positions in the copy, `values` what must stand there."""
    import torch
    from fly_bproject_amd.policy import split_bf16x3, split_f16x2
    out = {}
    for name, idx in (("F", pol.idx_f), ("T", pol.idx_t)):
        src = torch.nonzero(idx >= 0).squeeze(-1)
        out[name] = (idx[src].long(), P[src])
    for name, idx in (("FB", pol.idx_fb), ("TB", pol.idx_tb)):
        src = torch.nonzero(idx >= 0).squeeze(-1)
        dst = idx[src].long()
        planes = split_bf16x3(P[src])
        out[name] = (torch.cat([dst, dst + 512, dst + 1024]), torch.cat(planes))
        if wscales is not None:
            offs = torch.tensor(list(layer_offsets), device=P.device)
            layer = torch.bucketize(src, offs, right=True) - 1
            sc = torch.as_tensor(wscales, dtype=torch.float32, device=P.device)[layer]
            h = split_f16x2(P[src], sc)
            hd = _h2_pos(dst)
            out[name[0] + "H"] = (torch.cat([hd, hd + 512]), torch.cat(h))
    return out


def unaddressed(dst, size, device):
    """Positions of a copy of `size` words that no index map addresses (the words a launch must leave alone)."""
    import torch
    free = torch.ones(size, dtype=torch.bool, device=device)
    free[dst] = False
    return torch.nonzero(free).squeeze(-1)


# ---- forward-error bounds of the kernels' operation sequence -----------------------------------------------------------------------
# Both kernels evaluate, per element, with every fp32 operation rounding once (-ffp-contract=off, correctly rounded / and sqrt):
#     c   = coef * grad_scale                      (PPO; coef == 1 exactly when not clipped: then c == grad_scale, no rounding)
#     g   = G * c * mask                           one rounding (mask is 0 or 1: exact)
#     m'  = b1f * m + w1f * g                      two products + one sum;  b1f = fp32(beta1), w1f = 1.0f - b1f (exact: Sterbenz)
#     v'  = b2f * v + (w2f * g) * g                three products + one sum
#     D   = sqrtf(v') / bc2s + epsf                sqrt, quotient, sum
#     P'  = P - mask * (ss * (m' / D))             quotient, product, difference;  ss = lrf / bc1
# The reference uses the DOUBLE hyperparameters, so the distances |fp32(beta) - beta| etc. are part of the error; they are known
# numbers of the formats and enter the bounds as such.  What is uniform over the elements -- fp32(lr), the bias corrections bc1 and
# bc2s with their powf -- is measured as the step-size factor `s` and divided out (see `step_size_factor`).
def hyper(lr, betas, eps):
    f = lambda x: float(np.float32(x))     # noqa: E731
    b1, b2 = float(betas[0]), float(betas[1])
    b1f, b2f = f(b1), f(b2)
    w1f, w2f = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    return {"b1": b1, "b2": b2, "w1": 1.0 - b1, "w2": 1.0 - b2, "db1": abs(b1f - b1), "db2": abs(b2f - b2),
            "dw1": abs(w1f - (1.0 - b1)), "dw2": abs(w2f - (1.0 - b2)), "deps": abs(f(eps) - float(eps)), "eps": float(eps),
            "lr": float(lr)}


def coef_error(norm, clipped, k_norm):
    """Relative error of the kernel's c = coef * grad_scale: 0 when not clipped; else the norm's (k_norm roundings), the sum
    norm + 1e-6f (one rounding, and fp32(1e-6) for 1e-6), the quotient and the product by grad_scale."""
    if not clipped:
        return 0.0
    return (k_norm + 3.0) * UG + abs(float(np.float32(1e-6)) - 1e-6) / (norm + 1e-6)


def moment_bounds(g, m, v, e_c, hp):
    """Absolute bounds on |m'_hip - m'_64| and |v'_hip - v'_64| for unmasked elements; g = the reference's clipped gradient."""
    e_g = e_c + UG                                   # relative error of the kernel's g
    am, ag, gg = np.abs(m), np.abs(g), g * g
    e_m = am * (hp["db1"] + UG * hp["b1"]) + ag * (hp["dw1"] + hp["w1"] * (e_g + UG)) + UG * (hp["b1"] * am + hp["w1"] * ag) + 4 * SUB
    e_v = v * (hp["db2"] + UG * hp["b2"]) + gg * (hp["dw2"] + hp["w2"] * (2 * e_g + 2 * UG)) + UG * (hp["b2"] * v + hp["w2"] * gg) + 4 * SUB
    return e_m, e_v


def bias_terms(step, hp):
    """bc1, sqrt(bc2) of the reference at step number step + 1, and the a-priori bound on the relative error of the kernel's
    lr / bc1 (fp32(beta1) for beta1 through t multiplications, a pow() within POW_ULP, the difference, the quotient, fp32(lr))."""
    t = int(step) + 1
    bc1 = 1.0 - hp["b1"] ** t
    bc2s = float(np.sqrt(1.0 - hp["b2"] ** t))
    a = (t * hp["db1"] / hp["b1"] + POW_ULP * UG) * hp["b1"] ** t / bc1 + 2 * UG + abs(float(np.float32(hp["lr"])) - hp["lr"]) / hp["lr"]
    return bc1, bc2s, a


def update_weight(v2, step, hp):
    """w = (sqrt(v') / bc2s) / (sqrt(v') / bc2s + eps): the share of the denominator that carries bc2's error."""
    _, bc2s, _ = bias_terms(step, hp)
    sv = np.sqrt(v2) / bc2s
    return sv / (sv + hp["eps"])


def param_bound(P, m2, v2, upd, e_m, e_v, step, hp, s):
    """Absolute bound on |P'_hip - (P - upd (1 + (s - 1) w))| for unmasked elements: the reference's update with the uniform
    step-size factor divided out.  The factor acts on lr / bc1 in full and on the denominator only through sqrt(v') / bc2s, so
    where eps matters (w < 1) it applies with weight w, and the part of it that may sit in lr / bc1 (`a`, bounded a priori) is
    allowed on the rest."""
    bc1, bc2s, a = bias_terms(step, hp)
    sv = np.sqrt(v2)
    safe = v2 > 4 * e_v
    dsq = np.where(safe, e_v / (2 * np.sqrt(np.where(safe, v2 - e_v, 1.0))), np.sqrt(e_v))
    dsq = dsq + UG * (sv + dsq)                                         # the sqrt's own rounding
    D = sv / bc2s + hp["eps"]
    e_D = dsq / bc2s + UG * (sv / bc2s) + hp["deps"] + UG * D           # quotient, fp32(eps), sum
    q = np.abs(m2) / D
    e_q = e_m / (D - e_D) + np.abs(m2) * e_D / (D * (D - e_D)) + UG * q
    au = np.abs(upd)
    w = sv / bc2s / D
    return (hp["lr"] / bc1) * e_q + UG * au + UG * (np.abs(P) + au) + (abs(s - 1.0) + a) * (1.0 - w) * au, w


def step_size_factor(dP_hip, upd, w, lr, g, v2, hp):
    """s = median(dP_hip / dP_64) over the elements where the ratio is the UNIFORM factor and nothing else: eps plays no part
    (w >= 1 - 1e-4), the update is at least lr / 100 (P's own rounding is then a small, symmetric part of it), and the new
    gradient's share of v' is below 1 % -- v' = b2f v + w2f g g carries |fp32(1 - beta2) - 0.001| = 1.3e-5 (relative) on the g g
    term, which the per-element bound allows for but which is no part of the step size (at step 1 with v = 0 it even cancels
    the same error in bc2).  Returns s, the selection and the share admitted."""
    base = (w >= 1.0 - 1e-4) & (np.abs(upd) >= lr / 100.0)
    for share in (1e-2, 1e-1, 1.0):     # (a young optimizer has no element with a small share: then the smallest that gives 1000)
        sel = base & (hp["w2"] * g * g <= share * v2)
        if sel.sum() >= 1000:
            break
    return float(np.median(dP_hip[sel] / upd[sel])) if sel.any() else float("nan"), sel, share


def factor_uncertainty(e_p, upd, sel, share, hp):
    """What the measured factor can be off by.  The median over n elements: each ratio carries at most e_p / |upd| of its
    element's own error, signs at random, so the median of n of them is uncertain by about the typical one / sqrt(n); three
    times that is allowed.  And the admitted share of the new gradient in v' times half fp32(1 - beta2)'s relative distance
    from 1 - beta2 (half: the square root), which the selected elements may have in common."""
    return 3.0 * float(np.median(e_p[sel] / np.abs(upd[sel]))) / np.sqrt(float(sel.sum())) + 0.5 * share * hp["dw2"] / hp["w2"]
