"""No GPU: tests/adam_ref.py -- the float64 reference the optimizer kernels are held to (tests/test_adam_step_gpu.py) -- against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam themselves, run in float64."""
import numpy as np
import torch

from tests import adam_ref as R

N = 69587           # the policy's parameter count
STEPS = 120


def _problem(seed):
    rng = np.random.default_rng(seed)
    P = rng.standard_normal(N) * 0.05
    # the gradient's scale swings over the steps, so that clipping (max_norm = 1) is active on some and inactive on others
    scales = 10.0 ** rng.uniform(-4.0, 0.5, STEPS)
    return rng, P, scales


def test_clip_adam_equals_torch_float64_over_120_steps():
    rng, P, scales = _problem(0)
    p_t = torch.nn.Parameter(torch.from_numpy(P.copy()))
    opt = torch.optim.Adam([p_t], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    m, v, mask = np.zeros(N), np.zeros(N), np.ones(N)
    clipped = []
    for step in range(STEPS):
        G = rng.standard_normal(N) * scales[step]
        p_t.grad = torch.from_numpy(G.copy())
        gn = float(torch.nn.utils.clip_grad_norm_([p_t], 1.0))
        opt.step()
        P, m, v, norm, coef = R.clip_adam(P, G, m, v, step, mask, 1e-3, (0.9, 0.999), 1e-8, 1.0, 1.0)
        clipped.append(coef < 1.0)
        assert abs(norm - gn) <= 1e-12 * gn
        st = opt.state[p_t]
        for got, want in ((P, p_t.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), step
    assert any(clipped) and not all(clipped)


def test_clip_adam_grad_scale_and_mask():
    """grad_scale multiplies the gradient before the norm; a masked element keeps P, its moments only decay, and it does not
    count in the norm -- the same as torch on the unmasked elements alone."""
    rng = np.random.default_rng(1)
    n = 1000
    P, G, m, v = rng.standard_normal(n), rng.standard_normal(n) * 3, rng.standard_normal(n) * 0.1, rng.random(n)
    mask = (rng.random(n) < 0.8).astype(np.float64)
    P2, m2, v2, norm, coef = R.clip_adam(P, G, m, v, 7, mask, 1e-3, (0.9, 0.999), 1e-8, 1.0, 0.125)
    k = mask == 1
    Pk, mk, vk, nk, ck = R.clip_adam(P[k], G[k] * 0.125, m[k], v[k], 7, np.ones(int(k.sum())), 1e-3, (0.9, 0.999), 1e-8, 1.0, 1.0)
    assert abs(norm - nk) <= 1e-14 * nk and abs(coef - ck) <= 1e-14 * ck and coef < 1.0     # (another summation order)
    for got, want in ((P2[k], Pk), (m2[k], mk), (v2[k], vk)):
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    assert np.array_equal(P2[~k], P[~k]) and np.array_equal(m2[~k], 0.9 * m[~k]) and np.array_equal(v2[~k], 0.999 * v[~k])


def test_dqn_adam_soft_equals_torch_float64_over_120_steps():
    rng, P, scales = _problem(2)
    p_t = torch.nn.Parameter(torch.from_numpy(P.copy()))
    tgt_t = torch.from_numpy(P.copy())
    opt = torch.optim.Adam([p_t], lr=3e-4, betas=(0.9, 0.999), eps=1e-8)
    P_tgt, m, v, mask = P.copy(), np.zeros(N), np.zeros(N), np.ones(N)
    for step in range(STEPS):
        G = rng.standard_normal(N) * scales[step]
        p_t.grad = torch.from_numpy(G.copy())
        opt.step()
        with torch.no_grad():
            tgt_t.copy_(tgt_t * 0.995 + p_t.data * (1.0 - 0.995))          # soft_update of the reference program
        P, P_tgt, m, v = R.dqn_adam_soft(P, P_tgt, G, m, v, step, mask, 3e-4, (0.9, 0.999), 1e-8, 0.995)
        st = opt.state[p_t]
        for got, want in ((P, p_t.detach().numpy()), (P_tgt, tgt_t.numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), step


def test_bounds_hold_for_an_fp32_emulation_of_the_operation_sequence():
    """The forward-error bounds of adam_ref hold (and are not vacuous) for the operation sequence they were counted from, run in
    numpy float32 -- every operation rounds once, and numpy's float32 power is correctly rounded to within an ulp."""
    f = np.float32
    rng = np.random.default_rng(3)
    n = 20000
    hp = R.hyper(1e-3, (0.9, 0.999), 1e-8)
    for step in (0, 1, 9, 999):
        a = 10.0 ** rng.uniform(-12, 0, n)
        G = (a * rng.choice([-1.0, 1.0], n)).astype(f)
        m = (a * rng.uniform(-0.7, 0.7, n) * (1 - 0.9 ** step)).astype(f)
        v = (a * a * rng.uniform(0.6, 1.4, n) * (1 - 0.999 ** step)).astype(f)
        P = (rng.standard_normal(n) * 0.05).astype(f)
        b1, b2, lr, eps, ts = f(0.9), f(0.999), f(1e-3), f(1e-8), f(step + 1)
        mi = b1 * m + (f(1) - b1) * G
        vi = b2 * v + (f(1) - b2) * G * G
        ss = lr / (f(1) - np.power(b1, ts))
        bc2s = np.sqrt(f(1) - np.power(b2, ts))
        Pk = P - ss * (mi / (np.sqrt(vi) / bc2s + eps))
        P2, m2, v2, upd = R.adam(P.astype(np.float64), G.astype(np.float64), m.astype(np.float64), v.astype(np.float64), step,
                                 np.ones(n), 1e-3, (0.9, 0.999), 1e-8)
        e_m, e_v = R.moment_bounds(G.astype(np.float64), m.astype(np.float64), v.astype(np.float64), 0.0, hp)
        assert np.all(np.abs(mi - m2) <= e_m) and np.all(np.abs(vi - v2) <= e_v)
        w = R.update_weight(v2, step, hp)
        s, sel, share = R.step_size_factor(P.astype(np.float64) - Pk, upd, w, 1e-3, G.astype(np.float64), v2, hp)
        assert sel.sum() > 1000 and abs(s - 1) <= 2e-5
        e_p, w = R.param_bound(P.astype(np.float64), m2, v2, upd, e_m, e_v, step, hp, s)
        e_p = e_p + R.factor_uncertainty(e_p, upd, sel, share, hp) * np.abs(upd)
        ratio = np.abs(Pk - (P.astype(np.float64) - upd * (1 + (s - 1) * w))) / e_p
        assert ratio.max() <= 1.0, (step, ratio.max())
        assert ratio.max() >= 0.05          # the bound is of the order of the error, not orders above it
