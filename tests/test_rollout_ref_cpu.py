"""CPU: the float64 references of tests/rollout_ref.py are pinned before any kernel is held to them -- against the upstream
goldens (g5_sample, g6_gae: float32 outputs of the reference's own functions) to float32 rounding, and against cases small
enough to compute by hand."""
import numpy as np
import pytest

from tests import rollout_ref as R

U = R.U


@pytest.mark.parametrize("tag", ["v02", "v001", "vmix"])
def test_sample_logprob64_reproduces_the_upstream_golden(golden, tag):
    g = golden("g5_sample")
    mu, var, eps = g["mu"], g[tag + "_var"], g[tag + "_eps"]
    a, clipped, logp = R.sample_logprob64(mu, var, eps)
    L = np.sqrt(var.astype(np.float64))
    # float32 a = fl(mu + fl(fl(sqrt var) eps)): two roundings on the product, one on the sum
    a_tol = U * (2 * np.abs(L * eps) + np.abs(a)) + 1e-12
    assert (np.abs(g[tag + "_action"] - a) <= a_tol).all()
    assert (np.abs(g[tag + "_clipped"] - clipped) <= a_tol).all()
    assert ((np.abs(clipped) == 1.0) == (np.abs(g[tag + "_clipped"]) == 1.0)).all() and (np.abs(clipped) == 1.0).any()
    np.testing.assert_allclose(R.sample_action32(mu, var, eps), g[tag + "_clipped"], rtol=0, atol=1e-7)
    tol = 1e-5 + 2e-6 * np.abs(logp) + R.logprob_cancellation64(mu, var, eps)
    err = np.abs(g[tag + "_logp"] - logp)
    print("g5 %s: max logp error / bound %.3f" % (tag, (err / tol).max()))
    assert (err <= tol).all()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_td_gae64_reproduces_the_upstream_golden(golden, tag):
    g = golden("g6_gae")
    r, v, vn = g[tag + "_reward"][..., 0], g[tag + "_v"][..., 0], g[tag + "_v_next"][..., 0]
    d = g[tag + "_done"][..., 0].astype(np.float32)
    gamma, gl = R.gamma_gl32()
    ref = R.td_gae64(r, v, vn, d, gamma, gl, 0)
    assert (np.abs(g[tag + "_target"][..., 0] - ref.target) <= R.target_bound64(ref)).all()
    err = np.abs(g[tag + "_adv"][..., 0] - ref.adv)
    print("g6 %s: max advantage error / first-order bound %.3f" % (tag, (err / ref.bound).max()))
    assert (err <= 2 * ref.bound).all()
    # per-step done carrying the same mask is the same computation
    same = R.td_gae64(r, v, vn, np.broadcast_to(d, r.shape).copy(), gamma, gl, R.GAE_DONE_PER_STEP)
    assert np.array_equal(same.adv, ref.adv) and np.array_equal(same.target, ref.target)


def test_gamma_and_gl_are_the_float32_values_of_the_abi():
    gamma, gl = R.gamma_gl32()
    assert gamma == np.float32(0.99) and gl == np.float32(float(np.float32(0.99)) * float(np.float32(0.95)))
    assert abs(float(gl) - 0.9405) < 1e-7


def test_td_gae64_by_hand():
    one = np.float32(1.0)
    # T = 1: tg = r + gamma v' d, A = tg - v
    g = R.td_gae64([[2.0, 3.0]], [[0.5, 1.0]], [[4.0, 8.0]], [1.0, 0.0], np.float32(0.5), np.float32(0.25), 0)
    assert np.array_equal(g.target, [[4.0, 3.0]]) and np.array_equal(g.adv, [[3.5, 2.0]])
    assert np.array_equal(g.bound, U * g.B) and np.array_equal(g.B, [[2 + 2 + 4 + 3.5 + 0 + 3.5, 4 + 0 + 3 + 2 + 0 + 2]])
    # done = 0 everywhere: the bootstrap vanishes, tg = r; A_t = sum_s gl^(s - t) (r_s - v_s) in every mode
    r = np.array([[1.0], [2.0], [4.0]]); v = np.array([[0.5], [0.5], [1.0]]); vn = np.full((3, 1), 100.0)
    for mode, d in ((0, [0.0]), (1, np.zeros((3, 1)))):
        g = R.td_gae64(r, v, vn, d, np.float32(0.5), np.float32(0.5), mode)
        assert np.array_equal(g.target, r)
        assert np.array_equal(g.adv, [[0.5 + 0.5 * (1.5 + 0.5 * 3.0)], [1.5 + 0.5 * 3.0], [3.0]])
    # ... and with the masked recurrence done = 0 cuts every carry: A = delta
    g = R.td_gae64(r, v, vn, np.zeros((3, 1)), np.float32(0.5), np.float32(0.5), 3)
    assert np.array_equal(g.adv, r - v)
    # one zero in the middle of a per-step mask: the carry stops there (mode 3), the bootstrap of that step only (mode 1)
    d = np.array([[1.0], [0.0], [1.0]]); vn = np.full((3, 1), 2.0)
    g1 = R.td_gae64(r, v, vn, d, one, np.float32(0.5), 1)
    assert np.array_equal(g1.target, [[3.0], [2.0], [6.0]]) and np.array_equal(g1.adv, [[2.5 + 0.5 * 4.0], [1.5 + 0.5 * 5.0], [5.0]])
    g3 = R.td_gae64(r, v, vn, d, one, np.float32(0.5), 3)
    assert np.array_equal(g3.adv, [[2.5 + 0.5 * 1.5], [1.5], [5.0]])
    # gl = 0: A = delta, and the bound is one step's roundings
    g = R.td_gae64(r, v, vn, [1.0], np.float32(0.5), np.float32(0.0), 0)
    assert np.array_equal(g.adv, g.delta) and np.array_equal(g.adv, r + 1.0 - v) and np.array_equal(g.bound, U * g.B)


@pytest.mark.parametrize("T,want", [(1, [(0, 1)]), (2, [(1, 2), (0, 1)]), (64, None), (65, None), (129, None), (4097, None)])
def test_scan_chunks_cover_the_time_axis_once(T, want):
    ch = R.scan_chunks(T)
    if want:
        assert ch == want
    assert ch[0][1] == T and ch[-1][0] == 0 and len(ch) <= 64
    assert all(a[0] == b[1] for a, b in zip(ch, ch[1:])) and all(lo < hi for lo, hi in ch)
    assert len(ch) == -(-T // -(-T // 64))            # T = 65: 33 chunks of 2, the other 31 lanes run empty


def test_scan_carry_bound_is_zero_in_the_last_chunk_and_decays():
    rng = np.random.default_rng(0)
    delta = rng.normal(0, 1, (200, 2))
    extra = R.scan_carry_bound64(delta, np.float32(0.9405))
    assert (extra[196:] == 0).all() and (extra[:196] > 0).all()        # chunks of 4: the latest has no carry
    assert np.allclose(extra[194] / extra[195], float(np.float32(0.9405)))
    assert (R.scan_carry_bound64(delta[:1], np.float32(0.9405)) == 0).all()


def test_adv_normalise64_and_bookkeeping64_by_hand():
    out, s, mean, std = R.adv_normalise64(np.array([1.0, 2.0, 3.0, 6.0], np.float32), eps=0.0)
    assert s == 12.0 and mean == 3.0 and std == np.sqrt(14.0 / 3.0)
    np.testing.assert_allclose(out, np.array([-2.0, -1.0, 0.0, 3.0]) / np.sqrt(14.0 / 3.0), rtol=1e-15)
    rows = np.array([[1.0, 2.0, 3.0], [4.0, 4.0, 4.0]], np.float32)
    score, tol, var = R.bookkeeping64(rows, 0.25, 0.5, [0.2, 0.0105], 1e-3, 0.01)
    assert score == 0.25 + 1.0 + 2.0 and 0 < tol < 1e-5
    v = np.float32(0.2) - np.float32(1e-3)
    assert var[0] == v - np.float32(1e-3) and var[1] == np.float32(0.01) and var.dtype == np.float32
    _, _, var = R.bookkeeping64(rows, 0.25, 0.5, [0.2], 0.0, 0.3)
    assert var[0] == np.float32(0.2)                                   # decay = 0: untouched, the floor included


def test_combine_adv_stats_gives_the_all_rank_moments():
    """ppo.py's combine of the ranks' (sum, M2) pairs, on CPU tensors: the moments of the concatenation."""
    import torch
    from fly_bproject_amd.ppo import combine_adv_stats
    rng = np.random.default_rng(1)
    parts = [rng.normal(m, 1.0, 1000).astype(np.float32).astype(np.float64) for m in (0.0, 50.0, -7.0)]
    ranks = torch.tensor([[p.sum(), ((p - p.mean()) ** 2).sum()] for p in parts], dtype=torch.float32)
    tot = combine_adv_stats(ranks, 1000).numpy()
    whole = np.concatenate(parts)
    assert tot.dtype == np.float32
    np.testing.assert_allclose(tot[0], whole.sum(), rtol=2e-7)
    np.testing.assert_allclose(tot[1], ((whole - whole.mean()) ** 2).sum(), rtol=1e-6)
