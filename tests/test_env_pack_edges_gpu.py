"""GPU (-m gpu): fly_pack_reward, fly_pack_obs and Fly.reward_terms() on the branch tables of tests/env_pack_ref.py.

The two packs decide every reward, every `done` and every observation, through hard comparisons that no recorded or
rolled-out state ever lands on.  The split launches take their inputs from buffers a test can write (the unfused reward
even reads z, heading_proj and the observed actions from the obs rows), so here every threshold is hit exactly, one
ulp below and one ulp above, and EVERY row is checked: no exclusion mask.  The references are the plain-numpy float64
restatement (tests/env_pack_ref.py) and the fp32 oracle; tests/test_env_pack_cpu.py holds those two to each other and
shows that the tables pin each decision (coverage counts, mutants).  Run with -s for the measured maxima
(profiles/env_pack_edges.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import env_pack_ref as R
from tests.hip_helpers import cuda, make_env, pull_state, push_state

pytestmark = pytest.mark.gpu
F = np.float32
OBS_TOL = dict(rtol=3e-6, atol=3e-6)          # tests/test_hip_parity.py's


@pytest.fixture(scope="module")
def rtab():
    return R.build_reward_table(O.default_config(1))


@pytest.fixture(scope="module")
def otab():
    return R.build_obs_table(O.default_config(1))


@pytest.mark.parametrize("add_progress", [0, 1])
@pytest.mark.parametrize("reward", ["standing", "walking"])
def test_pack_reward_on_every_branch(rtab, reward, add_progress):
    """reset and progress bit-equal to the numpy reference AND to the oracle on every row, the non-finite ones included (NaN
    compares false, +-inf is dead); dead rows exactly death_cost; live rows |reward - r64| <= 16 * 2^-24 * mag.  16 counts
    the kernel's fp32 roundings on the longest path from an input to `total`: one product or difference, two in-lane
    adds, three cross-lane row_sum levels, one scale product, six adds of `total` = 13, so 16 holds with room (`mag` here
    scales each |a - o| by energy_cost_scale, as the reward does: tighter than the unscaled sum).  A wrong branch moves
    the reward by 0.1 (leg_reward) to 2.5 (death_cost); the bound is about 1e-5.
    The episode statistics follow the step's bookkeeping: rows that reset add into finished_* and clear episode_*,
    all others accumulate (each one fp32 add: bit-equal)."""
    n = rtab["n"]
    mode = 0 if reward == "standing" else 1
    cfg = O.default_config(n)
    cfg.reward_mode = mode
    env = make_env(n, reward=reward)
    assert env.params.reward_mode == mode
    s = R.fill_state(O.EnvState(n), rtab)
    push_state(env, s)
    rng = np.random.default_rng(3)
    pre = {k: rng.uniform(-5.0, 5.0, n).astype(F) for k in ("er", "dr")}
    pre["el"] = rng.integers(0, 900, n).astype(F)
    pre["dl"] = rng.integers(0, 5000, n).astype(F)
    pre["dc"] = rng.integers(0, 9, n).astype(F)
    for k, buf in (("er", env.episode_return_buf), ("el", env.episode_length_buf), ("dr", env.finished_return_sum),
                   ("dl", env.finished_length_sum), ("dc", env.finished_count)):
        buf.copy_(cuda(pre[k]))
    env._lib.fly_pack_reward(env._handle, C.byref(env._bufs), add_progress, None)
    got = pull_state(env)
    stats = [b.cpu().numpy() for b in (env.episode_return_buf, env.episode_length_buf, env.finished_return_sum,
                                       env.finished_length_sum, env.finished_count)]
    env.exit()
    ref = R.reward_ref(cfg, rtab["obs"], rtab["targets"], rtab["root"], rtab["contact"], rtab["pot"], rtab["prev_pot"],
                       rtab["progress"], rtab["reset"], add_progress=add_progress)
    if add_progress:
        s.progress += 1
    O.pack_reward(cfg, s)
    assert np.array_equal(got.reset, ref["reset"]), np.nonzero(got.reset != ref["reset"])[0][:10]
    assert np.array_equal(got.reset, s.reset)
    assert np.array_equal(got.progress, ref["progress"]) and np.array_equal(got.progress, s.progress)
    dead = ref["dead"]
    assert dead.sum() > 0 and np.all(got.reward[dead] == F(cfg.death_cost))
    err = np.abs(got.reward.astype(np.float64) - ref["reward"])
    ratio = err[~dead] / (R.U32 * ref["mag"][~dead])
    print("\nfly_pack_reward %s add_progress=%d: %d rows (%d dead, %d reset); max |reward - r64| = %.2f x 2^-24 mag; max |reward - oracle| = %.3g"
          % (reward, add_progress, n, dead.sum(), got.reset.sum(), ratio.max(), np.abs(got.reward - s.reward)[~dead].max()))
    assert np.all(err[~dead] <= R.reward_bound(ref["mag"][~dead])), float(ratio.max())
    for k in ("obs", "targets", "root", "contact", "pot", "prev_pot"):      # inputs are left alone
        assert np.array_equal(getattr(got, k), rtab[k], equal_nan=True), k
    # episode statistics
    rs = got.reset != 0
    er, el = pre["er"] + got.reward, pre["el"] + F(1.0)
    assert np.array_equal(stats[0], np.where(rs, F(0.0), er)) and np.array_equal(stats[1], np.where(rs, F(0.0), el))
    assert np.array_equal(stats[2], np.where(rs, pre["dr"] + er, pre["dr"]))
    assert np.array_equal(stats[3], np.where(rs, pre["dl"] + el, pre["dl"]))
    assert np.array_equal(stats[4], np.where(rs, pre["dc"] + F(1.0), pre["dc"]))


@pytest.mark.parametrize("binding", ["own", "misaligned"])
def test_pack_obs_on_every_branch(otab, binding):
    """EXACT_COLS bit-equal to the oracle; every other column within OBS_TOL of the fp32 oracle -- the sharp check at the
    ill-conditioned poses, because kernel and oracle feed bit-identical arguments to atan2f and asinf; every column
    within 3e-6 (1 + |ref64|) + 4 |oracle32 - ref64| of float64 (the CPU suite caps the share of elements where the second
    term is the larger one at 1 %).  Angles are compared as plain numbers, and on the circle only where the reference
    lies next to the wrap point 0 == 2 pi: a kernel that forgets to wrap is 2 pi off.  prev_pot is the pushed pot bit for
    bit, pot within 1e-6 relative of float64, up_vec and heading_vec within 1e-6.
    `misaligned`: bind_obs on a view one float into a guard-filled allocation, so the rows are not 16-byte aligned and
    the tile goes out through the scalar store path; the guards on both sides must be untouched."""
    n = otab["n"]
    cfg = O.default_config(n)
    env = make_env(n)
    s = R.fill_state(O.EnvState(n), otab)
    s.obs[:] = -123.0
    push_state(env, s)
    guard = None
    if binding == "misaligned":
        guard = torch.full((n * R.NOBS + 9,), -77777.0, device=env.device)
        view = guard[1:1 + n * R.NOBS].view(n, R.NOBS)
        assert view.data_ptr() % 16 != 0 and guard.data_ptr() % 16 == 0
        env.bind_obs(view)
    env.get_obs()
    got = pull_state(env)
    up, hd = env.up_vec.cpu().numpy(), env.heading_vec.cpu().numpy()
    if guard is not None:
        g = guard.cpu().numpy()
        assert g[0] == F(-77777.0) and np.all(g[1 + n * R.NOBS:] == F(-77777.0))
        assert np.array_equal(g[1:1 + n * R.NOBS].reshape(n, R.NOBS), got.obs)
    env.exit()
    ref = R.obs_ref(cfg, otab["root"], otab["dof_pos"], otab["dof_vel"], otab["targets"], otab["contact"], otab["pot"])
    O.pack_obs(cfg, s)
    for col in R.EXACT_COLS:
        assert np.array_equal(got.obs[:, col], s.obs[:, col]), col
    tol = OBS_TOL["atol"] + OBS_TOL["rtol"] * np.abs(s.obs.astype(np.float64))
    e32 = R.angle_err(got.obs, s.obs, np.full(s.obs.shape, 1e-4))
    groups = (("z", [0]), ("vel_loc", [1, 2, 3]), ("angvel_loc", [4, 5, 6]), ("yaw roll ang pitch", [7, 8, 9, 66]),
              ("up/heading proj", [10, 11]), ("dof_pos", range(12, 30)), ("dof_vel", range(30, 48)),
              ("actions", range(48, 66)), ("touching", range(67, 73)))
    print("\nfly_pack_obs (%s rows): %d rows; max (|kernel - oracle32| / OBS_TOL) per column group:" % (binding, n))
    for name, cols in groups:
        cols = list(cols)
        print("    %-20s %.3f   (max abs %.3g)" % (name, (e32[:, cols] / tol[:, cols]).max(), e32[:, cols].max()))
    assert np.all(e32 <= tol), np.argwhere(~(e32 <= tol))[:10]
    e64, bound, relaxed = R.obs_err_f64(got.obs, s.obs, ref["obs"])
    first = R.obs_bound(s.obs, ref["obs"])[0]
    print("    against float64: max err / bound = %.3f; where the bound is its first term alone, max err / (3e-6 (1 + |ref64|)) = %.3f; "
          "elements under the relaxed bound: %.3f %%" % ((e64 / bound).max(), (e64 / first)[~relaxed].max(), 100 * relaxed.mean()))
    assert np.all(e64 <= bound), np.argwhere(~(e64 <= bound))[:10]
    assert np.array_equal(got.prev_pot, otab["pot"])
    np.testing.assert_allclose(got.pot, ref["pot"], rtol=1e-6)
    np.testing.assert_allclose(up, ref["up_vec"], atol=1e-6)
    np.testing.assert_allclose(hd, ref["heading_vec"], atol=1e-6)
    for k in ("root", "dof_pos", "dof_vel", "targets", "contact"):
        assert np.array_equal(getattr(got, k), otab[k]), k


def test_reward_terms_on_every_branch(rtab):
    """Fly.reward_terms() (fly.py:504-546, the viewer's dump) on the reward table against the oracle's restatement: the
    selection and count terms bit-equal -- the table holds z at 1.4, heading_proj at 0.8, the observed actions at 0.9 of
    a limit and qz^2 + qw^2 at the dump's own 0.92, each exactly and one ulp either side -- and the three 18-term sums
    at 3e-6, as on the recorded inputs."""
    n = rtab["n"]
    env = make_env(n)
    s = R.fill_state(O.EnvState(n), rtab)
    push_state(env, s)
    got = {k: v.float().cpu().numpy() for k, v in env.reward_terms().items()}
    env.exit()
    want = O.reward_terms(O.default_config(n), s)
    assert set(got) == set(want) == set(O.REWARD_TERMS)
    for k in ("alive_reward", "up_reward", "orient_reward", "leg_reward", "dof_at_limit_cost", "progress_reward"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(got[k] != want[k])[0][:10])
    finite = np.isfinite(rtab["obs"][:, 0])
    for k in ("heading_reward", "actions_cost", "electricity_cost"):
        np.testing.assert_allclose(got[k], want[k], rtol=3e-6, atol=3e-6, err_msg=k)
        print("reward_terms %-18s max |got - oracle| = %.3g" % (k, np.abs(got[k] - want[k]).max()))
    ori = R.ori32(rtab["root"])
    t = F(0.92)
    for v, bonus in ((np.nextafter(t, F(-np.inf)), 0.0), (t, 0.0), (np.nextafter(t, F(np.inf)), 0.75)):
        rows = ori == v
        assert rows.sum() > 0 and np.all(got["orient_reward"][rows] == F(bonus)), v
    z = rtab["obs"][:, 0]
    assert np.all(got["up_reward"][z == F(1.4)] == 0) and np.all(got["up_reward"][z == R._ulps(1.4, 1)] == F(0.75))
    assert finite.sum() < n and np.all(got["up_reward"][np.isnan(z)] == 0)
