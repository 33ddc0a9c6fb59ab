"""GPU (-m gpu): PPO's fixed-grid post-rollout kernels past their first trip.  ppo_td_gae_vnorm_kernel, ppo_td_gae_vnorm_scan_kernel
(csrc/ppo_kernels.hip), gae_episodic_kernel<true>, gae_episodic_scan_kernel<true> / <false> (csrc/gae_episodic.hip) and
episode_stats_scan_kernel (csrc/episode_stats.hip) launch a fixed grid and stride over the envs beyond it, carrying float64
moments or an episode set from one env (or block of 64 envs) to the next while everything else about an env starts afresh.
The shapes of tests/strided_envs_cases.py are the smallest at which a workgroup makes a second and a third trip, with ragged
ends; tests/test_strided_envs_cpu.py holds the premises (trips, counts, flag kinds, the references' own bounds) without a GPU.

Launches go through the C ABI with the neighbouring files' helpers (imported, not copied), every output between sentinel guards
and pre-filled with the sentinel, so a row a kernel skips cannot pass.  References and bounds are those files' own:
  lane = env       targets and advantages bit for bit the float32 restatements (value_norm_ref.td_gae, gae_episodic_ref.episodic32);
                   the identity table bit for bit the plain kernel
  scan             targets bit for bit; advantages within SCAN_MARGIN x (first-order bound + re-associated carries) of float64:
                   tests/test_rollout_kernels_gpu.py::check_scan, tests/test_gae_episodic_gpu.py::check_scan
  moment sets      per workgroup the count of the documented assignment (env blocks / envs g, g + 256, ...), all 256 checked, the
                   empty ones zero; merged: count exactly T N, mean rtol 1e-10 / atol 1e-12, variance rtol 1e-10 against float64
  episode sets     tests/test_episode_stats_gpu.py's bounds; rows, episodes, length sums and time-outs of every workgroup exactly
A failing assertion names the first env that misses with its workgroup and trip.  profiles/strided_envs.txt records what these
tests say about kernels with a deliberately broken second trip, and the margins of the unbroken ones."""
import numpy as np
import pytest
import torch

from tests import episode_stats_ref as ER
from tests import gae_episodic_ref as E
from tests import rollout_ref as R
from tests import strided_envs_cases as S
from tests import test_episode_stats_gpu as ES
from tests import test_gae_episodic_gpu as GE
from tests import test_rollout_kernels_gpu as RK
from tests import test_value_norm_gpu as VG
from tests import value_norm_ref as V

pytestmark = pytest.mark.gpu
lib = GE.lib                                                  # the module-scoped fixture of tests/test_gae_episodic_gpu.py
TABLE = V.table(S.TABLE_S)
M0_TABLE = V.table(V.initial())                               # m = 0: with v = v_next = 0 the target is the reward
LANE = [(T, N, S.WAVE) for T, N in S.LANE_SHAPES]
SCAN = [(T, N, 1) for T, N in S.SCAN_SHAPES]
for _shapes in (LANE, SCAN, [(T, N, 1) for T, N in S.EPISODE_SCAN_SHAPES]):
    assert max(S.trips(N, per) for _, N, per in _shapes) == 3
assert max(S.trips(N, 1, S.plain_scan_grid(N)) for _, N in S.PLAIN_SCAN_SHAPES) == 3


def _where(per, grid=S.GRID):
    return lambda miss: S.describe(miss, per, grid)


def _trips(N, per, grid=S.GRID):
    """The trips of workgroup 0 at this shape -- asserted, not assumed: two, or three beyond twice the grid."""
    k = S.trips(N, per, grid)
    assert k == (3 if N > 2 * per * grid else 2) and N > per * grid
    return k


def _same(got, want, per, what, grid=S.GRID):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(got, want), "%s: %s" % (what, S.describe(got != want, per, grid))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _identical(run1, run2, what):
    for a, b in zip(run1, run2):
        assert np.array_equal(_bits(a), _bits(b)), "%s: two runs differ" % what


def _check_set_counts(sets, T, N, per, what):
    """Every one of the 256 moment sets holds the rows of the env blocks / envs g, g + 256, ...; the empty ones are zero."""
    want = S.set_counts(T, N, per)
    walks = np.bincount(S.workgroup_of(N, per)[::per], minlength=S.GRID)
    assert sets.shape == (S.GRID, 3)
    for g in np.flatnonzero(sets[:, 0] != want):
        raise AssertionError("%s: set %d counts %g targets; its workgroup walks %d env%s in %d trip(s): %g (%d sets are off)"
                             % (what, g, sets[g, 0], walks[g], " blocks" if per > 1 else "s", walks[g], want[g],
                                int((sets[:, 0] != want).sum())))
    assert sets[:, 0].sum() == T * N
    assert (sets[want == 0] == 0).all() and (sets[:, 2] >= 0).all()


def _check_sets(lib, sets, tgt, per, what):
    """The 256 moment sets of a launch that wrote the targets `tgt` [T][N]: set by set, and merged against float64."""
    _check_set_counts(sets, *tgt.shape, per, what)
    VG._assert_stats(GE._merged(lib, sets), V.moments(tgt))


def _vn_gae(S_v, case, mode):
    """ppo_td_gae_vnorm under the table of the statistics S_v, every output guarded -> (target, adv, sets)."""
    T, N = case[0].shape
    guards = (GE.Guarded(T * N), GE.Guarded(T * N), GE.Guarded(S.GRID * 3, dtype=torch.float64))
    return VG._VN(S_v).gae(*case, mode, guards=guards)


# ------------------------------------------------------------------------------------------- ppo_td_gae_vnorm, lane = env
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("T,N,per", LANE)
def test_td_gae_vnorm_lane(lib, T, N, per, mode):
    what = "ppo_td_gae_vnorm_kernel<%d> T=%d N=%d (%d trips)" % (mode, T, N, _trips(N, per))
    case = S.td_case(T, N, mode)
    run = _vn_gae(S.TABLE_S, case, mode)
    tg, adv, sets = run
    t32, a32 = V.td_gae(*case, TABLE, mode=mode)
    _same(tg, t32, per, what + " targets")
    _same(adv, a32, per, what + " advantages")
    _check_sets(lib, sets, tg, per, what)
    _identical(run, _vn_gae(S.TABLE_S, case, mode), what)
    ref = S.td_ref64(case, TABLE, mode)
    err = np.abs(adv - ref.adv)
    print("%s: max advantage error / first-order bound %.3f" % (what, RK._ratio(err, ref.bound)))
    assert (np.abs(tg - ref.target) <= R.target_bound64(ref)).all() and (err <= 2 * ref.bound).all()
    # the identity table: ppo_td_gae, which has one workgroup per block and no trips
    ti, ai, si = _vn_gae(VG.IDENTITY, case, mode)
    t0, a0 = GE.run_plain_gae(lib, *case, mode)
    _same(ti, t0, per, what + " identity targets")
    _same(ai, a0, per, what + " identity advantages")
    _check_sets(lib, si, ti, per, what + " identity")


# ------------------------------------------------------------------------------------------------- ppo_td_gae_vnorm, scan
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T,N,per", SCAN)
def test_td_gae_vnorm_scan(lib, T, N, per, mode):
    what = "ppo_td_gae_vnorm_scan_kernel<%d> T=%d N=%d (%d trips)" % (mode, T, N, _trips(N, per))
    case = S.td_case(T, N, mode)
    run = _vn_gae(S.TABLE_S, case, mode | R.GAE_SCAN)
    tg, adv, sets = run
    _same(tg, V.td_gae(*case, TABLE, mode=mode)[0], per, what + " targets")            # elementwise: bit for bit
    RK.check_scan(what, T, N, mode, tg, adv, S.td_ref64(case, TABLE, mode), where=_where(per))
    _check_sets(lib, sets, tg, per, what)
    _identical(run, _vn_gae(S.TABLE_S, case, mode | R.GAE_SCAN), what)
    # the identity table: ppo_td_gae's scan, one workgroup per env
    ti, ai, si = _vn_gae(VG.IDENTITY, case, mode | R.GAE_SCAN)
    t0, a0 = GE.run_plain_gae(lib, *case, mode | R.GAE_SCAN)
    _same(ti, t0, per, what + " identity targets")
    _same(ai, a0, per, what + " identity advantages")
    _check_sets(lib, si, ti, per, what + " identity")


# ------------------------------------------------------------------------------------- ppo_td_gae_episodic_vnorm, both forms
def _episodic_vnorm(lib, T, N, per, what):
    mode = R.GAE_SCAN if per == 1 else 0
    case = S.episodic_case(T, N, per)
    scaled = ((case[0] * 20).astype(np.float32),) + case[1:]
    run = GE.run_episodic(lib, scaled, mode, table=TABLE)
    tg, adv, sets = run
    ref = (GE.check_scan if per == 1 else GE.check_lane)(scaled, tg, adv, TABLE, where=_where(per))
    if ref is not None:                                       # lane = env: bit for bit, and this far from float64
        print("%s: max advantage error / first-order bound %.3f" % (what, RK._ratio(np.abs(adv - ref.adv), ref.bound)))
    stale = E.flags_of(*case[3:], S.MAXLEN)[2]
    assert stale.any() and np.array_equal(tg[stale], V.denormalize(case[1], TABLE)[stale]) and (adv[stale] == 0).all()
    _check_sets(lib, sets, tg, per, what)
    _identical(run, GE.run_episodic(lib, scaled, mode, table=TABLE), what)
    # the identity table: the plain kernel (one workgroup per block / per env at these N)
    t0, a0 = GE.run_episodic(lib, case, mode)
    ti, ai, si = GE.run_episodic(lib, case, mode, table=GE.IDENTITY)
    _same(ti, t0, per, what + " identity targets")
    _same(ai, a0, per, what + " identity advantages")
    _check_sets(lib, si, ti, per, what + " identity")


@pytest.mark.parametrize("T,N,per", LANE)
def test_episodic_vnorm_lane(lib, T, N, per):
    _episodic_vnorm(lib, T, N, per, "gae_episodic_kernel<true> T=%d N=%d (%d trips)" % (T, N, _trips(N, per)))


@pytest.mark.parametrize("T,N,per", SCAN)
def test_episodic_vnorm_scan(lib, T, N, per):
    _episodic_vnorm(lib, T, N, per, "gae_episodic_scan_kernel<true> T=%d N=%d (%d trips)" % (T, N, _trips(N, per)))


@pytest.mark.parametrize("T,N", S.PLAIN_SCAN_SHAPES)
def test_episodic_plain_scan_beyond_the_grid_cap(lib, T, N):
    grid = S.plain_scan_grid(N)
    what = "gae_episodic_scan_kernel<false> T=%d N=%d (%d trips of %d workgroups)" % (T, N, _trips(N, 1, grid), grid)
    assert grid == S.SCAN_GRID_MAX < N
    case = S.episodic_case(T, N, 1, grid)
    run = GE.run_episodic(lib, case, R.GAE_SCAN)
    GE.check_scan(case, *run, where=_where(1, grid))
    stale = E.flags_of(*case[3:], S.MAXLEN)[2]
    assert stale[:, grid:].any() and np.array_equal(run[0][stale], case[1][stale]) and (run[1][stale] == 0).all()
    _identical(run, GE.run_episodic(lib, case, R.GAE_SCAN), what)


# ----------------------------------------------------------------------------- moment sets on inputs that break naive sums
@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("T,N,per", LANE + SCAN)
def test_moment_sets_on_hard_rewards(lib, T, N, per, kind):
    """value_norm_ref.hard_rewards with v = v_next = 0 and m = 0: the target is the reward.  Every vnorm kernel of the form:
    the TD pass in each of its modes, and the episodic pass on flag rows without an end."""
    _trips(N, per)
    x, zeros, _ = S.hard_case(kind, T, N)
    scan = R.GAE_SCAN if per == 1 else 0
    for mode in ((0, 1) if per == 1 else (0, 1, 2, 3)):
        what = "hard rewards %s, td mode %d, T=%d N=%d" % (kind, mode | scan, T, N)
        d = np.ones((T, N) if mode & 1 else (N,), np.float32)
        run = _vn_gae(V.initial(), (x, zeros, zeros, d), mode | scan)
        _same(run[0], x, per, what + " targets")
        _check_sets(lib, run[2], x, per, what)
        _identical(run, _vn_gae(V.initial(), (x, zeros, zeros, d), mode | scan), what)
    what = "hard rewards %s, episodic mode %d, T=%d N=%d" % (kind, scan, T, N)
    case = (x, zeros, zeros) + S.no_flags(T, N)
    run = GE.run_episodic(lib, case, scan, table=M0_TABLE)
    _same(run[0], x, per, what + " targets")
    _check_sets(lib, run[2], x, per, what)
    _identical(run, GE.run_episodic(lib, case, scan, table=M0_TABLE), what)


# -------------------------------------------------------------------------------------------------- ppo_episode_stats, scan
def _check_episode_sets(sets, w, T, N, what):
    """Every workgroup's set against the walk's episodes of the envs it walks (g, g + 256, ...): rows, episodes, length sum
    and time-outs, all whole numbers held exactly."""
    env = np.array([ep.env for ep in w.episodes], np.int64) % S.GRID
    count = lambda weights: np.bincount(env, weights=weights, minlength=S.GRID)                 # noqa: E731
    want = {ER.ROWS: S.set_counts(T, N, 1), ER.N_: count(None).astype(np.float64),
            ER.LSUM: count([ep.length for ep in w.episodes]), ER.TIMEOUTS: count([float(ep.timeout) for ep in w.episodes])}
    walks = np.bincount(S.workgroup_of(N, 1), minlength=S.GRID)
    for field, name in ((ER.ROWS, "rows"), (ER.N_, "episodes"), (ER.LSUM, "length sum"), (ER.TIMEOUTS, "time-outs")):
        for g in np.flatnonzero(sets[:, field] != want[field]):
            raise AssertionError("%s: set %d has %s %g; its workgroup walks %d env(s) in %d trip(s): %g (%d sets are off)"
                                 % (what, g, name, sets[g, field], walks[g], walks[g], want[field][g],
                                    int((sets[:, field] != want[field]).sum())))


@pytest.mark.parametrize("T,N", S.EPISODE_SCAN_SHAPES)
def test_episode_stats_scan(T, N):
    _trips(N, 1)
    for pattern in ES.PATTERNS:
        for carry in (False, True):
            what = "episode_stats_scan_kernel T=%d N=%d %s carry=%s" % (T, N, pattern, carry)
            reward, reset, progress, cr, cl = ES._case(T, N, pattern, carry)
            w = ER.walk(reward, reset, progress, ES.MEL, cr, cl)
            run = ES._launch(reward, reset, progress, cr, cl, 4)
            sets, cr_out, cl_out = run
            assert np.array_equal(cl_out, w.carry_len), "%s carry_len: %s" % (what, S.describe(cl_out != w.carry_len, 1))
            _check_episode_sets(sets, w, T, N, what)
            ES._check_sets_shape(sets, T, N, 4)
            ES._check_set(ER.pool(sets), w, T * N, what)
            ES._check_carries(cr_out, cl_out, w, what)                                  # every env's, not only the first trip's
            if pattern == "none":
                assert not w.episodes and np.array_equal(cl_out, cl + T)
            if pattern in ("last", "every"):
                assert (cr_out == 0).all() and (cl_out == 0).all()
            if pattern == "every":
                assert ER.pool(sets)[ER.N_] == T * N
            if pattern in ("random", "span"):
                _identical(run, ES._launch(reward, reset, progress, cr, cl, 4), what)
    print("T %d N %d scan: worst |error| / bound so far %s" % (T, N, {k: "%.3g" % v for k, v in sorted(ES.WORST.items())}))


@pytest.mark.parametrize("T,N", S.EPISODE_SCAN_SHAPES)
def test_episode_stats_scan_two_chained_launches_equal_one(T, N):
    """2 T rows in two launches, the carries of all N envs handed on, against one launch over the concatenation: the
    neighbouring file's test at these shapes."""
    _trips(N, 1)
    ES.test_two_chained_launches_and_the_merge_equal_one_launch(T, N, 4)


# ------------------------------------------------------------------------------------------------------------ in the agent
def _agent(monkeypatch, n, gae, **kw):
    """One rollout of a new agent with value normalisation on, make_data in place of the update (tests/test_lambda_returns_gpu.py's
    construction: a committed table that is not the identity), and the `mode` every launch of the three entry points was given."""
    from fly_bproject_amd import _lib
    from tests.test_lambda_returns_gpu import COMMITTED, _rollout_with_make_data
    api, modes = _lib.api(), {}
    for name in ("ppo_td_gae_vnorm", "ppo_td_gae_episodic_vnorm", "ppo_episode_stats"):
        def spy(*args, _real=getattr(api, name), _name=name):
            modes.setdefault(_name, []).append(args[-2])                               # (..., sets, mode, stream)
            return _real(*args)
        monkeypatch.setattr(api, name, spy)
    seen = {}
    agent = _rollout_with_make_data(n, True, seen, normalize_value=True, gae=gae, **kw)
    got = {k: v.cpu().numpy() for k, v in seen.items() if k != "data" and not k.endswith("_adv_norm")}
    got["reward"] = agent.all_reward.cpu().numpy()[..., 0]
    got["sets"] = agent._value_sets.cpu().numpy()
    assert tuple(got["_value_stats"]) == COMMITTED
    np.testing.assert_array_equal(got["_value_table"], V.table(COMMITTED))
    return agent, got, modes


def _check_agent(agent, got, gae, per):
    """make_data's outputs against the references on the agent's own rewards, critic outputs and flag rows."""
    from tests.test_lambda_returns_gpu import COMMITTED
    T, n = agent.rollout_size, int(agent.args.num_envs)
    v, tab = got["_v_ring"][..., 0], got["_value_table"]
    raw, adv = got["_target"][..., 0], got["all_advantage"][..., 0]
    what = "PPO %d envs, T = %d, gae %s" % (n, T, gae)
    if gae == "episodic":
        mel = agent.env.max_episode_length
        case = (got["reward"], v[:T], v[1:], agent._reset_rows.cpu().numpy(), agent._progress_rows.cpu().numpy(),
                agent._ended_prev.cpu().numpy())
        ended, timeout, stale = E.flags_of(*case[3:], mel)
        assert stale[0].all()                                         # the first step performs the env's first reset
        print("%s: %d falls, %d time-outs" % (what, int((ended & ~timeout).sum()), int(timeout.sum())))
        (GE.check_scan if per == 1 else GE.check_lane)(case, raw, adv, tab, maxlen=mel, where=_where(per))
        assert (adv[stale] == 0).all() and np.array_equal(raw[stale], V.denormalize(v[:T], tab)[stale])
    else:
        case = (got["reward"], v[:T], v[1:], agent.all_done.to(torch.float32).cpu().numpy().reshape(-1))
        t32, a32 = V.td_gae(*case, tab, mode=0)
        _same(raw, t32, per, what + " targets")
        ref = S.td_ref64(case, tab, 0)
        if per == 1:
            RK.check_scan(what, T, n, 0, raw, adv, ref, where=_where(per))
        else:
            _same(adv, a32, per, what + " advantages")
            assert (np.abs(adv - ref.adv) <= 2 * ref.bound).all()
    # the moment sets, the scratch statistics and table, the normalised targets
    _check_set_counts(got["sets"], T, n, per, what)
    stats = tuple(float(x) for x in got["_value_stats_next"])
    wc, wmean, wvar = V.merge(COMMITTED, raw)
    print("%s: scratch statistics %r, float64 merge of the targets %r" % (what, stats, (wc, wmean, wvar)))
    assert stats[0] == wc == COMMITTED[0] + T * n
    np.testing.assert_allclose(stats[1], wmean, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(stats[2], wvar, rtol=1e-10, atol=0)
    np.testing.assert_array_equal(got["_value_table_next"], V.table(stats))
    np.testing.assert_array_equal(got["_target_norm"][..., 0], V.normalize(raw, got["_value_table_next"]))


@pytest.mark.parametrize("gae", ["reference", "episodic"])
def test_ppo_300_envs_takes_the_scan_kernels_past_the_grid(monkeypatch, gae):
    """The reference's recorded shape (300 envs, T = 2176) with value normalisation and episode statistics: make_data and the
    episode pass choose the scan form, whose 256 workgroups then walk 300 envs."""
    agent, got, modes = _agent(monkeypatch, 300, gae, episode_stats=True)
    T, n = agent.rollout_size, 300
    assert T == 2176 and n < 512 and T >= 1024                                         # the rule of make_data ...
    entry = "ppo_td_gae_episodic_vnorm" if gae == "episodic" else "ppo_td_gae_vnorm"
    assert modes == {entry: [4, 4], "ppo_episode_stats": [4]}, modes                  # ... and what it was seen to choose
    assert n > S.GRID and _trips(n, 1) == 2
    _check_agent(agent, got, gae, 1)
    # the episode pass: total, the carries of every env, every workgroup's set
    mel = agent.env.max_episode_length
    w = ER.walk(got["reward"], agent._reset_rows.cpu().numpy(), agent._progress_rows.cpu().numpy(), mel)
    what = "PPO 300 envs, gae %s, episode statistics" % gae
    assert len(w.episodes) > 100 and len({ep.env for ep in w.episodes if ep.env >= S.GRID}) > 10
    _check_episode_sets(agent._ep_sets.cpu().numpy(), w, T, n, what)
    ES._check_set(agent._ep_total.cpu().numpy(), w, T * n, what)
    ES._check_carries(agent._ep_carry_ret.cpu().numpy(), agent._ep_carry_len.cpu().numpy(), w, what)
    print("%s: worst |error| / bound so far %s" % (what, {k: "%.3g" % v for k, v in sorted(ES.WORST.items())}))
    agent.exit()


@pytest.mark.parametrize("gae", ["reference", "episodic"])
def test_ppo_20480_envs_takes_the_lane_kernels_past_the_grid(monkeypatch, gae):
    agent, got, modes = _agent(monkeypatch, 20480, gae)
    T, n = agent.rollout_size, 20480
    assert T == 32 and not (n < 512 and T >= 1024)
    assert modes == {"ppo_td_gae_episodic_vnorm" if gae == "episodic" else "ppo_td_gae_vnorm": [0, 0]}, modes
    assert n > S.WAVE * S.GRID and _trips(n, S.WAVE) == 2
    _check_agent(agent, got, gae, S.WAVE)
    agent.exit()
