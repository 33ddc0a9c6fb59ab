"""The strided-env tests' own premises, without a GPU: at every shape tests/test_strided_envs_gpu.py runs, the references
alone satisfy what that file asserts of the kernels.

  trips       every shape list reaches a second trip of some workgroup at every shape and a third at one of them
  counts      the per-set count formula (workgroup g walks env blocks / envs g, g + grid, ...) sums to T N, against a plain loop
  kinds       the flag generator puts every env kind into every trip of five or more envs; the lone env of a ragged last trip
              is not a quiet one; the flags have the properties their kind names
  float32     the float32 restatements the lane = env kernels are held to bit for bit stay within the stated bounds of their
              float64 references (2 x the first-order bound); the sequential float64 returns of the episode walk stay within
              the recursive-summation bound of the correctly rounded ones"""
import numpy as np
import pytest

from tests import episode_stats_ref as ER
from tests import gae_episodic_ref as E
from tests import rollout_ref as R
from tests import strided_envs_cases as S
from tests import value_norm_ref as V

LANE = [(T, N, S.WAVE, S.GRID) for T, N in S.LANE_SHAPES]
SCAN = [(T, N, 1, S.GRID) for T, N in S.SCAN_SHAPES]
PLAIN = [(T, N, 1, S.plain_scan_grid(N)) for T, N in S.PLAIN_SCAN_SHAPES]
EPISODE = [(T, N, 1, S.GRID) for T, N in S.EPISODE_SCAN_SHAPES]


@pytest.mark.parametrize("shapes", [LANE, SCAN, PLAIN, EPISODE], ids=["lane", "scan", "plain_scan", "episode_scan"])
def test_every_list_reaches_a_second_trip_everywhere_and_a_third_somewhere(shapes):
    assert all(S.trips(N, per, grid) >= 2 for _, N, per, grid in shapes)
    assert any(S.trips(N, per, grid) == 3 for _, N, per, grid in shapes)
    for _, N, per, grid in shapes:                            # ragged: the last trip is not a full one
        assert -(-N // per) % grid != 0


@pytest.mark.parametrize("T,N,per,grid", LANE + SCAN + PLAIN + EPISODE)
def test_set_counts_are_the_documented_assignment(T, N, per, grid):
    want = np.zeros(grid)
    for g in range(min(grid, S.GRID)):                        # the loop the kernels run, for the workgroups with a set
        e = g * per
        while e < N:
            want[g] += T * min(per, N - e)
            e += grid * per
    got = S.set_counts(T, N, per, grid)
    if grid == S.GRID:
        assert np.array_equal(got, want)
    assert got.sum() == T * N
    trip = S.trip_of(N, per, grid)
    assert np.array_equal(np.unique(trip), np.arange(S.trips(N, per, grid)))
    assert S.workgroup_of(N, per, grid)[trip > 0].min() == 0 and (S.workgroup_of(N, per, grid) < grid).all()


@pytest.mark.parametrize("T,N,per,grid", LANE + SCAN + PLAIN)
def test_flags_put_every_kind_into_every_trip(T, N, per, grid):
    case = S.episodic_case(T, N, per, grid)
    r, v, vn, reset, progress, prev = case
    kind, trip = S.kinds_of(N, per, grid), S.trip_of(N, per, grid)
    ended, timeout, stale = E.flags_of(reset, progress, prev, S.MAXLEN)
    for k in range(S.trips(N, per, grid)):
        here = trip == k
        if here.sum() >= len(S.KINDS):
            assert set(kind[here]) == set(range(len(S.KINDS))), k
            # and by what the rows hold, whatever the generator calls them
            assert (ended & ~timeout & ~stale)[:, here].any(), "trip %d: no fall" % k
            assert (timeout & ~stale)[:, here].any(), "trip %d: no time-out" % k
            assert (stale & ended)[:, here].any(), "trip %d: no end in a stale row" % k
            assert (prev[here] != 0).any() and (~ended.any(axis=0) & (prev == 0))[here].any(), k
            assert ((progress >= S.MAXLEN - 1) & ~ended)[:, here].any(), "trip %d: no progress at the limit without the flag" % k
            assert ((progress > S.MAXLEN - 1) & ended)[:, here].any() or T < 13, "trip %d: no time-out beyond the limit" % k
            if T > 1:
                assert (ended[1:] & ended[:-1])[:, here].any(), "trip %d: no two consecutive ends" % k
        else:
            assert here.sum() == 1 and k > 0 and S.KINDS[kind[here][0]] == ("carried", "fall_timeout")[k - 1]
    # the kinds are what they say
    of = {name: np.flatnonzero(kind == i) for i, name in enumerate(S.KINDS)}
    assert not ended[:, of["quiet"]].any() and not prev[of["quiet"]].any()
    assert stale[0, of["carried"]].all() and ended[min(1, T - 1), of["carried"]].all()
    assert ended[0, of["fall_timeout"]].all() and timeout[T - 1, of["fall_timeout"]].all()
    assert ended[:, of["boundary"]].any(axis=0).all()
    if len(R.scan_chunks(T)) >= 7:                            # an end in the last step of one chunk and in the first of another
        L = -(-T // 64)
        t_end = [np.flatnonzero(ended[:, e]) for e in of["boundary"][:4]]
        assert all(len(t) == 2 and (T - 1 - t[1]) % L == 0 and (T - 1 - t[0]) % L == L - 1 for t in t_end)


@pytest.mark.parametrize("T,N,per,grid", LANE + SCAN + PLAIN)
def test_episodic32_is_within_the_bounds_of_episodic64(T, N, per, grid):
    gamma, gl = R.gamma_gl32()
    for table in (None, V.table(S.TABLE_S)):
        case = S.episodic_case(T, N, per, grid)
        if table is not None:
            case = ((case[0] * 20).astype(np.float32),) + case[1:]
        t32, a32 = E.episodic32(*case, S.MAXLEN, table)
        ref = E.episodic64(*case, S.MAXLEN, gamma, gl, table)
        assert (np.abs(t32 - ref.target) <= 2 * ref.target_err).all()
        assert (np.abs(a32 - ref.adv) <= 2 * ref.bound).all()
        assert ref.moments[0] == T * N
        if per == 1:                                          # the scan form's allowance on top is finite and not negative
            extra = E.scan_carry_bound64_masked(ref.delta, ref.live, gl)
            assert np.isfinite(extra).all() and (extra >= 0).all()


@pytest.mark.parametrize("T,N,per,grid", LANE + SCAN)
def test_td_gae32_is_within_the_bounds_of_td_gae64(T, N, per, grid):
    table = V.table(S.TABLE_S)
    for mode in (range(4) if per == S.WAVE else (0, 1)):
        case = S.td_case(T, N, mode)
        t32, a32 = V.td_gae(*case, table, mode=mode)
        ref = S.td_ref64(case, table, mode)
        assert (np.abs(t32 - ref.target) <= R.target_bound64(ref)).all()
        assert (np.abs(a32 - ref.adv) <= 2 * ref.bound).all()
        if per == 1:
            extra = R.scan_carry_bound64(ref.delta, R.gamma_gl32()[1])
            assert np.isfinite(extra).all() and (extra >= 0).all()


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("T,N,per,grid", LANE + SCAN)
def test_hard_rewards_are_their_own_targets(T, N, per, grid, kind):
    """v = v_next = 0 under a table with m = 0: the float32 targets are the rewards, in both estimators."""
    x, zeros, _ = S.hard_case(kind, T, N)
    table = V.table(V.initial())
    assert table[0] == 0
    assert np.array_equal(V.td_gae(x, zeros, zeros, np.ones(N, np.float32), table)[0], x)
    assert np.array_equal(E.episodic32(x, zeros, zeros, *S.no_flags(T, N), S.MAXLEN, table)[0], x)
    assert V.moments(x)[0] == T * N == S.set_counts(T, N, per).sum()


@pytest.mark.parametrize("T,N,per,grid", EPISODE)
def test_episode_walks_are_within_their_summation_bound(T, N, per, grid):
    from tests.test_episode_stats_gpu import MEL, PATTERNS, _case
    for pattern in PATTERNS:
        for carry in (False, True):
            reward, reset, progress, cr, cl = _case(T, N, pattern, carry)
            w = ER.walk(reward, reset, progress, MEL, cr, cl)
            for ep in w.episodes:
                assert abs(ep.ret - ep.exact) <= ER.return_bound(ep)
            assert (np.abs(w.carry_ret - w.carry_exact) <= ER.return_bound(w.carry_terms, w.carry_abs)).all()
            # every env's rows are in some episode or in its carry: lengths add up, workgroup by workgroup
            rows = np.bincount(np.array([ep.env for ep in w.episodes], np.int64), weights=[ep.length for ep in w.episodes], minlength=N)
            walked = rows + w.carry_len - np.asarray(cl)
            assert np.array_equal(walked, np.full(N, T))
            assert np.array_equal(np.bincount(S.workgroup_of(N, 1), weights=walked, minlength=S.GRID), S.set_counts(T, N, 1))
