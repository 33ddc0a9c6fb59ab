"""Shapes, inputs and the env -> workgroup assignment of the strided-env tests (tests/test_strided_envs_gpu.py and
tests/test_strided_envs_cpu.py): PPO's post-rollout kernels that launch a fixed grid and stride over the envs beyond it.

    kernel                              one trip covers        workgroup g walks
    ppo_td_gae_vnorm_kernel<MODE>       a block of 64 envs     env blocks g, g + 256, ...
    gae_episodic_kernel<true>           a block of 64 envs     env blocks g, g + 256, ...
    ppo_td_gae_vnorm_scan_kernel<MODE>  one env                envs g, g + 256, ...
    gae_episodic_scan_kernel<true>      one env                envs g, g + 256, ...
    episode_stats_scan_kernel           one env                envs g, g + 256, ...
    gae_episodic_scan_kernel<false>     one env                envs g, g + grid, ... with grid = min(N, 65536)

`per` below is the envs of one trip (64: lane = env, 1: scan), `grid` the workgroups.  Nothing here needs a GPU or the library:
numpy, and the references of tests/value_norm_ref.py, tests/rollout_ref.py and tests/gae_episodic_ref.py."""
import functools

import numpy as np

from tests import rollout_ref as R
from tests import value_norm_ref as V

GRID = 256                                   # FLY_VALUE_NORM_SETS == FLY_EPISODE_SETS: the fixed grid, one set per workgroup
WAVE = 64
SCAN_GRID_MAX = 65536                        # gae_episodic.hip: the plain scan form's grid cap
MAXLEN = 50                                  # max_episode_length of the synthetic flag rows (tests/test_gae_episodic_gpu.py's)
TABLE_S = (1000.0, 37.5, 44444.0)            # mean 37.5, std ~ 211: tests/test_value_norm_gpu.py's non-trivial table
f32 = np.float32

# (T, N): the smallest N at which a workgroup makes a second and a third trip, with ragged ends; T tiny, but on both sides of
# the scan's chunking (T = 1: one lane owns everything; 64: one step per lane; 65, 129: a ragged last lane)
LANE_SHAPES = [(1, 16385), (3, 16384 + 65), (2, 2 * 16384 + 1)]
SCAN_SHAPES = [(1, 257), (65, 257), (129, 300), (64, 513)]
# the plain episodic scan: past its grid cap, and (2, 2 * 65536 + 1) for the third trip that 65537 envs cannot give it
PLAIN_SCAN_SHAPES = [(2, 65537), (65, 65537), (2, 2 * 65536 + 1)]
EPISODE_SCAN_SHAPES = [(T, N) for T in (1, 65, 129) for N in (257, 300, 513)]


# ---------------------------------------------------------------------------------------------------- who walks which env
def plain_scan_grid(N):
    return min(int(N), SCAN_GRID_MAX)


def workgroup_of(N, per, grid=GRID):
    """[N]: the workgroup that walks env e."""
    return (np.arange(N) // per) % grid


def trip_of(N, per, grid=GRID):
    """[N]: on which of its trips (0 = first) that workgroup reaches env e."""
    return (np.arange(N) // per) // grid


def trips(N, per, grid=GRID):
    """The trips of the busiest workgroup (workgroup 0)."""
    return int(trip_of(N, per, grid)[-1]) + 1


def set_counts(T, N, per, grid=GRID):
    """[grid] float64: the (t, e) rows workgroup g walks -- the count of its moment set, the `rows` of its episode set."""
    return T * np.bincount(workgroup_of(N, per, grid), minlength=grid).astype(np.float64)


def describe(miss, per, grid=GRID):
    """What an assertion says about a bool [T][N] (or [N]) of misses: the first one with its workgroup and trip, and the
    misses per trip."""
    miss = np.asarray(miss, bool)
    N = miss.shape[-1]
    trip = trip_of(N, per, grid)
    envs = miss.reshape(-1, N).any(axis=0)
    first = int(np.flatnonzero(envs)[0])
    t = int(np.flatnonzero(miss.reshape(-1, N)[:, first])[0])
    per_trip = {int(k): int(envs[trip == k].sum()) for k in range(int(trip[-1]) + 1)}
    return ("first miss at t = %d, env %d: workgroup %d on its trip %d (0 = first); envs with a miss per trip %r"
            % (t, first, int(workgroup_of(N, per, grid)[first]), int(trip[first]), per_trip))


# ------------------------------------------------------------------------------------------------ ppo_td_gae_vnorm inputs
def td_case(T, N, mode):
    """Rewards of scale 20, critic outputs of unit scale, done ~ Bernoulli(0.9) per step (mode & 1) or per env -- the inputs
    tests/test_value_norm_gpu.py::test_nontrivial_table_against_the_float32_reference draws."""
    rng = np.random.default_rng([T, N, mode & 3])
    r = (rng.normal(0, 1, (T, N)).astype(f32) * 20).astype(f32)
    v, vn = rng.normal(0, 1, (T, N)).astype(f32), rng.normal(0, 1, (T, N)).astype(f32)
    d = (rng.random((T, N) if mode & 1 else (N,)) < 0.9).astype(f32)
    return r, v, vn, d


def td_ref64(case, table, mode):
    """rollout_ref.td_gae64 on the critic outputs denormalised in float32 (value_norm_ref.denormalize: elementwise, so bit
    for bit what the kernels hold): its bounds are those of tests/test_rollout_kernels_gpu.py, in reward units."""
    r, v, vn, d = case
    gamma, gl = R.gamma_gl32()
    return R.td_gae64(r, V.denormalize(v, table), V.denormalize(vn, table), d, gamma, gl, mode & 3)


def hard_case(kind, T, N):
    """value_norm_ref.hard_rewards with v = v_next = 0 and done = 1: under a table with m = 0 the target IS the reward."""
    x = V.hard_rewards(kind, T, N, seed=N)
    zeros = np.zeros((T, N), f32)
    return x, zeros, zeros


# -------------------------------------------------------------------------------------------------------- episodic flags
KINDS = ("quiet", "carried", "fall_timeout", "boundary", "random")


def kinds_of(N, per, grid=GRID):
    """[N] index into KINDS: (lane + workgroup + trip) mod 5.  Neighbouring lanes, neighbouring workgroups and the successive
    trips of one workgroup all differ in kind, so a trip of at least five envs holds every kind; the lone env of a ragged last
    trip (lane 0 of workgroup 0) has kind `trip`: "carried" on the second trip, "fall_timeout" on the third."""
    e = np.arange(N)
    return (e % per + workgroup_of(N, per, grid) + trip_of(N, per, grid)) % len(KINDS)


@functools.lru_cache(maxsize=None)
def episodic_case(T, N, per, grid=GRID):
    """(reward, v, v_next, reset, progress, ended_prev), flags in the style of tests/test_gae_episodic_gpu.py's lane_case and
    scan_case, the env's kind from kinds_of:
      quiet         no end and none carried in; progress at the limit at T // 2 without the flag
      carried       an end carried in (row 0 is stale); ends at t = 1 and t = 2 (T < 3: in every row), falls: consecutive ends
      fall_timeout  a fall at t = 0 and a time-out at T - 1 (T = 1: the time-out)
      boundary      ends on the scan's chunk boundaries: the last step of chunk 2 and the first step of the chunk that follows
                    chunk 5 in time, a fall and a time-out, swapped from env to env (fewer than 7 chunks: a fall at T - 1 and
                    progress beyond the limit without the flag at t = 0)
      random        ends at random steps (8 % of them; T < 13: 40 %), half of them time-outs at and beyond the limit"""
    rng = np.random.default_rng([T, N, per, grid])
    r = rng.normal(0.5, 1, (T, N)).astype(f32)
    v, vn = rng.normal(0, 1, (T, N)).astype(f32), rng.normal(0, 1, (T, N)).astype(f32)
    reset = np.zeros((T, N), np.int64)
    progress = rng.integers(1, MAXLEN - 1, (T, N)).astype(np.int64)
    prev = np.zeros(N, np.int64)
    kind = kinds_of(N, per, grid)
    quiet, carried, fall_timeout, boundary, random = (np.flatnonzero(kind == k) for k in range(len(KINDS)))
    progress[T // 2, quiet] = MAXLEN - 1
    prev[carried] = 1
    rows = slice(1, 3) if T >= 3 else slice(0, T)
    reset[rows, carried], progress[rows, carried] = 1, 5
    reset[0, fall_timeout], progress[0, fall_timeout] = 1, 3
    reset[T - 1, fall_timeout], progress[T - 1, fall_timeout] = 1, MAXLEN - 1
    chunks = R.scan_chunks(T)
    if len(chunks) >= 7:
        last_of, first_of = chunks[2][1] - 1, chunks[5][1]
        assert first_of == chunks[4][0]
        reset[last_of, boundary] = reset[first_of, boundary] = 1
        progress[last_of, boundary] = np.where(boundary % 2 == 0, 7, MAXLEN - 1)
        progress[first_of, boundary] = np.where(boundary % 2 == 0, MAXLEN - 1, 7)
    else:
        reset[T - 1, boundary], progress[T - 1, boundary] = 1, 7
        progress[0, boundary] = MAXLEN + 1 if T > 1 else 7
    more = rng.random((T, len(random))) < (0.08 if T >= 13 else 0.4)
    late = more & (rng.random((T, len(random))) < 0.5)
    reset[:, random] = more
    progress[:, random] = np.where(late, MAXLEN - 1 + rng.integers(0, 3, late.shape), progress[:, random])
    return r, v, vn, reset, progress, prev


def no_flags(T, N):
    """Flag rows without an end: with v_next = 0 the episodic target is the reward in every row."""
    z = np.zeros((T, N), np.int64)
    return z, z + 1, np.zeros(N, np.int64)
