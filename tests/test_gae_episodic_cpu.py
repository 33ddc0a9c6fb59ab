"""CPU: the episode-aware advantage estimate (PPO gae="episodic") -- the references of tests/gae_episodic_ref.py against
hand-computed cases, against rollout_ref's masked recurrence when no flag is set, the independence of episodes (and its absence
under the reference's estimator: the defect this feature removes), the restated scan bound, and the public surface."""
import os
import re

import numpy as np
import pytest

from tests import gae_episodic_ref as E
from tests import rollout_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G32, GL32 = R.gamma_gl32()
G, GL = float(G32), float(GL32)
MAXLEN = 1000


def col(*x):
    return np.array(x, np.float32).reshape(-1, 1)


def flags(T, ends=(), timeouts=(), prev=0):
    """One env: reset / progress rows with ends at `ends` (falls) and `timeouts`, and the flag carried in."""
    reset, progress = np.zeros((T, 1), np.int64), np.full((T, 1), 7, np.int64)
    for t in ends:
        reset[t] = 1
    for t in timeouts:
        reset[t], progress[t] = 1, MAXLEN - 1
    return reset, progress, np.array([prev], np.int64)


def both(r, v, vn, fl, table=None):
    """The float64 reference and the float32 restatement; asserts that they agree to float32 rounding, returns float64."""
    ref = E.episodic64(r, v, vn, *fl, MAXLEN, G32, GL32, table)
    tg, adv = E.episodic32(r, v, vn, *fl, MAXLEN, table)
    assert (np.abs(tg - ref.target) <= 2 * ref.target_err).all() and (np.abs(adv - ref.adv) <= 2 * ref.bound).all()
    return ref.target[:, 0], ref.adv[:, 0]


R4, V4, VN4 = col(1.0, 2.0, 3.0, 4.0), col(0.5, 0.25, -1.0, 2.0), col(0.25, -1.0, 2.0, 8.0)
r, v, vn = R4[:, 0].astype(np.float64), V4[:, 0].astype(np.float64), VN4[:, 0].astype(np.float64)


def test_fall_at_t1():
    """T = 4, a fall at t = 1: no bootstrap at t = 1, the recurrence stops there, t = 2 is stale."""
    tg, a = both(R4, V4, VN4, flags(4, ends=[1]))
    a3 = r[3] + G * vn[3] - v[3]
    a1 = r[1] - v[1]
    np.testing.assert_allclose(tg, [r[0] + G * vn[0], r[1], v[2], r[3] + G * vn[3]], rtol=1e-15)
    np.testing.assert_allclose(a, [GL * a1 + (r[0] + G * vn[0] - v[0]), a1, 0.0, a3], rtol=1e-15)


def test_timeout_at_t1():
    """The same with a time-out: the target at t = 1 contains gamma v_next, the recurrence still stops."""
    tg, a = both(R4, V4, VN4, flags(4, timeouts=[1]))
    a1 = r[1] + G * vn[1] - v[1]
    assert tg[1] == r[1] + G * vn[1] and tg[2] == v[2]
    np.testing.assert_allclose(a, [GL * a1 + (r[0] + G * vn[0] - v[0]), a1, 0.0, r[3] + G * vn[3] - v[3]], rtol=1e-15)


def test_timeout_needs_the_end_flag_and_the_limit():
    """progress at the limit without the flag is no end; the flag with progress one short of the limit is a fall."""
    fl = flags(4)
    fl[1][1] = MAXLEN - 1
    tg, a = both(R4, V4, VN4, fl)
    ref = R.td_gae64(R4, V4, VN4, np.ones((4, 1), np.float32), G32, GL32, 3)
    assert np.array_equal(tg, ref.target[:, 0]) and np.array_equal(a, ref.adv[:, 0])
    fl = flags(4, ends=[1])
    fl[1][1] = MAXLEN - 2
    assert both(R4, V4, VN4, fl)[0][1] == r[1]
    fl[1][1] = MAXLEN + 5
    assert both(R4, V4, VN4, fl)[0][1] == r[1] + G * vn[1]


def test_stale_row_and_ended_prev():
    """ended_prev set: row 0 is stale -- a = 0, tg = v -- and nothing else changes."""
    tg, a = both(R4, V4, VN4, flags(4, prev=1))
    tg0, a0 = both(R4, V4, VN4, flags(4))
    assert a[0] == 0.0 and tg[0] == v[0]
    assert np.array_equal(tg[1:], tg0[1:]) and np.array_equal(a[1:], a0[1:])


def test_consecutive_ends():
    """Ends at t = 1 and t = 2: row 2 is stale (stale wins over ended), row 3 is stale too, row 1 is an ordinary fall."""
    tg, a = both(R4, V4, VN4, flags(4, ends=[1, 2]))
    np.testing.assert_allclose(tg, [r[0] + G * vn[0], r[1], v[2], v[3]], rtol=1e-15)
    np.testing.assert_allclose(a, [GL * (r[1] - v[1]) + (r[0] + G * vn[0] - v[0]), r[1] - v[1], 0.0, 0.0], rtol=1e-15)


def test_end_at_the_last_step():
    """A fall at t = T - 1: no bootstrap there; a time-out at t = T - 1: the bootstrap stays."""
    tg, a = both(R4, V4, VN4, flags(4, ends=[3]))
    assert tg[3] == r[3] and a[3] == r[3] - v[3]
    np.testing.assert_allclose(a[2], GL * a[3] + (r[2] + G * vn[2] - v[2]), rtol=1e-15)
    tg, a = both(R4, V4, VN4, flags(4, timeouts=[3]))
    assert tg[3] == r[3] + G * vn[3]


def test_under_a_value_table():
    """v and v_next are denormalised first; the stale target is the denormalised v."""
    table = np.array([3.0, 2.0, 0.5, 0.0], np.float32)
    tg, a = both(R4, V4, VN4, flags(4, ends=[1]), table)
    vd, vnd = 2 * v + 3, 2 * vn + 3
    np.testing.assert_allclose(tg, [r[0] + G * vnd[0], r[1], vd[2], r[3] + G * vnd[3]], rtol=1e-15)
    np.testing.assert_allclose(a[1:], [r[1] - vd[1], 0.0, r[3] + G * vnd[3] - vd[3]], rtol=1e-15)
    ref = E.episodic64(R4, V4, VN4, *flags(4, ends=[1]), MAXLEN, G32, GL32, table)
    assert ref.moments[0] == 4 and abs(ref.moments[1] - tg.mean()) < 1e-12 and abs(ref.moments[2] - tg.var()) < 1e-12


def _random(T, N, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(0, 1, (T, N)).astype(np.float32) for _ in range(3))


def test_no_flags_is_the_masked_recurrence_with_done_one():
    T, N = 37, 5
    rw, vv, vvn = _random(T, N, 1)
    z = np.zeros((T, N), np.int64)
    ref = E.episodic64(rw, vv, vvn, z, z + MAXLEN, np.zeros(N, np.int64), MAXLEN, G32, GL32)
    want = R.td_gae64(rw, vv, vvn, np.ones((T, N), np.float32), G32, GL32, R.GAE_DONE_PER_STEP | R.GAE_MASK_RECURRENCE)
    assert np.array_equal(ref.target, want.target) and np.array_equal(ref.adv, want.adv)
    assert np.array_equal(ref.bound, want.bound) and ref.live.all()
    t32, a32 = E.episodic32(rw, vv, vvn, z, z + MAXLEN, np.zeros(N, np.int64), MAXLEN)
    assert (np.abs(t32 - want.target) <= R.target_bound64(want)).all() and (np.abs(a32 - want.adv) <= 2 * want.bound).all()


@pytest.mark.parametrize("kind", ["fall", "timeout"])
def test_episodes_are_independent(kind):
    """Perturbing reward / v / v_next of any row after an end leaves every row at or before that end unchanged -- and changes
    them under the reference's estimator (mode 0), where the recurrence runs through the end."""
    T, N, end = 12, 3, 6
    rw, vv, vvn = _random(T, N, 2)
    reset, progress = np.zeros((T, N), np.int64), np.full((T, N), 3, np.int64)
    reset[end] = 1
    if kind == "timeout":
        progress[end] = MAXLEN - 1
    prev = np.zeros(N, np.int64)
    base = E.episodic64(rw, vv, vvn, reset, progress, prev, MAXLEN, G32, GL32)
    b32 = E.episodic32(rw, vv, vvn, reset, progress, prev, MAXLEN)
    old = R.td_gae64(rw, vv, vvn, np.ones(N, np.float32), G32, GL32, 0)
    for t in range(end + 1, T):
        for which in range(3):
            arrs = [rw.copy(), vv.copy(), vvn.copy()]
            arrs[which][t] += 10.0
            got = E.episodic64(*arrs, reset, progress, prev, MAXLEN, G32, GL32)
            assert np.array_equal(got.target[:end + 1], base.target[:end + 1]), (t, which)
            assert np.array_equal(got.adv[:end + 1], base.adv[:end + 1]), (t, which)
            g32 = E.episodic32(*arrs, reset, progress, prev, MAXLEN)
            assert np.array_equal(g32[0][:end + 1], b32[0][:end + 1]) and np.array_equal(g32[1][:end + 1], b32[1][:end + 1])
            leaked = R.td_gae64(*arrs, np.ones(N, np.float32), G32, GL32, 0)
            assert (leaked.adv[:end + 1] != old.adv[:end + 1]).all(), (t, which)       # the defect: every earlier row moves


@pytest.mark.parametrize("T", [1, 63, 65, 200, 1025])
def test_restated_scan_bound(T):
    """With every step live the restated bound is rollout_ref.scan_carry_bound64 value for value; an end cuts what reaches the
    rows before it to exactly nothing."""
    N = 2
    delta = np.random.default_rng(T).normal(0, 1, (T, N))
    assert np.array_equal(E.scan_carry_bound64_masked(delta, np.ones((T, N), bool), GL32), R.scan_carry_bound64(delta, GL32))
    if T < 65:
        return
    live = np.ones((T, N), bool)
    chunks = R.scan_chunks(T)
    t_lo, t_hi = chunks[1]
    live[t_lo, 0] = False                                    # env 0: an end at the first step of the second-latest chunk
    got = E.scan_carry_bound64_masked(delta, live, GL32)
    full = R.scan_carry_bound64(delta, GL32)
    assert np.array_equal(got[:, 1], full[:, 1])             # the other env is untouched
    assert np.array_equal(got[t_lo + 1:, 0], full[t_lo + 1:, 0]) and got[t_lo, 0] == 0      # after the end nothing changes
    loud = delta.copy()
    loud[t_lo + 1:, 0] *= 1e6                                # whatever lies after the end reaches no row at or before it
    assert np.array_equal(E.scan_carry_bound64_masked(loud, live, GL32)[:t_lo + 1, 0], got[:t_lo + 1, 0])
    assert not np.array_equal(R.scan_carry_bound64(loud, GL32)[:t_lo + 1, 0], full[:t_lo + 1, 0])


def test_trainer_flag():
    import trainer
    assert trainer.parse_args([]).gae == "reference"
    assert trainer.parse_args(["--gae", "episodic"]).gae == "episodic"
    with pytest.raises(SystemExit):
        trainer.parse_args(["--gae", "lambda"])
    assert "NOT the reference" in open(os.path.join(REPO, "trainer.py")).read()            # the help text says so


def test_abi_version_and_new_symbols():
    from fly_bproject_amd import _lib
    assert _lib.ABI_VERSION == 13
    for name in ("ppo_td_gae_episodic", "ppo_td_gae_episodic_vnorm"):
        assert name in _lib.SYMBOLS, name                            # (each row is held to the header: tests/test_abi_cpu.py)
    assert re.search(r"^#define FLY_ABI_VERSION 13\b", open(os.path.join(REPO, "include", "flyhip.h")).read(), flags=re.M)
    assert "return FLY_ABI_VERSION;" in open(os.path.join(REPO, "fly_bproject_amd", "csrc", "flyhip_abi.hip")).read()
