"""CPU: the oracle's observation and reward/done packs against the plain-numpy float64 restatement of
tests/env_pack_ref.py, on tables that land on every hard branch of the two packs (exactly, one ulp below and one ulp
above), plus the conditions that keep those tables honest: a count > 0 for each side of each branch, every
one-decision mutant of the restatement detected, and a cap on the share of observation elements that fp32 itself
cannot hold to float64."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import env_pack_ref as R

F = np.float32


def _cfg(n, mode):
    cfg = O.default_config(n)
    cfg.reward_mode = mode
    return cfg


@pytest.fixture(scope="module")
def rtab():
    return R.build_reward_table(O.default_config(1))


@pytest.fixture(scope="module")
def otab():
    return R.build_obs_table(O.default_config(1))


@pytest.fixture(scope="module")
def rref(rtab):
    """the unmutated reward reference, once per reward_mode"""
    out = {}
    for mode in (0, 1):
        cfg = _cfg(rtab["n"], mode)
        out[mode] = R.reward_ref(cfg, rtab["obs"], rtab["targets"], rtab["root"], rtab["contact"], rtab["pot"],
                                 rtab["prev_pot"], rtab["progress"], rtab["reset"])
    return out


@pytest.fixture(scope="module")
def oref(otab):
    cfg = O.default_config(otab["n"])
    ref = R.obs_ref(cfg, otab["root"], otab["dof_pos"], otab["dof_vel"], otab["targets"], otab["contact"], otab["pot"])
    s = R.fill_state(O.EnvState(otab["n"]), otab)
    up, hd = O.pack_obs(cfg, s, want_vecs=True)
    return dict(ref=ref, orc=s, up=up, hd=hd)


def test_tables_have_ragged_sizes(rtab, otab):
    for n in (rtab["n"], otab["n"]):
        assert n % 4 != 0 and n % 32 != 0 and n < 8192
    assert 3000 < rtab["n"] and 1000 < otab["n"] < 2500


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_reward_pack_vs_float64_on_every_branch(rtab, rref, mode):
    """reset and progress bit-equal on EVERY row (no exclusion mask: the table sits on the thresholds), dead rows exactly
    death_cost, live rows within 16 * 2^-24 * mag."""
    cfg = _cfg(rtab["n"], mode)
    s = R.fill_state(O.EnvState(rtab["n"]), rtab)
    O.pack_reward(cfg, s)
    ref = rref[mode]
    assert np.array_equal(s.reset, ref["reset"])
    assert np.array_equal(s.progress, ref["progress"])
    dead = ref["dead"]
    assert np.all(s.reward[dead] == F(cfg.death_cost))
    err = np.abs(s.reward.astype(np.float64) - ref["reward"])
    ratio = err[~dead] / (R.U32 * ref["mag"][~dead])
    print("reward_mode %d: %d rows, %d dead, max |reward - r64| = %.2f x 2^-24 mag" % (mode, rtab["n"], dead.sum(), ratio.max()))
    assert np.all(np.isfinite(ref["reward"])) and np.all(err[~dead] <= R.reward_bound(ref["mag"][~dead]))
    assert np.all(s.reset[rtab["reset"] != 0] == 1)                      # flagged on input: stays flagged
    # the abdomen table's stated verdicts, where nothing else kills the env
    other = ref["d_lo"] | ref["d_hi"] | ref["d_ori"]
    for k, (_, want_dead) in enumerate(R.ABDOMEN_CASES):
        rows = (rtab["abd_case"] == k) & ~other
        assert rows.sum() > 0 and np.all(ref["dead"][rows] == want_dead), k


def test_oracle_obs_pack_vs_float64_on_every_branch(otab, oref):
    """EXACT_COLS bit-equal; prev_pot the pushed pot; every other column within 3e-6 (1 + |ref64|) + 4 |oracle32 - ref64|
    -- which the oracle meets by construction, so what binds it is the CAP: the second term may exceed the first on at most
    1 % of the elements, and on none outside the columns that are ill-conditioned in fp32 (body-frame velocities that
    cancel from 1e4, the Euler angles at gimbal lock and asin next to +-1: columns 1-9 and 66)."""
    ref, s = oref["ref"], oref["orc"]
    for col in R.EXACT_COLS:
        assert np.array_equal(s.obs[:, col].astype(np.float64), ref["obs"][:, col]), col
    assert np.array_equal(s.prev_pot, otab["pot"])
    np.testing.assert_allclose(s.pot, ref["pot"], rtol=1e-6)
    np.testing.assert_allclose(oref["up"], ref["up_vec"], atol=1e-6)
    np.testing.assert_allclose(oref["hd"], ref["heading_vec"], atol=1e-6)
    err, bound, relaxed = R.obs_err_f64(s.obs, s.obs, ref["obs"])
    assert np.all(err <= bound)
    share = relaxed.mean()
    cols = sorted(set(np.nonzero(relaxed)[1].tolist()))
    print("obs table: %d rows; fp32 oracle beyond 3e-6 (1 + |ref|) on %.3f %% of the elements, columns %s" % (otab["n"], 100 * share, cols))
    assert share <= 0.01
    assert set(cols) <= set(range(1, 10)) | {66}


def test_reward_table_reaches_both_sides_of_every_branch(rtab, rref):
    ref = rref[0]
    ori = ref["ori"]
    for thr in (0.5, 0.98, 0.92):
        t = F(thr)
        for v in (np.nextafter(t, F(-np.inf)), t, np.nextafter(t, F(np.inf))):
            assert (ori == v).sum() > 0, (thr, v)
    z = rtab["obs"][:, 0]
    for thr in (O.default_config(1).termination_height, 1.4, 2.1, O.default_config(1).termination_height_up):
        t = F(thr)
        for v in (np.nextafter(t, F(-np.inf)), t, np.nextafter(t, F(np.inf))):
            assert (z == v).sum() > 0, (thr, v)
    assert np.isnan(z).sum() > 0 and np.isposinf(z).sum() > 0 and np.isneginf(z).sum() > 0
    causes = np.stack([ref["d_lo"], ref["d_hi"], ref["d_ori"], ref["d_abd"]], axis=1)
    for k in range(4):                                                   # dead by each cause ALONE
        alone = causes[:, k] & (causes.sum(1) == 1)
        assert alone.sum() > 0, k
    assert (ref["timeout"] & ~ref["dead"] & (rtab["reset"] == 0)).sum() > 0      # reset by the time limit alone
    assert (~ref["timeout"] & ~ref["dead"] & (rtab["reset"] == 0)).sum() > 0     # and rows that go on
    assert ((rtab["progress"] == 0) & (ref["progress"] == 1)).sum() > 0
    assert (ref["lim"] == 0).sum() > 0 and (ref["lim"] == 1).sum() > 0 and (ref["lim"] >= 2).sum() > 0
    hi9 = np.array(O.default_config(1).dof_hi[:], F) * F(0.9)
    lo9 = np.array(O.default_config(1).dof_lo[:], F) * F(0.9)
    oa = rtab["obs"][:, 48:66]
    assert (oa == hi9).sum() > 0 and (oa == np.nextafter(hi9, F(np.inf))).sum() > 0
    assert (oa == lo9).sum() > 0 and (oa == np.nextafter(lo9, F(-np.inf))).sum() > 0
    hp = rtab["obs"][:, 11]
    for v in (R._ulps(0.8, -1), F(0.8), R._ulps(0.8, 1)):
        assert ((hp == v) & ~ref["dead"]).sum() > 0
    _touch_coverage(rtab["contact"])


def _touch_coverage(contact):
    """touching flags of both values from a cancelling triple and from a subnormal one"""
    legs = contact[:, R.NABD:]
    sums = R.body_sums32(contact)[:, R.NABD:]
    cancel = (legs[..., 0] == 1.0) & (legs[..., 1] == -1.0) & (legs[..., 2] == 0.0)
    subn = (legs[..., 0] > 0) & (legs[..., 0] < F(1e-38)) & (legs[..., 1] == 0) & (legs[..., 2] == 0)
    assert cancel.sum() > 0 and np.all(sums[cancel] == 0)                # flag 0 from a triple whose parts are not 0
    assert subn.sum() > 0 and np.all(sums[subn] > 0)                     # flag 1 from a subnormal
    assert (sums < 0).sum() > 0 and (sums > F(1e-3)).sum() > 0


def test_obs_table_reaches_both_sides_of_every_branch(otab, oref):
    ref = oref["ref"]
    s32, s64 = np.abs(ref["sinp32"]), np.abs(ref["sinp"])
    assert (s32 == 1).sum() > 0 and (s32 > 1).sum() > 0 and ((s32 < 1) & (s32 > 1 - 1e-6)).sum() > 0
    assert (s64 == 1).sum() > 0 and (s64 > 1).sum() > 0 and ((s64 < 1) & (s64 > 1 - 1e-6)).sum() > 0
    for nrm in (ref["nrm32"], ref["nrm"]):
        assert (nrm == 0).sum() > 0 and ((nrm > 0) & (nrm < F(1e-9))).sum() > 0 and (nrm == F(1e-9)).sum() > 0
    assert np.signbit(oref["orc"].pot[ref["nrm32"] == 0]).all()          # pot = -0.0 on the target
    obs = ref["obs"]
    two_pi = R.TWO_PI32
    for col in (7, 8, 66):                                               # wrapped to just under 2 pi, and exactly 0
        assert ((obs[:, col] > two_pi - 1e-3) & (obs[:, col] < two_pi)).sum() > 0, col
        assert (obs[:, col] == 0).sum() > 0, col
    _touch_coverage(otab["contact"])
    lo, hi = np.array(O.default_config(1).dof_lo[:], F), np.array(O.default_config(1).dof_hi[:], F)
    assert np.all(otab["dof_pos"][0::3] == lo) and np.all(otab["dof_pos"][1::3] == hi)
    assert np.all(obs[0::3, 12:30] == -1.0) and np.all(obs[1::3, 12:30] == 1.0)


def _reward_mutant_differs(rtab, rref, mutant):
    hit = {}
    for mode in (0, 1):
        cfg = _cfg(rtab["n"], mode)
        m = R.reward_ref(cfg, rtab["obs"], rtab["targets"], rtab["root"], rtab["contact"], rtab["pot"], rtab["prev_pot"],
                         rtab["progress"], rtab["reset"], mutant=mutant)
        ref = rref[mode]
        d = (m["reset"] != ref["reset"]) | (m["progress"] != ref["progress"])
        d |= ~(np.abs(m["reward"] - ref["reward"]) <= R.reward_bound(ref["mag"]))
        hit[mode] = int(d.sum())
    return hit


@pytest.mark.parametrize("mutant", [m for m in R.REWARD_MUTANTS if m not in R.EQUIVALENT_MUTANTS])
def test_reward_table_detects_mutant(rtab, rref, mutant):
    """reset or progress on some row, or the reward by more than the bound.  The done mask is the same in both
    reward_modes; leg_reward is in the standing reward only, so a mutant must show in at least one mode -- and every
    mutant of the done mask in both."""
    hit = _reward_mutant_differs(rtab, rref, mutant)
    print(mutant, hit)
    assert hit[0] > 0 or hit[1] > 0
    if mutant in ("z_lo_le", "z_hi_ge", "ori50_le", "abd_ge", "abd_ne", "abd_onesum", "prog_gt", "prog_max", "prog0_keep",
                  "lim_hi_ge", "lim_lo_le", "lim_hi_only", "up14_ge", "up21_le", "ori98_ge"):
        assert hit[0] > 0 and hit[1] > 0


@pytest.mark.parametrize("mutant", [m for m in R.OBS_MUTANTS if m not in R.EQUIVALENT_MUTANTS])
def test_obs_table_detects_mutant(otab, oref, mutant):
    """an observation element beyond the float64 bound (the plain difference: a forgotten wrap is 2 pi off)"""
    cfg = O.default_config(otab["n"])
    m = R.obs_ref(cfg, otab["root"], otab["dof_pos"], otab["dof_vel"], otab["targets"], otab["contact"], otab["pot"], mutant=mutant)
    ref = oref["ref"]["obs"]
    first, second = R.obs_bound(oref["orc"].obs, ref)
    d = ~(np.abs(m["obs"] - ref) <= first + second)
    print(mutant, int(d.sum()), sorted(set(np.nonzero(d)[1].tolist())))
    assert d.sum() > 0
    # and the check the GPU test applies (circle only next to the wrap point) sees it too
    err = R.angle_err(m["obs"], ref, first + second)
    assert (~(err <= first + second)).sum() > 0 or mutant == "pymod_le"      # 0 -> 2 pi IS the wrap point


@pytest.mark.parametrize("mutant", sorted(R.EQUIVALENT_MUTANTS))
def test_equivalent_mutants_are_equivalent_at_their_decision_point(rtab, rref, otab, oref, mutant):
    """Four of the decisions cannot be pinned by any input: both arms give the same value where they meet.  Held here so
    that the claim is checked and not just made: the table has rows AT the decision point (asserted by the coverage
    tests: heading_proj == 0.8f, |sinp| == 1 and > 1, nrm == 1e-9f), and the mutant's output equals the unmutated one there
    and everywhere to within float64 rounding of a constant."""
    if mutant in R.REWARD_MUTANTS:
        assert _reward_mutant_differs(rtab, rref, mutant) == {0: 0, 1: 0}
        at = rtab["obs"][:, 11] == F(0.8)
        cfg = _cfg(rtab["n"], 1)
        m = R.reward_ref(cfg, rtab["obs"], rtab["targets"], rtab["root"], rtab["contact"], rtab["pot"], rtab["prev_pot"],
                         rtab["progress"], rtab["reset"], mutant=mutant)
        assert at.sum() > 0 and np.array_equal(m["reward"][at], rref[1]["reward"][at])
    else:
        cfg = O.default_config(otab["n"])
        m = R.obs_ref(cfg, otab["root"], otab["dof_pos"], otab["dof_vel"], otab["targets"], otab["contact"], otab["pot"], mutant=mutant)
        assert np.abs(m["obs"] - oref["ref"]["obs"]).max() <= 1e-7      # pi/2 as the fp32 constant vs asin(1.0): 4.4e-8
