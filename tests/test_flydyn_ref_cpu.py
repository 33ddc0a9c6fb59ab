"""CPU: the float64 numpy statement of one FlyDyn substep (tests/flydyn_ref.py) and the state families that drive it
(tests/flydyn_cases.py) -- (a) it agrees with the C oracle's float64 evaluation, (b) the families reach every branch they promise,
(c) the elements the GPU test leaves out are few, (d) the GPU test's bound rejects every mutant of the reference and accepts the
fp32 oracle."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flydyn_cases as Cs
from tests import flydyn_ref as R


def _scaled(got, ref):
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max())


@pytest.fixture(scope="module")
def evaluated():
    """(variant, family) -> everything the tests share about that family's one substep, computed once: the state, the reference's
    outputs and branches, the fp32 oracle's and the C float64 oracle's outputs."""
    out = {}
    for variant in Cs.VARIANTS:
        cfg = Cs.one_substep_config(O.default_config(Cs.N, variant))
        for fam in Cs.FAMILIES:
            st = Cs.make(fam, cfg)
            ref = R.substep(cfg, st.root, st.dof_pos, st.dof_vel, st.targets)
            s = O.EnvState(st.n)
            s.root[:], s.dof_pos[:], s.dof_vel[:], s.targets[:] = st.root, st.dof_pos, st.dof_vel, st.targets
            c64 = O.physics_step_f64(cfg, s.root, s.dof_pos, s.dof_vel, s.targets)
            O.physics_step(cfg, s)
            out[variant, fam] = dict(cfg=cfg, state=st, ref=R.fields(*ref[:4]), br=ref[4], c64=R.fields(*c64),
                                     f32=R.fields(s.root, s.dof_pos, s.dof_vel, s.contact))
    return out


def test_one_substep_config_keeps_the_products_step():
    for variant in Cs.VARIANTS:
        cfg = O.default_config(4, variant)
        one = Cs.one_substep_config(cfg)
        assert one.substeps == 1 and np.float32(one.dt) == np.float32(cfg.dt) / np.float32(cfg.substeps)
        assert one.kp == cfg.kp and one.gravity == cfg.gravity and list(one.dof_lo) == list(cfg.dof_lo)


@pytest.mark.parametrize("fam", Cs.FAMILIES)
@pytest.mark.parametrize("variant", Cs.VARIANTS)
def test_a_reference_equals_the_c_oracle_in_float64(evaluated, variant, fam):
    e = evaluated[variant, fam]
    for g in R.GROUPS:
        assert _scaled(e["ref"][g], e["c64"][g]) <= 1e-10, (g, _scaled(e["ref"][g], e["c64"][g]))
    assert e["state"].n == 257 and e["state"].root.dtype == np.float32


def _pose_actions(cfg, n):
    lo, hi, pose = np.array(cfg.dof_lo[:]), np.array(cfg.dof_hi[:]), np.array(cfg.dof_pose[:])
    return np.tile(((2 * pose - hi - lo) / (hi - lo)).astype(np.float32), (n, 1))


@pytest.mark.parametrize("variant", Cs.VARIANTS)
def test_a_fifteen_substeps_on_the_one_step_tests_states(variant):
    """The states of test_integrate_one_step_vs_oracle (tests/test_hip_parity.py: every fifth of a 40-step rollout around the
    standing pose, n = 256, noise 0.5, seed 7): the substep applied 15 times against orc_physics_step_f64 -- and, where the variant's
    own env step has another count (lowGrav: 2), that many times against the variant's own step as well."""
    n = 256
    cfg = O.default_config(n, variant)
    c15 = type(cfg).from_buffer_copy(cfg)
    c15.substeps, c15.dt = 15, float(cfg.dt) / cfg.substeps * 15                   # fifteen substeps of the variant's own length
    rng = np.random.default_rng(7)
    s = O.EnvState(n)
    a0 = _pose_actions(cfg, n)
    for t in range(40):
        a = np.clip(a0 + rng.normal(0, 0.5, (n, 18)), -1, 1).astype(np.float32)
        if t >= 5 and t % 5 == 0:
            tg = O.scale_actions(cfg, a)
            for c in (c15,) if cfg.substeps == 15 else (c15, cfg):
                want = R.fields(*O.physics_step_f64(c, s.root, s.dof_pos, s.dof_vel, tg))
                got = R.fields(*R.steps(c, s.root, s.dof_pos, s.dof_vel, tg, c.substeps)[:4])
                for g in R.GROUPS:
                    assert _scaled(got[g], want[g]) <= 1e-10, (t, c.substeps, g, _scaled(got[g], want[g]))
        O.env_step(cfg, s, a)


@pytest.mark.parametrize("fam", ["tumbling", "belly"])
@pytest.mark.parametrize("variant", Cs.VARIANTS)
def test_a_per_env_constants_equal_the_c_oracle_run_one_env_at_a_time(evaluated, variant, fam):
    """A sequence of n configs (per-env domain randomisation: tests/domain_rand_ref.env_config on wide multipliers) against
    orc_physics_step_f64 on each env's own config."""
    from tests import domain_rand_ref as DR
    wide = {"kp": (0.5, 2.0), "kd": (0.5, 2.0), "effort": (0.7, 1.3), "mass": (0.5, 2.0), "mu": (0.3, 3.0), "gravity": (0.8, 1.25)}
    e = evaluated[variant, fam]
    st = e["state"]
    cfgs = [DR.env_config(e["cfg"], m) for m in DR.multipliers(wide, 5, np.arange(st.n), 0)]
    got = R.fields(*R.substep(cfgs, st.root, st.dof_pos, st.dof_vel, st.targets)[:4])
    each = [O.physics_step_f64(cfgs[i], st.root[i:i + 1], st.dof_pos[i:i + 1], st.dof_vel[i:i + 1], st.targets[i:i + 1]) for i in range(st.n)]
    want = R.fields(*[np.concatenate([r[j] for r in each]) for j in range(4)])
    for g in R.GROUPS:
        assert _scaled(got[g], want[g]) <= 1e-10, (g, _scaled(got[g], want[g]))
    assert _scaled(got["v"], e["ref"]["v"]) > 1e-3                                # ... and they are not the shared constants


@pytest.mark.parametrize("fam", Cs.FAMILIES)
@pytest.mark.parametrize("variant", Cs.VARIANTS)
def test_b_every_promised_branch_occurs(evaluated, variant, fam):
    br = evaluated[variant, fam]["br"]
    for name in Cs.PROMISED[fam]:
        count = int(br[name].sum())
        if name == "effort_clamp" and variant == "lowGrav":
            assert count == 0, (name, count)                 # effort = 1e10
        else:
            assert count >= 8, (name, count)
    for name in Cs.ABSENT.get(fam, ()):
        assert int(br[name].sum()) == 0, name
    for name in br["margin"]:                                # a margin for every element of every edge
        assert np.isfinite(br["margin"][name]).all(), name
    for name, edge in (("effort_clamp", "effort_clamp"), ("vmax_clamp", "vmax_clamp"), ("lin_clamp", "lin_clamp"), ("ang_clamp", "ang_clamp"),
                       ("leg_in_ground", "leg_depth"), ("abd_in_ground", "abd_depth")):
        assert np.array_equal(br[name], br["margin"][edge] > 0), name


def test_b_the_families_together_reach_every_branch(evaluated):
    for variant in Cs.VARIANTS:
        names = [k for k in evaluated[variant, "belly"]["br"] if k not in ("margin", "x_pre")]
        assert len(names) == 16
        for name in names:
            best = max(int(evaluated[variant, fam]["br"][name].sum()) for fam in Cs.FAMILIES)
            assert best >= (0 if (name == "effort_clamp" and variant == "lowGrav") else 8), (variant, name, best)


@pytest.mark.parametrize("fam", Cs.FAMILIES)
@pytest.mark.parametrize("variant", Cs.VARIANTS)
def test_c_the_exclusion_is_at_most_one_percent(evaluated, variant, fam):
    e = evaluated[variant, fam]
    ex = R.excluded(e["cfg"], e["br"])
    assert ex.shape == (Cs.N, 18) and ex.sum() <= 0.01 * ex.size, int(ex.sum())


def _bounds(e):
    skip = {"qdot": R.excluded(e["cfg"], e["br"])}
    A = R.trig_allowance(e["cfg"], e["state"], e["ref"])
    bnd, M = R.bound(e["ref"], e["f32"], A, skip)
    return bnd, M, A, skip


@pytest.fixture(scope="module")
def bounds(evaluated):
    return {key: _bounds(e) for key, e in evaluated.items()}


@pytest.mark.parametrize("fam", Cs.FAMILIES)
@pytest.mark.parametrize("variant", Cs.VARIANTS)
def test_d_the_bound_accepts_the_fp32_oracle(evaluated, bounds, variant, fam):
    e = evaluated[variant, fam]
    bnd, M, A, skip = bounds[variant, fam]
    for g, (miss, ratio) in R.worst_ratio(e["f32"], e["ref"], bnd, skip).items():
        assert ratio <= 1.0, (g, miss, ratio)
        assert M[g] <= 1e-4, (g, M[g])                       # one substep in fp32 stays at rounding level on every family
    for g in ("q", "qdot"):
        assert not A[g].any()                                # no sine or cosine enters the joints
    no_tip = ~e["br"]["leg_in_ground"].any(axis=1)
    shifted_in = np.zeros(Cs.N, bool)                        # (a tip DELTA away from the ground may enter it under the shift)
    shifted_in |= (np.abs(e["br"]["margin"]["leg_depth"]) < 1e-5).any(axis=1)
    for g in R.GROUPS:
        assert not A[g][no_tip & ~shifted_in].any(), g       # A is zero wherever no leg tip is in the ground


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_d_the_bound_rejects_every_mutant(evaluated, bounds, mutant):
    """The fp32 oracle stands in for the kernel: held to a MUTANT of the reference under the bound the true reference sets, it
    misses by 10 x the bound or more on some element of some family, in both variants."""
    for variant in Cs.VARIANTS:
        best = 0.0
        for fam in Cs.FAMILIES:
            e = evaluated[variant, fam]
            bnd, _, _, skip = bounds[variant, fam]
            st = e["state"]
            mut = R.fields(*R.substep(e["cfg"], st.root, st.dof_pos, st.dof_vel, st.targets, mutant=mutant)[:4])
            best = max(best, max(r for _, r in R.worst_ratio(e["f32"], mut, bnd, skip).values()))
        assert best >= 10.0, (variant, mutant, best)
