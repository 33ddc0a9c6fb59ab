"""GPU (-m gpu): the HIP path, called through the C ABI (libflyhip.so via fly_bproject_amd),
against the CPU oracle and the golden vectors recorded from the reference's own functions.

Bars: bit-exact for integer/mask/copy outputs (reset, progress, touching flags, targets, TD
target, GAE); stated fp32 tolerance for trigonometric / reduced values."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.hip_helpers import cuda, make_args, make_env, pose_actions, pull_state, push_state

pytestmark = pytest.mark.gpu
OBS_TOL = dict(rtol=3e-6, atol=3e-6)
EXACT_COLS = [0] + list(range(48, 66)) + list(range(67, 73))


@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    return _lib


def test_library_is_the_hip_build_of_abi_13(lib):
    """ABI 13: mlp_adam_step's last int is the rescale period (applied steps, counted on the device) and the fp16x2 scale table holds
    the optimizer's rescale bookkeeping (MLP_H2_SCALE_FLOATS_ABI = 2386)."""
    l = lib.load()
    assert l.fly_abi_version() == lib.ABI_VERSION == 13
    assert torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


@pytest.mark.parametrize("n", [16, 257, 8192])
def test_scale_actions_bit_exact(n):
    env = make_env(n)
    cfg = O.default_config(n)
    rng = np.random.default_rng(n)
    a = rng.uniform(-1.2, 1.2, (n, 18)).astype(np.float32)
    env.set_actions(cuda(a))
    torch.cuda.synchronize()
    got = env.actions.cpu().numpy().reshape(n, 18)
    assert np.array_equal(got, O.scale_actions(cfg, a))
    env.exit()


@pytest.mark.parametrize("variant", ["bigGrav", "lowGrav"])
def test_reset_masked_bit_exact(variant):
    n = 100
    env = make_env(n, variant)
    cfg = O.default_config(n, variant)
    rng = np.random.default_rng(1)
    s = O.EnvState(n)
    s.root[:] = rng.normal(size=(n, 13)); s.dof_pos[:] = rng.normal(size=(n, 18)); s.dof_vel[:] = rng.normal(size=(n, 18))
    s.pot[:] = rng.normal(size=n); s.prev_pot[:] = rng.normal(size=n)
    s.reset[:] = rng.random(n) < 0.4; s.progress[:] = rng.integers(0, 1500, n)
    push_state(env, s)
    assert env.reset() is True
    got = pull_state(env)
    O.reset_masked(cfg, s)
    for k in ("root", "dof_pos", "dof_vel", "pot", "prev_pot", "reset", "progress"):
        assert np.array_equal(getattr(got, k), getattr(s, k)), k
    assert env.reset() is False          # nothing flagged any more (fly.py:449-450)
    env.exit()


@pytest.mark.parametrize("n", [16, 257])
def test_pack_obs_vs_reference_golden(golden, n):
    g = golden("g1_obs")
    p = "n%d_" % n
    env = make_env(n)
    s = O.EnvState(n)
    s.root[:] = g[p + "root"]; s.dof_pos[:] = g[p + "dof_pos"]; s.dof_vel[:] = g[p + "dof_vel"]
    s.targets[:] = g[p + "targets"]; s.contact[:] = g[p + "contact"]; s.pot[:] = g[p + "pot_in"]
    push_state(env, s)
    env.get_obs()
    got = pull_state(env)
    ref = g[p + "obs"]
    for col in EXACT_COLS:
        assert np.array_equal(got.obs[:, col], ref[:, col]), col
    np.testing.assert_allclose(got.obs, ref, **OBS_TOL)
    assert np.array_equal(got.prev_pot, g[p + "prev_pot"])
    np.testing.assert_allclose(got.pot, g[p + "pot"], rtol=1e-6)
    # and against the oracle on the same inputs
    cfg = O.default_config(n)
    O.pack_obs(cfg, s)
    np.testing.assert_allclose(got.obs, s.obs, **OBS_TOL)
    np.testing.assert_allclose(env.up_vec.cpu().numpy(), g[p + "up_vec"], atol=1e-6)
    np.testing.assert_allclose(env.heading_vec.cpu().numpy(), g[p + "heading_vec"], atol=1e-6)
    env.exit()


@pytest.mark.parametrize("n", [16, 257])
@pytest.mark.parametrize("variant,ecs", [("big", 0.005), ("low", 1.0)])
def test_pack_reward_vs_reference_golden(golden, n, variant, ecs):
    g = golden("g2_reward")
    p = "n%d_" % n
    from fly_bproject_amd.params import default_params
    from fly_bproject_amd.fly import Fly
    from tests.hip_helpers import make_args
    prm = default_params(n)
    prm.energy_cost_scale = ecs
    env = Fly(make_args(n), params=prm)
    s = O.EnvState(n)
    s.obs[:] = g[p + "obs"]; s.targets[:] = g[p + "targets"]; s.root[:] = g[p + "root"]
    s.contact[:] = g[p + "contact"]; s.pot[:] = g[p + "pot"]; s.prev_pot[:] = g[p + "prev_pot"]
    s.progress[:] = g[p + "progress"]; s.reset[:] = g[p + "reset_in"]
    push_state(env, s)
    env.get_reward()
    got = pull_state(env)
    assert np.array_equal(got.reset, g[p + variant + "_reset"])                 # done mask: bit-exact
    np.testing.assert_allclose(got.reward, g[p + variant + "_reward"], rtol=3e-6, atol=3e-6)
    env.exit()


@pytest.mark.parametrize("n", [16, 257])
def test_reward_terms_vs_oracle_on_golden_inputs(golden, n):
    """`Fly.reward_terms()` (the reference viewer's P-key dump, fly.py:504-546) entry by entry against the oracle's restatement
    on g2's inputs -- including the dump's 0.92 orientation threshold (fly.py:518; the reward itself uses 0.98, fly.py:728):
    envs whose qz^2 + qw^2 lies between the two get the dump's orient_reward and no reward bonus."""
    from fly_bproject_amd.fly import Fly
    from tests.hip_helpers import make_args
    g = golden("g2_reward")
    p = "n%d_" % n
    env = Fly(make_args(n))
    s = O.EnvState(n)
    s.obs[:] = g[p + "obs"]; s.targets[:] = g[p + "targets"]; s.root[:] = g[p + "root"]
    s.contact[:] = g[p + "contact"]; s.pot[:] = g[p + "pot"]; s.prev_pot[:] = g[p + "prev_pot"]
    s.progress[:] = g[p + "progress"]; s.reset[:] = g[p + "reset_in"]
    push_state(env, s)
    got = {k: v.float().cpu().numpy() for k, v in env.reward_terms().items()}
    want = O.reward_terms(O.default_config(n), s)
    assert set(got) == set(want) == set(O.REWARD_TERMS)
    for k in ("alive_reward", "up_reward", "orient_reward", "leg_reward", "dof_at_limit_cost", "progress_reward"):
        assert np.array_equal(got[k], want[k]), k                   # selections, counts and one subtraction: bit-exact
    for k in ("heading_reward", "actions_cost", "electricity_cost"):
        np.testing.assert_allclose(got[k], want[k], rtol=3e-6, atol=3e-6, err_msg=k)   # torch's reduction order over 18 terms
    ori = s.root[:, 5] ** 2 + s.root[:, 6] ** 2
    band = (ori > 0.92) & (ori <= 0.98)
    assert band.sum() >= 1 and np.all(got["orient_reward"][band] == 0.75)
    # and the reward of those envs carries no orientation bonus (0.98): the kernel's reward against the golden one
    env.get_reward()
    np.testing.assert_allclose(pull_state(env).reward, g[p + "big_reward"], rtol=3e-6, atol=3e-6)
    assert float(want["electricity_cost"].max()) > 0                 # g2 feeds obs[48:66] != targets (Q4 is not in force here)
    env.exit()


def test_walking_reward_mode_vs_oracle():
    """reward_mode 1 = the walking formula the reference keeps commented out (fly.py:747-748);
    no reference run can pin it, the oracle restates the commented expression."""
    from fly_bproject_amd.fly import Fly
    from tests.hip_helpers import make_args
    n = 512
    cfg = O.default_config(n)
    cfg.reward_mode = 1
    env = Fly(make_args(n, reward="walking"))
    assert env.params.reward_mode == 1
    for t, (s, a) in enumerate(_rollout_states(O.default_config(n), n, 30, 0.7, 21)[10:]):
        push_state(env, s)
        env.step(cuda(a))
        got = pull_state(env)
        O.env_step(cfg, s, a)
        z, ori = s.root[:, 2], s.root[:, 5] ** 2 + s.root[:, 6] ** 2
        ok = (np.abs(z - 1.1) > 1e-3) & (np.abs(z - 1.4) > 1e-3) & (np.abs(z - 2.1) > 1e-3) & \
            (np.abs(ori - 0.98) > 1e-3) & (np.abs(ori - 0.5) > 1e-3) & (s.reset == got.reset)
        # progress_reward = (pot - prev_pot) * 2 with pot ~ -6e4: absolute fp32 noise ~ 0.02
        np.testing.assert_allclose(got.reward[ok], s.reward[ok], rtol=1e-3, atol=0.05)
    env.exit()


def _rollout_states(cfg, n, steps, noise, seed):
    rng = np.random.default_rng(seed)
    s = O.EnvState(n)
    a0 = pose_actions(cfg, n)
    out = []
    for t in range(steps):
        a = np.clip(a0 + rng.normal(0, noise, (n, 18)), -1, 1).astype(np.float32)
        out.append((s.copy(), a))
        O.env_step(cfg, s, a)
    return out


@pytest.mark.parametrize("variant", ["bigGrav", "lowGrav"])
def test_integrate_one_step_vs_oracle(variant):
    """FlyDyn (build-defined; parity unpinned vs PhysX): one env step of substeps from identical
    states.  Tolerance vs the fp32 oracle and vs its fp64 evaluation: 2e-4 positions/quats/joints,
    5e-3 velocities (stiff contact amplifies rounding; sincos differs by ulps from libm)."""
    n = 256
    cfg = O.default_config(n, variant)
    env = make_env(n, variant)
    for s, a in _rollout_states(cfg, n, 40, 0.5, 7)[5::5]:
        s = s.copy()
        s.targets[:] = O.scale_actions(cfg, a)
        s.reset[:] = 0
        push_state(env, s)
        env.simulate()
        got = pull_state(env)
        r64, q64, qd64, c64 = O.physics_step_f64(cfg, s.root, s.dof_pos, s.dof_vel, s.targets)
        O.physics_step(cfg, s)
        for ref_root, ref_q, ref_qd in ((s.root, s.dof_pos, s.dof_vel), (r64, q64, qd64)):
            np.testing.assert_allclose(got.root[:, :7], ref_root[:, :7], rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(got.root[:, 7:], ref_root[:, 7:], rtol=5e-3, atol=5e-3)
            np.testing.assert_allclose(got.dof_pos, ref_q, rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(got.dof_vel, ref_qd, rtol=5e-3, atol=5e-3)
        np.testing.assert_allclose(got.contact, s.contact, rtol=2e-2, atol=2e-2)
    env.exit()


@pytest.mark.parametrize("n", [256, 8192])
@pytest.mark.parametrize("variant", ["bigGrav", "lowGrav"])
def test_fused_step_vs_oracle_resynced(variant, n):
    """fly_step (one launch) against orc_env_step, restarted from the oracle's state every step so
    that rounding cannot compound: checks the orchestration (reset before/after simulate, progress
    counting, obs/reward of the post-step state) on 48 different states including resets.  n = 8192 is the
    bench configuration (256 workgroups, one per CU)."""
    cfg = O.default_config(n, variant)
    env = make_env(n, variant)
    seen_reset = 0
    for t, (s, a) in enumerate(_rollout_states(cfg, n, 48, 0.7, 11)):
        if t == 20:
            s.progress[3] = 1497
        if t in (7, 30):
            s.reset[5:9] = 1                                # flagged from outside (the viewer's R key, fly.py:498-500)
        seen_reset += int(s.reset.sum())
        push_state(env, s)
        env.step(cuda(a))
        got = pull_state(env)
        # the same physics in float64 from the same pre-physics state (fly.py:626-663: scale, then reset before simulate -- bigGrav)
        pre = s.copy()
        pre.targets[:] = O.scale_actions(cfg, a)
        flagged = pre.reset != 0
        if not cfg.reset_after_sim:
            O.reset_masked(cfg, pre)
        r64, q64, qd64, _ = O.physics_step_f64(cfg, pre.root, pre.dof_pos, pre.dof_vel, pre.targets)
        O.env_step(cfg, s, a)
        live = ~flagged if cfg.reset_after_sim else np.ones(n, bool)       # (lowGrav: a flagged env ends the step in the reset pose)
        # DERIVED velocity tolerance (fly.py:624-681's step is 15 stiff substeps in fp32): an element may miss float64 by the stated
        # 5e-3 (abs + rel) -- or by K = 4 times what the fp32 ORACLE itself misses float64 by on that very element, whichever is larger.
        # So the kernel's tail is bounded by the restatement's own sensitivity at that state, not by a count of outliers.
        K = 4.0
        for hip, f32, f64 in ((got.root[:, 7:], s.root[:, 7:], r64[:, 7:]), (got.dof_vel, s.dof_vel, qd64)):
            bound = np.maximum(5e-3 * (1.0 + np.abs(f64)), K * np.abs(f32.astype(np.float64) - f64))
            over = (np.abs(hip.astype(np.float64) - f64) > bound) & live[:, None]
            assert not over.any(), (t, int(over.sum()), float(np.abs(hip - f64)[over].max()), float(np.abs(f32 - f64)[over].max()))
        assert np.array_equal(got.targets, s.targets)
        assert np.array_equal(got.progress, s.progress), t
        # masks are bit-exact wherever the deciding quantities are not within rounding of a threshold
        z, ori = s.root[:, 2], s.root[:, 5] ** 2 + s.root[:, 6] ** 2
        abd = s.contact[:, :5].sum(axis=(1, 2))
        safe = (np.abs(z - 1.1) > 1e-3) & (np.abs(z - 6) > 1e-3) & (np.abs(ori - 0.5) > 1e-3) & \
            ((abd == 0) | (np.abs(abd) > 1e-3))
        assert safe.mean() > 0.95
        assert np.array_equal(got.reset[safe], s.reset[safe]), t
        np.testing.assert_allclose(got.root[:, :7], s.root[:, :7], rtol=2e-4, atol=2e-4)
        lin = [0, 1, 2, 3, 4, 5, 6, 10, 11]
        # observation columns built from those velocities (rotated into the body frame): against the fp32 oracle, the same rule with
        # the oracle's own distance from float64 on the env's root velocities as the element's sensitivity
        sens = K * np.abs(s.root[:, 7:].astype(np.float64) - r64[:, 7:]).max(axis=1)
        dv = np.abs(got.obs[:, lin] - s.obs[:, lin]) - 5e-3 * (1.0 + np.abs(s.obs[:, lin])) - 2.5 * sens[:, None]      # (a rotation mixes three components)
        assert not (safe & live).any() or dv[safe & live].max() <= 0.0, (t, float(dv[safe & live].max()))
        for col in (7, 8, 9, 66):                           # angles live on a circle: 0 == 2*pi
            dang = np.abs((got.obs[safe][:, col] - s.obs[safe][:, col] + np.pi) % (2 * np.pi) - np.pi)
            assert dang.max() < 5e-3, (t, col, dang.max())
        np.testing.assert_allclose(got.obs[:, 12:30], s.obs[:, 12:30], rtol=2e-4, atol=2e-4)
        assert np.array_equal(got.obs[:, 48:66], s.obs[:, 48:66])
        stable = safe & (np.abs(z - 1.4) > 1e-3) & (np.abs(z - 2.1) > 1e-3) & (np.abs(ori - 0.98) > 1e-3) & \
            np.all(got.obs[:, 67:] == s.obs[:, 67:], axis=1)
        np.testing.assert_allclose(got.reward[stable], s.reward[stable], rtol=1e-5, atol=1e-5)
        seen_reset += int(s.reset.sum())
    assert seen_reset > 0
    env.exit()


def test_fused_step_vs_reference_golden(golden):
    """The reference's own Fly.step orchestration (g3, recorded with FlyDyn plugged in as
    simulate()): restart from the recorded state each step, compare EVERY recorded field of the next
    step: progress and reset masks bit for bit, root / joints / potentials / all 73 observation
    columns (angles on the circle) / reward within the stated fp32 tolerances."""
    g = golden("g3_step")
    checked_reward = checked_reset = 0
    for variant in ("bigGrav", "lowGrav"):
        acts = g[variant + "_actions"]
        steps, n, _ = acts.shape
        cfg = O.default_config(n, variant)
        env = make_env(n, variant)
        s = O.EnvState(n)
        R = lambda k: g[variant + "_" + k][t]   # noqa: E731
        for t in range(steps):
            push_state(env, s)
            env.step(cuda(acts[t]))
            got = pull_state(env)
            O.env_step(cfg, s, acts[t])                     # == golden (asserted in the CPU suite)
            ref_progress = R("progress").copy()
            if t == 20:
                ref_progress[3] = s.progress[3]             # the fixture holds the generator's override for env 3 here ...
                s.progress[3] = 1497                        # ... applied AFTER step 20 (so step 21 must count 1498, and reset at 1499)
            assert np.array_equal(got.progress, ref_progress), (variant, t)
            ref_root = R("root")
            np.testing.assert_allclose(got.root[:, :7], ref_root[:, :7], rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(got.root[:, 7:], ref_root[:, 7:], rtol=5e-3, atol=5e-3)
            np.testing.assert_allclose(got.dof_pos, R("dof_pos"), rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(got.dof_vel, R("dof_vel"), rtol=5e-3, atol=5e-3)
            # potentials = -|target - pos| / dt: position tolerance x 60, on a value of ~ -6e4
            np.testing.assert_allclose(got.pot, R("pot"), rtol=1e-6, atol=2e-2)
            np.testing.assert_allclose(got.prev_pot, R("prev_pot"), rtol=1e-6, atol=2e-2)
            ref_obs, ref_reset = R("obs"), R("reset")
            z, ori = ref_root[:, 2], ref_root[:, 5] ** 2 + ref_root[:, 6] ** 2
            abd = s.contact[:, :5].sum(axis=(1, 2))
            safe = (np.abs(z - 1.1) > 1e-3) & (np.abs(z - 6) > 1e-3) & (np.abs(ori - 0.5) > 1e-3) & \
                ((abd == 0) | (np.abs(abd) > 1e-3))
            assert np.array_equal(got.reset[safe], ref_reset[safe]), (variant, t)
            checked_reset += int(ref_reset[safe].sum())
            lin = [0, 1, 2, 3, 4, 5, 6, 10, 11]
            np.testing.assert_allclose(got.obs[:, lin], ref_obs[:, lin], rtol=5e-3, atol=5e-3)
            for col in (7, 8, 9, 66):                       # angles live on a circle: 0 == 2*pi
                dang = np.abs((got.obs[:, col] - ref_obs[:, col] + np.pi) % (2 * np.pi) - np.pi)
                assert dang.max() < 5e-3, (variant, t, col, dang.max())
            np.testing.assert_allclose(got.obs[:, 12:30], ref_obs[:, 12:30], rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(got.obs[:, 30:48], ref_obs[:, 30:48], rtol=5e-3, atol=5e-3)      # dof_vel * 0.2
            assert np.array_equal(got.obs[:, 48:66], ref_obs[:, 48:66])
            touch_same = np.all(got.obs[:, 67:] == ref_obs[:, 67:], axis=1)
            assert touch_same.mean() > 0.8, (variant, t)     # a foot within rounding of the ground may flip its flag
            stable = safe & touch_same & (np.abs(z - 1.4) > 1e-3) & (np.abs(z - 2.1) > 1e-3) & (np.abs(ori - 0.98) > 1e-3)
            np.testing.assert_allclose(got.reward[stable], R("reward")[stable], rtol=1e-5, atol=1e-5)
            checked_reward += int(stable.sum())
        env.exit()
    assert checked_reward > 1000 and checked_reset > 0


def test_fused_equals_unfused_bit_exact():
    """One fused launch == scale, reset, integrate, obs, progress+reward as separate launches."""
    n = 1000
    cfg = O.default_config(n)
    fused, split = make_env(n), make_env(n)
    for t, (s, a) in enumerate(_rollout_states(cfg, n, 12, 0.7, 5)):
        push_state(fused, s); push_state(split, s)
        fused.step(cuda(a))
        split.set_actions(cuda(a))
        split._lib.fly_reset_masked(split._handle, C.byref(split._bufs), None)
        split.simulate()
        split.get_obs()
        split._lib.fly_pack_reward(split._handle, C.byref(split._bufs), 1, None)
        f, u = pull_state(fused), pull_state(split)
        for k in ("root", "dof_pos", "dof_vel", "targets", "contact", "pot", "prev_pot", "obs", "reward", "reset", "progress"):
            assert np.array_equal(getattr(f, k), getattr(u, k)), (t, k)
    fused.exit(); split.exit()


def death_seed_state(cfg, n):
    """A first state from which every way of ending an episode occurs within a few steps: the start pose (one oracle step
    from the all-flagged initial state), then a few envs moved above termination_height_up, a few below termination_height,
    a few rolled by 120 degrees (qz^2 + qw^2 = 0.25 < 0.5), a few pitched nose-up by 60 degrees at z = 1.5 (qz^2 + qw^2 = 0.75:
    alive, with the abdomen's tail under the ground: abdomen contact in the first step, in either gravity), one at
    progress = max - 3.  Envs 0..7 are the fallers (the caller drives every joint of theirs to its upper limit)."""
    s = O.EnvState(n)
    s.root[:, 2], s.root[:, 6] = cfg.start_height, 1.0   # (lowGrav integrates before it resets: give it a pose to integrate)
    s.dof_pos[:] = np.array(cfg.dof_pose[:], np.float32)
    O.env_step(cfg, s, pose_actions(cfg, n))
    assert not s.reset.any() and np.isfinite(s.contact).all()
    s.root[10:14, 2] = 20.0
    s.root[14:18, 2] = np.array([0.9, 0.3, 1.0, 0.6], np.float32)
    s.root[14:18, 7:] = 0.0
    s.root[18:22, 3:7] = np.array([np.sin(np.pi / 3), 0.0, 0.0, np.cos(np.pi / 3)], np.float32)
    s.root[22:26, 2] = 1.5
    s.root[22:26, 3:7] = np.array([0.0, -0.5, 0.0, np.sqrt(0.75)], np.float32)
    s.root[22:26, 7:] = 0.0
    s.progress[30] = cfg.max_episode_length - 3
    return s


@pytest.mark.parametrize("variant", ["bigGrav", "lowGrav"])
def test_fused_equals_unfused_bit_exact_through_deaths(variant):
    """The fused launch against the split launches where envs DIE: the `dead` and time-limit branches of the fused
    instantiation, in both variants' order (reset before `simulate`, or after it with reset_after_sim).  The fused env runs
    freely for 60 steps from death_seed_state; before each step its state is pushed to the split env, after it all eleven
    buffers are compared bit for bit.  Each way of ending an episode must occur, classified from the post-step buffers
    with the numpy reference of tests/env_pack_ref.py (which the fused done mask must equal on every row, too): above
    termination_height_up, below termination_height, tilted, abdomen contact, the time limit, flagged from outside."""
    from tests import env_pack_ref as R
    n, steps = 257, 60
    cfg = O.default_config(n, variant)
    fused, split = make_env(n, variant), make_env(n, variant)
    push_state(fused, death_seed_state(cfg, n))
    rng = np.random.default_rng(17)
    a0 = pose_actions(cfg, n)
    seen = dict(d_hi=0, d_lo=0, d_ori=0, d_abd=0, abd_alone=0, timeout_alone=0, outside=0, resets=0)
    for t in range(steps):
        a = np.clip(a0 + rng.normal(0, 0.7, (n, 18)), -1, 1).astype(np.float32)
        a[:8] = 1.0                                        # every joint to its upper limit: these fall over
        if t in (7, 30):
            fused.reset_buf[40:44] = 1                      # flagged from outside (the viewer's R key, fly.py:498-500)
        pre = pull_state(fused)
        seen["outside"] += int(pre.reset[40:44].sum()) if t in (7, 30) else 0
        seen["resets"] += int(pre.reset.sum())
        push_state(split, pre)
        fused.step(cuda(a))
        split.set_actions(cuda(a))
        if not cfg.reset_after_sim:
            split._lib.fly_reset_masked(split._handle, C.byref(split._bufs), None)
        split.simulate()
        if cfg.reset_after_sim:
            split._lib.fly_reset_masked(split._handle, C.byref(split._bufs), None)
        split.get_obs()
        split._lib.fly_pack_reward(split._handle, C.byref(split._bufs), 1, None)
        f, u = pull_state(fused), pull_state(split)
        for k in ("root", "dof_pos", "dof_vel", "targets", "contact", "pot", "prev_pot", "obs", "reward", "reset", "progress"):
            assert np.array_equal(getattr(f, k), getattr(u, k)), (variant, t, k)
        ref = R.reward_ref(cfg, f.obs, f.targets, f.root, f.contact, f.pot, f.prev_pot, f.progress, np.zeros(n, np.int64))
        assert np.array_equal(f.reset, ref["reset"]), (variant, t)
        assert np.all(f.reward[ref["dead"]] == np.float32(cfg.death_cost))
        for k in ("d_hi", "d_lo", "d_ori", "d_abd"):
            seen[k] += int(ref[k].sum())
        seen["abd_alone"] += int((ref["d_abd"] & ~(ref["d_hi"] | ref["d_lo"] | ref["d_ori"])).sum())
        seen["timeout_alone"] += int((ref["timeout"] & ~ref["dead"]).sum())
    fused.exit(); split.exit()
    print(variant, seen)
    seen.pop("abd_alone")                                  # (reported only: whether a later faller meets no other end first is chaotic)
    assert all(v > 0 for v in seen.values()), (variant, seen)
    assert seen["resets"] > seen["outside"] + 20           # and the flagged envs did go through the reset, many times


@pytest.mark.parametrize("n", [8192, 8190, 4099, 16384])
def test_full_size_properties(n):
    """BASELINE size (8192 envs) and ragged tails: determinism, env-permutation equivariance
    (envs are independent: permuting the batch permutes every output bit-exactly), identical
    envs stay identical, nothing non-finite."""
    cfg = O.default_config(n)
    rng = np.random.default_rng(0)
    a0 = pose_actions(cfg, n)
    acts = [np.clip(a0 + rng.normal(0, 0.6, (n, 18)), -1, 1).astype(np.float32) for _ in range(25)]
    for a in acts:
        a[-3:] = a0[-3:]                                   # three identical envs at the ragged end
        a[:8] = 1.0                                        # every joint to its upper limit: these fall over
    perm = rng.permutation(n)

    def run(order):
        env = make_env(n)
        rets = torch.zeros(n, device="cuda:0")
        for a in acts:
            env.step(cuda(a[order]))
            rets += env.reward_buf
        st = pull_state(env)
        env.exit()
        return st, rets.cpu().numpy()
    acts = acts + acts                                     # 50 steps: long enough for the fallers to die
    s1, r1 = run(np.arange(n))
    s2, r2 = run(np.arange(n))
    s3, r3 = run(perm)
    for k in ("root", "dof_pos", "obs", "reward", "reset", "progress", "contact"):
        assert np.array_equal(getattr(s1, k), getattr(s2, k)), k            # deterministic
        assert np.array_equal(getattr(s1, k)[perm], getattr(s3, k)), k      # equivariant
    assert np.array_equal(r1[perm], r3)
    assert np.isfinite(s1.root).all() and np.isfinite(s1.obs).all()
    assert np.array_equal(s1.obs[-1], s1.obs[-2]) and np.array_equal(s1.obs[-1], s1.obs[-3])
    assert s1.progress.max() <= 50 and (s1.progress < 50).any(), "some envs must have died and reset"


@pytest.mark.parametrize("tag", ["v02", "v001", "vmix"])
def test_sample_logprob_vs_reference_golden(golden, lib, tag):
    g = golden("g5_sample")
    l = lib.load()
    mu, var, eps = cuda(g["mu"]), cuda(g[tag + "_var"]), cuda(g[tag + "_eps"])
    act = torch.empty_like(mu); logp = torch.empty(mu.shape[0], device="cuda:0")
    lib.check(l.ppo_sample_logprob(mu.data_ptr(), var.data_ptr(), eps.data_ptr(), act.data_ptr(),
                                   logp.data_ptr(), mu.shape[0], None), "sample")
    torch.cuda.synchronize()
    np.testing.assert_allclose(act.cpu().numpy(), g[tag + "_clipped"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(logp.cpu().numpy(), g[tag + "_logp"], rtol=2e-6, atol=2e-5)
    a2, lp2 = O.sample_logprob(g["mu"], g[tag + "_var"], g[tag + "_eps"])
    assert np.array_equal(act.cpu().numpy(), a2)
    np.testing.assert_allclose(logp.cpu().numpy(), lp2, rtol=2e-6, atol=1e-5)   # 18 device logf vs libm


def test_sample_logprob_full_size(lib):
    n = 8192 + 37
    rng = np.random.default_rng(2)
    mu = rng.normal(0, 0.7, (n, 18)).astype(np.float32); eps = rng.normal(0, 1, (n, 18)).astype(np.float32)
    var = np.full(18, 0.2, np.float32)
    act = torch.empty(n, 18, device="cuda:0"); logp = torch.empty(n, device="cuda:0")
    dmu, dvar, deps = cuda(mu), cuda(var), cuda(eps)
    lib.check(lib.load().ppo_sample_logprob(dmu.data_ptr(), dvar.data_ptr(), deps.data_ptr(),
                                            act.data_ptr(), logp.data_ptr(), n, None), "sample")
    torch.cuda.synchronize()
    a2, lp2 = O.sample_logprob(mu, var, eps)
    assert np.array_equal(act.cpu().numpy(), a2)
    np.testing.assert_allclose(logp.cpu().numpy(), lp2, rtol=2e-6, atol=1e-5)   # 18 device logf vs libm


@pytest.mark.parametrize("tag", ["a", "b"])
def test_td_gae_vs_reference_golden_bit_exact(golden, lib, tag):
    g = golden("g6_gae")
    r, v, vn = g[tag + "_reward"][..., 0], g[tag + "_v"][..., 0], g[tag + "_v_next"][..., 0]
    d = g[tag + "_done"][..., 0].astype(np.float32)
    T, N = r.shape
    tgt = torch.empty(T, N, device="cuda:0"); adv = torch.empty(T, N, device="cuda:0")
    dr, dv, dvn, dd = cuda(r), cuda(v), cuda(vn), cuda(d)      # keep the device copies alive
    lib.check(lib.load().ppo_td_gae(dr.data_ptr(), dv.data_ptr(), dvn.data_ptr(), dd.data_ptr(),
                                    0.99, 0.95, T, N, tgt.data_ptr(), adv.data_ptr(), 0, None), "gae")
    torch.cuda.synchronize()
    assert np.array_equal(tgt.cpu().numpy(), g[tag + "_target"][..., 0])
    assert np.array_equal(adv.cpu().numpy(), g[tag + "_adv"][..., 0])


@pytest.mark.parametrize("T,N,mode", [(80, 8192, 0), (160, 4096, 0), (32, 16384, 3), (7, 130, 1)])
def test_td_gae_full_size_vs_oracle(lib, T, N, mode):
    rng = np.random.default_rng(T)
    r = rng.normal(0, 1, (T, N)).astype(np.float32); v = rng.normal(0, 1, (T, N)).astype(np.float32)
    vn = rng.normal(0, 1, (T, N)).astype(np.float32)
    d = (rng.random((T, N) if mode & 1 else (N,)) < 0.9).astype(np.float32)
    tgt = torch.empty(T, N, device="cuda:0"); adv = torch.empty(T, N, device="cuda:0")
    dr, dv, dvn, dd = cuda(r), cuda(v), cuda(vn), cuda(d)
    lib.check(lib.load().ppo_td_gae(dr.data_ptr(), dv.data_ptr(), dvn.data_ptr(), dd.data_ptr(),
                                    0.99, 0.95, T, N, tgt.data_ptr(), adv.data_ptr(), mode, None), "gae")
    torch.cuda.synchronize()
    t2, a2 = O.td_gae(r, v, vn, d, mode_flags=mode)
    assert np.array_equal(tgt.cpu().numpy(), t2) and np.array_equal(adv.cpu().numpy(), a2)
    # property: the recurrence is linear in (reward, v, v_next)
    if mode == 0:
        dr2, dv2, dvn2 = cuda(2 * r), cuda(2 * v), cuda(2 * vn)
        lib.check(lib.load().ppo_td_gae(dr2.data_ptr(), dv2.data_ptr(), dvn2.data_ptr(),
                                        dd.data_ptr(), 0.99, 0.95, T, N, tgt.data_ptr(), adv.data_ptr(), 0, None), "gae")
        torch.cuda.synchronize()
        np.testing.assert_allclose(adv.cpu().numpy(), 2 * a2, rtol=1e-5, atol=1e-5)


def test_abi_rejects_bad_arguments(lib):
    l = lib.load()
    from fly_bproject_amd.params import default_params
    p = default_params(16); p.substeps = 0
    h = C.c_void_p()
    assert l.fly_create(C.byref(p), C.byref(h)) == -3 and b"substeps" in l.fly_last_error()
    assert l.ppo_td_gae(None, None, None, None, 0.99, 0.95, 1, 1, None, None, 0, None) == -1
    env = make_env(16)
    with pytest.raises(ValueError):
        env.step(torch.zeros(15, 18, device="cuda:0"))
    env.exit()
    from tests.hip_helpers import make_args
    from fly_bproject_amd.fly import Fly
    with pytest.raises(lib.FlyHipError):
        Fly(make_args(16, sim_device="cpu"))                # no CPU path in the product


def test_mean_episode_return_vs_oracle():
    """BASELINE's second metric: mean episode return of the HIP sim vs the oracle on identical initial
    states and action sequences, free-running (no re-sync).  Trajectories diverge chaotically at the
    1e-6 level, so the comparison is statistical: same mean return / length within 5 %."""
    n, steps = 1024, 300
    cfg = O.default_config(n)
    env = make_env(n)
    s = O.EnvState(n)
    rng = np.random.default_rng(4)
    a0 = pose_actions(cfg, n)
    drift = np.zeros((n, 18), np.float32)
    ep_ret = np.zeros(n); ep_len = np.zeros(n); done_ret = []; done_len = []
    for t in range(steps):
        drift = 0.9 * drift + 0.25 * rng.normal(0, 1, (n, 18)).astype(np.float32)
        a = np.clip(a0 + drift, -1, 1).astype(np.float32)
        env.step(cuda(a))
        O.env_step(cfg, s, a)
        ep_ret += s.reward; ep_len += 1
        fin = s.reset != 0
        done_ret += list(ep_ret[fin]); done_len += list(ep_len[fin])
        ep_ret[fin] = 0; ep_len[fin] = 0
    mr, ml, cnt = env.episode_stats()
    assert cnt > 200 and len(done_ret) > 200, "the action noise must finish enough episodes"
    assert abs(cnt - len(done_ret)) <= 0.05 * len(done_ret) + 5
    assert abs(mr - np.mean(done_ret)) <= 0.05 * abs(np.mean(done_ret)) + 0.05, (mr, np.mean(done_ret))
    assert abs(ml - np.mean(done_len)) <= 0.05 * np.mean(done_len) + 1, (ml, np.mean(done_len))
    terms = env.reward_terms()
    assert set(terms) >= {"up_reward", "orient_reward", "electricity_cost", "dof_at_limit_cost", "leg_reward"}
    assert float(terms["electricity_cost"].abs().max()) == 0.0           # Q4: identically zero upstream
    env.exit()


@pytest.mark.parametrize("T,N,mode", [(40960, 16, 0), (640, 100, 1), (80, 8, 0), (3, 5, 0)])
def test_td_gae_wave_scan_vs_sequential(lib, T, N, mode):
    """PPO_GAE_SCAN (time on lanes, shuffle scan of chunk carries) against the oracle's sequential
    loop: same TD targets bit for bit, advantages to fp32 rounding (carries are re-associated)."""
    rng = np.random.default_rng(T + N)
    r = rng.normal(0, 1, (T, N)).astype(np.float32); v = rng.normal(0, 1, (T, N)).astype(np.float32)
    vn = rng.normal(0, 1, (T, N)).astype(np.float32)
    d = (rng.random((T, N) if mode & 1 else (N,)) < 0.9).astype(np.float32)
    tgt = torch.empty(T, N, device="cuda:0"); adv = torch.empty(T, N, device="cuda:0")
    dr, dv, dvn, dd = cuda(r), cuda(v), cuda(vn), cuda(d)
    lib.check(lib.load().ppo_td_gae(dr.data_ptr(), dv.data_ptr(), dvn.data_ptr(), dd.data_ptr(),
                                    0.99, 0.95, T, N, tgt.data_ptr(), adv.data_ptr(), mode | 4, None), "gae scan")
    torch.cuda.synchronize()
    t2, a2 = O.td_gae(r, v, vn, d, mode_flags=mode)
    assert np.array_equal(tgt.cpu().numpy(), t2)
    np.testing.assert_allclose(adv.cpu().numpy(), a2, rtol=2e-5, atol=2e-5)
    assert lib.load().ppo_td_gae(dr.data_ptr(), dv.data_ptr(), dvn.data_ptr(), dd.data_ptr(), 0.99, 0.95, T, N,
                                 tgt.data_ptr(), adv.data_ptr(), 4 | 2, None) == -1      # masked recurrence: rejected


@pytest.mark.parametrize("n", [655360, 1000, 7])
def test_advantage_normalisation(lib, n):
    rng = np.random.default_rng(n)
    a = (rng.normal(0.3, 2.0, n)).astype(np.float32)
    da = cuda(a); stats = torch.zeros(514, device="cuda:0")
    l = lib.load()
    lib.check(l.ppo_adv_stats(da.data_ptr(), n, stats.data_ptr(), None), "stats")
    lib.check(l.ppo_adv_apply(da.data_ptr(), n, stats.data_ptr(), float(n), 1e-8, None), "apply")
    torch.cuda.synchronize()
    want = (a.astype(np.float64) - a.astype(np.float64).mean()) / (a.astype(np.float64).std(ddof=1) + 1e-8)
    np.testing.assert_allclose(da.cpu().numpy(), want, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(float(stats[0]), a.astype(np.float64).sum(), rtol=1e-4, atol=1e-2)


def test_integrator_against_closed_form_recurrences():
    """FlyDyn has no reference oracle (PhysX is a closed binary), and the C oracle is the build's own.  This test
    holds the HIP integrator to the SPECIFICATION equations (oracle/fly_physics.inc header) directly, on cases whose
    discrete recurrence can be written down in float64 without any shared code:
      * contact-free flight: v <- (v + h g) (1 - h lin_damp); z <- z + h v; x/y drift with damped velocity;
      * torque-free spin about a principal body axis: w_b <- w_b (1 - h ang_damp), and the quaternion advances by
        the first-order update q <- normalise(q + h/2 (w,0) (x) q) -- compared through the rotation ANGLE about that axis;
      * the PD position drive of a free joint (leg in the air): tau = clamp(kp (tgt - q) - kd qd, effort),
        qd <- clamp(qd + h tau / J, vmax), q <- q + h qd, clamped at the joint limits."""
    n = 64
    for variant in ("bigGrav", "lowGrav"):
        cfg = O.default_config(n, variant)
        env = make_env(n, variant)
        rng = np.random.default_rng(3)
        s = O.EnvState(n)
        pose = np.array(cfg.dof_pose[:], np.float64)
        lo, hi = np.array(cfg.dof_lo[:], np.float64), np.array(cfg.dof_hi[:], np.float64)
        s.root[:] = 0
        s.root[:, 2] = 5000.0                                  # far above the plane: no contact during the test
        s.root[:, 6] = 1.0
        s.root[:, 7:10] = rng.normal(0, 3, (n, 3))
        axis = rng.integers(0, 3, n)                            # spin about body x, y or z (identity orientation: body = world)
        w0 = rng.uniform(-5, 5, n)
        s.root[np.arange(n), 10 + axis] = w0
        s.dof_pos[:] = np.clip(pose + rng.normal(0, 0.3, (n, 18)), lo, hi)
        s.dof_vel[:] = rng.normal(0, 0.2, (n, 18))
        tgt = np.clip(pose + rng.normal(0, 0.5, (n, 18)), lo, hi).astype(np.float32)
        s.targets[:] = tgt
        s.reset[:] = 0
        push_state(env, s)
        steps = 3
        for _ in range(steps):
            env.simulate()
        got = pull_state(env)
        h = float(cfg.dt) / cfg.substeps
        ld, ad = 1.0 - h * float(cfg.lin_damp), 1.0 - h * float(cfg.ang_damp)
        g = float(cfg.gravity)
        pos = s.root[:, :3].astype(np.float64).copy(); vel = s.root[:, 7:10].astype(np.float64).copy()
        w = w0.astype(np.float64).copy(); ang = np.zeros(n)
        q = s.dof_pos.astype(np.float64).copy(); qd = s.dof_vel.astype(np.float64).copy()
        kp, kd, eff, vmax, J = float(cfg.kp), float(cfg.kd), float(cfg.effort), float(cfg.vmax), float(cfg.joint_inertia)
        for _ in range(steps * cfg.substeps):
            tau = np.clip(kp * (tgt.astype(np.float64) - q) - kd * qd, -eff, eff)
            qd = np.clip(qd + h * tau / J, -vmax, vmax)
            q = q + h * qd
            below, above = q < lo, q > hi
            qd = np.where(below, np.maximum(qd, 0), np.where(above, np.minimum(qd, 0), qd))
            q = np.clip(q, lo, hi)
            vel = vel + h * np.array([0.0, 0.0, g])
            vel = np.clip(vel * ld, -float(cfg.max_lin_vel), float(cfg.max_lin_vel))
            pos = pos + h * vel
            w = np.clip(w * ad, -float(cfg.max_ang_vel), float(cfg.max_ang_vel))
            # first-order quaternion update about a fixed axis: (cos a, sin a) <- normalise((cos a, sin a) + h/2 w (-sin a, cos a))
            half = ang / 2
            c, sn = np.cos(half) - 0.5 * h * w * np.sin(half), np.sin(half) + 0.5 * h * w * np.cos(half)
            ang = 2 * np.arctan2(sn, c)
        scale = np.maximum(1.0, np.abs(pos))
        assert np.max(np.abs(got.root[:, :3] - pos) / scale) < 2e-6, variant          # fp32 rounding of |z| = 5000
        np.testing.assert_allclose(got.root[:, 7:10], vel, rtol=2e-5, atol=2e-4)
        np.testing.assert_allclose(got.root[np.arange(n), 10 + axis], w, rtol=2e-5, atol=1e-5)
        off = np.array([[1, 2], [0, 2], [0, 1]])[axis]                                # the other two components stay 0
        assert np.abs(got.root[np.arange(n)[:, None], 10 + off]).max() < 1e-5
        got_ang = 2 * np.arctan2(got.root[np.arange(n), 3 + axis].astype(np.float64), got.root[:, 6].astype(np.float64))
        d = np.abs((got_ang - ang + np.pi) % (2 * np.pi) - np.pi)
        assert d.max() < 2e-5, (variant, d.max())
        np.testing.assert_allclose(got.dof_pos, q, rtol=2e-5, atol=2e-5)
        # the stiff drive (kp h / J ~ 80 per substep) amplifies fp32 rounding of q in the unsaturated band: the suite's
        # velocity tolerance
        np.testing.assert_allclose(got.dof_vel, qd, rtol=5e-3, atol=5e-3)
        assert np.all(got.contact == 0)
        env.exit()


@pytest.mark.parametrize("variant", ["bigGrav", "lowGrav"])
def test_contact_model_against_closed_form_recurrences(variant):
    """The CONTACT law of FlyDyn (oracle/fly_physics.inc header, step 2) held to its own equations with no code shared
    with the oracle.  `FlyConfig` is data, so the body is reduced to cases whose discrete recurrence can be written in
    float64 numpy: identity orientation, legs folded clear of the plane (zero-length segments attached ABOVE the body),
    joints resting at their targets, and
      (A) "drop": the five abdomen points on the body z-axis at different offsets a_k, purely vertical motion -- per
          point d_k = a_k - z, fn_k = max(kc d_k (1 - cdamp vz), 0) for d_k > 0, no tangential force, no torque (r x f = 0
          for collinear r and f): vz <- clamp((vz + h (sum fn_k / m + g)) (1 - h lin_damp)), z <- z + h vz.  Initial
          heights / speeds cover free approach, partial contact (some points in, some out), deep penetration, fast
          rebound (1 - cdamp vz < 0: the clamp at zero) and the static depth d = m |g| / (n kc) that the drop settles to;
      (B) "slide": all five points at the body origin (no lever arm, so friction exerts no torque), tangential velocity
          -- ft = min(cvisc |u_t|, mu fn) per point, direction -u_t / (|u_t| + 1e-9): both the viscous and the capped
          (sliding) regime, coupled to the vertical recurrence through fn."""
    from fly_bproject_amd.fly import Fly
    from fly_bproject_amd.params import default_params
    n, steps = 64, 3
    rng = np.random.default_rng(11)
    for case in ("drop", "slide"):
        prm = default_params(n, variant)
        prm.femur_len, prm.tibia_len = 0.0, 0.0
        for l in range(6):
            prm.leg_attach[l][:] = (0.0, 0.0, 1.0e4)             # leg tips far above the body: never in contact
        offs = np.array([0.25, 0.30, 0.35, 0.40, 0.45]) if case == "drop" else np.zeros(5)
        for k in range(5):
            prm.abdomen_pts[k][:] = (0.0, 0.0, -float(offs[k]))
        env = Fly(make_args(n, variant=variant), params=prm)
        m, g, kc, cd, mu, cv = (float(prm.mass), float(prm.gravity), float(prm.kc), float(prm.cdamp), float(prm.mu), float(prm.cvisc))
        h = float(prm.dt) / int(prm.substeps)
        ld, vlim = 1.0 - h * float(prm.lin_damp), float(prm.max_lin_vel)
        d_static = m * abs(g) / (5 * kc)
        s = O.EnvState(n)
        s.root[:] = 0
        s.root[:, 6] = 1.0
        top = offs.max()
        # heights: from well above first touch to deep inside; a few envs exactly at the static depth of five equal points
        s.root[:, 2] = top + rng.uniform(-6.0 * d_static - 0.05, 0.2, n)
        s.root[:, 9] = rng.uniform(-30.0, 30.0, n)               # |vz| > 1 / cdamp = 20 reaches the clamp at zero
        if case == "slide":
            s.root[:8, 2] = -d_static                            # resting depth: gravity and five springs balance
            s.root[:8, 9] = 0.0
            ut = np.concatenate([rng.uniform(0.0, 5.0, n // 2), rng.uniform(50.0, 800.0, n - n // 2)])   # viscous / capped
            ang = rng.uniform(0, 2 * np.pi, n)
            s.root[:, 7], s.root[:, 8] = ut * np.cos(ang), ut * np.sin(ang)
        pose = np.array(prm.dof_pose[:], np.float32)
        s.dof_pos[:] = pose
        s.dof_vel[:] = 0
        s.targets[:] = pose
        s.reset[:] = 0
        push_state(env, s)
        for _ in range(steps):
            env.simulate()
        got = pull_state(env)
        z = s.root[:, 2].astype(np.float64).copy()
        xy = np.zeros((n, 2))
        v = s.root[:, 7:10].astype(np.float64).copy()
        seen_partial = seen_clamp = seen_cap = seen_visc = 0
        fn_last = np.zeros((n, 5)); ft_last = np.zeros((n, 5, 2))
        for _ in range(steps * int(prm.substeps)):
            d = offs[None, :] - z[:, None]                       # penetration depth of each point
            inside = d > 0
            fn = np.where(inside, np.maximum(kc * d * (1.0 - cd * v[:, 2:3]), 0.0), 0.0)
            utn = np.hypot(v[:, 0], v[:, 1])
            ft = np.where(inside, np.minimum(cv * utn[:, None], mu * fn), 0.0)
            sc = ft / (utn[:, None] + 1e-9)
            fxy = -sc[:, :, None] * v[:, None, :2]
            seen_partial += int(np.any(inside.any(1) & ~inside.all(1)))
            seen_clamp += int(np.any(inside & (kc * d * (1.0 - cd * v[:, 2:3]) < 0)))
            seen_cap += int(np.any(inside & (cv * utn[:, None] > mu * fn) & (utn[:, None] > 0)))
            seen_visc += int(np.any(inside & (cv * utn[:, None] < mu * fn) & (utn[:, None] > 0)))
            fn_last, ft_last = fn, fxy
            F = np.concatenate([fxy.sum(1), fn.sum(1, keepdims=True)], axis=1)
            v = (v + h * (F / m + np.array([0.0, 0.0, g]))) * ld
            v = np.clip(v, -vlim, vlim)
            xy = xy + h * v[:, :2]
            z = z + h * v[:, 2]
        # the cases the docstring promises did occur
        assert seen_clamp > 0 and (seen_partial > 0 if case == "drop" else (seen_cap > 0 and seen_visc > 0)), (case, variant)
        np.testing.assert_allclose(got.root[:, 2], z, rtol=2e-4, atol=2e-4, err_msg="%s %s z" % (case, variant))
        np.testing.assert_allclose(got.root[:, :2], xy, rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(got.root[:, 7:10], v, rtol=5e-3, atol=5e-3)
        np.testing.assert_allclose(got.contact[:, :5, 2], fn_last, rtol=2e-3, atol=2e-3 * max(1.0, m * abs(g)))
        np.testing.assert_allclose(got.contact[:, :5, :2], ft_last, rtol=5e-3, atol=5e-3 * max(1.0, m * abs(g)))
        assert np.all(got.contact[:, 5:] == 0)                    # the folded legs never touch
        # no lever arm or collinear force: orientation and spin stay exactly at rest
        assert np.abs(got.root[:, 3:6]).max() < 1e-6 and np.abs(got.root[:, 10:13]).max() < 1e-5
        np.testing.assert_allclose(got.dof_pos, np.broadcast_to(pose, (n, 18)), atol=1e-6)
        if case == "slide":       # a body placed at the static depth with no vertical speed stays there (until friction is all that acts)
            np.testing.assert_allclose(got.root[:8, 2], -d_static, rtol=1e-3, atol=1e-5)
        env.exit()
