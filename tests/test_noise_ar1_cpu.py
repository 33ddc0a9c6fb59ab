"""CPU: temporally correlated exploration noise (PPO action_noise="ar1") -- the reference filter of tests/noise_ar1_ref.py
(continuity through the carry, the moments of the process) and the public surface: the binding, the trainer flags and PPO's
validation of the two arguments."""
import os
import re
import types

import numpy as np
import pytest

from tests import noise_ar1_ref as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_and_abi_version():
    from fly_bproject_amd import _lib
    assert _lib.ABI_VERSION == 13
    assert "ppo_noise_ar1" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["ppo_noise_ar1"]) == 6                   # (held to the header: tests/test_abi_cpu.py)
    assert re.search(r"^#define FLY_ABI_VERSION 13\b", open(os.path.join(REPO, "include", "flyhip.h")).read(), flags=re.M)
    assert "return FLY_ABI_VERSION;" in open(os.path.join(REPO, "fly_bproject_amd", "csrc", "flyhip_abi.hip")).read()
    launch = open(os.path.join(REPO, "fly_bproject_amd", "csrc", "launch.h")).read()
    assert re.search(r"\bhipError_t\s+flyhip_launch_noise_ar1\s*\(", launch)


def test_trainer_flags():
    import trainer
    a = trainer.parse_args([])
    assert a.action_noise == "white" and a.noise_rho == 0.5
    a = trainer.parse_args(["--action_noise", "ar1", "--noise_rho", "0.9"])
    assert a.action_noise == "ar1" and a.noise_rho == 0.9
    with pytest.raises(SystemExit):
        trainer.parse_args(["--action_noise", "pink"])
    assert "--action_noise ar1" in trainer.__doc__ and "--noise_rho" in trainer.__doc__


def test_ppo_validates_the_noise_arguments_before_the_env_exists(monkeypatch):
    from fly_bproject_amd import ppo

    def no_env(args):
        raise AssertionError("the env was built before the argument was validated")

    monkeypatch.setattr(ppo, "Fly", no_env)
    with pytest.raises(ValueError, match="action_noise"):
        ppo.PPO(types.SimpleNamespace(num_envs=16, action_noise="pink"))
    for rho in (0, 1, -0.1, 0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="noise_rho"):
            ppo.PPO(types.SimpleNamespace(num_envs=16, action_noise="ar1", noise_rho=rho))
    for ok in (dict(), dict(action_noise="white"), dict(action_noise="ar1"), dict(action_noise="ar1", noise_rho=0.9)):
        with pytest.raises(AssertionError, match="before the argument"):    # a good value gets as far as the env
            ppo.PPO(types.SimpleNamespace(num_envs=16, **ok))


def test_scale_is_formed_in_double_from_the_float32_rho():
    assert A.scale(0.5) == np.float32(np.sqrt(0.75))
    r = float(np.float32(0.999))
    assert A.scale(0.999) == np.float32(np.sqrt(1.0 - r * r)) and 0.0 < A.scale(0.999) < 0.05
    x = np.array([[1.0, -2.0]], np.float32)
    y, c = A.ar1(x, np.array([4.0, 0.0], np.float32), 0.5)
    assert np.array_equal(y, np.array([[np.float32(2.0) + A.scale(0.5), np.float32(-2.0) * A.scale(0.5)]], np.float32))
    assert np.array_equal(c, y[0])


@pytest.mark.parametrize("rho", [0.5, 0.9, 0.999])
def test_a_pass_in_two_parts_is_the_pass_in_one(rho):
    """The carry makes consecutive rollouts one continuous process: T rows at once = the first 1000 rows, then the rest from
    the returned carry, bitwise."""
    rng = np.random.default_rng(7)
    T, C = 2500, 54
    x = rng.standard_normal((T, C), dtype=np.float32)
    c0 = rng.standard_normal(C, dtype=np.float32)
    y, c = A.ar1(x, c0, rho)
    y1, c1 = A.ar1(x[:1000], c0, rho)
    y2, c2 = A.ar1(x[1000:], c1, rho)
    assert np.array_equal(y.view(np.int32), np.concatenate((y1, y2)).view(np.int32))
    assert np.array_equal(c.view(np.int32), c2.view(np.int32)) and np.array_equal(c1, y[999]) and np.array_equal(c, y[-1])
    assert np.array_equal(x, np.random.default_rng(7).standard_normal((T, C), dtype=np.float32))      # inputs left alone


@pytest.mark.parametrize("rho", [0.5, 0.9])
def test_moments_of_the_process(rho):
    """Unit variance, zero mean, corr(y[t], y[t + k]) = rho^k, pooled over T = 4096 rows of C = 144 columns from a stationary
    carry, seeds 0..9.  The caps catch a wrong s or a lost carry; they measure nothing."""
    T, C = 4096, 144
    worst = np.zeros(4)
    for seed in range(10):
        rng = np.random.default_rng(seed)
        c0 = rng.standard_normal(C, dtype=np.float32)
        x = rng.standard_normal((T, C), dtype=np.float32)
        y, _ = A.ar1(x, c0, rho)
        mean, var, (r1, r5) = A.stats(y)
        worst = np.maximum(worst, [abs(var - 1), abs(r1 - rho), abs(r5 - rho ** 5), abs(mean)])
    print("rho=%g worst |var-1| %.4f |r1-rho| %.4f |r5-rho^5| %.4f |mean| %.4f" % (rho, *worst))
    assert worst[0] < 0.03 and worst[1] < 0.01 and worst[2] < 0.015 and worst[3] < 0.04
