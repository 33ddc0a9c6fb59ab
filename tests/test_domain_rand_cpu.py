"""CPU: per-env physics domain randomisation -- the numpy restatement of the draw, trainer.py's flags, the Python-side
validation (which runs before any GPU call) and the new ABI symbols."""
import os
import re

import numpy as np
import pytest

from tests import domain_rand_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_uniforms_in_unit_interval_and_deciles_flat():
    e = np.arange(1 << 17, dtype=np.uint32)
    u = np.concatenate([R.uniforms(12345, e, k) for k in range(8)]).reshape(-1)     # 6.3e6 draws
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    # exact in fp32: multiples of 2^-24
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, np.floor(u.astype(np.float64) * 2.0 ** 24))
    first = u[:1_000_000]
    frac = np.bincount(np.minimum((first * 10).astype(np.int64), 9), minlength=10) / first.size
    assert np.all(np.abs(frac - 0.1) <= 0.003), frac


def test_equal_bounds_give_exactly_lo():
    ranges = {n: (v, v) for n, v in zip(R.NAMES, (0.75, 1.0, 1.3, 3.0, 0.1, 2.5))}
    m = R.multipliers(ranges, 9, np.arange(1000), 17)
    assert np.array_equal(m, np.tile(np.array([0.75, 1.0, 1.3, 3.0, 0.1, 2.5], np.float32), (1000, 1)))
    ones = R.multipliers({}, 3, np.arange(100), 0)
    assert np.array_equal(ones, np.ones((100, 6), np.float32))


def test_multipliers_in_range():
    ranges = {"kp": (0.5, 2.0), "mu": (0.3, 3.0), "mass": (0.8, 1.2)}
    m = R.multipliers(ranges, 1, np.arange(50000), 0)
    lo, hi = R.bounds(ranges)
    assert (m >= lo).all() and (m <= hi).all()


def test_streams_differ_by_seed_env_count_and_parameter():
    e = np.arange(4096)
    base = R.uniforms(1, e, 0)
    assert (base != R.uniforms(2, e, 0)).mean() > 0.99
    assert (base != R.uniforms(1, e, 1)).mean() > 0.99
    assert (base[1:] != base[:-1]).mean() > 0.99
    assert (base[:, 1:] != base[:, :-1]).mean() > 0.99
    # a pure function: the same (seed, e, k) gives the same bits
    assert np.array_equal(base, R.uniforms(1, e, 0))
    # uint32 wrap-around of the count and the seed
    assert np.array_equal(R.uniforms(2 ** 32 + 5, e, 0), R.uniforms(5, e, 0))
    assert np.isfinite(R.uniforms(0xFFFFFFFF, e, 0xFFFFFFFF)).all()


def test_lowbias32_known_values():
    # fixed points of the restatement (uint32, wrapping): 0 -> 0, and a value worked by hand in Python ints
    def ref(x):
        m = 0xFFFFFFFF
        x ^= x >> 16; x = (x * 0x7FEB352D) & m
        x ^= x >> 15; x = (x * 0x846CA68B) & m
        x ^= x >> 16
        return x
    xs = np.array([0, 1, 2, 0x9E3779B9, 0xFFFFFFFF, 123456789], np.uint32)
    assert [int(v) for v in R.lowbias32(xs)] == [ref(int(v)) for v in xs]


def test_trainer_flags():
    import trainer
    a = trainer.parse_args([])
    assert a.randomize is False and a.dr_seed is None
    assert a.dr_kp == [0.8, 1.2] and a.dr_kd == [0.8, 1.2] and a.dr_effort == [1.0, 1.0]
    assert a.dr_mass == [0.8, 1.2] and a.dr_mu == [0.5, 1.5] and a.dr_gravity == [1.0, 1.0]
    a = trainer.parse_args(["--randomize", "--dr_mass", "0.5", "2", "--dr_mu", "0.3", "3", "--dr_seed", "7"])
    assert a.randomize and a.dr_mass == [0.5, 2.0] and a.dr_mu == [0.3, 3.0] and a.dr_seed == 7


def test_dr_args_seed_per_rank():
    import trainer
    from fly_bproject_amd.fly import DR_DEFAULT_RANGES, dr_args
    a = trainer.parse_args(["--randomize", "--seed", "11"])
    ranges, seed = dr_args(a)
    assert seed == 11 and ranges == DR_DEFAULT_RANGES
    a.rank = 3
    assert dr_args(a)[1] == (11 + 3 * 0x9E3779B9) % 2 ** 32
    a.dr_seed = 5
    a.rank = 0
    assert dr_args(a)[1] == 5


@pytest.mark.parametrize("ranges", [{"kp": (1.2, 0.8)}, {"mass": (0.0, 1.0)}, {"mu": (-1.0, 1.0)}, {"kd": (float("nan"), 1.0)},
                                    {"gravity": (1.0, float("inf"))}, {"effort": (1e-50, 1.0)}, {"stiffness": (1.0, 1.0)},
                                    {"kp": (1.0,)}])
def test_python_validation_rejects(ranges):
    from fly_bproject_amd.fly import dr_bounds
    with pytest.raises(ValueError):
        dr_bounds(ranges)


def test_python_validation_accepts_and_fills_ones():
    from fly_bproject_amd.fly import dr_bounds
    lo, hi = dr_bounds({"kp": (0.5, 2.0), "mu": (1.0, 1.0)})
    assert lo == [0.5, 1.0, 1.0, 1.0, 1.0, 1.0] and hi == [2.0, 1.0, 1.0, 1.0, 1.0, 1.0]


def test_symbols_in_header_and_binding():
    from fly_bproject_amd import _lib
    text = open(os.path.join(REPO, "include", "flyhip.h")).read()
    assert re.search(r"\bint\s+fly_set_randomization\s*\(", text)
    assert "typedef struct FlyRandomization" in text
    assert re.search(r"#define FLY_DR_PARAMS 6\b", text) and re.search(r"#define FLY_DR_ROW 8\b", text)
    assert "fly_set_randomization" in _lib.SYMBOLS
    assert _lib.DR_PARAMS == 6 and _lib.DR_ROW == 8
    import ctypes as C
    assert C.sizeof(_lib.FlyRandomization) == 56
