"""CPU: shuffled PPO minibatches (PPO minibatch="shuffled") -- the permutation of tests/minibatch_ref.py (a bijection, keyed,
evaluable position by position, mixing), the rank-seed rule, and the public surface: the binding, the trainer flags and PPO's
validation of the argument."""
import os
import re
import types

import numpy as np
import pytest

from tests import minibatch_ref as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [(0, 0), (0, 1), (12345, 7), (0xFFFFFFFF, 0xFFFFFFFF)]


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 63, 64, 65, 4096, 4097, 5120, 655360])
def test_perm_index_is_a_bijection(R):
    for seed, key in KEYS:
        pi = M.perm_index(R, seed, key, np.arange(R))
        assert pi.min() == 0 and pi.max() == R - 1
        assert np.array_equal(np.sort(pi), np.arange(R)), (R, seed, key)


def test_epoch_keys_give_different_permutations():
    R = 655360
    a, b = M.perm_index(R, 0, 0, np.arange(R)), M.perm_index(R, 0, 1, np.arange(R))
    assert (a == b).mean() < 0.01
    c = M.perm_index(R, 1, 0, np.arange(R))                 # and so do seeds
    assert (a == c).mean() < 0.01


def test_a_subset_of_positions_is_the_slice_of_the_full_evaluation():
    rng = np.random.default_rng(0)
    for R in (5, 65, 4097, 81920):
        full = M.perm_index(R, 3, 9, np.arange(R))
        pos = rng.integers(0, R, size=min(R, 500))
        assert np.array_equal(M.perm_index(R, 3, 9, pos), full[pos])
        assert np.array_equal(M.perm_index(R, 3, 9, np.arange(R - 1, -1, -1)), full[::-1])
    assert M.perm_index(7, 0, 0, []).size == 0


@pytest.mark.parametrize("R,n", [(5120, 320), (81920, 5120)])
def test_windows_mix_the_time_chunks(R, n):
    """The chi-square statistic of a window's source chunks (16 chunks, 15 degrees of freedom; 14.06 expected without
    replacement) stays below 50 for every window of epoch keys 0..19 at seed 0: a cap against a broken round function."""
    worst, total = 0.0, []
    for key in range(20):
        chi = M.chunk_chi_square(R, n, 0, key)
        assert len(chi) == 16
        worst = max(worst, max(chi))
        total += chi
    print("R=%d n=%d: chi-square mean %.2f worst %.2f" % (R, n, np.mean(total), worst))
    assert worst < 50


def test_rank_seed_wraps_as_uint32():
    assert M.rank_seed(5, 0) == 5
    assert M.rank_seed(0, 1) == 0x9E3779B9
    assert M.rank_seed(0x70000000, 1) == (0x70000000 + 0x9E3779B9) - 2 ** 32
    assert M.rank_seed(0, 3) == (3 * 0x9E3779B9) % 2 ** 32
    assert all(0 <= M.rank_seed(s, r) < 2 ** 32 for s in (0, 2 ** 32 - 1) for r in range(16))
    assert M.epoch_key(2, 5, 3) == 13 and M.epoch_key(2 ** 32 // 5 + 1, 5, 0) == (2 ** 32 // 5 + 1) * 5 - 2 ** 32


def test_binding_and_abi_version():
    from fly_bproject_amd import _lib
    assert _lib.ABI_VERSION == 13
    assert "ppo_minibatch_gather" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["ppo_minibatch_gather"]) == 17          # (held to the header: tests/test_abi_cpu.py)
    assert re.search(r"^#define FLY_ABI_VERSION 13\b", open(os.path.join(REPO, "include", "flyhip.h")).read(), flags=re.M)
    assert "return FLY_ABI_VERSION;" in open(os.path.join(REPO, "fly_bproject_amd", "csrc", "flyhip_abi.hip")).read()


def test_trainer_flags():
    import trainer
    a = trainer.parse_args([])
    assert a.minibatch == "reference" and a.minibatch_seed is None
    a = trainer.parse_args(["--minibatch", "shuffled"])
    assert a.minibatch == "shuffled"
    assert trainer.parse_args(["--minibatch", "shuffled", "--minibatch_seed", "9"]).minibatch_seed == 9
    with pytest.raises(SystemExit):
        trainer.parse_args(["--minibatch", "random"])
    assert "--minibatch shuffled" in trainer.__doc__


def test_ppo_validates_minibatch_before_the_env_exists(monkeypatch):
    from fly_bproject_amd import ppo

    def no_env(args):
        raise AssertionError("the env was built before the argument was validated")

    monkeypatch.setattr(ppo, "Fly", no_env)
    with pytest.raises(ValueError, match="minibatch"):
        ppo.PPO(types.SimpleNamespace(num_envs=16, minibatch="random"))
    for ok in ("reference", "shuffled"):                    # a good value gets as far as the env
        with pytest.raises(AssertionError, match="before the argument"):
            ppo.PPO(types.SimpleNamespace(num_envs=16, minibatch=ok))
