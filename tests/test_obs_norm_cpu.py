"""CPU: observation normalisation's host side -- trainer flags, the checkpoint key split, the table derived from the
statistics, and the float64 reference helpers the GPU tests hold the kernels to."""
import numpy as np
import pytest
import torch

from tests import obs_norm_ref as R


def test_trainer_flags():
    import trainer
    a = trainer.parse_args([])
    assert a.normalize_obs is False and a.obs_clip == 5.0
    a = trainer.parse_args(["--normalize_obs", "--obs_clip", "3.5"])
    assert a.normalize_obs is True and a.obs_clip == 3.5


def _reference_state_dict():
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(0)
    return Net(73, 18).state_dict()


def test_reference_checkpoint_loads_strict_with_and_without_flag():
    from fly_bproject_amd.ppo import Net, split_obs_rms
    for flag in (False, True):
        sd = dict(_reference_state_dict())
        assert split_obs_rms(sd, flag) == {}
        Net(73, 18).load_state_dict(sd)                      # strict


def test_checkpoint_with_statistics():
    from fly_bproject_amd.ppo import OBS_RMS_KEYS, Net, split_obs_rms
    rms = {"obs_rms.mean": torch.zeros(73, dtype=torch.float64), "obs_rms.var": torch.ones(73, dtype=torch.float64),
           "obs_rms.count": torch.tensor(5.0, dtype=torch.float64)}
    sd = dict(_reference_state_dict(), **rms)
    with pytest.raises(ValueError, match="--normalize_obs"):
        split_obs_rms(dict(sd), False)
    got = split_obs_rms(sd, True)
    assert sorted(got) == sorted(OBS_RMS_KEYS)
    Net(73, 18).load_state_dict(sd)                          # the rest loads strict
    bad = dict(_reference_state_dict(), **{"obs_rms.mean": rms["obs_rms.mean"]})
    with pytest.raises(ValueError, match="incomplete"):
        split_obs_rms(bad, True)


def test_reference_moments_match_numpy():
    x = R.hard_ring(6, 50, seed=3).reshape(-1, 73)
    c, mu, var = R.moments(x)
    x64 = x.astype(np.float64)
    assert c == x.shape[0]
    np.testing.assert_allclose(mu, np.mean(x64, axis=0), rtol=1e-13, atol=0)
    np.testing.assert_allclose(var, np.var(x64, axis=0), rtol=1e-10, atol=1e-14)
    assert var[1] == 0.0


def test_reference_merge_is_the_moments_of_everything():
    x = R.hard_ring(9, 40, seed=4)
    S = R.merge(R.initial(), x[1:5])
    assert S[0] == 4 * 40
    np.testing.assert_array_equal(S[1], R.moments(x[1:5])[1])          # first merge: exactly the batch's
    S = R.merge(S, x[5:])
    c, mu, var = R.moments(x[1:])
    assert S[0] == c
    np.testing.assert_allclose(S[1], mu, rtol=1e-12)
    np.testing.assert_allclose(S[2], var, rtol=1e-9, atol=1e-12)


def test_table_and_normalisation_helpers_agree_with_torch():
    from fly_bproject_amd.ppo import normalize_obs_ref, obs_norm_table
    x = R.hard_ring(3, 20, seed=5)
    c, mu, var = R.moments(x.reshape(-1, 73))
    stats = torch.cat([torch.tensor([c]), torch.from_numpy(mu), torch.from_numpy(var)]).double()
    tab = obs_norm_table(stats, 5.0)
    assert tab.dtype == torch.float32 and tab.shape == (147,)
    np.testing.assert_array_equal(tab.numpy(), R.table((c, mu, var), 5.0))
    xx = torch.from_numpy(x[0]).clone()
    xx[0] = float("nan")
    xx[1] = 1e9
    xx[2] = -1e9
    got = normalize_obs_ref(xx, tab)
    want = R.normalize(xx.numpy(), tab.numpy())
    np.testing.assert_array_equal(got.numpy(), want)       # NaN == NaN for assert_array_equal
    assert torch.isnan(got[0]).all()
    assert (got[1] == 5.0).all() and (got[2] == -5.0).all()
