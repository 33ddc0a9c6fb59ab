"""CPU: checkpoint wire format (reference ppo.py:147-149, :266-273).  The reference ships 95
state-dicts of the current architecture; where /root/reference is present (build container only)
a few of them are loaded with weights_only=True straight into this build's Net."""
import glob
import os

import numpy as np
import pytest
import torch

REF_SAVES = "/root/reference/saves"
KEYS = ["shared_net.0.weight", "shared_net.0.bias", "shared_net.2.weight", "shared_net.2.bias",
        "to_mean.0.weight", "to_mean.0.bias", "to_mean.2.weight", "to_mean.2.bias",
        "to_value.0.weight", "to_value.0.bias", "to_value.2.weight", "to_value.2.bias"]


def test_net_has_the_reference_state_dict_layout():
    from fly_bproject_amd.ppo import Net
    net = Net(73, 18)
    sd = net.state_dict()
    assert list(sd) == KEYS
    assert sum(v.numel() for v in sd.values()) == 69587
    assert sd["to_mean.2.weight"].shape == (18, 64) and sd["to_value.2.weight"].shape == (1, 64)


@pytest.mark.skipif(not os.path.isdir(REF_SAVES), reason="reference checkpoints exist only in the build container")
def test_reference_checkpoints_load():
    from fly_bproject_amd.ppo import Net
    from oracle import ppo_oracle as PO
    files = sorted(glob.glob(os.path.join(REF_SAVES, "save9_1_23", "*.pth")))[:3] + \
        sorted(glob.glob(os.path.join(REF_SAVES, "save8_bigGrav", "*.pth")))[:2]
    assert files
    x = torch.randn(32, 73, generator=torch.Generator().manual_seed(0))
    for f in files:
        sd = torch.load(f, map_location="cpu", weights_only=True)     # never unpickles code
        net = Net(73, 18)
        net.load_state_dict(sd)                                       # strict: same keys, same shapes
        ref = PO.OracleNet()
        ref.load_state_dict(sd)
        with torch.no_grad():
            np.testing.assert_allclose(net.pi(x).numpy(), ref.pi(x).numpy(), rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(net.v(x).numpy(), ref.v(x).numpy(), rtol=1e-6, atol=1e-6)


def test_trainer_flags_match_reference():
    """trainer.py:6-20: same flags, same derived save/load/record switches."""
    import trainer
    a = trainer.parse_args(["--num_envs", "300", "--save_path", "/tmp/x_", "--load_path", "/tmp/y.pth",
                            "--record_dir_name", "r", "--testing", "True", "--rl_device", "cuda:0"])
    assert a.num_envs == 300 and a.save and a.load and a.record and a.testing and a.sim_device == "cuda:0"
    d = trainer.parse_args([])
    assert d.num_envs == 1000 and d.save_freq == 100 and d.time_steps_per_recorded_frame == 2 and not d.save


def test_refresh_asks_for_a_new_fp16x2_calibration():
    """PackedPolicy.refresh() follows an out-of-band change of the weights (a loaded checkpoint, averaged ranks): the fp16x2 step's
    activation / gradient scales were measured on the old network, so the next update must calibrate them again."""
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(0)
    pol = PackedPolicy(Net(73, 18), "cpu")              # layout tables only (no kernel is launched on the CPU)
    pol.h2_calibrated = True
    with torch.no_grad():
        pol.P.mul_(0.5)
    pol.refresh()
    assert not pol.h2_calibrated
    assert torch.equal(pol.PF[pol._dst_f], pol.P[pol._src_f])
