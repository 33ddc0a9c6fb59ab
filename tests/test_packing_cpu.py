"""CPU: the packed-network format (fly_bproject_amd/packing.py) as the PPO policy and the DQN Q-net declare it.

Written against the public names of `policy` / `dqn` only, so the digests and gradient masks below also characterise the
commit before packing.py existed (they were taken there): same maps, element for element.  Beside the digests every index rule
is restated once as the layout headers' comments spell it, with the headers' offsets typed in, and checked at hand-picked
elements; tests/test_abi_cpu.py::test_python_layout_matches_the_headers holds the derived offsets to the compiled headers."""
import hashlib

import numpy as np
import pytest
import torch


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()[:16]


@pytest.fixture(scope="module")
def maps():
    """{"policy" | "dqn": (module, idx_f, idx_t, idx_fb, idx_tb)}: built once, never written."""
    from fly_bproject_amd import dqn, policy
    out = {}
    for name, m in (("policy", policy), ("dqn", dqn)):
        arrays = m.build_index_maps() + m.build_plane_maps()
        for a in arrays:
            assert a.dtype == np.int32 and a.shape == (m.PACKED,)
            a.setflags(write=False)
        out[name] = (m,) + tuple(arrays)
    return out


DIGESTS = {"policy": ("b1b09e17280a733e", "6e5fc16383aa7e56", "c2cb65d91a17b0cf", "8897fcec24ecb99b"),
           "dqn": ("773f32e2e9b400d3", "df3dcf18ff49a907", "aa6a4097a49535f3", "14579d687b66a4ab")}


@pytest.mark.parametrize("net", ["policy", "dqn"])
def test_map_digests(maps, net):
    assert tuple(_digest(a) for a in maps[net][1:]) == DIGESTS[net]


def test_sizes():
    from fly_bproject_amd import dqn as D, policy as P
    assert (P.PACKED, P.FRAG, P.FRAG_T, P.PB_HALVES, P.PTB_HALVES, P.PH_HALVES, P.PTH_HALVES) == \
        (74272, 73728, 53248, 221184, 159744, 147456, 106496)
    assert (D.PACKED, D.FRAG, D.FRAG_T, D.QB_HALVES, D.QTB_HALVES, D.QH_HALVES, D.QTH_HALVES) == \
        (94752, 94208, 73728, 282624, 221184, 188416, 147456)


# ---- the rules as csrc/mlp_layout.h and csrc/dqn_layout.h state them -------------------------------------------------------
def _frag(n, k, K):
    """(((n/32) * (K/8) + kq) * 64 + (h*32 + n%32)) * 4 + q,   h = k / (K/2), kk = k % (K/2), kq = kk / 4, q = kk % 4"""
    h, kk = k // (K // 2), k % (K // 2)
    kq, q = kk // 4, kk % 4
    return (((n // 32) * (K // 8) + kq) * 64 + (h * 32 + n % 32)) * 4 + q


def _mlp_l4(n, k):
    """((w*4 + kq) * 64 + (h*32 + n)) * 4 + q,   w = k/32, h = (k%32)/16, kq = (k%16)/4, q = k%4"""
    w, h, kq, q = k // 32, (k % 32) // 16, (k % 16) // 4, k % 4
    return ((w * 4 + kq) * 64 + (h * 32 + n)) * 4 + q


def _dqn_l3(n, k):
    """((w*8 + kq)*64 + (h*32 + n))*4 + q,   w = k/64, h = (k%64)/32, kq = (k%32)/4, q = k%4"""
    w, h, kq, q = k // 64, (k % 64) // 32, (k % 32) // 4, k % 4
    return ((w * 8 + kq) * 64 + (h * 32 + n)) * 4 + q


def _plane(n, k, K, p=0):
    """(((n/32) * (K/16) + k/16) * 3 + p) * 512 + (((k%16)/8) * 32 + n%32) * 8 + k%8"""
    return (((n // 32) * (K // 16) + k // 16) * 3 + p) * 512 + (((k % 16) // 8) * 32 + n % 32) * 8 + k % 8


def _policy_cases():
    """(master index, idx_f, idx_t, idx_fb, idx_tb) of hand-picked elements; the offsets are mlp_layout.h's comments."""
    rows = []
    for n, k in ((0, 0), (255, 79), (100, 41)):                                      # L1 [256][80] at 0: no transposed copy
        rows.append((0 + n * 80 + k, 0 + _frag(n, k, 80), -1, 0 + _plane(n, k, 80), -1))
    for n, k in ((0, 0), (127, 255), (37, 100), (37, 200)):                          # L2 [128][256] at 20736: two K = 128 operands
        half, kk = k // 128, k % 128
        rows.append((20736 + n * 256 + k, 20480 + half * 128 * 128 + _frag(n, kk, 128), 0 + _frag(k, n, 128),
                     61440 + half * 3 * 128 * 128 + _plane(n, kk, 128), 0 + _plane(k, n, 128)))
    for n, k in ((0, 0), (127, 127), (70, 45)):                                      # L3 [128][128] at 53632
        rows.append((53632 + n * 128 + k, 53248 + _frag(n, k, 128), 32768 + _frag(k, n, 128),
                     159744 + _plane(n, k, 128), 98304 + _plane(k, n, 128)))
    for n, k in ((0, 0), (31, 127), (5, 3), (5, 32 + 17), (5, 64 + 30), (5, 96 + 9)):  # L4 [32][128] at 70144: one per wave
        rows.append((70144 + n * 128 + k, 69632 + _mlp_l4(n, k), 49152 + _frag(k, n, 32),
                     208896 + _plane(n, k, 128), 147456 + _plane(k, n, 32)))
    return rows


def _dqn_cases():
    """The same for dqn_layout.h: W3^T comes before W2^T in the transposed buffers."""
    rows = []
    for n, k in ((0, 0), (255, 79), (100, 41)):                                      # L1 [256][80] at 0
        rows.append((0 + n * 80 + k, 0 + _frag(n, k, 80), -1, 0 + _plane(n, k, 80), -1))
    for n, k in ((0, 0), (255, 255), (37, 200)):                                     # L2 [256][256] at 20736
        rows.append((20736 + n * 256 + k, 20480 + _frag(n, k, 256), 8192 + _frag(k, n, 256),
                     61440 + _plane(n, k, 256), 24576 + _plane(k, n, 256)))
    for n, k in ((0, 0), (31, 255), (5, 40), (5, 64 + 3), (5, 128 + 63), (5, 192 + 33)):   # L3 [32][256] at 86528: one per wave
        rows.append((86528 + n * 256 + k, 86016 + _dqn_l3(n, k), 0 + _frag(k, n, 32),
                     258048 + _plane(n, k, 256), 0 + _plane(k, n, 32)))
    return rows


@pytest.mark.parametrize("net", ["policy", "dqn"])
def test_rules_restated_from_the_headers(maps, net):
    _, idx_f, idx_t, idx_fb, idx_tb = maps[net]
    for src, f, t, fb, tb in (_policy_cases() if net == "policy" else _dqn_cases()):
        assert (int(idx_f[src]), int(idx_t[src]), int(idx_fb[src]), int(idx_tb[src])) == (f, t, fb, tb), (net, src)


# ---- gradient masks ------------------------------------------------------------------------------------------------------------
def test_dqn_grad_mask():
    from fly_bproject_amd import dqn as D
    pk = D.QNetPacked(D.Net(), D.Net(), "cpu")
    mask = pk.grad_mask.numpy()
    assert mask.dtype == np.float32 and set(np.unique(mask)) == {0.0, 1.0}
    assert int(mask.sum()) == 89362 and _digest(mask.astype(np.int32)) == "42af2a982bfa4979"


def test_policy_grad_mask():
    """PackedPolicy loads the library even for a layout-only use on the CPU (as tests/test_dist_cpu.py needs it)."""
    from fly_bproject_amd import _lib, policy as P
    from fly_bproject_amd.ppo import Net
    _lib.build()
    pol = P.PackedPolicy(Net(P.IN, P.NACT), "cpu")
    mask = pol.grad_mask.numpy()
    assert mask.dtype == np.float32 and set(np.unique(mask)) == {0.0, 1.0}
    assert int(mask.sum()) == 69587 and _digest(mask.astype(np.int32)) == "c959555093cd777b"
    assert mask[P.ERR_SLOT] == 0.0                      # the "gradient invalid" mark lies on masked padding


# ---- plane refresh -----------------------------------------------------------------------------------------------------------
def _seeded(size):
    torch.manual_seed(0)
    return torch.randn(size) * torch.logspace(-6, 3, size)


def _check_planes(buf, master, idx):
    """The three planes at idx, idx + 512, idx + 1024 sum to master exactly wherever idx names a position; all else is zero."""
    src = np.nonzero(idx >= 0)[0]
    dst = torch.from_numpy(idx[src].astype(np.int64))
    terms = [buf[dst + 512 * t].view(torch.bfloat16).float() for t in range(3)]
    assert torch.equal(terms[0] + terms[1] + terms[2], master[torch.from_numpy(src)])
    named = torch.zeros(buf.numel(), dtype=torch.bool)
    for t in range(3):
        named[dst + 512 * t] = True
    assert not buf[~named].any()
    return int(named.sum())


@pytest.mark.parametrize("net", ["policy", "dqn"])
def test_write_planes_reconstructs_the_master_exactly(maps, net):
    from fly_bproject_amd import packing
    m, _, _, idx_fb, idx_tb = maps[net]
    master = _seeded(m.PACKED)
    sizes = (m.PB_HALVES, m.PTB_HALVES) if net == "policy" else (m.QB_HALVES, m.QTB_HALVES)
    for idx, size in zip((idx_fb, idx_tb), sizes):
        buf = torch.zeros(size + 1024, dtype=torch.int16)         # a margin behind the buffer: nothing is written past its end
        _, src, dst = packing.scatter_pairs(np.array(idx), "cpu")
        packing.write_planes(buf[:size], master, src, dst)
        assert _check_planes(buf, master, idx) == size


def test_qnet_refresh_rebuilds_every_derived_copy(maps):
    """The packer's own refresh(): fragment copies and planes of both networks follow the masters."""
    from fly_bproject_amd import dqn as D
    _, idx_f, idx_t, idx_fb, idx_tb = maps["dqn"]
    pk = D.QNetPacked(D.Net(), D.Net(), "cpu")
    with torch.no_grad():
        pk.P.copy_(_seeded(D.PACKED))
        pk.P_tgt.copy_(_seeded(D.PACKED).flip(0))
    pk.refresh()
    for buf, master, idx in ((pk.PF, pk.P, idx_f), (pk.PT, pk.P, idx_t), (pk.PF_tgt, pk.P_tgt, idx_f)):
        src = np.nonzero(idx >= 0)[0]
        assert torch.equal(buf[torch.from_numpy(idx[src].astype(np.int64))], master[torch.from_numpy(src)])
    for buf, master, idx in ((pk.QB, pk.P, idx_fb), (pk.QTB, pk.P, idx_tb), (pk.QB_tgt, pk.P_tgt, idx_fb)):
        assert _check_planes(buf, master.detach(), idx) == buf.numel()
