"""The seeded launches behind tests/test_fused_h2_heads_gpu.py and its golden file (not a test module).

    FLYHIP_LIB=<a build of the PARENT commit> python -m tests.fused_h2_heads_cases tests/golden/fused_h2_heads.json <parent hash>

writes a SHA-256 of everything one `mlp_fused_grad_h2` call (fused launch + slab reduction, fuse_norm form) leaves behind -- G, the
loss partials of the tiles, the class maxima and unscale factors behind the slabs, h2_scales, h2_overflow, the norm partials, the step
word -- for the shapes at which the heads of the two kernels can go wrong, under a frozen and a live scale table; the test runs the
same launches on the library under test and compares.  Inputs come from numpy generators and a CPU-initialised network
(tests/adam_round_trips_seq.py's batches): the same on every machine."""
import ctypes as C
import json
import os
import sys

import torch

from tests.adam_round_trips_seq import DEV, _batch, _sha, compiler_string

# (id, rows, x offset in floats, grid override): 1 row; one whole + one ragged tile; one workgroup of 256 with a second, ragged tile;
# whole tiles with x off 16-byte alignment (the plain-load fetch path); 7 workgroups (every warm-up share index 0)
CASES = (("rows1", 1, 0, 0), ("rows33", 33, 0, 0), ("rows8193", 8193, 0, 0), ("rows8224-x-unaligned", 32 * 257, 1, 0),
         ("rows8193-grid7", 8193, 0, 7))
TABLES = ("frozen", "live")
BUFFERS = ("G", "loss_part", "wsmax", "h2_scales", "h2_overflow", "partials", "step")
MAX_ROWS = 32 * 257


def make_policy(seed=77):
    """One f16x2 policy for all cases (CPU-initialised, seeded) and the float64 copy of its weights the batches are made from."""
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(seed)
    net = Net(73, 18)
    sd = {k: v.detach().double().numpy().copy() for k, v in net.state_dict().items()}
    pol = PackedPolicy(net.to(DEV), DEV)
    pol.init_training(MAX_ROWS)
    pol.gemm = "f16x2"
    assert pol.h2_live()
    return pol, sd


def _set_grid(pol, grid):
    lib = pol._lib
    lib.flyhip_debug_set_fused_grid.argtypes = [C.c_int]
    lib.flyhip_debug_set_fused_grid.restype = None
    lib.flyhip_debug_set_fused_grid(grid)


def _wsmax(pol, rows, grid_override):
    """The class maxima [grid][8] and the 8 unscale factors behind them, as the launcher lays the workspace out."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slab = (int(pol._lib.mlp_fused_h2_workspace_floats()) - 8) // cus - 8
    grid = min((rows + 31) // 32, cus, grid_override if grid_override > 0 else cus)
    return pol._fused_ws[cus * slab: cus * slab + grid * 8 + 8]


def run_case(pol, sd, case):
    """-> {table: {buffer: sha256}} for one case; every launch of a case starts from the same calibrated scale table."""
    from fly_bproject_amd import policy as Pm
    cid, rows, xoff, grid = case
    x, action, old_logp, adv, target, var = _batch(sd, rows, 1000 + rows)
    if xoff:
        buf = torch.zeros(rows * 73 + xoff, device=DEV)
        buf[xoff:].copy_(x.reshape(-1))
        x = buf[xoff:].view(rows, 73)
        assert x.is_contiguous() and x.data_ptr() % 16 != 0
    for t in (x, action, old_logp, adv, target):
        assert bool(torch.isfinite(t).all())
    out = {}
    _set_grid(pol, grid)
    try:
        pol.h2_freeze = False
        pol.calibrate_h2(x, action, old_logp, adv, target, var, 0.2)
        start = pol.h2_scales.clone()
        start[4:8] *= 0.25                  # the gradient classes two binades under their window (exact, nothing overflows, far above
        start[Pm.H2_INV + 4:Pm.H2_INV + 8] *= 4.0     # the floor): a live table has something to move, a frozen one must not
        for table in TABLES:
            pol.h2_scales.copy_(start)
            pol.h2_overflow.zero_()
            pol.step.zero_()
            pol.G.fill_(float("nan"))
            pol.loss_part.fill_(float("nan"))
            pol._fused_ws.fill_(float("nan"))
            pol._norm_ws.fill_(float("nan"))
            pol.h2_freeze = table == "frozen"
            pol.minibatch_grad(x, action, old_logp, adv, target, var, 0.2, fuse_norm=True)
            torch.cuda.synchronize()
            assert int(pol.h2_overflow) == 0 and float(pol.G[Pm.ERR_SLOT]) == 0.0 and int(pol.step) == 1, (cid, table)
            assert bool(torch.isfinite(pol.G).all()), (cid, table)
            if table == "frozen":
                assert torch.equal(pol.h2_scales[:32], start[:32]), (cid, "a frozen table moved")
            else:
                assert not torch.equal(pol.h2_scales[4:8], start[4:8]), (cid, "a live table did not move")
            out[table] = {"G": _sha(pol.G), "loss_part": _sha(pol.loss_part[: (rows + 31) // 32]), "wsmax": _sha(_wsmax(pol, rows, grid)),
                          "h2_scales": _sha(pol.h2_scales), "h2_overflow": _sha(pol.h2_overflow), "partials": _sha(pol._norm_ws[1:292]),
                          "step": _sha(pol.step)}
    finally:
        _set_grid(pol, 0)
        pol.h2_freeze = False
    return out


def run_all():
    pol, sd = make_policy()
    return {case[0]: run_case(pol, sd, case) for case in CASES}


def main(path, parent):
    from fly_bproject_amd import _lib
    first, second = run_all(), run_all()
    assert first == second, "two runs of the cases in one process disagree"
    doc = {"what": "SHA-256 of what one mlp_fused_grad_h2 call (fuse_norm form) leaves behind, per case of tests/fused_h2_heads_cases.py "
                   "and scale-table mode, from a build of the parent commit",
           "parent": parent, "compiler": compiler_string(), "library": os.path.basename(_lib.LIB_PATH), "cases": first}
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    for cid, r in first.items():
        print(cid, {t: d["G"][:12] for t, d in r.items()})


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
