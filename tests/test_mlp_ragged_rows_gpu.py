"""GPU (-m gpu): the policy MLP and the rollout launches around it at ragged 32-row tiles, with every output between sentinel
guards that start where include/flyhip.h says the buffer ends, and every input inside an allocation whose other words are NaN.

A fresh torch allocation is rounded up and usually reads as zeros, which hides what a 32-row tile kernel gets wrong at its
last tile: a store to rows n .. ceil32(n) - 1 of a row-major output lands in slack, and a padded row that leaks into a loss
sum, a dW or a scale maximum adds nothing.  Here the first is a tripped guard and the second a NaN (or a moved bit) in a
result that is compared bit for bit with the same launch on plain, zero-surrounded allocations.  Nothing here launches on a
bad pointer or expects a fault; a load past a buffer whose value reaches no result is not looked for.

  entry point            shapes (n rows / envs)                              arithmetic            guarded, poisoned in
  mlp_forward            1, 31, 33, 65; 131105 (the persistent walk)         f32, bf16x3           part A; part B three_launch
  mlp_forward_sample     1, 31, 33, 65; 12, 33 (x T = 3, the reference)      f32, bf16x3           part A (part C: plain)
  mlp_backward_dx        1, 31, 33, 65                                       f32, bf16x3           part B three_launch
  mlp_grad_w             1, 31, 33, 65                                       f32, bf16x3           part B three_launch, fwd_bwd
  mlp_forward_backward   1, 31, 33, 65                                       f32, bf16x3           part B fwd_bwd
  mlp_fused_grad         1, 31, 33, 65                                       bf16x3                part B fused
  mlp_fused_grad_h2      1, 31, 33, 65                                       f16x2                 part B fused
  ppo_rollout_step       12, 33 (three calls); 33 with NORM + DR             f32, bf16x3           part C
  ppo_rollout_all        12, 33 (T = 3; rollout_all_kernel); 33 NORM + DR    f32, bf16x3           part C
                         32 (T = 2; rollout_all_fs_kernel, one tile)         bf16x3                part C
                         32 (CUs + 1) (T = 2; its MULTI instantiation)       bf16x3                part C

Part A holds rows < n to the same call on plain allocations bit for bit (tests/test_ppo_gpu.py and
tests/test_rollout_kernels_gpu.py hold that call to torch and float64), part B every path of PackedPolicy.minibatch_grad to
itself on plain allocations bit for bit and to float64 at the suite's own bars (2e-5 of each tensor's / block's largest entry;
tests/test_mlp_ragged_rows_cpu.py shows plain float32 torch inside a quarter of them at these n, and so does each case here
on its own rows), part C both rollout launches to the header's contract: T calls of mlp_forward_sample + fly_step on a second
env, every row and the env state bit for bit.  Each part moves one NaN into a valid row once and asserts that the compared
outputs do change; the guards are shown to bite by a word written from the host after a launch has finished."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from fly_bproject_amd import _lib
from fly_bproject_amd.policy import untile
from tests import ragged_rows_cases as RC
from tests.hip_helpers import make_env
from tests.test_fused_h2_gpu import _errs, _fp64_chain
from tests.test_fused_step_gpu import WIDTH, _chain, _poison
from tests.test_mlp_train_gpu import _setup
from tests.test_rollout_kernels_gpu import SENTINEL, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GEMMS = ["f32", "bf16x3"]
SAVES = ("out", "h1", "h2", "h3")
DZ = ("dz4", "dz3", "dz2", "dz1")
VAR_DECAY, VAR_MIN = 1e-3, 0.01


def _stream():
    return _lib.stream_ptr()


def _policy(gemm, seed):
    """(ref, pol): a Net with torch's default initialisation as packed parameters under `gemm`, and an untouched copy."""
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(seed)
    net = Net(73, 18).to(DEV)
    ref = Net(73, 18).to(DEV)
    ref.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    pol = PackedPolicy(net, DEV)
    pol.gemm = gemm
    return ref, pol


def _host_x(n, seed, scale=1.5):
    return (torch.randn(n, 73, generator=torch.Generator().manual_seed(seed)) * scale).numpy()


def _variance():
    """Spread over the schedule's range, the smallest entry within three decays of the floor: the variance moves AND clamps."""
    return torch.linspace(VAR_MIN + 2 * VAR_DECAY, 0.2, 18).to(DEV)


def _guards(n, names):
    sz = RC.buffer_sizes(n)
    return {k: Guarded(sz[k]) for k in names}


def _plain(n, names):
    sz = RC.buffer_sizes(n)
    return {k: torch.full((sz[k],), SENTINEL, device=DEV) for k in names}


def _t(buf):
    return buf.t if isinstance(buf, Guarded) else buf


def _forward(pol, x, n, out):
    """mlp_forward with mu_out, v_out and all four saves; `out`: name -> Guarded or tensor."""
    _lib.api().mlp_forward(pol.P, pol.PF, x, n, _t(out["mu"]), _t(out["v"]), _t(out["out"]), _t(out["h1"]), _t(out["h2"]),
                          _t(out["h3"]), pol.infer_pb_ptr(), _stream())


def _forward_sample(pol, x, n, eps, var, steps, out):
    _lib.api().mlp_forward_sample(pol.P, pol.PF, x, n, eps, var, steps, VAR_DECAY, VAR_MIN, _t(out["act"]), _t(out["logp"]),
                                 _t(out["mu"]), _t(out["v"]), pol.infer_pb_ptr(), None, _stream())


def _valid(buf, n, name):
    """Rows < n of an output as a device tensor [n][width]; a Guarded has its guards checked first."""
    if isinstance(buf, Guarded):
        buf.get()
    t = _t(buf)
    return untile(t, n, WIDTH[name]) if name in WIDTH else t.view(n, -1)


def _check_outputs(got, want, n, what):
    """Every guarded output: guards intact, rows < n all written, finite, and bit for bit the plain run's."""
    torch.cuda.synchronize()
    for k in got:
        a, b = _valid(got[k], n, k), _valid(want[k], n, k)
        RC.assert_all_written(a, SENTINEL, "%s %s" % (what, k))
        assert torch.isfinite(a).all(), (what, k)
        assert RC.same_bits(a, b), (what, k, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ A. inference entry points
@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("n", RC.RAGGED_N)
def test_forward_between_guards_on_poisoned_rows(n, gemm):
    ref, pol = _policy(gemm, 100 + n)
    xh = _host_x(n, n)
    names = ("mu", "v") + SAVES
    got, want = _guards(n, names), _plain(n, names)
    _forward(pol, RC.poisoned(xh, DEV), n, got)
    _forward(pol, RC.embedded(xh, 0.0, DEV), n, want)
    _check_outputs(got, want, n, "mlp_forward n=%d %s" % (n, gemm))


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("n", RC.RAGGED_N)
def test_forward_sample_between_guards_on_poisoned_rows(n, gemm):
    ref, pol = _policy(gemm, 200 + n)
    xh = _host_x(n, 2 * n)
    eh = torch.randn(n, 18, generator=torch.Generator().manual_seed(3 * n)).numpy()
    var = _variance()
    names = ("act", "logp", "mu", "v")
    got, want, undecayed = _guards(n, names), _plain(n, names), _plain(n, names)
    _forward_sample(pol, RC.poisoned(xh, DEV), n, RC.poisoned(eh, DEV), var, 3, got)
    _forward_sample(pol, RC.embedded(xh, 0.0, DEV), n, RC.embedded(eh, 0.0, DEV), var, 3, want)
    _forward_sample(pol, RC.embedded(xh, 0.0, DEV), n, RC.embedded(eh, 0.0, DEV), var, 0, undecayed)
    _check_outputs(got, want, n, "mlp_forward_sample n=%d %s" % (n, gemm))
    assert not RC.same_bits(_t(want["logp"]), _t(undecayed["logp"]))          # three decays did move the variance
    assert RC.same_bits(_t(want["mu"]), _t(undecayed["mu"]))


def test_a_nan_in_the_last_valid_row_changes_that_row_and_no_other():
    """The poison control of part A: the comparison reads what the kernel wrote from the rows it was given."""
    n = 33
    for gemm in GEMMS:
        ref, pol = _policy(gemm, 7)
        xh = _host_x(n, 7)
        names = ("mu", "v") + SAVES
        clean, dirty = _plain(n, names), _plain(n, names)
        x = RC.poisoned(xh, DEV)
        _forward(pol, x, n, clean)
        x[n - 1, 5] = NAN
        _forward(pol, x, n, dirty)
        torch.cuda.synchronize()
        for k in names:
            a, b = _valid(clean[k], n, k), _valid(dirty[k], n, k)
            assert RC.same_bits(a[:n - 1], b[:n - 1]), (gemm, k)
            assert not RC.same_bits(a[n - 1], b[n - 1]) and torch.isnan(b[n - 1]).any(), (gemm, k)


def test_a_host_written_word_in_a_guard_is_reported_after_a_launch():
    """The guard control: after a launch has finished and passed, one word written from the host into either guard of an
    output fails its read; so does a sentinel written into a valid row."""
    n = 33
    ref, pol = _policy("bf16x3", 9)
    names = ("mu", "v") + SAVES
    got = _guards(n, names)
    _forward(pol, RC.poisoned(_host_x(n, 9), DEV), n, got)
    torch.cuda.synchronize()
    for k in names:
        g = got[k]
        g.get()
        for word in (g.lo - 1, g.lo + g.n):                                   # the words next to the array, on both sides
            g.full[word] = 0.0
            with pytest.raises(AssertionError, match="wrote"):
                g.get()
            g.full[word] = SENTINEL
        g.get()
    got["v"].t[n - 1] = SENTINEL
    with pytest.raises(AssertionError, match="never written"):
        RC.assert_all_written(_valid(got["v"], n, "v"), SENTINEL, "v")


# the switch in flyhip_launch_mlp_forward (csrc/mlp_mfma.hip): `tiles <= 4 * PERSIST_GRID ? tiles : PERSIST_GRID` workgroups,
# PERSIST_GRID = 256 * WGS_PER_CU = 1024 (csrc/mlp_forward.inc) -- above 4096 tiles the fp32-MFMA kernel walks tiles
# g, g + 1024, ... with the next tile's rows prefetched.  The bf16x3 kernel launches one workgroup per tile at any size.
PERSIST_TILES = 4 * 1024
PERSIST_N = PERSIST_TILES * 32 + 33             # the smallest row count past the switch with a ragged last tile


@pytest.mark.parametrize("gemm", GEMMS)
def test_persistent_walk_equals_two_plain_launches_and_float64(gemm):
    n, half = PERSIST_N, 65536
    assert RC.tiles(n) > PERSIST_TILES >= RC.tiles(n - half) and half % 32 == 0 and n % 32 == 1
    ref, pol = _policy(gemm, 11)
    xh = _host_x(n, 11)
    names = ("mu", "v") + SAVES
    got = _guards(n, names)
    x = RC.poisoned(xh, DEV)
    _forward(pol, x, n, got)
    torch.cuda.synchronize()
    xp = torch.from_numpy(xh).to(DEV)
    parts = []
    for lo, hi in ((0, half), (half, n)):                                     # (i) neither part takes the persistent form
        part = _plain(hi - lo, names)
        _forward(pol, xp[lo:hi].contiguous(), hi - lo, part)
        parts.append(part)
    torch.cuda.synchronize()
    rows = {}
    for k in names:
        a = _valid(got[k], n, k)
        b = torch.cat([_valid(parts[0][k], half, k), _valid(parts[1][k], n - half, k)])
        RC.assert_all_written(a, SENTINEL, k)
        assert RC.same_bits(a, b), (k, int((RC.bits(a) != RC.bits(b)).any(1).nonzero()[0]))
        rows[k] = a
    with torch.no_grad():                                                     # (ii) float64 torch at the forward's bar
        r64 = ref.double()
        x64 = xp.double()
        h1 = r64.shared_net[1](r64.shared_net[0](x64))
        h2 = r64.shared_net(x64)
        h3 = torch.cat([r64.to_mean[1](r64.to_mean[0](h2)), r64.to_value[1](r64.to_value[0](h2))], dim=1)
        want = {"mu": r64.to_mean(h2), "v": r64.to_value(h2), "h1": h1, "h2": h2, "h3": h3}
    for k, w in want.items():
        torch.testing.assert_close(rows[k], w.float(), rtol=2e-5, atol=2e-5, msg=lambda m, k=k: "%s: %s" % (k, m))
    torch.testing.assert_close(rows["out"][:, :18], want["mu"].float(), rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(rows["out"][:, 18:19], want["v"].float(), rtol=2e-5, atol=2e-5)


# -------------------------------------------------------------------------------------- B. the minibatch gradient, every path
# (path, arithmetic) -> what PackedPolicy.update_path() must name
PATHS = [("three_launch", "f32", "mlp_forward + mlp_backward_dx + mlp_grad_w"),
         ("three_launch", "bf16x3", "mlp_forward + mlp_backward_dx + mlp_grad_w"),
         ("fwd_bwd", "f32", "mlp_forward_backward"), ("fwd_bwd", "bf16x3", "mlp_forward_backward"),
         ("fused", "bf16x3", "mlp_fused_grad ("), ("fused", "f16x2", "mlp_fused_grad_h2")]


class GradCase:
    """One path of PackedPolicy.minibatch_grad on n rows: the policy set up as tests/test_mlp_train_gpu.py does (the fp16x2
    scales calibrated on the plain batch), its scratch either its own plain tensors or guarded ones of the header's sizes."""

    def __init__(self, n, path, gemm, names, seed=13):
        self.n, self.path, self.gemm = n, path, gemm
        self.net, self.ref, self.pol, self.batch = _setup(n, seed, gemm=gemm)
        pol = self.pol
        pol.fused_step = path == "fused"
        pol.fuse_fwd_bwd = path == "fwd_bwd"
        assert names in pol.update_path() and pol.step_gemm == gemm, pol.update_path()
        if pol._fused_ws is None:
            pol._fused_ws = torch.empty(int(max(pol._lib.mlp_fused_workspace_floats(), pol._lib.mlp_fused_h2_workspace_floats())),
                                        device=DEV)
        self.scales = pol.h2_scales.clone()                     # every run starts from the calibrated table
        self.plain = (pol.saves, pol.dz, pol.loss_part, pol.G, pol._tile_flags)
        self.guards = None

    def use_guards(self):
        n, pol = self.n, self.pol
        g = _guards(n, SAVES + DZ + ("loss_part", "G"))
        g["flags"] = Guarded(RC.tiles(n), dtype=torch.int32, init=np.zeros(RC.tiles(n), np.int32))
        pol.saves, pol.dz = {k: g[k].t for k in SAVES}, {k: g[k].t for k in DZ}
        pol.loss_part, pol.G, pol._tile_flags = g["loss_part"].t.view(-1, 2), g["G"].t, g["flags"].t
        self.guards = g

    def use_plain(self):
        pol = self.pol
        pol.saves, pol.dz, pol.loss_part, pol.G, pol._tile_flags = self.plain
        self.guards = None

    def prefill(self):
        pol = self.pol
        _poison(pol)                                            # saves, dz, loss_part, G
        pol._fused_ws.fill_(NAN)
        pol.workspace.fill_(NAN)
        pol.h2_scales.copy_(self.scales)
        pol.h2_overflow.zero_()

    def result(self):
        torch.cuda.synchronize()
        pol, n = self.pol, self.n
        if self.guards is not None:
            for g in self.guards.values():
                g.get()
        assert int(pol.tile_wait_error) == 0 and int(pol.h2_overflow) == 0
        return {"chain": _chain(pol, n), "loss": pol.loss_part[:RC.tiles(n)].clone(), "G": pol.G.clone(),
                "scales": pol.h2_scales[:40].clone()}

    def run(self, batch):
        self.prefill()
        self.pol.minibatch_grad(*batch, 0.2, **({"dump": True} if self.path == "fused" else {}))
        return self.result()

    def run_three_launches(self, batch, between):
        """The three launches of minibatch_grad's last branch by hand, `between` called after the first and the second."""
        x, action, old_logp, adv, target, var = batch
        pol, n, api, st = self.pol, self.n, _lib.api(), _stream()
        s, d = pol.saves, pol.dz
        self.prefill()
        api.mlp_forward(pol.P, pol.PF, x, n, None, None, s["out"], s["h1"], s["h2"], s["h3"], pol.pb_ptr(), st)
        between()
        api.mlp_backward_dx(pol.PT, s["out"], s["h1"], s["h2"], s["h3"], action, old_logp, adv, target, var, n, 1.0 / n, 0.2,
                            d["dz4"], d["dz3"], d["dz2"], d["dz1"], pol.loss_part, pol.ptb_ptr(), st)
        between()
        api.mlp_grad_w(x, s["h1"], s["h2"], s["h3"], d["dz1"], d["dz2"], d["dz3"], d["dz4"], n, pol.workspace, pol.G, None, None,
                       None, pol.tile_wait_error, 1 if pol.gemm == "bf16x3" else 0, st)
        return self.result()

    def nan_the_padded_rows(self):
        for k, w in WIDTH.items():
            buf = self.pol.saves[k] if k in self.pol.saves else self.pol.dz[k]
            buf.view(-1)[RC.padded_row_mask(self.n, w, DEV)] = NAN


def _same_result(a, b, what):
    for k in WIDTH:
        assert RC.same_bits(a["chain"][k], b["chain"][k]), (what, k)
    for k in ("loss", "G", "scales"):
        assert RC.same_bits(a[k], b[k]), (what, k)


def _embed_batch(batch, how):
    return tuple(how(t) for t in batch[:5]) + (batch[5],)


@pytest.mark.parametrize("path,gemm,names", PATHS)
@pytest.mark.parametrize("n", RC.RAGGED_N)
def test_minibatch_gradient_between_guards_on_poisoned_rows(n, path, gemm, names):
    case = GradCase(n, path, gemm, names)
    pol, batch = case.pol, case.batch
    what = "%s %s n=%d" % (path, gemm, n)
    # 1. guarded scratch of the header's sizes, NaN-prefilled; every per-row input inside NaN
    case.use_guards()
    got = case.run(_embed_batch(batch, lambda t: RC.poisoned(t, DEV)))
    assert torch.isfinite(got["G"][pol.grad_mask > 0]).all() and torch.isfinite(got["loss"]).all(), what
    for k in WIDTH:
        assert torch.isfinite(got["chain"][k]).all(), (what, k)
    # 2. bit for bit the same path on plain allocations with zeros around the inputs
    case.use_plain()
    want = case.run(_embed_batch(batch, lambda t: RC.embedded(t, 0.0, DEV)))
    _same_result(got, want, what + ": poisoned against plain")
    # 3. the header leaves the padded rows of the scratch unspecified: no consumer may read them
    if path == "three_launch":
        case.use_guards()
        nanned = case.run_three_launches(_embed_batch(batch, lambda t: RC.poisoned(t, DEV)), case.nan_the_padded_rows)
        _same_result(nanned, want, what + ": padded rows of the scratch overwritten with NaN between the launches")
    # 4. dW = dZ^T A and db = colsum(dZ) against float64 on the chain the launch left; 5. that chain against float64
    x = batch[0]
    grad = RC.grad_errs(RC.grad_blocks(got["G"]), x, got["chain"])
    chain64 = _fp64_chain(case.ref, *batch)
    chain = _errs(got["chain"], chain64)
    # what plain float32 torch reaches on these very rows: a quarter of the bar at most, or the bar would say nothing here
    f32 = RC.f32_chain(case.ref, *batch)
    chain_f32 = _errs(f32, chain64)
    grad_f32 = RC.grad_errs(RC.f32_grad_blocks(x, got["chain"]), x, got["chain"])
    print("%s: dW / db of each block's largest %s (float32 torch %s); chain of each tensor's largest %s (float32 torch %s)"
          % (what, " ".join("%.1e/%.1e" % e for e in grad), " ".join("%.1e/%.1e" % e for e in grad_f32),
             " ".join("%s %.1e" % kv for kv in chain.items()), " ".join("%.1e" % e for e in chain_f32.values())))
    assert max(max(e) for e in grad_f32) <= RC.BAR / 4 and max(chain_f32.values()) <= RC.BAR / 4, (what, grad_f32, chain_f32)
    assert max(max(e) for e in grad) <= RC.BAR, (what, grad)
    assert max(chain.values()) <= RC.BAR, (what, chain)
    W1 = got["G"][:256 * 80].view(256, 80)
    assert torch.all(W1[:, 73:] == 0), what            # the padding columns of W1 see x == 0; element 76 (the mark) is 0


@pytest.mark.parametrize("path,gemm,names", PATHS)
def test_a_nan_advantage_in_the_last_valid_row_reaches_the_gradient(path, gemm, names):
    """The poison control of part B: one NaN moved from the slack into row n - 1 of `adv` does change what is compared."""
    n = 33
    case = GradCase(n, path, gemm, names)
    batch = _embed_batch(case.batch, lambda t: RC.poisoned(t, DEV))
    clean = case.run(batch)
    batch[3][n - 1] = NAN
    case.prefill()
    case.pol.minibatch_grad(*batch, 0.2, **({"dump": True} if path == "fused" else {}))
    torch.cuda.synchronize()
    G, loss = case.pol.G.clone(), case.pol.loss_part[:RC.tiles(n)].clone()
    assert not RC.same_bits(G, clean["G"]) and not RC.same_bits(loss, clean["loss"])
    assert torch.isnan(loss[1]).any() and torch.isfinite(loss[0]).all()       # row 32 is the second tile's only row
    if gemm == "f16x2":
        assert int(case.pol.h2_overflow) != 0                                 # and the fp16x2 step refuses it
    else:
        assert torch.isnan(G[case.pol.grad_mask > 0]).any()


# ---------------------------------------------------------------------------------------------------- C. the rollout launches
RING = {"obs": (73, torch.float32, 1), "act": (18, torch.float32, 0), "logp": (1, torch.float32, 0), "v": (1, torch.float32, 0),
        "reward": (1, torch.float32, 0), "reset": (1, torch.int64, 0), "progress": (1, torch.int64, 0)}    # width, dtype, extra rows


def _rings(T, n, guarded):
    """The rollout tensors of T steps of n envs (obs_ring has T + 1 rows), exactly that large, pre-filled with the sentinel."""
    out = {}
    for k, (w, dtype, extra) in RING.items():
        size = (T + extra) * n * w
        out[k] = Guarded(size, dtype=dtype) if guarded else torch.full((size,), SENTINEL, dtype=dtype, device=DEV)
    return out


def _row(rings, k, t, n):
    w = RING[k][0]
    return _t(rings[k])[t * n * w:(t + 1) * n * w]


def _guard_state(env):
    """Every state tensor of the env (Fly._STATE_TENSORS: exactly n rows each) moved between guards."""
    guards = {}
    for k in env._STATE_TENSORS:
        t = getattr(env, k)
        g = Guarded(t.numel(), dtype=t.dtype, init=t.cpu().numpy())
        setattr(env, k, g.t.view(t.shape))
        guards[k] = g
    env._refresh_pointers()
    return guards


class RolloutCase:
    """Two envs from the same state, one policy, the noise of T steps: env 0 runs the launch under test on guarded rows with
    the noise inside NaN, env 1 the header's contract -- per step mlp_forward_sample (on the normalised row when a table is
    registered) and fly_step -- on plain rows."""

    def __init__(self, n, T, gemm, norm=False, dr=False, seed=5):
        from fly_bproject_amd.ppo import normalize_obs_ref
        self.n, self.T = n, T
        assert "FLY_ROLLOUT_FS" not in os.environ          # nothing overrides the launcher's choice of kernel
        self.ref, self.pol = _policy(gemm, seed)
        self.envs = [make_env(n), make_env(n)]
        self.table = None
        self.dr_guard = None
        if dr:
            from tests.test_domain_rand_gpu import WIDE
            # the table [n][FLY_DR_ROW] the kernels redraw at every reset: env 0's between guards too (counts zeroed, as the
            # header asks before the first registration)
            self.dr_guard = Guarded(n * _lib.DR_ROW, init=np.zeros(n * _lib.DR_ROW, np.float32))
            self.envs[0]._dr_table = self.dr_guard.t.view(n, _lib.DR_ROW)
            for env in self.envs:
                env.set_randomization(WIDE, seed=17)
            assert torch.equal(self.envs[0]._dr_table, self.envs[1]._dr_table) and float(self.envs[0].env_params.std()) > 0.05
        if norm:
            g = torch.Generator().manual_seed(seed)
            table = torch.cat([0.2 * torch.randn(73, generator=g), 0.5 + 1.5 * torch.rand(73, generator=g), torch.tensor([2.0])])
            self.table = table.to(DEV)
            _lib.api().fly_set_obs_norm(self.envs[0]._handle, self.table)
            self.normalise = lambda x: normalize_obs_ref(x, self.table)
        g = torch.Generator().manual_seed(seed + 1)
        self.obs0 = (0.5 * torch.randn(n, 73, generator=g)).to(DEV)
        self.eps_host = torch.randn(T, n, 18, generator=g)
        self.var = _variance()
        self.state_guards = _guard_state(self.envs[0])
        self.got, self.want = _rings(T, n, True), _rings(T, n, False)
        for rings in (self.got, self.want):
            _row(rings, "obs", 0, n).copy_(self.obs0.view(-1))

    def reference(self, eps):
        n, T, env, pol, r = self.n, self.T, self.envs[1], self.pol, self.want
        for t in range(T):
            x = _row(r, "obs", t, n).view(n, 73)
            if self.table is not None:
                x = self.normalise(x).contiguous()
            _lib.api().mlp_forward_sample(pol.P, pol.PF, x, n, eps[t], self.var, t, VAR_DECAY, VAR_MIN, _row(r, "act", t, n),
                                         _row(r, "logp", t, n), None, _row(r, "v", t, n), pol.infer_pb_ptr(), None, _stream())
            env.bind_obs(_row(r, "obs", t + 1, n).view(n, 73))
            env.bind_reward(_row(r, "reward", t, n))
            _lib.api().fly_step(env._handle, _row(r, "act", t, n), C.byref(env._bufs), _stream())
            _row(r, "reset", t, n).copy_(env.reset_buf)
            _row(r, "progress", t, n).copy_(env.progress_buf)

    def launch_all(self, eps):
        env, pol, g = self.envs[0], self.pol, self.got
        _lib.api().ppo_rollout_all(env._handle, C.byref(env._bufs), pol.P, pol.PF, g["obs"].t, eps, self.var, VAR_DECAY, VAR_MIN,
                                  g["act"].t, g["logp"].t, g["v"].t, g["reward"].t, self.T, None, pol.infer_pb_ptr(),
                                  g["reset"].t, g["progress"].t, _stream())

    def launch_steps(self, eps):
        """T calls of ppo_rollout_step, rows bound as PPO._launch_step binds them; the env's own (guarded) flags are copied
        to row t after each step, as that method does."""
        n, env, pol, g = self.n, self.envs[0], self.pol, self.got
        for t in range(self.T):
            env.bind_obs(_row(g, "obs", t + 1, n).view(n, 73))
            env.bind_reward(_row(g, "reward", t, n))
            _lib.api().ppo_rollout_step(env._handle, C.byref(env._bufs), pol.P, pol.PF, _row(g, "obs", t, n), eps[t], self.var, t,
                                       VAR_DECAY, VAR_MIN, _row(g, "act", t, n), _row(g, "logp", t, n), _row(g, "v", t, n),
                                       pol.infer_pb_ptr(), None, _stream())
            _row(g, "reset", t, n).copy_(env.reset_buf)
            _row(g, "progress", t, n).copy_(env.progress_buf)

    def compare(self, all_in_one, what):
        torch.cuda.synchronize()
        for k, g in self.got.items():
            a, b = g.get(), self.want[k].cpu().numpy()
            RC.assert_all_written(a, SENTINEL, "%s %s" % (what, k))
            assert RC.same_bits(a, b), (what, k, np.flatnonzero(RC.bits(a) != RC.bits(b))[:8].tolist())
        assert np.isfinite(self.got["reward"].get()).all() and np.isfinite(self.got["obs"].get()).all(), what
        ref = self.envs[1]
        for k, g in self.state_guards.items():
            a, b = g.get().reshape(-1), getattr(ref, k).cpu().numpy().reshape(-1)
            if all_in_one and k in ("reset_buf", "progress_buf"):
                # with flag rows the one-launch form only READS b->reset / b->progress: the current flags are row T - 1
                assert np.array_equal(a, np.ones_like(a) if k == "reset_buf" else np.zeros_like(a)), (what, k)
                a = _row(self.got, k[:-4], self.T - 1, self.n).cpu().numpy()
            assert RC.same_bits(a, b), (what, k)
        if self.dr_guard is not None:
            table = self.dr_guard.get().reshape(self.n, _lib.DR_ROW)
            assert RC.same_bits(table, ref._dr_table.cpu().numpy()), what
            assert (table[:, 6].view(np.int32) >= 2).all(), what       # the registration draw and step 0's reset, at least

    def close(self):
        for env in self.envs:
            env.exit()


def _rollout(n, T, gemm, entry, **kw):
    case = RolloutCase(n, T, gemm, **kw)
    what = "%s n=%d T=%d %s %s" % (entry, n, T, gemm, kw)
    case.reference(case.eps_host.to(DEV))
    eps = RC.poisoned(case.eps_host, DEV)
    (case.launch_all if entry == "ppo_rollout_all" else case.launch_steps)(eps)
    case.compare(entry == "ppo_rollout_all", what)
    assert torch.isnan(RC.surroundings(eps)).all()
    case.close()


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("n", [12, 33])
@pytest.mark.parametrize("entry", ["ppo_rollout_all", "ppo_rollout_step"])
def test_rollout_between_guards_equals_sample_then_step(entry, n, gemm):
    """12 envs: one ragged tile; 33: one whole tile and one env.  A ragged n selects rollout_all_kernel whatever the
    environment says about the fused-style kernel (and nothing does)."""
    _rollout(n, 3, gemm, entry)


def test_rollout_all_whole_tiles_take_the_fused_style_kernel():
    """n % 32 == 0 under bf16x3 selects rollout_all_fs_kernel: one tile, and one tile more than the device has CUs -- the MULTI
    instantiation, whose workgroup 0 walks a second tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n in (32, 32 * (cus + 1)):
        _rollout(n, 2, "bf16x3", "ppo_rollout_all")


@pytest.mark.parametrize("entry", ["ppo_rollout_all", "ppo_rollout_step"])
def test_rollout_with_obs_norm_and_domain_randomisation_on_a_ragged_tile(entry):
    """The NORM and DR instantiations at 33 envs: a non-identity table (the reference normalises in torch, which the header
    states bit for bit) and the wide ranges of tests/test_domain_rand_gpu.py, drawn alike on both envs."""
    _rollout(33, 3, "bf16x3", entry, norm=True, dr=True)


def test_a_nan_in_the_last_env_noise_changes_that_env_rows():
    """The poison control of part C: one NaN moved into the last valid row of eps_all reaches the compared rows."""
    n, T = 33, 3
    case = RolloutCase(n, T, "bf16x3")
    case.reference(case.eps_host.to(DEV))
    eps = RC.poisoned(case.eps_host, DEV)
    eps[T - 1, n - 1, 0] = NAN
    case.launch_all(eps)
    torch.cuda.synchronize()
    for k in ("act", "logp"):
        a, b = case.got[k].get(), case.want[k].cpu().numpy()
        w = RING[k][0]
        last = slice(((T - 1) * n + n - 1) * w, T * n * w)
        assert RC.same_bits(a[:last.start], b[:last.start]) and not RC.same_bits(a[last], b[last]), k
    case.close()
