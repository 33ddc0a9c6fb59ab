"""Packed parameter storage of `Net` and the MFMA forward (`mlp_forward`, include/flyhip.h).

`PackedPolicy` owns ONE flat fp32 buffer in the layout of csrc/mlp_layout.h and re-points the
`.data` of every `Net` parameter at a strided view into it, so torch (checkpoint I/O, autograd,
optimizers) and the HIP kernels see the same memory.  Padding and the structural zeros of the
stacked last layer never receive gradient (`grad_mask`).  The format itself -- offsets, sizes, index maps -- is
packing.py's: this module declares the four layers to it (tests/test_abi_cpu.py holds the result to the header).
"""
import ctypes as C
import os

import torch

from . import _lib, options, packing
from .packing import split_bf16x3, split_f16x2, untile   # noqa: F401  (read from here by tests and tools)

p = _lib.ptr

IN, IN_PAD, H1, H2, H3, OUT, NACT = 73, 80, 256, 128, 128, 32, 18
LAYOUT = packing.Layout([
    packing.Layer("W1", H1, IN_PAD, "plain", None, "plain"),
    # layer 2 forward: two K = 128 operands (k < 128, k >= 128), one per half of H1 in LDS
    packing.Layer("W2", H2, H1, "two_halves", 0, "two_halves"),
    packing.Layer("W3", H3, H2, "plain", 1, "plain"),
    # layer 4 forward: split-K over the four waves (the planes keep the generic order)
    packing.Layer("W4", OUT, H3, "split_k4", 2, "plain")])
OFF_W1, OFF_W2, OFF_W3, OFF_W4 = LAYOUT.off_w
OFF_B1, OFF_B2, OFF_B3, OFF_B4 = LAYOUT.off_b
PACKED = LAYOUT.packed
ERR_SLOT = OFF_W1 + 76                     # a masked padding element of W1: the "this gradient is invalid" mark (csrc/mlp_grad_w.inc)
OFF_F1, OFF_F2, OFF_F3, OFF_F4 = LAYOUT.off_f
FRAG = LAYOUT.frag
_, OFF_TF2, OFF_TF3, OFF_TF4 = LAYOUT.off_t
FRAG_T = LAYOUT.frag_t
PB_HALVES, PTB_HALVES = LAYOUT.pb_halves, LAYOUT.ptb_halves
OFF_PB, OFF_PTB = LAYOUT.off_pb, LAYOUT.off_ptb
build_index_maps, build_plane_maps = LAYOUT.index_maps, LAYOUT.plane_maps

# fp16x2 planes of the fused optimizer step (csrc/mlp_fused_h2.inc): PB's / PTB's layout with two terms per k block
PH_HALVES, PTH_HALVES = LAYOUT.ph_halves, LAYOUT.pth_halves
H2_INV, H2_W0 = 16, 8                               # (csrc/mlp_adam.inc: [40, 41] and [64 ..) are mlp_adam_step's rescale bookkeeping)
H2_SINCE, H2_WMAX, H2_WMAX_SLOTS = 40, 64, (PACKED + 63) // 64
H2_SCALE_FLOATS = H2_WMAX + 2 * H2_WMAX_SLOTS       # two tables of max |w| per 64 packed elements behind the scales
H2_CLASSES = ("x", "h1", "h2", "h3", "dz4", "dz3", "dz2", "dz1")
# where the step steers a class maximum of |scaled value| -- [2^e, 2^(e + 1)) -- and the floor under which a launch is refused
# (csrc/fs_h2.inc: H2_TARGET_EXP_ACT / _GRAD, H2_CLASS_FLOOR; the tests derive their windows and bars from these)
H2_TARGET_EXP_ACT, H2_TARGET_EXP_GRAD, H2_CLASS_FLOOR = 7, 2, 2.0 ** -8


def h2_weight_scale(wmax):
    """The power of two mlp_h2_rescale gives a layer whose largest |w| is `wmax`: max(wmax, 2^-4) lands in [2^11, 2^12)."""
    import math
    m = min(max(float(wmax), 2.0 ** -4), 2.0 ** 60)
    return 2.0 ** (11 - math.floor(math.log2(m)))


class PackedPolicy:
    def __init__(self, net, device):
        self.device = torch.device(device)
        self._lib = _lib.load()
        self.P = torch.zeros(PACKED, dtype=torch.float32, device=self.device)
        self.PF = torch.zeros(FRAG, dtype=torch.float32, device=self.device)      # forward operands, fragment order
        self.PT = torch.zeros(FRAG_T, dtype=torch.float32, device=self.device)    # W^T operands, fragment order
        # GEMM arithmetic of the MFMA kernels: "bf16x3" (default) = three-term bf16 split of both fp32 operands on
        # v_mfma_f32_32x32x16_bf16, fp32 accumulate (held to the reference's golden vectors at the fp32 tolerances and to fp64:
        # tests/test_ppo_gpu.py, tests/test_mlp_train_gpu.py, csrc/mlp_layout.h); "f32" = v_mfma_f32_32x32x2_f32.  What the
        # environment selects for a policy of its own (options.resolve_gemm has the rule and names the variables)
        self._gemm, step_gemm = options.resolve_gemm(None, os.environ)
        self.gemm_infer = os.environ.get("FLY_GEMM_INFER", self._gemm)
        assert self._gemm in ("f32", "bf16x3") and self.gemm_infer in ("f32", "bf16x3")
        self.PB = torch.zeros(PB_HALVES, dtype=torch.int16, device=self.device)
        self.PTB = torch.zeros(PTB_HALVES, dtype=torch.int16, device=self.device)
        # Arithmetic of the fused optimizer-step gradient (only): "bf16x3" (mlp_fused_grad) or "f16x2" (mlp_fused_grad_h2: two fp16 terms
        # per operand, three products per k block, per-class power-of-two scales; csrc/mlp_fused_h2.inc).  The rollout's policy, the
        # critic pass and every fallback stay on `gemm`.  policy.step_gemm = ...
        # DEFAULT (round 5): f16x2, with bf16x3 as the A/B and as the fallback of a refused step; `policy.gemm = "bf16x3"`
        # names every GEMM, the step included.  (Under f32 the step is f32 and this selection is not looked at: see step_gemm.)
        self._step_gemm = step_gemm if self._gemm == "bf16x3" else "bf16x3"
        assert self._step_gemm in ("bf16x3", "f16x2")
        self.PH = torch.zeros(PH_HALVES, dtype=torch.int16, device=self.device)
        self.PTH = torch.zeros(PTH_HALVES, dtype=torch.int16, device=self.device)
        self.h2_scales = torch.zeros(H2_SCALE_FLOATS, dtype=torch.float32, device=self.device)
        self.h2_overflow = torch.zeros(1, dtype=torch.int32, device=self.device)     # sticky: a launch's values did not fit fp16
        self.h2_freeze = False              # tests: the reduction leaves the scale table alone
        self.h2_calibrated = False
        self.h2_suspended = False           # True while refused steps are redone on the bf16x3 kernel (the planes stay maintained)
        self.h2_overflows = 0               # updates in which the fp16x2 step was refused and redone on bf16x3
        self.h2_calibration_failures = 0    # data-parallel updates run on bf16x3 because some rank's calibrate_h2 did not settle
        self._h2_reset_scales()
        idx_fb, idx_tb = build_plane_maps()
        self.idx_fb, self._src_fb, self._dst_fb = packing.scatter_pairs(idx_fb, self.device)
        self.idx_tb, self._src_tb, self._dst_tb = packing.scatter_pairs(idx_tb, self.device)
        idx_f, idx_t = build_index_maps()
        self.idx_f, self._src_f, self._dst_f = packing.scatter_pairs(idx_f, self.device)
        self.idx_t, self._src_t, self._dst_t = packing.scatter_pairs(idx_t, self.device)
        (self.W1, self.b1), (self.W2, self.b2), (self.W3, self.b3), (self.W4, self.b4) = LAYOUT.matrices(self.P)
        self.views = {
            "shared_net.0.weight": self.W1[:, :IN], "shared_net.0.bias": self.b1,
            "shared_net.2.weight": self.W2, "shared_net.2.bias": self.b2,
            "to_mean.0.weight": self.W3[:64], "to_mean.0.bias": self.b3[:64],
            "to_value.0.weight": self.W3[64:], "to_value.0.bias": self.b3[64:],
            "to_mean.2.weight": self.W4[:NACT, :64], "to_mean.2.bias": self.b4[:NACT],
            "to_value.2.weight": self.W4[NACT:NACT + 1, 64:], "to_value.2.bias": self.b4[NACT:NACT + 1],
        }
        packing.bind_parameters(net, self.views)
        self.grad_mask = packing.grad_mask(self.views, PACKED, self.device)
        assert int(self.grad_mask.sum().item()) == 69587            # every reference parameter exactly once
        self.refresh()

    def refresh(self):
        """Rebuild the fragment-ordered copies from the master weights (after a load or any
        out-of-band change of the parameters; mlp_adam_step keeps them in step by itself).  The fp16x2
        activation / gradient scales were measured on the old weights: the next update calibrates again."""
        with torch.no_grad():
            self.PF[self._dst_f] = self.P[self._src_f]
            self.PT[self._dst_t] = self.P[self._src_t]
            self._refresh_planes()
        self.h2_calibrated = False
        self.version += 1

    refresh_transposes = refresh

    def _refresh_planes(self):
        packing.write_planes(self.PB, self.P, self._src_fb, self._dst_fb)
        packing.write_planes(self.PTB, self.P, self._src_tb, self._dst_tb)
        if self.h2_live():
            self._refresh_planes_h2()

    def h2_live(self):
        return self._step_gemm == "f16x2" and self._gemm == "bf16x3"

    def _h2_reset_scales(self):
        """Starting scales of the activation / gradient classes (calibrate_h2 replaces them by measured ones)."""
        s = torch.ones(H2_SCALE_FLOATS)
        s[:4] = 2.0 ** 4                    # x, h1 .. h3: O(1 .. 100)
        s[4:8] = 2.0 ** 28                  # dz4 .. dz1: O(1e-6)
        s[H2_INV:H2_INV + 16] = 1.0 / s[:16]
        s[32:] = 0.0
        self.h2_scales.copy_(s)
        self.h2_calibrated = False

    def _refresh_planes_h2(self):
        """fp16x2 weight planes and their per-layer scales from the master weights (`mlp_h2_rescale`: one small launch, no host sync).
        The scales then stay fixed while mlp_adam_step splits the updated weights under them; an Adam step moves a weight by at most
        3.2 lr, and overflowing needs a weight to travel 15/16 at least, so a rescale every `0.9 / (3.2 lr)` applied steps keeps fp16
        safe (mlp_adam_step rescales by itself; this launch also seeds its bookkeeping in the table)."""
        if self.device.type != "cuda":
            return                                  # (layout-only uses of the class on the CPU: tests/test_dist_cpu.py)
        _lib.api().mlp_h2_rescale(self.P, self.idx_fb, self.idx_tb, self.PH, self.PTH, self.h2_scales, _lib.stream_ptr())

    def _planes_live(self):
        return self._gemm == "bf16x3" or self.gemm_infer == "bf16x3"

    @property
    def step_gemm(self):
        return self._step_gemm if self._gemm == "bf16x3" else self._gemm

    @step_gemm.setter
    def step_gemm(self, mode):
        assert mode in ("bf16x3", "f16x2")
        was = self.h2_live()
        self._step_gemm = mode
        if self.h2_live() and not was:
            self._refresh_planes_h2()

    @property
    def gemm(self):
        return self._gemm

    @gemm.setter
    def gemm(self, mode):
        """Arithmetic of EVERY MLP GEMM of this policy: the update's forward, dX chain and dW, the rollout's
        policy launch and the critic pass.  Switching to bf16x3 rebuilds the term planes: the Adam kernel only
        maintains them while a bf16x3 mode is active (six extra scattered stores per weight otherwise wasted)."""
        if mode == "f16x2":                 # bf16x3 everywhere, the fused optimizer step in fp16x2 (the default configuration)
            self.gemm = "bf16x3"
            self.step_gemm = "f16x2"
            return
        assert mode in ("f32", "bf16x3")
        was_live, was_h2 = self._planes_live(), self.h2_live()
        self._gemm = mode
        self.gemm_infer = mode
        self._step_gemm = "bf16x3"          # an explicit arithmetic names every GEMM, the optimizer step included
        if self._planes_live() and not was_live:
            self._refresh_planes()
        elif self.h2_live() and not was_h2:
            self._refresh_planes_h2()
    version = 0         # bumped whenever the weights change: consumers of cached network outputs compare it

    def _plane_args(self):
        if not self._planes_live():
            return (None, None, None, None)
        return (p(self.PB), p(self.PTB), p(self.idx_fb), p(self.idx_tb))

    def _h2_args(self):
        if not self.h2_live():
            return (None, None, None, C.c_int(0))
        # a RESCALE step (the kernel re-derives the weight scales from the weights before it splits under them) every `period` APPLIED
        # steps -- the kernel counts them on the device, a refused step does not count --, often enough that a weight cannot have
        # drifted out of the scale's 16x headroom: an Adam step moves it by at most 3.2 lr
        period = max(1, min(64, int(0.9 / (3.2 * self.lr))))
        return (p(self.PH), p(self.PTH), p(self.h2_scales), C.c_int(period))

    def pb_ptr(self):
        """Term planes for the UPDATE's forward (minibatch_grad); inference launches (rollout policy,
        critic rows, Net.pi / Net.v) stay on the fp32 MFMA body, which at one tile per CU is bound by
        latency, not by matrix time."""
        return C.c_void_p(self.PB.data_ptr()) if self.gemm == "bf16x3" else None

    def infer_pb_ptr(self):
        return C.c_void_p(self.PB.data_ptr()) if self.gemm_infer == "bf16x3" else None

    def ptb_ptr(self):
        return C.c_void_p(self.PTB.data_ptr()) if self.gemm == "bf16x3" else None

    def forward(self, x, want_mu=True, want_v=True, saves=None):
        """x f32 [..., 73] on the device -> (mu [..., 18] | None, v [..., 1] | None)."""
        lead = x.shape[:-1]
        x2 = x.reshape(-1, IN)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        n = x2.shape[0]
        mu = torch.empty((n, NACT), device=self.device) if want_mu else None
        v = torch.empty((n,), device=self.device) if want_v else None
        s = saves or {}
        _lib.api().mlp_forward(self.P, self.PF, x2, n, mu, v, s.get("out"), s.get("h1"), s.get("h2"), s.get("h3"),
                              self.pb_ptr() if saves else self.infer_pb_ptr(), _lib.stream_ptr())
        return (mu.view(*lead, NACT) if want_mu else None), (v.view(*lead, 1) if want_v else None)

    # ---- training on the MFMA kernels (ppo.py:184-199) ------------------------------------------
    def init_training(self, max_rows, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0):
        dev = self.device
        self.lr, self.betas, self.eps, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        self.G = torch.zeros(PACKED, device=dev)
        self.exp_avg = torch.zeros(PACKED, device=dev)
        self.exp_avg_sq = torch.zeros(PACKED, device=dev)
        self._step2 = torch.zeros(2, dtype=torch.int32, device=dev)    # the step counter (two words: see adam_step)
        self._step_idx = 0
        self.steps_issued = 0              # adam_step calls so far; the device counter lags iff a step was refused (fail closed)
        self._norm_ws = torch.zeros(1280, device=dev)      # [0] = pre-clip gradient norm, rest partial sums
        self.grad_norm = self._norm_ws[:1]
        self.workspace = torch.empty(int(self._lib.mlp_grad_workspace_floats()), device=dev)
        self.max_rows = int(max_rows)
        r = (self.max_rows + 31) // 32 * 32        # whole 32-row tiles: the saved tensors are stored tile by tile
        self.saves = {"out": torch.empty(r, OUT, device=dev), "h1": torch.empty(r, H1, device=dev),
                      "h2": torch.empty(r, H2, device=dev), "h3": torch.empty(r, H3, device=dev)}
        self.dz = {"dz4": torch.empty(r, OUT, device=dev), "dz3": torch.empty(r, H3, device=dev),
                   "dz2": torch.empty(r, H2, device=dev), "dz1": torch.empty(r, H1, device=dev)}
        self.loss_part = torch.zeros((r + 31) // 32, 2, device=dev)
        # mlp_forward_backward: per-tile "forward done" words (compared against a per-call epoch,
        # never reset) and the word a workgroup sets if it ever gives up waiting (stays 0)
        self._tile_flags = torch.zeros((r + 31) // 32, dtype=torch.int32, device=dev)
        self.tile_wait_error = torch.zeros(1, dtype=torch.int32, device=dev)
        self._epoch = 0
        # bf16x3 only: the whole minibatch gradient in ONE persistent launch (csrc/mlp_fused_step.inc: forward, loss, dX chain and
        # dW of a tile in the workgroup that owns it; nothing but x, the per-row scalars and one partial slab per CU touches
        # HBM).  FLY_FUSED_STEP=0 keeps the three-launch path (the A/B).
        self.fused_step = os.environ.get("FLY_FUSED_STEP", "1") != "0"
        self._fused_ws = None
        self.fuse_fwd_bwd = os.environ.get("FLY_FUSE_FWD_BWD", "1") != "0"
        # how a tile travels from its forward to its backward workgroup inside the one launch
        # (csrc/mlp_backward.inc): "sc1" = write-through stores + L1-bypassing loads, no placement
        # assumption (default); "xcd" = plain accesses, producer and consumer must share an XCD
        self.handoff = os.environ.get("FLY_FWD_BWD_HANDOFF", "sc1")
        assert self.handoff in ("sc1", "xcd")
        if self.fuse_fwd_bwd:
            self._probe_fused_launch()

    def _probe_fused_launch(self):
        """One small fused launch over 64 tiles (8 per XCD) at start-up: if a backward workgroup cannot
        get its tile (no in-order dispatch: err 1; "xcd" hand-off on a device that places workgroups
        differently: err 2) the two-launch path is used from the start -- same results."""
        n = min(self.max_rows, 64 * 32)
        z = lambda *shape: torch.zeros(*shape, device=self.device)   # noqa: E731
        was, self.h2_suspended = self.h2_suspended, True        # (not a launch whose values the fp16x2 scales should be judged on)
        try:
            self.minibatch_grad(z(n, IN), z(n, NACT), z(n), z(n), z(n), torch.full((NACT,), 0.2, device=self.device), 0.2)
        finally:
            self.h2_suspended = was
        self.check_fused_launch()

    def update_can_be_refused(self):
        """True when a launch of the current update path can leave an invalid gradient that the optimizer kernels then refuse on
        the device (the fused forward+backward launch's tile hand-off; a value of the fp16x2 step that did not fit fp16): the caller
        must read the step counter after the update and redo what was refused.  The bf16x3 fused optimizer step (`mlp_fused_grad`)
        and the two-launch path cannot."""
        if self.fused_step and self.gemm == "bf16x3":
            return self.h2_live() and os.environ.get("FLY_H2_DIAG_NO_STEP_READ") != "1"     # (diagnostic: what the blocking read costs)
        return bool(self.fuse_fwd_bwd)

    def check_fused_launch(self):
        """Host sync.  Returns the err word of the fused launches since the last check (0 = all fine) and
        clears it; a nonzero word switches this policy to the two-launch path.  The optimizer kernels
        have already refused every step whose gradient came from a failed launch (they fail closed on
        the device), so the caller only has to redo those minibatches (PPO._update_hip)."""
        err = int(self.tile_wait_error.item())
        if err != 0:
            self.fuse_fwd_bwd = False
            self.fused_launch_failures = getattr(self, "fused_launch_failures", 0) + 1
            self.tile_wait_error.zero_()
        return err

    def minibatch_grad(self, x, action, old_logp, adv, target, var, clip, global_rows=None, fuse_norm=False, dump=False):
        """Forward + loss + backward of one minibatch; leaves the packed gradient in `self.G`.
        `fuse_norm` (single rank): the partial reduction also prepares the clip norm and advances the
        step, so `adam_step(norm_ready=True)` is one launch."""
        n = x.shape[0]
        assert n <= self.max_rows and x.is_contiguous() and action.is_contiguous()
        for t in (old_logp, adv, target):
            assert t.is_contiguous() and t.numel() == n
        s, d = self.saves, self.dz
        st = _lib.stream_ptr()
        inv_b = 1.0 / float(global_rows if global_rows else n)
        if self.fused_step and self.gemm == "bf16x3":
            return self._fused_grad(x, action, old_logp, adv, target, var, clip, inv_b, fuse_norm, dump)
        if dump:
            raise ValueError("dump=True is a debugging aid of the fused step")
        if self.fuse_fwd_bwd:
            # one launch: the backward workgroup of a row tile starts when that tile's forward is done
            if self._epoch >= (1 << 27) - 1:
                self._tile_flags.zero_()
                self._epoch = 0
            self._epoch += 1
            _lib.api().mlp_forward_backward(
                self.P, self.PF, self.PT, x, n, s["out"], s["h1"], s["h2"], s["h3"], action, old_logp, adv, target, var, inv_b, clip,
                d["dz4"], d["dz3"], d["dz2"], d["dz1"], self.loss_part, self._tile_flags, self._epoch, self.tile_wait_error,
                self.pb_ptr(), self.ptb_ptr(), 1 if self.handoff == "sc1" else 0, st)
        else:
            _lib.api().mlp_forward(self.P, self.PF, x, n, None, None, s["out"], s["h1"], s["h2"], s["h3"], self.pb_ptr(), st)
            _lib.api().mlp_backward_dx(self.PT, s["out"], s["h1"], s["h2"], s["h3"], action, old_logp, adv, target, var, n, inv_b,
                                      clip, d["dz4"], d["dz3"], d["dz2"], d["dz1"], self.loss_part, self.ptb_ptr(), st)
        nm = (self.grad_mask, self._norm_ws, self.step) if fuse_norm else (None, None, None)
        _lib.api().mlp_grad_w(x, s["h1"], s["h2"], s["h3"], d["dz1"], d["dz2"], d["dz3"], d["dz4"], n, self.workspace, self.G, *nm,
                             self.tile_wait_error, 1 if self.gemm == "bf16x3" else 0, st)

    def _fused_grad(self, x, action, old_logp, adv, target, var, clip, inv_b, fuse_norm, dump):
        """`mlp_fused_grad`: one persistent launch + the slab reduction.  dump=True (tests) also writes the chain's values into
        self.saves / self.dz exactly as the three-launch path leaves them."""
        n = x.shape[0]
        if self._fused_ws is None:
            self._fused_ws = torch.empty(int(max(self._lib.mlp_fused_workspace_floats(), self._lib.mlp_fused_h2_workspace_floats())),
                                         device=self.device)
        nm = (self.grad_mask, self._norm_ws, self.step) if fuse_norm else (None, None, None)
        dptr = None
        if dump:
            s, d = self.saves, self.dz
            arr = (C.c_void_p * 8)(*[t.data_ptr() for t in (s["out"], s["h1"], s["h2"], s["h3"], d["dz4"], d["dz3"], d["dz2"], d["dz1"])])
            dptr = arr
        if self.h2_live() and not self.h2_suspended:
            _lib.api().mlp_fused_grad_h2(self.P, self.PH, self.PTH, self.h2_scales, self.h2_overflow, 1 if self.h2_freeze else 0, x, n,
                                        action, old_logp, adv, target, var, inv_b, clip, self._fused_ws, self.G, *nm, self.loss_part,
                                        dptr, _lib.stream_ptr())
            return
        _lib.api().mlp_fused_grad(self.P, self.PB, self.PTB, x, n, action, old_logp, adv, target, var, inv_b, clip, self._fused_ws,
                                 self.G, *nm, self.loss_part, dptr, _lib.stream_ptr())

    def calibrate_h2(self, x, action, old_logp, adv, target, var, clip, global_rows=None, max_launches=12):
        """Bring the activation / gradient scales of the fp16x2 step to the data (host-synchronising; before the first update on a new
        network or after an overflow): launch the gradient on one minibatch -- the result is discarded, the step counter untouched --
        until a launch fits fp16 and leaves the scales it found.  Every launch sets each class's scale from the maximum it saw, and an
        overflowing class garbles only what lies downstream of it, so the table settles in at most one launch per class.  Returns
        the number of launches."""
        assert self.h2_live()
        frozen, self.h2_freeze = self.h2_freeze, False
        try:
            for k in range(1, max_launches + 1):
                self.h2_overflow.zero_()
                before = self.h2_scales[:8].clone()
                self.minibatch_grad(x, action, old_logp, adv, target, var, clip, global_rows=global_rows, fuse_norm=False)
                fit = int(self.h2_overflow.item()) == 0
                if fit and torch.equal(before, self.h2_scales[:8]):
                    self.h2_calibrated = True
                    return k
            raise _lib.FlyHipError("calibrate_h2: the fp16x2 scales did not settle in %d launches (maxima %s)"
                                   % (max_launches, self.h2_scales[32:40].tolist()))
        finally:
            self.h2_overflow.zero_()
            self.h2_freeze = frozen

    def update_path(self):
        """Which launches one optimizer step is made of (for the bench line)."""
        if self.fused_step and self.h2_live():
            return ("mlp_fused_grad_h2 (ONE persistent launch: forward + loss + dX chain + dW per tile in fp16x2, slabs reduced, scales "
                    "tracked) + mlp_adam_step, gemm=bf16x3, step_gemm=f16x2")
        if self.fused_step and self.gemm == "bf16x3":
            return "mlp_fused_grad (ONE persistent launch: forward + loss + dX chain + dW per tile, slabs reduced) + mlp_adam_step, gemm=bf16x3"
        if self.fuse_fwd_bwd:
            return "mlp_forward_backward (one launch, per-tile flags) + mlp_grad_w (+reduce) + mlp_adam_step, gemm=" + self.gemm
        return "mlp_forward + mlp_backward_dx + mlp_grad_w (+reduce) + mlp_adam_step, gemm=" + self.gemm

    def loss_value(self, n):
        """ppo.py:194/:197 scalar of the last minibatch_grad call (diagnostics; one small reduction)."""
        parts = self.loss_part[: (n + 31) // 32].sum(0)
        return (parts[0] + parts[1]) / n

    @property
    def step(self):
        """Device int32 [1]: optimizer steps applied so far."""
        return self._step2[self._step_idx:self._step_idx + 1]

    # ---- exact resume (train_state.py) ------------------------------------------
    # The master weights and Adam's moments and counter; the derived copies PF / PT / PB / PTB as mlp_adam_step's scatter left
    # them (stored, not rebuilt: nothing then rests on the torch-side split matching the kernel's bit for bit); the fp16x2 step
    # verbatim -- the planes, and the whole scale table with the lagged class scales, the weight scales and the rescale
    # bookkeeping in it.  G, the norm workspace, the saved activations, the tile flags and the sticky words are scratch of an
    # optimizer step: between updates they hold nothing a later step reads.
    _STATE_TENSORS = ("P", "exp_avg", "exp_avg_sq", "_step2", "PF", "PT", "PB", "PTB", "PH", "PTH", "h2_scales")
    _STATE_VALUES = (("_step_idx", int), ("steps_issued", int), ("h2_calibrated", bool), ("h2_overflows", int),
                     ("h2_calibration_failures", int), ("fuse_fwd_bwd", bool))

    def training_state(self):
        """Everything of this policy that an interrupted run needs back, tensors on the CPU.  A host sync."""
        from .train_state import pack
        state = {k.lstrip("_"): pack(getattr(self, k)) for k in self._STATE_TENSORS}
        state.update({k.lstrip("_"): kind(getattr(self, k)) for k, kind in self._STATE_VALUES})
        return state

    def load_training_state(self, state):
        """training_state() back, in place -- and NOT through refresh(), which would rebuild the planes, rewrite the scale
        table and clear the calibration.  Call it after everything that does (a gemm selection, broadcast_policy)."""
        from .train_state import restore, value
        for k in self._STATE_TENSORS:
            restore(getattr(self, k), state, "policy", k.lstrip("_"))
        for k, kind in self._STATE_VALUES:
            setattr(self, k, value(state, "policy", k.lstrip("_"), kind))
        self.h2_overflow.zero_()
        self.h2_suspended = False
        self.version += 1                                   # cached network outputs are of other weights

    def adam_step(self, grad_scale=1.0, norm_ready=False, self_norm=False, grad_invalid=None):
        """clip_grad_norm_ + Adam on the packed parameters.  norm_ready: mlp_grad_w has already left the norm
        partials and advanced the step (single rank).  self_norm: ONE launch that also sums the gradient
        (data-parallel ranks: G comes out of the all-reduce); the step counter then ping-pongs between two
        device words so that no workgroup reads a value another one has already advanced.  grad_invalid: optional int32 device
        word (the err word of the peer-to-peer exchange); nonzero = the launch refuses the step (fail closed)."""
        self.version += 1
        self.steps_issued += 1
        step_in = self.step
        step_out = None
        if self_norm:
            self._step_idx ^= 1
            step_out = self.step
        _lib.api().mlp_adam_step(self.P, self.PF, self.PT, self.idx_f, self.idx_t, self.G, self.grad_mask, self.exp_avg,
                                self.exp_avg_sq, step_in, self.lr, self.betas[0], self.betas[1], self.eps, self.max_norm, grad_scale,
                                self._norm_ws, 1 if norm_ready else 0, *self._plane_args(), step_out, grad_invalid,
                                *self._h2_args(), _lib.stream_ptr())
