"""The packed-network format: the one Python statement of csrc/mlp_layout.h and csrc/dqn_layout.h.

A network is a list of `Layer`s; `Layout` derives from it every offset and size of the master buffer `P`, of its
fragment-ordered copies `PF` / `PT`, of the three-term bf16 planes `PB` / `PTB` and of the two-term fp16 planes, and builds
the index maps the optimizer kernels scatter through.  policy.py (the PPO actor-critic) and dqn.py (the Q-network) declare
their layers and call the constructor helpers below; tests/test_abi_cpu.py compiles the two headers and include/flyhip.h
and holds the numbers derived here to their macros.  Pure host code (numpy and torch on the CPU): it needs no library.
"""
import collections

import numpy as np
import torch

# name; N outputs; K reduced (padded); forward fragment form: "plain", "two_halves" (two K/2 operands, first half of k first)
# or "split_k4" (split-K over the four waves); position of W^T in the transposed buffers (None: no transposed copy);
# forward plane form: "plain" or "two_halves"
Layer = collections.namedtuple("Layer", "name N K frag t_pos plane")


def frag_index(n, k, K):
    """Fragment-order offset of element (n, k) of an operand with K reduced (csrc/mlp_layout.h)."""
    h, kk = k // (K // 2), k % (K // 2)
    return (((n // 32) * (K // 8) + kk // 4) * 64 + (h * 32 + n % 32)) * 4 + kk % 4


def split_k4_index(n, k, K):
    """Fragment-order offset of element (n, k) of a last layer (32 outputs), split-K over the four waves: wave w reduces
    k in [w K/4, (w + 1) K/4) as one operand of its own (csrc/mlp_layout.h at K = 128, csrc/dqn_layout.h at K = 256)."""
    kw = K // 4
    w, h, kq, q = k // kw, (k % kw) // (kw // 2), (k % (kw // 2)) // 4, k % 4
    return ((w * (kw // 8) + kq) * 64 + (h * 32 + n)) * 4 + q


def plane_index(n, k, K):
    """Position (16-bit words) of term 0 of element (n, k) of a bf16x3 operand with K reduced
    (csrc/mlp_layout.h); terms 1 and 2 follow 512 and 1024 words later."""
    return (((n // 32) * (K // 16) + k // 16) * 3) * 512 + (((k % 16) // 8) * 32 + n % 32) * 8 + k % 8


class Layout:
    """Offsets, sizes and index maps of one packed network; per-layer tuples are in layer order."""

    def __init__(self, layers):
        self.layers = tuple(layers)
        self.off_w, self.off_b, self.off_f = [], [], []
        self.packed = self.frag = 0
        for l in self.layers:               # P: weights then bias per layer; PF: the weights alone
            self.off_w.append(self.packed)
            self.off_b.append(self.packed + l.N * l.K)
            self.packed += l.N * l.K + l.N
            self.off_f.append(self.frag)
            self.frag += l.N * l.K
        self.off_t = [None] * len(self.layers)
        self.frag_t = 0
        for li in sorted((li for li, l in enumerate(self.layers) if l.t_pos is not None), key=lambda li: self.layers[li].t_pos):
            self.off_t[li] = self.frag_t    # PT: the W^T operands in the order the layers name
            self.frag_t += self.layers[li].N * self.layers[li].K
        self.off_w, self.off_b, self.off_f, self.off_t = (tuple(o) for o in (self.off_w, self.off_b, self.off_f, self.off_t))
        # the planes hold the fragment copies' operands in the same order, three (bf16) or two (fp16) 16-bit terms per weight
        self.off_pb = tuple(3 * o for o in self.off_f)
        self.off_ptb = tuple(None if o is None else 3 * o for o in self.off_t)
        self.pb_halves, self.ptb_halves = 3 * self.frag, 3 * self.frag_t
        self.ph_halves, self.pth_halves = self.pb_halves * 2 // 3, self.ptb_halves * 2 // 3

    def _maps(self, index, form, terms):
        fwd = np.full(self.packed, -1, np.int32)
        tr = np.full(self.packed, -1, np.int32)
        for li, l in enumerate(self.layers):
            N, K = l.N, l.K
            n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
            src = self.off_w[li] + n * K + k
            how = getattr(l, form)
            if how == "two_halves":         # two K/2 operands (k < K/2, k >= K/2): the forward kernel keeps one half of its input in LDS
                pos = (k // (K // 2)) * (terms * N * (K // 2)) + index(n, k % (K // 2), K // 2)
            elif how == "split_k4":
                pos = split_k4_index(n, k, K)
            else:
                assert how == "plain", l
                pos = index(n, k, K)
            fwd[src] = terms * self.off_f[li] + pos
            if self.off_t[li] is not None:  # W^T: K outputs, N reduced
                tr[src] = terms * self.off_t[li] + index(k, n, N)
        for idx, size in ((fwd, terms * self.frag), (tr, terms * self.frag_t)):     # injective, and the buffer exactly covered
            used = idx[idx >= 0].astype(np.int64)
            allpos = np.concatenate([used + 512 * t for t in range(terms)])
            assert len(np.unique(allpos)) == len(allpos) == size and allpos.max() == size - 1
        return fwd, tr

    def index_maps(self):
        """int32 [packed] maps master index -> position in PF / PT (-1: no copy)."""
        return self._maps(frag_index, "frag", 1)

    def plane_maps(self):
        """int32 [packed] maps master index -> term-0 position in PB / PTB (-1: no copy)."""
        return self._maps(plane_index, "plane", 3)

    def matrices(self, buf):
        """[(W [N][K], b [N]), ...]: the layers as views of a packed buffer."""
        return [(buf[w:b].view(l.N, l.K), buf[b:b + l.N]) for l, w, b in zip(self.layers, self.off_w, self.off_b)]


def scatter_pairs(idx, device):
    """A map on `device`, with the master indices that have a copy and where each goes: (idx, src, dst)."""
    idx = torch.from_numpy(idx).to(device)
    src = torch.nonzero(idx >= 0).squeeze(-1)
    return idx, src, idx[src].long()


def bind_parameters(module, views):
    """Copy every parameter of `module` into its view of a packed buffer and re-point it there: one copy of truth."""
    params = dict(module.named_parameters())
    assert set(params) == set(views), "Net does not have the reference's parameter set"
    with torch.no_grad():
        for k, view in views.items():
            view.copy_(params[k].data.to(view.device))
            params[k].data = view


def grad_mask(views, size, device):
    """f32 [size] on `device`: 1 where some view of the packed buffer lies, 0 on padding and structural zeros."""
    mask = np.zeros(size, np.float32)
    for view in views.values():
        idx = torch.arange(size).as_strided(view.shape, view.stride(), view.storage_offset())
        mask[idx.reshape(-1).numpy()] = 1.0
    return torch.from_numpy(mask).to(device)


def write_planes(dst_buf, master, src, dst):
    """The three bf16 terms of master[src] into a plane buffer at dst, dst + 512, dst + 1024."""
    with torch.no_grad():
        for term, plane in enumerate(split_bf16x3(master[src])):
            dst_buf[dst + 512 * term] = plane


def split_bf16x3(w):
    """fp32 tensor -> three int16 tensors holding the bf16 terms w0 + w1 + w2 == w (exact)."""
    w0 = w.to(torch.bfloat16)
    r1 = w - w0.float()
    w1 = r1.to(torch.bfloat16)
    w2 = (r1 - w1.float()).to(torch.bfloat16)
    return [t.view(torch.int16) for t in (w0, w1, w2)]


def split_f16x2(w, scale):
    """fp32 tensor -> two int16 tensors holding the fp16 terms h0 + h1 ~= w * scale (|error| <= 2^-23 |w scale|)."""
    y = w * scale
    h0 = y.to(torch.float16)
    h1 = (y - h0.float()).to(torch.float16)
    return [t.view(torch.int16) for t in (h0, h1)]


def untile(t, n, N):
    """[rows][N] view of a saved activation / dZ buffer, which the kernels keep in tile-fragment order
    (csrc/mlp_mfma.hip, frag_off): per 32-row tile and 32-column tile a block of 1024 floats
    [g][lane][4] with lane = 32 * ((col % 8) // 4) + row % 32, g = (col % 32) // 8."""
    rows = torch.arange(n, device=t.device).view(-1, 1)
    cols = torch.arange(N, device=t.device).view(1, -1)
    c = cols % 32
    off = ((rows // 32) * (N // 32) + cols // 32) * 1024 + ((c // 8) * 64 + ((c // 4) % 2) * 32 + rows % 32) * 4 + c % 4
    return t.reshape(-1)[off]
