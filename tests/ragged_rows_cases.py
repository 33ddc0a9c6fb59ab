"""What tests/test_mlp_ragged_rows_gpu.py and its CPU pins (tests/test_mlp_ragged_rows_cpu.py) share: buffer sizes as
include/flyhip.h states them, inputs embedded in poisoned allocations, the padded rows of a tile-fragment tensor, and a plain
float32 torch evaluation of the minibatch chain beside tests/test_fused_h2_gpu.py's float64 one.  Pure torch / numpy: every
function takes the device it works on, so all of it runs without a GPU."""
import re

import numpy as np
import torch

from fly_bproject_amd.policy import LAYOUT, untile
from tests.abi_header import header_text

SLACK = 64                      # words of fill on each side of an embedded input (256 or 512 bytes: the base stays 16-byte aligned)
RAGGED_N = (1, 31, 33, 65)      # one valid row; one row short of a tile; one row past it; two tiles and one row
BAR = 2e-5                      # the suite's bar on the chain (of each tensor's largest value) and on dW / db (of each block's)
SAVE_WIDTH = {"out": 32, "h1": 256, "h2": 128, "h3": 128}
DZ_WIDTH = {"dz4": 32, "dz3": 128, "dz2": 128, "dz1": 256}


def header_int(name):
    """The value of an integer `#define` of include/flyhip.h."""
    m = re.search(r"^#define\s+%s\s+(-?\d+)\b" % re.escape(name), header_text(), flags=re.M)
    assert m, name
    return int(m.group(1))


def ceil32(n):
    return (n + 31) // 32 * 32


def tiles(n):
    return (n + 31) // 32


def buffer_sizes(n):
    """Elements of every buffer the policy MLP's entry points write for n rows, as the header states them: row-major tensors
    hold exactly n rows, the tile-fragment scratch ceil32(n), loss_part one pair per tile, G the packed layout."""
    obs, act = header_int("FLY_NUM_OBS"), header_int("FLY_NUM_DOF")
    sizes = {"x": n * obs, "mu": n * act, "act": n * act, "v": n, "logp": n, "loss_part": tiles(n) * 2,
             "G": header_int("MLP_PACKED_FLOATS_ABI")}
    for k, w in list(SAVE_WIDTH.items()) + list(DZ_WIDTH.items()):
        sizes[k] = ceil32(n) * w
    return sizes


def embedded(host, fill, device):
    """`host` (numpy array or tensor) on `device` in the middle of an allocation whose every other word is `fill`, SLACK words
    on each side, the base 16-byte aligned.  Returns the contiguous view that holds the data (it keeps the allocation alive)."""
    t = host.detach().cpu() if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host))
    t = t.contiguous()
    full = torch.full((SLACK + t.numel() + SLACK,), fill, dtype=t.dtype, device=device)
    assert full.data_ptr() % 16 == 0 and (SLACK * full.element_size()) % 16 == 0
    view = full[SLACK:SLACK + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def poisoned(host, device):
    """An INPUT whose surroundings poison whatever reads past it: NaN around floating-point data, 0x7fff... around integers."""
    t = host if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host))
    fill = float("nan") if t.dtype.is_floating_point else torch.iinfo(t.dtype).max
    return embedded(t, fill, device)


def surroundings(view):
    """The SLACK words in front of and behind an embedded view, as one tensor (the view's own storage)."""
    full = torch.as_strided(view, (2 * SLACK + view.numel(),), (1,), view.storage_offset() - SLACK)
    return torch.cat([full[:SLACK], full[SLACK + view.numel():]])


def padded_row_mask(n, width, device="cpu"):
    """Flat indices of rows n .. ceil32(n) - 1 inside a tile-fragment tensor of ceil32(n) rows of `width` columns: the inverse
    of policy.untile, restricted to the padded rows (derived from untile itself, so the two cannot drift apart)."""
    r = ceil32(n)
    where = untile(torch.arange(r * width, device=device), r, width)       # [row][col] -> flat index
    return where[n:].reshape(-1)


def bits(a):
    """The 32- or 64-bit patterns of a float array or tensor, for comparisons that NaN must not defeat."""
    if torch.is_tensor(a):
        return a.contiguous().view(torch.int64 if a.element_size() == 8 else torch.int32)
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.itemsize == 8 else np.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return bool(torch.equal(a, b)) if torch.is_tensor(a) else bool(np.array_equal(a, b))


def assert_all_written(rows, sentinel, what=""):
    """No element of the valid rows still holds the pre-fill: the kernel wrote every one of them."""
    left = rows == sentinel
    assert not bool(left.any()), "%s: %d element(s) of the valid rows were never written" % (what, int(left.sum()))


def batch_like_setup(n, seed, device="cpu"):
    """A minibatch of the distribution tests/test_mlp_train_gpu.py::_setup draws (that one draws on the GPU), and the network:
    (ref, (x, action, old_logp, adv, target, var)).  For the CPU pin of the reference's own error."""
    from fly_bproject_amd.ppo import Net, diag_gauss_logprob
    torch.manual_seed(seed)
    ref = Net(73, 18).to(device)
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, 73, device=device, generator=g)
    var = torch.full((18,), 0.15, device=device)
    with torch.no_grad():
        mu = ref.to_mean(ref.shared_net(x))
        action = (mu + 0.4 * torch.randn(n, 18, device=device, generator=g)).clamp(-1, 1)
        old_logp = diag_gauss_logprob(mu, action, var) + 0.3 * torch.randn(n, device=device, generator=g)
    adv = torch.randn(n, device=device, generator=g)
    target = torch.randn(n, device=device, generator=g) * 1.5
    return ref, (x, action, old_logp, adv, target, var)


def f32_chain(ref, x, action, old_logp, adv, target, var, clip=0.2):
    """The minibatch's chain (ppo.py:184-197) in plain float32 torch: the layers of `ref` as torch evaluates them and every dZ
    from autograd at the pre-activations.  Not a reference: it shows what float32 arithmetic reaches against the float64
    chain on the rows a test uses, so that the bar the kernels are held to is known to be reachable there."""
    from fly_bproject_amd.ppo import diag_gauss_logprob
    elu = torch.nn.functional.elu
    n = x.shape[0]
    pre = []

    def keep(z):
        z.retain_grad()
        pre.append(z)
        return z
    with torch.enable_grad():
        h1 = elu(keep(ref.shared_net[0](x.detach())))
        h2 = elu(keep(ref.shared_net[2](h1)))
        a1, c1 = elu(keep(ref.to_mean[0](h2))), elu(keep(ref.to_value[0](h2)))
        mu = elu(keep(ref.to_mean[2](a1)))
        v = keep(ref.to_value[2](c1))
        ratio = torch.exp(diag_gauss_logprob(mu, action, var) - old_logp).unsqueeze(-1)
        A = adv.unsqueeze(-1)
        loss = (-torch.min(ratio * A, ratio.clamp(1 - clip, 1 + clip) * A)
                + torch.nn.functional.smooth_l1_loss(v, target.unsqueeze(-1))).mean()
        grads = torch.autograd.grad(loss, pre)
    z1, z2, za, zc, zm, zv = grads
    out = torch.zeros(n, 32, device=x.device)
    out[:, :18], out[:, 18:19] = mu.detach(), v.detach()
    dz4 = torch.zeros(n, 32, device=x.device)
    dz4[:, :18], dz4[:, 18:19] = zm, zv
    return {"out": out, "h1": h1.detach(), "h2": h2.detach(), "h3": torch.cat([a1, c1], 1).detach(), "dz4": dz4,
            "dz3": torch.cat([za, zc], 1), "dz2": z2, "dz1": z1}


def grad_blocks(G):
    """[(dW [N][K used], db [N])] of the four layers: views of a packed gradient (layer 1 without its padding columns)."""
    (W1, b1), rest = LAYOUT.matrices(G)[0], LAYOUT.matrices(G)[1:]
    return [(W1[:, :73], b1)] + list(rest)


def grad_operands(x, chain):
    """Per layer (A, dZ): dW = dZ^T A and db = colsum(dZ), on the chain values a launch left (any dtype)."""
    return [(x, chain["dz1"]), (chain["h1"], chain["dz2"]), (chain["h2"], chain["dz3"]), (chain["h3"], chain["dz4"])]


def grad_errs(blocks, x, chain):
    """Per layer the error of (dW, db) against float64 on `chain`, each relative to its block's largest float64 entry."""
    errs = []
    for (W, b), (A, Z) in zip(blocks, grad_operands(x.double(), {k: v.double() for k, v in chain.items()})):
        W64, b64 = Z.T @ A, Z.sum(0)
        errs.append((float((W.double() - W64).abs().max()) / (float(W64.abs().max()) + 1e-300),
                     float((b.double() - b64).abs().max()) / (float(b64.abs().max()) + 1e-300)))
    return errs


def f32_grad_blocks(x, chain):
    """The same products in plain float32 torch (see f32_chain)."""
    return [(Z.float().T @ A.float(), Z.float().sum(0)) for A, Z in grad_operands(x, chain)]
