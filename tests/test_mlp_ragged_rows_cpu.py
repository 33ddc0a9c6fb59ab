"""CPU pins of what tests/test_mlp_ragged_rows_gpu.py rests on (tests/ragged_rows_cases.py): the padded-row mask against
policy.untile, the header's buffer sizes, the poisoned embedding, the guard and "every valid row written" checks biting, and
the float64 reference's own distance from plain float32 torch at the ragged row counts -- a quarter of the bar at most, so the
bar the kernels are held to (2e-5) is reachable at n = 1, 31, 33, 65."""
import numpy as np
import pytest
import torch

from fly_bproject_amd.policy import PACKED, untile
from tests import ragged_rows_cases as RC
from tests import test_rollout_kernels_gpu as RK
from tests.test_fused_h2_gpu import _errs, _fp64_chain
from tests.test_fused_step_gpu import WIDTH


@pytest.mark.parametrize("width", [32, 128, 256])
@pytest.mark.parametrize("n", RC.RAGGED_N + (32, 64))
def test_padded_row_mask_is_the_inverse_of_untile_on_the_padded_rows(n, width):
    r = RC.ceil32(n)
    mask = RC.padded_row_mask(n, width)
    assert mask.numel() == (r - n) * width == mask.unique().numel()
    t = torch.zeros(r * width)
    t[mask] = float("nan")
    rows = untile(t, n, width)
    assert rows.shape == (n, width) and torch.isfinite(rows).all()            # no valid row holds a masked word
    assert int(torch.isnan(t).sum()) == (r - n) * width
    valid = untile(torch.arange(r * width), n, width).reshape(-1)
    assert torch.equal(torch.cat([valid, mask]).sort().values, torch.arange(r * width))     # and together they are the tensor


def test_buffer_sizes_are_the_headers():
    assert RC.header_int("MLP_PACKED_FLOATS_ABI") == PACKED == RC.buffer_sizes(1)["G"]
    assert set(WIDTH) == set(RC.SAVE_WIDTH) | set(RC.DZ_WIDTH) and all(WIDTH[k] == w for k, w in RC.SAVE_WIDTH.items())
    assert all(WIDTH[k] == w for k, w in RC.DZ_WIDTH.items())
    s = RC.buffer_sizes(33)
    assert (s["x"], s["mu"], s["act"], s["v"], s["logp"]) == (33 * 73, 33 * 18, 33 * 18, 33, 33)      # row-major: exactly n rows
    assert (s["out"], s["h1"], s["h2"], s["h3"]) == (64 * 32, 64 * 256, 64 * 128, 64 * 128)            # scratch: ceil32(n) rows
    assert (s["dz4"], s["dz3"], s["dz2"], s["dz1"]) == (64 * 32, 64 * 128, 64 * 128, 64 * 256)
    assert s["loss_part"] == 4 and RC.buffer_sizes(32)["loss_part"] == 2 and RC.buffer_sizes(1)["h1"] == 32 * 256


def test_poisoned_inputs_are_surrounded_by_poison():
    x = np.arange(33 * 73, dtype=np.float32).reshape(33, 73)
    px = RC.poisoned(x, "cpu")
    assert px.is_contiguous() and px.data_ptr() % 16 == 0 and np.array_equal(px.numpy(), x)
    around = RC.surroundings(px)
    assert around.numel() == 2 * RC.SLACK and torch.isnan(around).all()
    flags = RC.poisoned(np.arange(5, dtype=np.int64), "cpu")
    assert (RC.surroundings(flags) == 0x7fffffffffffffff).all() and flags.tolist() == [0, 1, 2, 3, 4]
    assert (RC.surroundings(RC.poisoned(np.zeros(3, np.int32), "cpu")) == 0x7fffffff).all()
    zeros = RC.embedded(torch.from_numpy(x), 0.0, "cpu")
    assert (RC.surroundings(zeros) == 0).all() and torch.equal(zeros, px)
    nan = np.float32("nan")
    assert RC.same_bits(np.array([nan, 1.0], np.float32), np.array([nan, 1.0], np.float32))
    assert not RC.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))


@pytest.fixture
def host_guards(monkeypatch):
    """tests/test_rollout_kernels_gpu.py's Guarded on the host: the same class, its arrays on the CPU."""
    monkeypatch.setattr(RK, "DEV", "cpu")
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return RK.Guarded


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
def test_a_word_in_either_guard_fails_the_read(host_guards, dtype):
    g = host_guards(33, dtype=dtype)
    g.t.fill_(1)
    assert (g.get() == 1).all()
    for word in (0, g.lo - 1, g.lo + g.n, g.full.numel() - 1):            # both ends of both guards
        g.full[word] = 0
        with pytest.raises(AssertionError, match="wrote"):
            g.get()
        g.full[word] = RK.SENTINEL
        g.get()


def test_a_surviving_sentinel_fails_the_written_check(host_guards):
    g = host_guards(33 * 18)
    g.t.fill_(0.5)
    rows = g.get().reshape(33, 18)
    RC.assert_all_written(rows, RK.SENTINEL, "rows")
    g.t[32 * 18 + 17] = RK.SENTINEL                                        # the last element of the last valid row
    with pytest.raises(AssertionError, match="never written"):
        RC.assert_all_written(g.get().reshape(33, 18), RK.SENTINEL, "rows")
    with pytest.raises(AssertionError, match="never written"):
        RC.assert_all_written(torch.from_numpy(g.get()), RK.SENTINEL, "rows")


@pytest.mark.parametrize("n", RC.RAGGED_N)
def test_float32_torch_is_inside_a_quarter_of_the_bar(n):
    """The float64 references (the chain of tests/test_fused_h2_gpu.py, dW = dZ^T A, db = colsum dZ) against the same
    evaluation in plain float32 torch, on minibatches of the distribution the GPU tests use: if float32 arithmetic sat near
    the bar at these row counts, a kernel missing it there would say nothing about the kernel."""
    worst = {}
    for seed in (13, 31):
        ref, batch = RC.batch_like_setup(n, seed)
        want = _fp64_chain(ref, *batch)
        got = RC.f32_chain(ref, *batch)
        errs = _errs(got, want)
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
        chain = {k: v.float() for k, v in want.items()}                     # the products on ONE chain, in both precisions
        for i, (eW, eb) in enumerate(RC.grad_errs(RC.f32_grad_blocks(batch[0], chain), batch[0], chain)):
            worst["dW%d" % (i + 1)] = max(worst.get("dW%d" % (i + 1), 0.0), eW)
            worst["db%d" % (i + 1)] = max(worst.get("db%d" % (i + 1), 0.0), eb)
    print("n=%d float32 torch against float64, of each tensor's largest value: %s"
          % (n, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) <= RC.BAR / 4, worst
