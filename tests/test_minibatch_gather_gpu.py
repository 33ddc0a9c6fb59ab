"""GPU (-m gpu): ppo_minibatch_gather against tests/minibatch_ref.py.  The operation is a copy, so every comparison is bitwise
(int32 views; the tolerance is zero): sources are random bits with NaN payloads, infinities and -0 planted."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import minibatch_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 0, 1), (3, 1, 2), (5, 0, 5), (64, 0, 64), (65, 0, 65), (65, 64, 1), (4097, 1000, 3097), (5120, 320, 320),
          (5120, 4800, 320), (655360, 614400, 40960)]
SEED, KEY = 0x9E3779B9, 3
SPECIAL = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], np.uint32)


@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    return _lib.load()


_sources = {}


def sources(R):
    """The five source arrays of R rows as int32 words (numpy), computed once per R and left unchanged, and their device copies."""
    if R not in _sources:
        rng = np.random.default_rng(R)
        words = [rng.integers(0, 2 ** 32, size=s, dtype=np.uint32) for s in ((R, 73), (R, 18), (R,), (R,), (R,))]
        for w in words:                                     # NaNs with payloads, +-inf, -0, denormals
            flat = w.reshape(-1)
            where = rng.integers(0, flat.size, size=max(8, flat.size // 16))
            flat[where] = SPECIAL[rng.integers(0, SPECIAL.size, size=where.size)]
        host = [w.view(np.float32) for w in words]
        _sources[R] = (host, [torch.from_numpy(h).to(DEV) for h in host])
    return _sources[R]


def p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def outputs(n, fill=0x5A):
    return [torch.full(s, fill, dtype=torch.uint8, device=DEV).view(torch.float32)
            for s in ((n, 73 * 4), (n, 18 * 4), (n * 4,), (n * 4,), (n * 4,))]


def gather(lib, src, R, first, n, seed=SEED, key=KEY, index=True, outs=None):
    outs = outs if outs is not None else outputs(n)
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV) if index else None
    rc = lib.ppo_minibatch_gather(*[p(s) for s in src], C.c_int64(R), C.c_uint32(seed), C.c_uint32(key), C.c_int64(first),
                                  C.c_int64(n), *[p(o) for o in outs], p(idx), None)
    torch.cuda.synchronize()
    return rc, outs, idx


def words(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("R,first,n", SHAPES)
def test_gather_is_the_reference_bit_for_bit(lib, R, first, n):
    host, dev = sources(R)
    want, want_idx = M.gather_ref(*host, SEED, KEY, first, n)
    rc, outs, idx = gather(lib, dev, R, first, n)
    assert rc == 0
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    for got, ref in zip(outs, want):
        assert np.array_equal(words(got).reshape(ref.shape), ref)
    rc, outs2, _ = gather(lib, dev, R, first, n, index=False)           # index_out = NULL: the same five outputs
    assert rc == 0
    for a, b in zip(outs, outs2):
        assert np.array_equal(words(a), words(b))


@pytest.mark.parametrize("R,first,n", [(65, 0, 65), (4097, 1000, 3097)])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_sources_with_4_byte_alignment_only(lib, R, first, n, offset):
    """Every source `offset` floats into a larger allocation (the observation rows behind a 3-row prefix besides): rollout views
    promise no more than 4-byte alignment."""
    host, _ = sources(R)
    dev = []
    for h in host:
        flat = torch.from_numpy(h).reshape(-1)
        pre = 3 * 73 + offset if h.ndim == 2 and h.shape[1] == 73 else offset
        buf = torch.zeros(flat.numel() + pre + 4, dtype=torch.float32, device=DEV)
        view = buf[pre:pre + flat.numel()]
        view.copy_(flat.to(DEV))
        assert view.data_ptr() % 16 == (4 * pre) % 16
        dev.append(view)
    want, want_idx = M.gather_ref(*host, SEED, KEY, first, n)
    rc, outs, idx = gather(lib, dev, R, first, n)
    assert rc == 0 and np.array_equal(idx.cpu().numpy(), want_idx)
    for got, ref in zip(outs, want):
        assert np.array_equal(words(got).reshape(ref.shape), ref)


def test_repeated_and_reordered_calls_give_the_same_bits(lib):
    """What the redo of refused optimizer steps relies on: a window's bits do not depend on what was gathered before it."""
    R, n = 5120, 320
    _, dev = sources(R)
    in_order = [[words(o) for o in gather(lib, dev, R, w * n, n, index=False)[1]] for w in range(16)]
    again = [words(o) for o in gather(lib, dev, R, 5 * n, n, index=False)[1]]
    assert all(np.array_equal(a, b) for a, b in zip(in_order[5], again))
    outs = outputs(n)                                       # one staging set, windows in reverse order
    for w in reversed(range(16)):
        rc, got, _ = gather(lib, dev, R, w * n, n, index=False, outs=outs)
        assert rc == 0
        assert all(np.array_equal(words(a), b) for a, b in zip(got, in_order[w])), w
    seen = np.concatenate([M.perm_index(R, SEED, KEY, np.arange(w * n, (w + 1) * n)) for w in range(16)])
    assert np.array_equal(np.sort(seen), np.arange(R))


def test_bad_arguments_are_refused_and_touch_nothing(lib):
    from fly_bproject_amd._lib import FlyHipError, check
    R, n = 65, 8
    _, dev = sources(R)
    outs = outputs(n)
    before = [words(o).copy() for o in outs]
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)

    def call(src=dev, R=R, first=0, n=n, out=outs):
        rc = lib.ppo_minibatch_gather(*[p(s) for s in src], C.c_int64(R), C.c_uint32(1), C.c_uint32(2), C.c_int64(first),
                                      C.c_int64(n), *[p(o) for o in out], p(idx), None)
        torch.cuda.synchronize()
        return rc

    bad = [dict(R=0), dict(R=-1), dict(R=2 ** 31), dict(n=0), dict(n=-3), dict(first=-1), dict(first=R - n + 1), dict(first=R),
           dict(n=R + 1)]
    for i in range(5):                                      # every required pointer, null
        bad.append(dict(src=[None if k == i else s for k, s in enumerate(dev)]))
        bad.append(dict(out=[None if k == i else o for k, o in enumerate(outs)]))
    for i in range(5):                                      # an output that is its own source
        bad.append(dict(out=[dev[i] if k == i else o for k, o in enumerate(outs)], n=1 if i else n))
    bad.append(dict(out=[outs[0].view(-1)[1:]] + outs[1:]))  # a staging tensor that is not 16-byte aligned
    for kw in bad:
        assert call(**kw) == -1, kw                         # FLY_E_ARG
    with pytest.raises(FlyHipError):
        check(call(n=0), "ppo_minibatch_gather")
    assert all(np.array_equal(words(o), b) for o, b in zip(outs, before))
    assert (idx == -1).all()
    assert call() == 0                                      # and the good call goes through
