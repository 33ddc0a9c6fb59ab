"""GPU (-m gpu): ppo_noise_ar1 against tests/noise_ar1_ref.py.  Every op of the definition is a separately rounded fp32 op, so
every comparison is bitwise (int32 views; the tolerance is zero)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import noise_ar1_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (T, C): one word; one env; C % 4 == 2; a ragged last block of steps; N = 33; a wave with a ragged tail of lanes whether a lane
# takes 1, 2 or 4 columns; more than one workgroup; and T with no, one, an even and an odd count of whole blocks of steps at block
# depths 8 and 16 (the kernel drains two register buffers in turn), with and without a ragged end
SHAPES = [(1, 1), (1, 18), (2, 54), (9, 54), (80, 72), (17, 594), (130, 4 * 64 * 3 + 4), (80, 18 * 256), (27, 54), (43, 72)]
RHOS = [0.5, 0.999]
GUARD = 8                   # floats of guard fill before and after each buffer
FILL = -7.25                # the guards' value: not a value the filter produces from them


@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    return _lib.load()


_inputs = {}


def inputs(T, C_):
    """The white draw x [T, C] and the carry [C] of a shape (numpy float32), made once per shape and left unchanged."""
    if (T, C_) not in _inputs:
        rng = np.random.default_rng(1000 * T + C_)
        _inputs[(T, C_)] = (rng.standard_normal((T, C_), dtype=np.float32), rng.standard_normal(C_, dtype=np.float32))
    return _inputs[(T, C_)]


_refs = {}


def reference(T, C_, rho):
    if (T, C_, rho) not in _refs:
        _refs[(T, C_, rho)] = A.ar1(*inputs(T, C_), rho)
    return _refs[(T, C_, rho)]


def guarded(host, offset):
    """`host` on the device inside a guard-filled allocation, `offset` floats past a 16-byte boundary: (allocation, view)."""
    flat = torch.from_numpy(np.ascontiguousarray(host)).reshape(-1)
    pad = GUARD + (-GUARD) % 4 + offset                      # the allocation is 16-byte aligned (asserted below)
    buf = torch.full((pad + flat.numel() + GUARD,), FILL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[pad:pad + flat.numel()]
    view.copy_(flat.to(DEV))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    hi = lo + view.numel()
    return bool((buf[:lo] == FILL).all()) and bool((buf[hi:] == FILL).all()) and buf.numel() - hi == GUARD and lo >= GUARD


def call(lib, eps, carry, T, C_, rho):
    rc = lib.ppo_noise_ar1(C.c_void_p(eps.data_ptr()) if eps is not None else None,
                           C.c_void_p(carry.data_ptr()) if carry is not None else None, C.c_int64(T), C.c_int64(C_),
                           C.c_float(rho), None)
    torch.cuda.synchronize()
    return rc


def words(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("T,C_", SHAPES)
def test_filter_is_the_reference_bit_for_bit(lib, T, C_, offset, rho):
    """From a 16-byte-aligned base and from one a float past it (eps and carry both), with the words around both untouched."""
    x, c0 = inputs(T, C_)
    want_y, want_c = reference(T, C_, rho)
    eb, eps = guarded(x, offset)
    cb, carry = guarded(c0, offset)
    assert call(lib, eps, carry, T, C_, rho) == 0
    assert np.array_equal(words(eps).reshape(T, C_), bits(want_y))
    assert np.array_equal(words(carry), bits(want_c))
    assert np.array_equal(words(carry), words(eps).reshape(T, C_)[-1])
    assert guards_intact(eb, eps) and guards_intact(cb, carry)


@pytest.mark.parametrize("eps_off,carry_off", [(0, 2), (2, 0), (2, 2), (0, 1), (3, 0)])
def test_mixed_alignments_of_the_two_bases(lib, eps_off, carry_off):
    """The lane width follows the less aligned of the two bases (8-byte and 4-byte cases)."""
    T, C_ = 80, 72
    x, c0 = inputs(T, C_)
    want_y, want_c = reference(T, C_, 0.5)
    eb, eps = guarded(x, eps_off)
    cb, carry = guarded(c0, carry_off)
    assert call(lib, eps, carry, T, C_, 0.5) == 0
    assert np.array_equal(words(eps).reshape(T, C_), bits(want_y)) and np.array_equal(words(carry), bits(want_c))
    assert guards_intact(eb, eps) and guards_intact(cb, carry)


@pytest.mark.parametrize("offset", [0, 1])
def test_special_values_stay_in_their_columns(lib, offset):
    """A NaN, +inf, -inf and -0 planted in single columns (in the draw and in the carry): every other column is bitwise the
    reference, the planted columns go non-finite where the reference does (and bitwise equal where they are finite: a NaN's
    payload is not part of the definition), and no other column does."""
    T, C_ = 17, 594
    x, c0 = (a.copy() for a in inputs(T, C_))
    x[3, 5], x[0, 100], x[9, 101], x[4, 333], c0[7], c0[590] = np.nan, np.inf, -np.inf, -0.0, np.nan, np.inf
    x[10, 590] = -np.inf                                    # +inf carried into -inf: NaN from there on
    x[:, 12], c0[12] = -0.0, -0.0                           # a column of -0 stays -0, sign included
    planted = [5, 100, 101, 333, 7, 590, 12]
    clean = np.setdiff1d(np.arange(C_), planted)
    want_y, want_c = A.ar1(x, c0, 0.5)
    eb, eps = guarded(x, offset)
    cb, carry = guarded(c0, offset)
    assert call(lib, eps, carry, T, C_, 0.5) == 0
    got_y, got_c = eps.cpu().numpy().reshape(T, C_), carry.cpu().numpy()
    assert np.array_equal(bits(got_y[:, clean]), bits(want_y[:, clean])) and np.array_equal(bits(got_c[clean]), bits(want_c[clean]))
    assert np.isfinite(got_y[:, clean]).all()
    for got, want in ((got_y, want_y), (got_c, want_c)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got)[ok], bits(want)[ok])
    assert np.isnan(got_y[3:, 5]).all() and np.isnan(got_y[:, 7]).all() and np.isnan(got_y[10:, 590]).all()
    assert (got_y[:, 100] == np.inf).all() and (got_y[9:, 101] == -np.inf).all()
    assert np.array_equal(bits(got_y[:, 12]), np.full(T, -2 ** 31, np.int32))
    assert guards_intact(eb, eps) and guards_intact(cb, carry)


@pytest.mark.parametrize("T,C_,cut", [(80, 72, 40), (130, 4 * 64 * 3 + 4, 65), (9, 54, 1)])
def test_two_launches_over_the_halves_are_one_launch_over_the_whole(lib, T, C_, cut):
    x, c0 = inputs(T, C_)
    want_y, want_c = reference(T, C_, 0.999)
    _, one = guarded(x, 0)
    _, one_c = guarded(c0, 0)
    assert call(lib, one, one_c, T, C_, 0.999) == 0
    _, two = guarded(x, 0)
    _, two_c = guarded(c0, 0)
    assert call(lib, two, two_c, cut, C_, 0.999) == 0
    assert np.array_equal(words(two_c), bits(want_y[cut - 1]))
    assert call(lib, two[cut * C_:], two_c, T - cut, C_, 0.999) == 0
    assert np.array_equal(words(one), words(two)) and np.array_equal(words(one_c), words(two_c))
    assert np.array_equal(words(two).reshape(T, C_), bits(want_y)) and np.array_equal(words(two_c), bits(want_c))


def test_the_same_inputs_give_the_same_bits(lib):
    T, C_ = 80, 18 * 256
    x, c0 = inputs(T, C_)
    runs = []
    for _ in range(2):
        _, eps = guarded(x, 0)
        _, carry = guarded(c0, 0)
        assert call(lib, eps, carry, T, C_, 0.5) == 0
        runs.append((words(eps), words(carry)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_bad_arguments_are_refused_and_touch_nothing(lib):
    from fly_bproject_amd._lib import FlyHipError, check
    T, C_ = 9, 54
    x, c0 = inputs(T, C_)
    eb, eps = guarded(x, 0)
    cb, carry = guarded(c0, 0)
    bad = [dict(eps=None), dict(carry=None), dict(T=0), dict(T=-1), dict(C_=0), dict(C_=-18), dict(rho=0.0), dict(rho=1.0),
           dict(rho=float("nan")), dict(rho=-0.5), dict(rho=1.5), dict(rho=float("inf"))]
    for kw in bad:
        a = dict(eps=eps, carry=carry, T=T, C_=C_, rho=0.5)
        a.update(kw)
        assert call(lib, **a) == -1, kw                     # FLY_E_ARG
    with pytest.raises(FlyHipError, match="rho"):
        check(call(lib, eps, carry, T, C_, 1.0), "ppo_noise_ar1")
    assert np.array_equal(words(eps).reshape(T, C_), bits(x)) and np.array_equal(words(carry), bits(c0))
    assert guards_intact(eb, eps) and guards_intact(cb, carry)
    assert call(lib, eps, carry, T, C_, 0.5) == 0           # and the good call goes through
    assert np.array_equal(words(eps).reshape(T, C_), bits(reference(T, C_, 0.5)[0]))
