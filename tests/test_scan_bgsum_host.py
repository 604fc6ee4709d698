"""Host side of the quad scan's binary32 background sums (gs_common.h kBg32Range,
kBg32RefMax, bg32_sub_err, bg32_acc_err): the limits keep every value
inside the number formats, and the two error terms bound what they are derived for,
checked here in numpy's binary32 against exact rational arithmetic.  No device is
touched: the library's scan_bg32_model returns the constants and the terms as the
kernel computes them."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from gibbssampling_amd import _native

U = 2.0 ** -24


@pytest.fixture(scope="module")
def model():
    lib = _native.load_library()
    f = lib.scan_bg32_model
    f.argtypes = [C.c_int32, C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_double)]
    f.restype = None

    def call(W, lmax, lmin, R):
        out = (C.c_double * 4)()
        f(W, lmax, lmin, R, out)
        return tuple(out)

    return call


def test_limits_stay_inside_the_formats(model):
    rng_, ref, _, _ = model(12, -2.0, -2.0, 16)
    assert rng_ == 96.0 and ref == 900.0
    # a weight 2^d, |d| < range, and a lane sum of 64 + 3 of them are binary32 normals
    assert -126 < -rng_ and rng_ + np.log2(67) < 127
    # the scaled sum 2^r (sum), |r| < ref, is a binary64 normal
    assert ref + rng_ + np.log2(67) < 1023 and -(ref + rng_) > -1022
    # r is exact in binary32 and as an int
    assert np.float32(ref) == ref and ref < 2 ** 24


@pytest.mark.parametrize("W,lmax,lmin", [(4, -2.0, -2.0), (12, -1.9, -2.1), (16, -0.03, -7.1),
                                         (32, -0.5, -25.4), (12, 3.5, -4.0)])
def test_sub_err_is_the_formula_and_bounds_the_subtraction(model, W, lmax, lmin):
    _, _, sub, _ = model(W, lmax, lmin, 4)
    assert sub == (W * (lmax - lmin) + 1.0) * U
    # lg = a sum of W logs in [lmin, lmax] (binary32), r = rint(W lmax): fl(lg - r)
    rng = np.random.default_rng(W)
    lq = rng.uniform(lmin, lmax, (4096, W)).astype(np.float32)
    lq[0, :], lq[1, :] = np.float32(lmin), np.float32(lmax)
    lg = lq[:, 0].copy()
    for j in range(1, W):
        lg = (lg + lq[:, j]).astype(np.float32)
    r = np.rint(np.float32(W) * np.float32(lmax)).astype(np.float32)
    d = (lg - r).astype(np.float32)
    exact = lg.astype(np.float64) - float(r)  # (exact in binary64: 24-bit operands)
    assert np.all(np.abs(d.astype(np.float64) - exact) <= sub)
    assert np.all(np.abs(exact) <= W * (float(np.float32(lmax)) - float(np.float32(lmin))) + 1.0)


@pytest.mark.parametrize("R", [4, 8, 16, 64])
def test_acc_err_is_the_formula_and_bounds_a_binary32_sum(model, R):
    _, _, _, acc = model(12, -2.0, -2.0, R)
    assert acc == 1.02 * (R + 3) * U
    n = R + 4
    g = (n - 1) * U / (1.0 - (n - 1) * U)
    assert g * (1.0 + 0.012) <= acc  # e (1 + g) + g <= e + acc for e < 0.012
    rng = np.random.default_rng(R)
    for trial in range(200):
        # weights 2^d over the scan's range, a few of them dominant
        d = rng.uniform(-95.0, 1.0, n) if trial % 2 else rng.uniform(-3.0, 1.0, n)
        t = np.exp2(d).astype(np.float32)
        s = np.float32(0.0)
        for x in t:
            s = np.float32(s + x)
        exact = sum(Fraction(float(x)) for x in t)
        err = abs(Fraction(float(s)) - exact)
        assert err <= Fraction(acc) * exact and err <= Fraction(acc) * Fraction(float(s))
