"""The kernel divides by R = 30000 and by the QP constant n'P^-1 n = 90.00000000000153 as q = x*inv; r = fma(-q, d, x);
fma(r, inv, q) (csrc/mg_env.h div_const). Check on the host that this is the correctly
rounded quotient x / d, as the reference's Python division is."""

import ctypes

import numpy as np
import pytest

import merge_oracle as mo

libm = ctypes.CDLL("libm.so.6")
libm.fma.restype = ctypes.c_double
libm.fma.argtypes = [ctypes.c_double] * 3


@pytest.mark.parametrize("d,lo,hi", [(3.0, -45.0, 45.0), (30000.0, -5e3, 2e5),
                                     (90.00000000000153, -45.0, 45.0)])
def test_fma_corrected_division_is_correctly_rounded(d, lo, hi):
    rng = np.random.default_rng(int(d))
    xs = np.concatenate([rng.uniform(lo, hi, 60000),
                         rng.uniform(-1, 1, 20000) * 2.0 ** rng.integers(-30, 30, 20000)])
    inv = 1.0 / d
    bad = 0
    for x in xs.tolist():
        q = x * inv
        r = libm.fma(-q, d, x)
        bad += libm.fma(r, inv, q) != x / d
    assert bad == 0


# The divisors away from the default mg_params (tests/params_cases.py): R of cases A-D, and the QP
# constant z'n of the horizons 2.0, 0.7 and 5.0 (mg_params.qp_nz, computed as merge_oracle.qpgen2_factor
# does). Numerators over the ranges those divisions see: positions from -5e3 to 2e5 (a car that drives
# on after arriving), speed differences up to +-250 (action speeds to 200 and beyond).
PARAM_DIVISORS = [(20000.0, -5e3, 2e5), (300.0, -5e3, 2e5), (9000.0, -5e3, 2e5), (17000.0, -5e3, 2e5)] + [
    (mo.qpgen2_factor(t)[2], -250.0, 250.0) for t in (2.0, 0.7, 5.0)]


@pytest.mark.parametrize("d,lo,hi", PARAM_DIVISORS)
def test_fma_corrected_division_is_correctly_rounded_at_params(d, lo, hi):
    rng = np.random.default_rng(int(d * 1000) % 2 ** 31)
    xs = np.concatenate([rng.uniform(lo, hi, 60000),
                         rng.uniform(-1, 1, 20000) * 2.0 ** rng.integers(-30, 30, 20000)])
    inv = 1.0 / d
    bad = 0
    for x in xs.tolist():
        q = x * inv
        r = libm.fma(-q, d, x)
        bad += libm.fma(r, inv, q) != x / d
    assert bad == 0, (d, bad)
