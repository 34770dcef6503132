"""trf::termination (csrc/trf_math.h): scipy's check_termination as the native driver and the device both run it — the four outcomes and the
two boundaries of its strict comparisons, against scipy's own function."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize._lsq.common import check_termination

from tests.native_build import NATIVE, load_native

NONE = -100


@pytest.fixture(scope="module")
def th():
    lib = load_native(NATIVE / "termination_harness.cpp")
    lib.th_termination.restype = C.c_int
    lib.th_termination.argtypes = [C.c_double] * 7
    lib.th_reduction_ratio.restype = C.c_double
    lib.th_reduction_ratio.argtypes = [C.c_double] * 2
    lib.th_none.restype = C.c_int
    return lib


FTOL, XTOL = 1e-8, 1e-6
F, XN = 3.0, 5.0
DX_SMALL, DX_LARGE = 0.5 * XTOL * (XTOL + XN), 2.0 * XTOL * (XTOL + XN)
DF_SMALL, DF_LARGE = 0.5 * FTOL * F, 2.0 * FTOL * F


def test_none_is_the_drivers_code(th):
    assert th.th_none() == NONE


@pytest.mark.parametrize("dF, dx, ratio, expected", [
    (DF_SMALL, DX_SMALL, 0.9, 4),      # both
    (DF_SMALL, DX_LARGE, 0.9, 2),      # ftol
    (DF_LARGE, DX_SMALL, 0.9, 3),      # xtol
    (DF_LARGE, DX_LARGE, 0.9, NONE),   # neither
    (DF_SMALL, DX_LARGE, 0.1, NONE),   # a small reduction of a poor step is not convergence
    (DF_SMALL, DX_SMALL, 0.1, 3),
    (-1.0, DX_LARGE, 0.0, NONE),       # a rejected trial (ratio 0) never satisfies ftol ...
    (-1.0, DX_SMALL, 0.0, 3),          # ... but its step can be below xtol
])
def test_the_four_outcomes(th, dF, dx, ratio, expected):
    got = th.th_termination(dF, F, dx, XN, ratio, FTOL, XTOL)
    assert got == expected
    ref = check_termination(dF, F, dx, XN, ratio, FTOL, XTOL)
    assert got == (NONE if ref is None else ref)


def test_boundaries_are_strict(th):
    # ratio == 0.25 exactly: `ratio > 0.25` fails; the next double passes
    assert th.th_termination(DF_SMALL, F, DX_LARGE, XN, 0.25, FTOL, XTOL) == NONE
    assert th.th_termination(DF_SMALL, F, DX_LARGE, XN, np.nextafter(0.25, 1.0), FTOL, XTOL) == 2
    # dF == ftol * F exactly: `dF < ftol * F` fails; the double below passes
    edge = FTOL * F
    assert th.th_termination(edge, F, DX_LARGE, XN, 0.9, FTOL, XTOL) == NONE
    assert th.th_termination(np.nextafter(edge, 0.0), F, DX_LARGE, XN, 0.9, FTOL, XTOL) == 2
    # dx == xtol * (xtol + |x|) exactly
    edge_x = XTOL * (XTOL + XN)
    assert th.th_termination(DF_LARGE, F, edge_x, XN, 0.9, FTOL, XTOL) == NONE
    assert th.th_termination(DF_LARGE, F, np.nextafter(edge_x, 0.0), XN, 0.9, FTOL, XTOL) == 3
    for dF, dx, ratio in [(edge, DX_LARGE, 0.9), (DF_SMALL, DX_LARGE, 0.25), (DF_LARGE, edge_x, 0.9)]:
        assert check_termination(dF, F, dx, XN, ratio, FTOL, XTOL) is None


def test_nan_never_terminates(th):
    assert th.th_termination(np.nan, F, np.nan, XN, 0.9, FTOL, XTOL) == NONE
    assert th.th_termination(DF_SMALL, np.nan, DX_LARGE, XN, 0.9, FTOL, XTOL) == NONE


def test_reduction_ratio(th):
    assert th.th_reduction_ratio(1.0, 4.0) == 0.25
    assert th.th_reduction_ratio(0.0, 0.0) == 1.0
    assert th.th_reduction_ratio(1.0, 0.0) == 0.0
    assert th.th_reduction_ratio(1.0, -2.0) == 0.0
    assert th.th_reduction_ratio(-1.0, 2.0) == -0.5
