"""g++ build of caliscope_amd/csrc/time_offset_math.h (tests/native/time_offset_harness.cpp), the `_solver` hook that runs on it, the
bar of the comparison with tests/time_offset_oracle.py and the comparison itself, which the CPU and the GPU tests share.

The bar.  The yardstick is the disagreement of the oracle's float64 and longdouble runs on a scene: the sensitivity of the arithmetic
itself.  Offsets are measured in units of sqrt((S^-1)_cc) (sigma / sigma0, seconds per pixel of noise), positions in units of the
slot's own sqrt(diag H^-1) (metres per pixel of noise), the largest over the scene; compensated pixels in pixels.  The bar of the g++
build and of the device is 100 times the yardstick (a different summation order, contraction, the reciprocal square root).  It is
computed here from the two runs of the oracle, never from the code under test, and asserted to lie below 1e-8 so that an oracle gone
wrong does not widen it unseen.  Measured (printed by `bar`; the figures move by a third with the BLAS behind `lstsq`): EDGE offsets
3.4e-14, positions 2.6e-13 and pixels 3.0e-13 px; EXACT 3.0e-14, 2.1e-13 and 3.1e-13 px.  EDGE17, whose two runs of the oracle take a
quarter of a minute, is compared at EDGE's bar in units from `time_offset_oracle.units`.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.reconstruction import TrajDesc
from caliscope_amd.time_offsets import (FIELDS, TimeOffsetOptions, TimeOffsetOptionsStruct, TimeOffsetOut, options_struct, run_time_offset_call)
from tests import time_offset_oracle as TO
from tests import time_offset_scenes as TS
from tests.native_build import CSRC, NATIVE, load_native

FACTOR = 100.0


@functools.cache
def harness():
    lib = load_native(NATIVE / "time_offset_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.toh_last_error.restype = C.c_char_p
    lib.toh_estimate_time_offsets.restype = C.c_int
    lib.toh_estimate_time_offsets.argtypes = [C.POINTER(TrajDesc), C.POINTER(TimeOffsetOptionsStruct), C.POINTER(TimeOffsetOut)]
    return lib


class HarnessTimeOffsetSolver:
    """The `_solver` hook on the g++ build, with `estimate` as caliscope_amd.time_offsets.DeviceTimeOffsetSolver."""

    def __init__(self, memory_limit: int = 0):
        self.memory_limit = memory_limit
        self.calls = 0

    def estimate(self, grid, options):
        self.calls += 1
        lib = harness()
        return run_time_offset_call(lib.toh_estimate_time_offsets, grid, options, self.memory_limit, lambda: lib.toh_last_error().decode())


def run_scene(solver, sc, options: TimeOffsetOptions = TimeOffsetOptions()):
    return solver.estimate(sc.grid, options_struct(options, sc.grid))


@functools.cache
def oracles(name: str, huber_px=None):
    """(float64, longdouble) runs of the oracle on the scene `name`, computed once and not changed."""
    sc = getattr(TS, name)()
    return TO.estimate(sc.grid, np.float64, huber_px=huber_px), TO.estimate(sc.grid, np.longdouble, huber_px=huber_px)


def disagreement(got, ref, scale):
    """(offsets in sqrt((S^-1)_cc), positions in sqrt(diag H^-1), compensated pixels in px), the largest each; `scale`: the oracle run
    the units are taken from."""
    at = np.isfinite(np.asarray(ref.offsets, dtype=np.float64)) & (np.asarray(scale.unit_offset, dtype=np.float64) > 0)
    off = float(np.max(np.abs(np.asarray(got.offsets, dtype=np.longdouble)[at] - np.asarray(ref.offsets, dtype=np.longdouble)[at]) /
                       scale.unit_offset[at])) if at.any() else 0.0
    v = np.asarray(ref.valid) != 0
    pos = float(np.max(np.abs(np.asarray(got.xyz, dtype=np.longdouble)[v] - np.asarray(ref.xyz, dtype=np.longdouble)[v]) / scale.unit_xyz[v]))
    px = float(np.max(np.abs(np.asarray(got.row_xy, dtype=np.longdouble) - np.asarray(ref.row_xy, dtype=np.longdouble))))
    return off, pos, px


@functools.cache
def bar(name: str):
    """(offsets, positions, pixels): FACTOR times the disagreement of the oracle's two runs on the scene."""
    f64, ld = oracles(name)
    assert f64.rounds == ld.rounds and np.array_equal(f64.status, ld.status)
    off, pos, px = disagreement(f64, ld, ld)
    print(f"yardstick on {name} (oracle in float64 against longdouble, {f64.rounds} rounds): offsets {off:.3e} sqrt((S^-1)_cc), positions {pos:.3e} "
          f"sqrt(diag H^-1), compensated pixels {px:.3e} px")
    out = FACTOR * off, FACTOR * pos, FACTOR * px
    assert all(0.0 < b < 1e-8 for b in out), out
    return out


def same_pattern(what, got, ref):
    """Statuses, counts, flags and NaN patterns equal."""
    assert np.array_equal(got.status, ref.status), (what, got.status, ref.status)
    assert np.array_equal(got.rows, ref.rows) and np.array_equal(got.valid, ref.valid) and np.array_equal(got.row_used, ref.row_used), what
    assert got.rounds == ref.rounds and got.converged == ref.converged, (what, got.rounds, ref.rounds)
    for name in ("offsets", "sigma", "rms_before", "rms_after", "xyz", "frame_time"):
        assert np.array_equal(np.isnan(np.asarray(getattr(got, name), dtype=np.float64)), np.isnan(np.asarray(getattr(ref, name), dtype=np.float64))), (what, name)


def compare(what, name, got, ref, scale=None):
    """`got` against the oracle run `ref` (or against the g++ build) within the bar of the scene `name`; prints and returns the ratios
    to it.  `scale`: where the units come from when `ref` is not of that scene (default: the scene's longdouble run)."""
    same_pattern(what, got, ref)
    scale = oracles(name)[1] if scale is None else scale
    off, pos, px = disagreement(got, ref, scale)
    b_off, b_pos, b_px = bar(name)
    at = np.isfinite(np.asarray(ref.sigma, dtype=np.float64)) & (np.asarray(ref.sigma, dtype=np.float64) > 0)
    # (sigma / sigma0 = sqrt((S^-1)_cc): on a scene without noise sigma0 is what rounding left of the residuals, and is compared on its own)
    unit_got, unit_ref = np.asarray(got.sigma, dtype=np.float64)[at] / float(got.sigma0_px), np.asarray(ref.sigma, dtype=np.float64)[at] / float(ref.sigma0_px)
    sig = float(np.max(np.abs(unit_got / unit_ref - 1.0))) if at.any() else 0.0
    used = np.asarray(ref.rows) > 0
    rms = max(float(np.max(np.abs(np.asarray(getattr(got, n), dtype=np.float64)[used] - np.asarray(getattr(ref, n), dtype=np.float64)[used])))
              for n in ("rms_before", "rms_after"))
    s0 = abs(float(got.sigma0_px) - float(ref.sigma0_px))
    tau = float(np.nanmax(np.abs(np.asarray(got.frame_time, dtype=np.float64) - np.asarray(ref.frame_time, dtype=np.float64))))
    print(f"{what}: offsets {off:.3e} ({off / b_off:.3f} of the bar), positions {pos:.3e} ({pos / b_pos:.3f}), compensated pixels {px:.3e} px "
          f"({px / b_px:.3f}); sigma / sigma0 {sig:.3e} relative, rms {rms:.3e} px, sigma0 {s0:.3e} px, tau {tau:.3e} s")
    assert off <= b_off and pos <= b_pos and px <= b_px, what
    # sigma / sigma0 is a function of the iterate and of S alone; the RMS figures and sigma0 are sums of the same residuals: 1e-9 relative / 1e-9 px is far
    # above their rounding and far below any use of them.  tau is a mean of a few stamps, added in another order or in longdouble: a few ulp
    assert sig <= 1e-9 and rms <= 1e-9 and s0 <= 1e-9 and tau <= 4.0 * np.spacing(np.nanmax(np.asarray(ref.frame_time, dtype=np.float64))), what
    return off / b_off, pos / b_pos, px / b_px


__all__ = ["FACTOR", "FIELDS", "HarnessTimeOffsetSolver", "bar", "compare", "disagreement", "harness", "oracles", "run_scene", "same_pattern"]
