"""g++ build of caliscope_amd/csrc/vertical_math.h (tests/native/vertical_harness.cpp), a `_solver` hook for caliscope_amd.vertical
that runs on it, and the fixtures, tolerances and synthetic fields the vertical tests share.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd import vertical as V
from caliscope_amd.exceptions import BackendError
from tests.native_build import CSRC, NATIVE, ROOT, load_native

GOLDEN = ROOT / "tests" / "golden" / "vertical"
I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)
F64 = C.POINTER(C.c_double)

# Tolerances against the reference's recorded answers: angles absolute, uncertainties and costs relative, stop_step equal.
ANGLE_ATOL = 1e-12
REL_TOL = 1e-10


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "vertical_harness.cpp", include=(CSRC,))
    lib.vh_last_error.restype = C.c_char_p
    lib.vh_constants.restype = None
    lib.vh_constants.argtypes = [I32]
    lib.vh_n_chunks.restype = C.c_int64
    lib.vh_n_chunks.argtypes = [C.c_int64]
    lib.vh_gravity_vec.restype = None
    lib.vh_gravity_vec.argtypes = [C.c_double, C.c_double, F64]
    lib.vh_roll_pitch.restype = None
    lib.vh_roll_pitch.argtypes = [F64, F64]
    lib.vh_vertical_fit.restype = C.c_int
    lib.vh_vertical_fit.argtypes = [C.c_int32, C.c_int32, C.c_int64, I32, I32, F64, F64, I64] + [C.c_void_p] * 5 + [C.c_int32, F64, I32, I32]
    return lib


def constants() -> dict:
    out = np.zeros(6, dtype=np.int32)
    harness().vh_constants(out.ctypes.data_as(I32))
    return dict(zip(("chunk_pixels", "block", "wave", "n_sums", "max_side", "max_steps"), out.tolist()))


def n_chunks(n_pixels: int) -> int:
    return int(harness().vh_n_chunks(n_pixels))


def native_roll_pitch(vec) -> tuple[float, float]:
    vec, out = np.ascontiguousarray(vec, dtype=np.float64), np.zeros(2)
    harness().vh_roll_pitch(vec.ctypes.data_as(F64), out.ctypes.data_as(F64))
    return float(out[0]), float(out[1])


def native_gravity_vec(roll: float, pitch: float) -> np.ndarray:
    out = np.zeros(3)
    harness().vh_gravity_vec(roll, pitch, out.ctypes.data_as(F64))
    return out


class HarnessVerticalFit:
    """The `_solver` hook on the g++ build: same arguments, checks, result and error type as caliscope_amd.vertical.DeviceVerticalFit.
    `raw=True` skips the Python-side checks, so that the header's own validation answers."""

    def __init__(self, raw: bool = False):
        self.raw = raw
        self.calls = 0

    def vertical_fit(self, planes, height, width, focal_x, focal_y, offset, num_steps=V.DEFAULT_NUM_STEPS):
        if self.raw:
            dtype = np.float32 if all(np.asarray(p).dtype == np.float32 for p in planes) else np.float64
            planes = [np.ascontiguousarray(p, dtype=dtype).reshape(-1) for p in planes]
            height, width = np.ascontiguousarray(height, dtype=np.int32), np.ascontiguousarray(width, dtype=np.int32)
            focal_x, focal_y = np.ascontiguousarray(focal_x, dtype=np.float64), np.ascontiguousarray(focal_y, dtype=np.float64)
            offset = np.ascontiguousarray(offset, dtype=np.int64)
        else:
            planes, height, width, focal_x, focal_y, offset, num_steps = V.check_vertical_arguments(planes, height, width, focal_x, focal_y, offset, num_steps)
        self.calls += 1
        n = len(height)
        fits, stop, status = np.zeros((n, 8), dtype=np.float64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        rc = harness().vh_vertical_fit(n, num_steps, len(planes[0]), height.ctypes.data_as(I32), width.ctypes.data_as(I32), focal_x.ctypes.data_as(F64),
                                       focal_y.ctypes.data_as(F64), offset.ctypes.data_as(I64), *(p.ctypes.data for p in planes),
                                       int(planes[0].dtype == np.float32), fits.ctypes.data_as(F64), stop.ctypes.data_as(I32), status.ctypes.data_as(I32))
        if rc:
            raise BackendError(f"cba_vertical_fit failed (code {rc}): {harness().vh_last_error().decode()}")
        return fits, stop, status


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

FIT_FIELDS = ("roll_rad", "pitch_rad", "roll_uncertainty_rad", "pitch_uncertainty_rad", "gravity_uncertainty_rad", "initial_cost", "final_cost")


VARIANTS = ("random", "ones")  # the confidences a case was answered with: the stored uniform-random ones, or all ones


def fixture_names() -> list[str]:
    return sorted(p.stem for p in GOLDEN.glob("fit_*.npz") if "__" not in p.stem)


_CACHE: dict = {}


def load(name: str) -> dict:
    """A fixture with the planes of its side files (NAME__PLANE.npz) merged in, read once per process and shared (callers must
    not modify the arrays)."""
    if name not in _CACHE:
        data = {}
        for path in [GOLDEN / f"{name}.npz"] + sorted(GOLDEN.glob(f"{name}__*.npz")):
            with np.load(path) as z:
                data.update({k: z[k] for k in z.files})
        if "up_field" not in data and "up_field_0" in data:
            data["up_field"] = np.stack([data.pop("up_field_0"), data.pop("up_field_1")])
        _CACHE[name] = data
    return _CACHE[name]


def field_set(fx: dict, variant: str = "random") -> tuple:
    uc, lc = fx["up_confidence"], fx["latitude_confidence"]
    if variant == "ones":
        uc, lc = np.ones_like(uc), np.ones_like(lc)
    return fx["up_field"], uc, fx["latitude_field"], lc, float(fx["focal"][0]), float(fx["focal"][1])


def differences(fit: V.GravityFit, expected, stop_step: int) -> dict:
    """Angle differences (absolute), uncertainty / cost differences (relative) and whether stop_step agrees, against the reference's
    seven numbers `expected`."""
    got = np.array([getattr(fit, f) for f in FIT_FIELDS])
    expected = np.asarray(expected, dtype=np.float64)
    return {"angle": float(np.abs(got[:2] - expected[:2]).max()),
            "rel": float((np.abs(got[2:] - expected[2:]) / np.abs(expected[2:])).max()),
            "stop_equal": fit.stop_step == int(stop_step)}


def assert_matches(fit: V.GravityFit, expected, stop_step: int, label="") -> dict:
    d = differences(fit, expected, stop_step)
    print(f"{label}: angle {d['angle']:.3e} rad, relative {d['rel']:.3e}, stop_step {fit.stop_step} (expected {int(stop_step)})")
    assert d["stop_equal"], (label, fit.stop_step, int(stop_step))
    assert d["angle"] <= ANGLE_ATOL, (label, d)
    assert d["rel"] <= REL_TOL, (label, d)
    return d


# ---- synthetic fields -------------------------------------------------------------------------------------------------------------

def analytic_fields(roll: float, pitch: float, focal_x: float, focal_y: float, height: int, width: int, dtype=np.float64):
    """Exact up and latitude fields of a pinhole camera at (roll, pitch) with the principal point at (w / 2, h / 2), confidences one:
    the up vector of a pixel is the image-plane projection of world up, the latitude the arcsine of ray . up."""
    vec = V.gravity_vec_from_roll_pitch(roll, pitch)
    xs, ys = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    u, v = (xs - width / 2) / focal_x, (ys - height / 2) / focal_y
    up = np.stack([vec[0] - vec[2] * u, vec[1] - vec[2] * v])
    up = up / np.linalg.norm(up, axis=0, keepdims=True)
    rays = np.stack([u, v, np.ones_like(u)])
    rays = rays / np.linalg.norm(rays, axis=0, keepdims=True)
    lat = np.arcsin(np.clip(np.tensordot(vec, rays, axes=1), -1 + 1e-6, 1 - 1e-6))
    ones = np.ones((height, width), dtype=dtype)
    return up.astype(dtype), ones, lat[None].astype(dtype), ones


def noisy_fields(roll, pitch, focal_x, focal_y, height, width, seed, uniform_confidence=False):
    """float32 fields with rotated up vectors, latitude noise and 5 % latitude outliers; random or all-ones confidences."""
    rng = np.random.default_rng(seed)
    up, _, lat, _ = analytic_fields(roll, pitch, focal_x, focal_y, height, width)
    ang = rng.normal(0.0, 0.02, (height, width))
    up = np.stack([np.cos(ang) * up[0] - np.sin(ang) * up[1], np.sin(ang) * up[0] + np.cos(ang) * up[1]])
    lat = lat + rng.normal(0.0, 0.02, lat.shape)
    lat = lat + np.where(rng.random(lat.shape) < 0.05, rng.normal(0.0, 0.5, lat.shape), 0.0)
    if uniform_confidence:
        uc, lc = np.ones((height, width)), np.ones((height, width))
    else:
        uc, lc = rng.random((height, width)), rng.random((height, width))
    return tuple(a.astype(np.float32) for a in (up, uc, lat, lc)) + (float(focal_x), float(focal_y))


def chunk_edge_shapes() -> list[tuple[int, int]]:
    """(h, w) with chunk - 1, chunk and chunk + 1 pixels: the nearest-to-square factorisations with both sides >= 2."""
    chunk, shapes = constants()["chunk_pixels"], []
    for n in (chunk - 1, chunk, chunk + 1):
        h = max(d for d in range(2, int(n**0.5) + 1) if n % d == 0)
        shapes.append((h, n // h))
    return shapes
