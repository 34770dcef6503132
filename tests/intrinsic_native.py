"""g++ build of caliscope_amd/csrc/intrinsic_math.h (tests/native/intrinsic_harness.cpp) and a `_solver` hook for
caliscope_amd.calibrate_intrinsics that runs on it — the CPU side of the intrinsic-calibration tests."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests.native_build import CSRC, NATIVE, load_native

D = C.POINTER(C.c_double)
I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)


def _p(a, t=D):
    return None if a is None else a.ctypes.data_as(t)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "intrinsic_harness.cpp", include=(CSRC,))
    lib.ih_work_stride.restype = C.c_int
    lib.ih_start.restype = None
    lib.ih_start.argtypes = [C.c_int, C.c_double, C.c_double, D]
    lib.ih_point.restype = C.c_int
    lib.ih_point.argtypes = [C.c_int, D, D, D, D, D, D, D]
    lib.ih_intrinsics_batch.restype = None
    lib.ih_intrinsics_batch.argtypes = [C.c_int32, I32, D, D, C.c_int64, I64, I32, D, D, C.c_int, C.c_int, D, D, I32, I32, D, D, I32]
    return lib


def start_intrinsics(model, width, height):
    out = np.zeros(9)
    harness().ih_start(int(model), float(width), float(height), _p(out))
    return out


def point(model, intr, R, t, X, u):
    """(in_front, e[2], J[2, 6 + NI]) of one corner: pose columns (w, t) first, then the intrinsics."""
    ni = 8 if model else 9
    intr = np.ascontiguousarray(intr, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    t, X, u = (np.ascontiguousarray(a, dtype=np.float64) for a in (t, X, u))
    e, J = np.zeros(2), np.zeros((2, 6 + ni))
    front = harness().ih_point(int(model), _p(intr), _p(R), _p(t), _p(X), _p(u), _p(e), _p(J))
    return bool(front), e, J


class HarnessIntrinsics:
    """The `_solver` hook of caliscope_amd.calibrate_intrinsics on the g++ build: same arguments and results as DeviceIntrinsics."""

    def intrinsics_batch(self, cam_model, cam_size, cam_start, view_start, view_cam, obs_xy, obs_obj, float32_io=True, max_iter=0):
        cam_model = np.ascontiguousarray(cam_model, dtype=np.int32)
        cam_size = np.ascontiguousarray(cam_size, dtype=np.float64).reshape(-1, 2)
        cam_start = None if cam_start is None else np.ascontiguousarray(cam_start, dtype=np.float64).reshape(-1, 9)
        view_start = np.ascontiguousarray(view_start, dtype=np.int64)
        view_cam = np.ascontiguousarray(view_cam, dtype=np.int32)
        obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
        obs_obj = np.ascontiguousarray(obs_obj, dtype=np.float64).reshape(-1, 3)
        n_cams, n_views = len(cam_model), len(view_start) - 1
        intr, rmse = np.zeros((n_cams, 9)), np.zeros(n_cams)
        status, iters = np.zeros(n_cams, dtype=np.int32), np.zeros(n_cams, dtype=np.int32)
        pose, view_rmse, view_status = np.zeros((n_views, 12)), np.zeros(n_views), np.zeros(n_views, dtype=np.int32)
        harness().ih_intrinsics_batch(n_cams, _p(cam_model, I32), _p(cam_size), _p(cam_start), n_views, _p(view_start, I64), _p(view_cam, I32),
                                      _p(obs_xy), _p(obs_obj), 1 if float32_io else 0, int(max_iter), _p(intr), _p(rmse), _p(status, I32),
                                      _p(iters, I32), _p(pose), _p(view_rmse), _p(view_status, I32))
        return intr, rmse, status, iters, pose, view_rmse, view_status
