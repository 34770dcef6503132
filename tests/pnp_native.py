"""g++ build of caliscope_amd/csrc/pnp_math.h (tests/native/pnp_harness.cpp) and a `_pnp` hook for caliscope_amd.pose_network
that runs on it — the CPU side of the pose-bootstrap tests."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests.native_build import CSRC, NATIVE, load_native

D = C.POINTER(C.c_double)
I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)


def _p(a, t=D):
    return a.ctypes.data_as(t)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "pnp_harness.cpp", include=(CSRC,))
    lib.ph_pnp_view.restype = C.c_int
    lib.ph_pnp_view.argtypes = [D, D, C.c_int, C.c_int, C.c_int, D, D, D]
    lib.ph_pnp_batch.restype = None
    lib.ph_pnp_batch.argtypes = [C.c_int64, I64, I32, I32, D, D, D, C.c_int, C.c_int, D, D, D, I32]
    lib.ph_pair_rmse.restype = None
    lib.ph_pair_rmse.argtypes = [C.c_int64, D, I64, D, D, D, I64]
    return lib


def pnp_view(obj, uv, min_points=4, f32=False):
    """(status, R, t, rmse) of one view with normalised image points."""
    obj = np.ascontiguousarray(obj, dtype=np.float64).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    R, t, rmse = np.zeros(9), np.zeros(3), np.zeros(1)
    st = harness().ph_pnp_view(_p(obj), _p(uv), len(obj), min_points, 1 if f32 else 0, _p(R), _p(t), _p(rmse))
    return st, R.reshape(3, 3), t, float(rmse[0])


class HarnessPnP:
    """The `_pnp` hook of caliscope_amd.pose_network on the g++ build: same arguments and results as the device calls."""

    def pnp_batch(self, view_start, view_cam, cam_model, cam_intr, obs_xy, obs_obj, min_points, float32_io):
        n_views = len(view_start) - 1
        view_start = np.ascontiguousarray(view_start, dtype=np.int64)
        view_cam = np.ascontiguousarray(view_cam, dtype=np.int32)
        cam_model = np.ascontiguousarray(cam_model, dtype=np.int32)
        cam_intr = np.ascontiguousarray(cam_intr, dtype=np.float64)
        obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64)
        obs_obj = np.ascontiguousarray(obs_obj, dtype=np.float64)
        und = np.zeros_like(obs_xy)
        pose, rmse, status = np.zeros((n_views, 12)), np.zeros(n_views), np.zeros(n_views, dtype=np.int32)
        harness().ph_pnp_batch(n_views, _p(view_start, I64), _p(view_cam, I32), _p(cam_model, I32), _p(cam_intr), _p(obs_xy), _p(obs_obj),
                               int(min_points), 1 if float32_io else 0, _p(und), _p(pose), _p(rmse), _p(status, I32))
        return pose, rmse, status, und

    def pair_rmse(self, pair_pose, pair_start, obs_a, obs_b):
        n_pairs = len(pair_start) - 1
        pair_pose = np.ascontiguousarray(pair_pose, dtype=np.float64)
        pair_start = np.ascontiguousarray(pair_start, dtype=np.int64)
        obs_a = np.ascontiguousarray(obs_a, dtype=np.float64)
        obs_b = np.ascontiguousarray(obs_b, dtype=np.float64)
        rmse, count = np.zeros(n_pairs), np.zeros(n_pairs, dtype=np.int64)
        harness().ph_pair_rmse(n_pairs, _p(pair_pose), _p(pair_start, I64), _p(obs_a), _p(obs_b), _p(rmse), _p(count, I64))
        return rmse, count
