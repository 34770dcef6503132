"""g++ build of caliscope_amd/csrc/frame_select_math.h (tests/native/frame_select_harness.cpp) and a `_solver` hook for
caliscope_amd.frame_selector that runs on it — the CPU side of the frame-selection tests."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.frame_selector import FrameSelection, check_selection_arguments
from tests.native_build import CSRC, NATIVE, load_native

D = C.POINTER(C.c_double)
I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)
U64 = C.POINTER(C.c_uint64)


def _p(a, t=D):
    return None if a is None else a.ctypes.data_as(t)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "frame_select_harness.cpp", include=(CSRC,))
    lib.fh_homography.restype = C.c_int
    lib.fh_homography.argtypes = [D, D, C.c_int, C.c_int, D, D, D]
    lib.fh_select_frames.restype = None
    lib.fh_select_frames.argtypes = [C.c_int32, I64, D, C.c_int64, I64, I64, I32, D, D, C.c_int, C.c_int, C.c_int, C.c_int, U64, D, D, I32, D,
                                     I32, I32, I32, I32, I32]
    return lib


def homography(obj_xy, img_xy, float32_io=True):
    """(status, H[3, 3] with h33 = 1, orientation[3], transfer rmse in pixels) of one frame."""
    obj_xy = np.ascontiguousarray(obj_xy, dtype=np.float64).reshape(-1, 2)
    img_xy = np.ascontiguousarray(img_xy, dtype=np.float64).reshape(-1, 2)
    H, o, r = np.zeros(9), np.zeros(3), np.zeros(1)
    st = harness().fh_homography(_p(obj_xy), _p(img_xy), len(obj_xy), 1 if float32_io else 0, _p(H), _p(o), _p(r))
    return int(st), H.reshape(3, 3), o, float(r[0])


class HarnessFrameSelection:
    """The `_solver` hook of caliscope_amd.frame_selector on the g++ build: same arguments, checks and results as DeviceFrameSelection."""

    def select_frames(self, cam_frame_start, cam_size, frame_start, obs_xy, obs_obj, homog_start=None, homog_count=None, *, grid_size=5,
                      min_corners=6, target_count=30, float32_io=True):
        a = check_selection_arguments(cam_frame_start, cam_size, frame_start, obs_xy, obs_obj, homog_start, homog_count, grid_size, min_corners,
                                      target_count)
        out = FrameSelection.empty(a.n_cams, a.n_frames, a.target_count)
        if a.n_cams and a.n_frames:
            harness().fh_select_frames(a.n_cams, _p(a.cam_frame_start, I64), _p(a.cam_size), a.n_frames, _p(a.frame_start, I64), _p(a.homog_start, I64),
                                       _p(a.homog_count, I32), _p(a.obs_xy), _p(a.obs_obj), a.grid_size, a.min_corners, a.target_count,
                                       1 if float32_io else 0, _p(out.cell_mask, U64), _p(out.pose_features), _p(out.orientation),
                                       _p(out.homography_status, I32), _p(out.homography_rmse), _p(out.selected, I32), _p(out.n_selected, I32),
                                       _p(out.n_anchors, I32), _p(out.bin_mask, I32), _p(out.eligible, I32))
        return out
