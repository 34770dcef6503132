"""Reprojection statistics and the outlier filter between the solver passes in one device call.

``CaptureVolume.compute_reprojection_report`` takes the pixel errors from the device and does every group-by on the host, and
``filter_by_percentile_error`` sorts the observations by camera and calls ``np.percentile`` per camera.  Here one call,
``cba_reprojection_filter`` (``include/caliscope_report.h``, ``csrc/report_math.h``, ``csrc/report_lib.hip``), projects every
observation, sums the squared errors per camera and per (object, keypoint) group, finds the percentile thresholds with a radix
select over the bit patterns of the errors (exact: no sort, integer atomics only), and returns the keep mask with the safety floor
applied.  :meth:`CaptureVolume.reprojection_summary` and :meth:`CaptureVolume.filter_outliers` are built on it; the existing
report and filters stay as they are and are what the new path is tested against.

There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.  ``_solver`` of the two methods replaces
the device call (an object with ``reprojection_filter``, as :class:`DeviceReprojectionStats`) — the CPU test-suite passes a g++
build of the same select, mask and floor logic.

Counts, thresholds, the keep mask and the kept counts are exact and the same from run to run; the floating sums are added in the
order of arrival and vary in their last bits.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import pandas as pd

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError

MODES = {"stats": 0, "percentile": 1, "absolute": 2}
SCOPES = {"per_camera": 0, "overall": 1}


class ReportDesc(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_points", C.c_int64), ("n_obs", C.c_int64), ("n_groups", C.c_int32),
                ("cam_model", _lib.c_int32_p), ("cam_const", _lib.c_double_p), ("cam_pose", _lib.c_double_p), ("points", _lib.c_double_p),
                ("obs_cam", _lib.c_int32_p), ("obs_pt", _lib.c_int32_p), ("obs_uv", _lib.c_double_p), ("obs_group", _lib.c_int32_p),
                ("err_in", _lib.c_double_p), ("mode", C.c_int32), ("scope", C.c_int32), ("value", C.c_double), ("min_per_camera", C.c_int64)]


class ReportOut(C.Structure):
    _fields_ = [("err_xy", _lib.c_double_p), ("err", _lib.c_double_p), ("cam_sumsq", _lib.c_double_p), ("cam_count", _lib.c_int64_p),
                ("group_sumsq", _lib.c_double_p), ("group_count", _lib.c_int64_p), ("overall_sumsq", _lib.c_double_p),
                ("n_nonfinite", _lib.c_int64_p), ("cam_threshold", _lib.c_double_p), ("keep", _lib.c_uint8_p), ("cam_kept", _lib.c_int64_p),
                ("n_floor_cams", _lib.c_int64_p)]


REPORT_SIGNATURES = {
    "cba_reprojection_filter": (C.c_int, [C.POINTER(ReportDesc), C.c_int32, C.POINTER(ReportOut)]),
}


@dataclass(frozen=True)
class ReprojectionFilterResult:
    """What one ``reprojection_filter`` call returns.  ``err_xy`` is None when the errors were given (``err_in``) or not asked for;
    the filter fields are None for ``mode="stats"`` and when ``n_nonfinite`` is not zero (the library does not filter then)."""

    err_xy: np.ndarray | None
    err: np.ndarray | None
    cam_sumsq: np.ndarray
    cam_count: np.ndarray
    group_sumsq: np.ndarray
    group_count: np.ndarray
    overall_sumsq: float
    n_nonfinite: int
    cam_threshold: np.ndarray | None = None
    keep: np.ndarray | None = None
    cam_kept: np.ndarray | None = None
    n_floor_cams: int | None = None


def check_reprojection_arguments(cam_model, cam_const, cam_pose, points, obs_cam, obs_pt, obs_uv, obs_group, n_groups, err_in, mode, scope,
                                 value, min_per_camera):
    """The arguments of a ``reprojection_filter`` call in the layout of ``cba_report_desc``, as a dict (``ValueError`` for an unknown
    mode or scope, arrays of the wrong shape or mismatched lengths; the range of every index and the values of ``err_in`` are the
    library's check)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if scope not in SCOPES:
        raise ValueError(f"scope must be 'per_camera' or 'overall', got {scope}")
    cam_model = np.ascontiguousarray(cam_model, dtype=np.int32).reshape(-1)
    n_cams = len(cam_model)
    cam_const = np.ascontiguousarray(cam_const, dtype=np.float64).reshape(-1, 12)
    cam_pose = np.ascontiguousarray(cam_pose, dtype=np.float64).reshape(-1, 6)
    if len(cam_const) != n_cams or len(cam_pose) != n_cams:
        raise ValueError("reprojection_filter: cam_model, cam_const and cam_pose differ in length")
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    n_obs = len(obs_cam)
    if err_in is None:
        obs_pt = np.ascontiguousarray(obs_pt, dtype=np.int32).reshape(-1)
        obs_uv = np.ascontiguousarray(obs_uv, dtype=np.float64).reshape(-1, 2)
        if len(obs_pt) != n_obs or len(obs_uv) != n_obs:
            raise ValueError("reprojection_filter: obs_cam, obs_pt and obs_uv differ in length")
    else:
        err_in = np.ascontiguousarray(err_in, dtype=np.float64).reshape(-1)
        obs_pt = obs_uv = None
        if len(err_in) != n_obs:
            raise ValueError("reprojection_filter: obs_cam and err_in differ in length")
    if obs_group is not None:
        obs_group = np.ascontiguousarray(obs_group, dtype=np.int32).reshape(-1)
        if len(obs_group) != n_obs:
            raise ValueError("reprojection_filter: obs_cam and obs_group differ in length")
        if int(n_groups) < 0:
            raise ValueError("reprojection_filter: n_groups must not be negative")
    return dict(cam_model=cam_model, cam_const=cam_const, cam_pose=cam_pose, points=points, obs_cam=obs_cam, obs_pt=obs_pt, obs_uv=obs_uv,
                obs_group=obs_group, n_groups=int(n_groups) if obs_group is not None else 0, err_in=err_in, mode=MODES[mode], scope=SCOPES[scope],
                value=float(value), min_per_camera=int(min_per_camera))


def run_reprojection_call(call, args: dict, want_errors: bool, what: str, last_error) -> ReprojectionFilterResult:
    """Fill ``cba_report_desc`` / ``cba_report_out`` from checked arguments, run ``call(desc_ref, out_ref) -> code`` and collect the
    result (shared by the device binding and the test harness: same structures, same error type and message)."""
    n_cams, n_obs, n_groups = len(args["cam_model"]), len(args["obs_cam"]), args["n_groups"]
    project, filtering = args["err_in"] is None, args["mode"] != MODES["stats"]
    err_xy = np.zeros((n_obs, 2)) if want_errors and project else None
    err = np.zeros(n_obs) if want_errors else None
    cam_sumsq, cam_count = np.zeros(n_cams), np.zeros(n_cams, dtype=np.int64)
    group_sumsq, group_count = np.zeros(n_groups), np.zeros(n_groups, dtype=np.int64)
    overall, n_bad, n_floor = np.zeros(1), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    threshold = np.zeros(n_cams) if filtering else None
    keep = np.zeros(n_obs, dtype=np.uint8) if filtering else None
    kept = np.zeros(n_cams, dtype=np.int64) if filtering else None
    desc = ReportDesc(n_cams=n_cams, n_points=len(args["points"]), n_obs=n_obs, n_groups=n_groups, cam_model=_lib.ptr(args["cam_model"]),
                      cam_const=_lib.ptr(args["cam_const"]), cam_pose=_lib.ptr(args["cam_pose"]), points=_lib.ptr(args["points"]),
                      obs_cam=_lib.ptr(args["obs_cam"]), obs_pt=_lib.ptr(args["obs_pt"]), obs_uv=_lib.ptr(args["obs_uv"]),
                      obs_group=_lib.ptr(args["obs_group"]), err_in=_lib.ptr(args["err_in"]), mode=args["mode"], scope=args["scope"],
                      value=args["value"], min_per_camera=args["min_per_camera"])
    out = ReportOut(err_xy=_lib.ptr(err_xy), err=_lib.ptr(err), cam_sumsq=_lib.ptr(cam_sumsq), cam_count=_lib.ptr(cam_count),
                    group_sumsq=_lib.ptr(group_sumsq), group_count=_lib.ptr(group_count), overall_sumsq=_lib.ptr(overall),
                    n_nonfinite=_lib.ptr(n_bad), cam_threshold=_lib.ptr(threshold), keep=_lib.ptr(keep),
                    cam_kept=_lib.ptr(kept), n_floor_cams=_lib.ptr(n_floor))
    rc = call(C.byref(desc), C.byref(out))
    if rc != 0:
        raise BackendError(f"{what} failed (code {rc}): {last_error()}")
    filtered = filtering and int(n_bad[0]) == 0
    return ReprojectionFilterResult(err_xy=err_xy, err=err, cam_sumsq=cam_sumsq, cam_count=cam_count, group_sumsq=group_sumsq, group_count=group_count,
                                    overall_sumsq=float(overall[0]), n_nonfinite=int(n_bad[0]), cam_threshold=threshold if filtered else None,
                                    keep=keep.astype(bool) if filtered else None, cam_kept=kept if filtered else None,
                                    n_floor_cams=int(n_floor[0]) if filtered else None)


class DeviceReprojectionStats:
    """The device call ``cba_reprojection_filter`` on ``device_id``.  ``err_in`` set on the object replaces the argument (the public
    methods never pass one): Euclidean errors that are given, so that projection is skipped."""

    def __init__(self, device_id: int = 0, err_in=None):
        self.device_id = device_id
        self.err_in = err_in

    def reprojection_filter(self, cam_model, cam_const, cam_pose, points, obs_cam, obs_pt, obs_uv, *, obs_group=None, n_groups=0, err_in=None,
                            mode="stats", scope="per_camera", value=0.0, min_per_camera=10, want_errors=True) -> ReprojectionFilterResult:
        """Errors, sums and, for ``mode`` "percentile" (``value``: percent to remove) or "absolute" (``value``: largest pixel error
        kept), the keep mask of one call; see ``include/caliscope_report.h``."""
        args = check_reprojection_arguments(cam_model, cam_const, cam_pose, points, obs_cam, obs_pt, obs_uv, obs_group, n_groups,
                                            self.err_in if self.err_in is not None else err_in, mode, scope, value, min_per_camera)
        lib = _lib.bind(_lib.load(), REPORT_SIGNATURES)
        return run_reprojection_call(lambda d, o: lib.cba_reprojection_filter(d, self.device_id, o), args, want_errors, "cba_reprojection_filter",
                                     lambda: _lib.last_error(lib))


@dataclass(frozen=True)
class ReprojectionSummary:
    """The numbers of ``ReprojectionReport`` without its per-observation table: ``raw_errors`` is None unless it was asked for
    (``reprojection_summary(raw=True)``; the same columns as ``ReprojectionReport.raw_errors`` then)."""

    overall_rmse: float
    by_camera: dict
    by_point: dict
    n_unmatched_observations: int
    unmatched_rate: float
    unmatched_by_camera: dict
    n_observations_matched: int
    n_observations_total: int
    n_cameras: int
    n_points: int
    raw_errors: pd.DataFrame | None = None


__all__ = ["DeviceReprojectionStats", "ReprojectionFilterResult", "ReprojectionSummary", "check_reprojection_arguments", "run_reprojection_call",
           "REPORT_SIGNATURES", "MODES", "SCOPES"]
