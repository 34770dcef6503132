"""Robust reprojection refinement of the trajectories of a recording, with rejection of the views that contradict a point.

``reconstruct_trajectories`` leaves the reference's DLT point in every slot: the minimiser of an algebraic error with all views
weighted alike, which one mistracked landmark in one camera drags by centimetres.  ``cba_reconstruct_trajectories_refined``
(``include/caliscope/trajectory_refine.h``, ``csrc/trajectory_refine_math.h``, ``k_traj_refine`` of ``csrc/trajectory_lib.hip``) is
the same device call with one more kernel between the triangulation and the 3-D fill: Levenberg-Marquardt on the pixel reprojection
error of every slot under one of scipy's robust losses, then up to ``max_reject`` rounds that drop the view with the largest
residual above ``reject_px`` and minimise again, and per slot the views kept, the reprojection RMS and maximum, the evaluations and a
status.  The 3-D fill and the filter run on the refined points.

``reconstruct_trajectories(..., refine=RefineOptions(...))`` makes this call; with ``return_quality=True`` it also returns
``quality_frame``'s table.  The method has a limit that no tuning removes: with 3 views and one outlier, or 5 views and two, the
view with the largest residual is the wrong one in a few percent of slots — rejection needs the bad views to be a clear minority.

There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import pandas as pd

from caliscope_amd import _lib
from caliscope_amd.reconstruction import TrajDesc, TrajectoryGrid, TrajectoryResult, TrajOut, run_trajectory_call

LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}
STATUS_NO_POINT, STATUS_CONVERGED, STATUS_ITERATION_CAP, STATUS_KEPT_DLT = 0, 1, 2, 3
VIEW_NONE, VIEW_USED, VIEW_REJECTED = 0, 1, 2


@dataclass(frozen=True)
class RefineOptions:
    """``loss`` and ``f_scale`` (pixels) as in ``scipy.optimize.least_squares``; ``max_iter`` evaluations per round; a view is
    dropped when its residual exceeds ``reject_px`` (0: never) while ``min_views`` remain, in at most ``max_reject`` rounds.  The
    library checks the values (``ValueError`` with the field named)."""

    loss: str = "huber"
    f_scale: float = 2.0
    max_iter: int = 20
    reject_px: float = 0.0
    max_reject: int = 2
    min_views: int = 2


class TrajRefine(C.Structure):
    _fields_ = [("loss", C.c_int32), ("max_iter", C.c_int32), ("f_scale", C.c_double), ("reject_px", C.c_double), ("max_reject", C.c_int32),
                ("min_views", C.c_int32)]


class TrajQuality(C.Structure):
    _fields_ = [("views", _lib.c_int32_p), ("rms_px", _lib.c_double_p), ("max_px", _lib.c_double_p), ("iterations", _lib.c_int32_p),
                ("status", _lib.c_uint8_p), ("view_state", _lib.c_uint8_p)]


REFINE_SIGNATURES = {
    "cba_reconstruct_trajectories_refined": (C.c_int, [C.POINTER(TrajDesc), C.POINTER(TrajRefine), C.c_int32, C.POINTER(TrajOut),
                                                       C.POINTER(TrajQuality)]),
}


@dataclass(frozen=True)
class TrajectoryQuality:
    """Per slot of the grid (cells that ``xyz_gap`` filled: ``views`` 0, NaN)."""

    views: np.ndarray       # [n_slots] int32 views in use at the end
    rms_px: np.ndarray      # [n_slots] sqrt(mean d_c^2) over them
    max_px: np.ndarray      # [n_slots] max d_c over them
    iterations: np.ndarray  # [n_slots] int32 evaluations, all rounds together
    status: np.ndarray      # [n_slots] uint8: 0 no point, 1 converged, 2 iteration cap, 3 kept the DLT point
    view_state: np.ndarray  # [n_cams, n_slots] uint8: 0 none, 1 used, 2 rejected


def refine_struct(options: RefineOptions) -> TrajRefine:
    """``cba_traj_refine`` of the options; an unknown loss name is a ``ValueError`` here, everything else is the library's to check."""
    if options.loss not in LOSSES:
        raise ValueError(f"reconstruct_trajectories: refine.loss must be one of {sorted(LOSSES)}, got {options.loss!r}")
    try:
        return TrajRefine(loss=LOSSES[options.loss], max_iter=int(options.max_iter), f_scale=float(options.f_scale), reject_px=float(options.reject_px),
                          max_reject=int(options.max_reject), min_views=int(options.min_views))
    except (TypeError, OverflowError) as exc:
        raise ValueError(f"reconstruct_trajectories: refine options are not numbers: {exc}") from exc


def run_refined_call(call, grid: TrajectoryGrid, options: RefineOptions, xy_gap: int, xyz_gap: int, filt, float32_io: bool, memory_limit: int,
                     want_grids: bool, what: str, last_error) -> tuple[TrajectoryResult, TrajectoryQuality]:
    """``run_trajectory_call`` with the two further structures: ``call(desc_ref, refine_ref, out_ref, quality_ref) -> code`` (shared by
    the device binding and the test harness)."""
    n_slots = grid.n_slots
    quality = TrajectoryQuality(views=np.zeros(n_slots, dtype=np.int32), rms_px=np.full(n_slots, np.nan), max_px=np.full(n_slots, np.nan),
                                iterations=np.zeros(n_slots, dtype=np.int32), status=np.zeros(n_slots, dtype=np.uint8),
                                view_state=np.zeros((grid.n_cams, n_slots), dtype=np.uint8))
    refine = refine_struct(options)
    q = TrajQuality(views=_lib.ptr(quality.views), rms_px=_lib.ptr(quality.rms_px), max_px=_lib.ptr(quality.max_px), iterations=_lib.ptr(quality.iterations),
                    status=_lib.ptr(quality.status), view_state=_lib.ptr(quality.view_state))
    result = run_trajectory_call(lambda d, o: call(d, C.byref(refine), o, C.byref(q)), grid, xy_gap, xyz_gap, filt, float32_io, memory_limit, want_grids,
                                 what, last_error)
    return result, quality


class DeviceRefinedTrajectorySolver:
    """The device call ``cba_reconstruct_trajectories_refined`` on ``device_id``; ``memory_limit`` as ``DeviceTrajectorySolver``."""

    def __init__(self, device_id: int = 0, memory_limit: int = 0):
        self.device_id = device_id
        self.memory_limit = memory_limit

    def reconstruct_refined(self, grid: TrajectoryGrid, options: RefineOptions, *, xy_gap=0, xyz_gap=0, filt=None, float32_io=True,
                            want_grids=False) -> tuple[TrajectoryResult, TrajectoryQuality]:
        lib = _lib.bind(_lib.load(), REFINE_SIGNATURES)
        return run_refined_call(lambda d, r, o, q: lib.cba_reconstruct_trajectories_refined(d, r, self.device_id, o, q), grid, options, xy_gap, xyz_gap,
                                filt, float32_io, self.memory_limit, want_grids, "cba_reconstruct_trajectories_refined", lambda: _lib.last_error(lib))


def quality_frame(grid: TrajectoryGrid, result: TrajectoryResult, quality: TrajectoryQuality) -> pd.DataFrame:
    """One row per row of ``world_points_of(grid, result)``, in its order: the keys, ``n_views``, ``n_rejected``, ``reproj_rms_px``,
    ``reproj_max_px``, ``status`` and ``rejected_cam_ids`` (a tuple of ``cam_id``, ascending)."""
    s = np.flatnonzero(result.valid)
    f, j = s // max(grid.n_traj, 1), s % max(grid.n_traj, 1)
    rejected = quality.view_state[:, s] == VIEW_REJECTED  # [n_cams, rows]
    ids = [tuple(int(c) for c in grid.cam_ids[rejected[:, i]]) for i in range(len(s))]
    return pd.DataFrame({
        "sync_index": f + grid.sync_min, "object_id": grid.traj_object[j], "keypoint_id": grid.traj_keypoint[j],
        "n_views": quality.views[s].astype(np.int64), "n_rejected": rejected.sum(axis=0).astype(np.int64), "reproj_rms_px": quality.rms_px[s],
        "reproj_max_px": quality.max_px[s], "status": quality.status[s].astype(np.int64), "rejected_cam_ids": pd.Series(ids, dtype=object),
    })


QUALITY_COLUMNS = ("sync_index", "object_id", "keypoint_id", "n_views", "n_rejected", "reproj_rms_px", "reproj_max_px", "status", "rejected_cam_ids")

__all__ = ["DeviceRefinedTrajectorySolver", "LOSSES", "QUALITY_COLUMNS", "REFINE_SIGNATURES", "RefineOptions", "TrajQuality", "TrajRefine",
           "TrajectoryQuality", "quality_frame", "refine_struct", "run_refined_call"]
