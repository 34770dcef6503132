"""The 3-D covariance of every sample of the reconstructed trajectories: how accurate a landmark is at a frame, in world units.

The quality table of the refined call says how well a point fits its views (views, reprojection RMS).  That is fit, not
determination: a two-view sample with a 5 degree baseline reprojects to 0.2 px and is uncertain by centimetres in depth, and none of
the calibration's own uncertainty (``CaptureVolume.parameter_uncertainty``) reaches the trajectories.
``cba_reconstruct_trajectories_uncertain`` (``include/caliscope/trajectory_uncertainty.h``, where the mathematics and its limits are
stated; ``csrc/trajectory_cov_math.h``; ``k_traj_cov`` of ``csrc/trajectory_lib.hip``) is the plain or the refined device call with
one more kernel in front of the 3-D fill: per slot ``cov = sigma_px^2 V^-1 + sum_{c,c'} M_c cam_cov[c,c'] M_c'^T``, the pixel noise
of the recording and the covariance of the camera parameters propagated to first order through the reprojection-error minimiser.

``reconstruct_trajectories(..., covariance=CovarianceOptions(sigma_px, report))`` makes this call and returns
``covariance_frame``'s table as the last element of its result.  The covariance is that of the sample before the 3-D fill and the
filter, relative to the free-network datum of the calibration (no overall similarity), exact under the linear loss, first-order
for an unrefined (DLT) point and approximate under a robust loss.

There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import pandas as pd

from caliscope_amd import _lib
from caliscope_amd.bundle_parameterization import BundleParameterization
from caliscope_amd.reconstruction import TrajDesc, TrajectoryGrid, TrajectoryResult, TrajOut, run_trajectory_call
from caliscope_amd.trajectory_refinement import RefineOptions, TrajectoryQuality, TrajQuality, TrajRefine, refine_struct

COV_NO_POINT, COV_OK, COV_NOT_COMPUTABLE = 0, 1, 2
_WHAT = "cba_reconstruct_trajectories_uncertain"


@dataclass(frozen=True)
class CovarianceOptions:
    """``sigma_px``: standard deviation of a tracked 2-D landmark in pixels (a tracker's noise, not the board corners').
    ``calibration``: the :class:`~caliscope_amd.uncertainty.UncertaintyReport` of the calibration, whose ``cam_cov_full`` is
    propagated into every sample; None gives the noise term alone.  The camera array of the reconstruction has to be the one the
    report was computed at (``parameter_uncertainty()`` of the volume that holds it, with the ``refine_intrinsics`` of its
    optimisation): the Jacobians are evaluated at its parameters, and the widths of the report's blocks say which of them are free."""

    sigma_px: float = 1.0
    calibration: object | None = None


class TrajUncertainty(C.Structure):
    _fields_ = [("cam_nparams", _lib.c_int32_p), ("cam_const", _lib.c_double_p), ("cam_x", _lib.c_double_p), ("cam_offset", _lib.c_int64_p),
                ("ncp", C.c_int64), ("cam_cov", _lib.c_double_p), ("sigma_px", C.c_double)]


class TrajCovOut(C.Structure):
    _fields_ = [("cov", _lib.c_double_p), ("cov_calib", _lib.c_double_p), ("cov_status", _lib.c_uint8_p)]


TRAJ_UNCERTAINTY_SIGNATURES = {
    "cba_reconstruct_trajectories_uncertain": (C.c_int, [C.POINTER(TrajDesc), C.POINTER(TrajRefine), C.POINTER(TrajUncertainty), C.c_int32,
                                                         C.POINTER(TrajOut), C.POINTER(TrajQuality), C.POINTER(TrajCovOut)]),
}


@dataclass(frozen=True)
class UncertaintyTables:
    """``cba_traj_uncertainty`` as arrays, per camera of the grid (rows of unposed cameras are not read)."""

    cam_nparams: np.ndarray     # [n_cams] int32: 6 or 9
    cam_const: np.ndarray       # [n_cams, 12]
    cam_x: np.ndarray           # [n_cams, 9]
    cam_offset: np.ndarray      # [n_cams] int64: first row in cam_cov, -1: the camera is exact
    cam_cov: np.ndarray | None  # [ncp, ncp]; None: the noise term only
    sigma_px: float


@dataclass(frozen=True)
class TrajectoryCovariance:
    """Per slot of the grid; rows are xx xy xz yy yz zz in world units squared, NaN unless ``cov_status`` is 1."""

    cov: np.ndarray                # [n_slots, 6] noise + calibration
    cov_calib: np.ndarray | None   # [n_slots, 6] the calibration term alone; None without a calibration
    cov_status: np.ndarray         # [n_slots] uint8: 0 no point, 1 ok, 2 not computable (a view behind its camera, V singular, filled by xyz_gap)


def uncertainty_tables(grid: TrajectoryGrid, camera_array, options: CovarianceOptions) -> UncertaintyTables:
    """The tables of the call for the cameras of ``grid``: ``cam_const`` and ``cam_x`` from
    ``BundleParameterization.from_camera_array(...).device_tables()`` / ``pack``, as ``CaptureVolume.parameter_uncertainty`` hands
    them to its call.  With ``options.calibration`` the order and the widths of ``cam_cov_full`` are the insertion order of
    ``report.cameras`` and ``param_cov.shape[0]``.  ``ValueError`` naming the ``cam_id``: a posed camera of the grid that the report
    does not have, a width the parameterisation cannot give (anything but 6 or 9; 9 for a fisheye camera), widths that do not add up
    to ``cam_cov_full.shape[0]``.  ``camera_array`` has to be the one the report was computed at."""
    report = options.calibration
    n_cams = grid.n_cams
    widths, offsets, cam_cov = {}, {}, None
    if report is not None:
        cam_cov = np.ascontiguousarray(report.cam_cov_full, dtype=np.float64)
        if cam_cov.ndim != 2 or cam_cov.shape[0] != cam_cov.shape[1]:
            raise ValueError(f"reconstruct_trajectories: covariance.calibration.cam_cov_full must be square, got shape {cam_cov.shape}")
        at, last = 0, None
        for cam_id, cam in report.cameras.items():
            width = int(np.asarray(cam.param_cov).shape[0])
            if at + width > cam_cov.shape[0]:
                raise ValueError(f"reconstruct_trajectories: covariance.calibration: the block of camera {int(cam_id)} ({width} wide, from row {at}) "
                                 f"does not fit cam_cov_full of {cam_cov.shape[0]} rows: the widths of the report do not match it")
            widths[int(cam_id)], offsets[int(cam_id)], last = width, at, int(cam_id)
            at += width
        if at != cam_cov.shape[0]:
            raise ValueError(f"reconstruct_trajectories: covariance.calibration: the widths of the report add up to {at} after camera {last}, "
                             f"cam_cov_full has {cam_cov.shape[0]} rows")
    fixed = BundleParameterization.from_camera_array(camera_array, 0, refine_intrinsics=False)
    free = BundleParameterization.from_camera_array(camera_array, 0, refine_intrinsics=True)
    rows = {}
    for par in (fixed, free):
        const, x = par.device_tables()["cam_const"], par.pack(camera_array, np.zeros((0, 3)))
        for i, (blk, off) in enumerate(zip(par.blocks, par.camera_param_offsets)):
            rows[(blk.cam_id, blk.n_params)] = (const[i], x[off:off + blk.n_params])
    cam_nparams, cam_const, cam_x = np.zeros(n_cams, dtype=np.int32), np.zeros((n_cams, 12)), np.zeros((n_cams, 9))
    cam_offset = np.full(n_cams, -1, dtype=np.int64)
    for c in np.flatnonzero(grid.cam_posed):
        cam_id = int(grid.cam_ids[c])
        if report is not None and cam_id not in widths:
            raise ValueError(f"reconstruct_trajectories: covariance.calibration has no camera {cam_id}, which is posed and has rows in the recording "
                             f"(the report must be that of the camera array in use)")
        width = widths.get(cam_id, 6)
        if (cam_id, width) not in rows:
            kind = "a fisheye camera has no free intrinsics" if width == 9 and camera_array.cameras[cam_id].fisheye else "a camera has 6 or 9 parameters"
            raise ValueError(f"reconstruct_trajectories: covariance.calibration gives camera {cam_id} {width} parameters: {kind}")
        cam_nparams[c], cam_offset[c] = width, offsets.get(cam_id, -1)
        cam_const[c], cam_x[c, :width] = rows[(cam_id, width)]
    return UncertaintyTables(cam_nparams=cam_nparams, cam_const=cam_const, cam_x=cam_x, cam_offset=cam_offset, cam_cov=cam_cov,
                             sigma_px=float(options.sigma_px))


def run_uncertain_call(call, grid: TrajectoryGrid, tables: UncertaintyTables, refine: RefineOptions | None, xy_gap: int, xyz_gap: int, filt,
                       float32_io: bool, memory_limit: int, want_grids: bool, what: str, last_error):
    """``run_trajectory_call`` with the further structures: ``call(desc_ref, refine_ref, uncertainty_ref, out_ref, quality_ref, cov_ref)
    -> code``, ``refine_ref`` and ``quality_ref`` None for the plain call (shared by the device binding and the test harness).
    Returns ``(TrajectoryResult, TrajectoryQuality | None, TrajectoryCovariance)``."""
    n_slots = grid.n_slots
    cov = TrajectoryCovariance(cov=np.full((n_slots, 6), np.nan), cov_calib=np.full((n_slots, 6), np.nan) if tables.cam_cov is not None else None,
                               cov_status=np.zeros(n_slots, dtype=np.uint8))
    cam_cov = None if tables.cam_cov is None else np.ascontiguousarray(tables.cam_cov, dtype=np.float64)
    keep = [np.ascontiguousarray(tables.cam_nparams, dtype=np.int32), np.ascontiguousarray(tables.cam_const, dtype=np.float64),
            np.ascontiguousarray(tables.cam_x, dtype=np.float64), np.ascontiguousarray(tables.cam_offset, dtype=np.int64)]
    try:
        u = TrajUncertainty(cam_nparams=_lib.ptr(keep[0]), cam_const=_lib.ptr(keep[1]), cam_x=_lib.ptr(keep[2]), cam_offset=_lib.ptr(keep[3]),
                            ncp=0 if cam_cov is None else cam_cov.shape[0], cam_cov=_lib.ptr(cam_cov), sigma_px=float(tables.sigma_px))
    except (TypeError, ValueError) as exc:
        raise ValueError(f"reconstruct_trajectories: covariance options are not numbers: {exc}") from exc
    co = TrajCovOut(cov=_lib.ptr(cov.cov), cov_calib=_lib.ptr(cov.cov_calib), cov_status=_lib.ptr(cov.cov_status))
    quality, r_ref, q_ref = None, None, None
    if refine is not None:
        quality = TrajectoryQuality(views=np.zeros(n_slots, dtype=np.int32), rms_px=np.full(n_slots, np.nan), max_px=np.full(n_slots, np.nan),
                                    iterations=np.zeros(n_slots, dtype=np.int32), status=np.zeros(n_slots, dtype=np.uint8),
                                    view_state=np.zeros((grid.n_cams, n_slots), dtype=np.uint8))
        r = refine_struct(refine)
        q = TrajQuality(views=_lib.ptr(quality.views), rms_px=_lib.ptr(quality.rms_px), max_px=_lib.ptr(quality.max_px),
                        iterations=_lib.ptr(quality.iterations), status=_lib.ptr(quality.status), view_state=_lib.ptr(quality.view_state))
        r_ref, q_ref = C.byref(r), C.byref(q)
    result = run_trajectory_call(lambda d, o: call(d, r_ref, C.byref(u), o, q_ref, C.byref(co)), grid, xy_gap, xyz_gap, filt, float32_io, memory_limit,
                                 want_grids, what, last_error)
    return result, quality, cov


class DeviceUncertainTrajectorySolver:
    """The device call ``cba_reconstruct_trajectories_uncertain`` on ``device_id``; ``memory_limit`` as ``DeviceTrajectorySolver``."""

    def __init__(self, device_id: int = 0, memory_limit: int = 0):
        self.device_id = device_id
        self.memory_limit = memory_limit

    def reconstruct_uncertain(self, grid: TrajectoryGrid, options: CovarianceOptions | UncertaintyTables, refine: RefineOptions | None = None, *,
                              camera_array=None, xy_gap=0, xyz_gap=0, filt=None, float32_io=True, want_grids=False):
        """``(TrajectoryResult, TrajectoryQuality | None, TrajectoryCovariance)``.  ``options``: the tables of the call, or
        :class:`CovarianceOptions`, which ``uncertainty_tables`` turns into them at ``camera_array`` (the one ``grid`` was made with)."""
        tables = options if isinstance(options, UncertaintyTables) else uncertainty_tables(grid, camera_array, options)
        lib = _lib.bind(_lib.load(), TRAJ_UNCERTAINTY_SIGNATURES)
        return run_uncertain_call(lambda d, r, u, o, q, c: lib.cba_reconstruct_trajectories_uncertain(d, r, u, self.device_id, o, q, c), grid, tables,
                                  refine, xy_gap, xyz_gap, filt, float32_io, self.memory_limit, want_grids, _WHAT, lambda: _lib.last_error(lib))


COVARIANCE_COLUMNS = ("sync_index", "object_id", "keypoint_id", "cov_xx", "cov_xy", "cov_xz", "cov_yy", "cov_yz", "cov_zz", "std_x", "std_y", "std_z",
                      "std_major", "calib_share", "cov_status")


def full_matrices(rows: np.ndarray) -> np.ndarray:
    """[n, 6] rows xx xy xz yy yz zz as [n, 3, 3]."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    return rows[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def covariance_frame(grid: TrajectoryGrid, result: TrajectoryResult, cov: TrajectoryCovariance) -> pd.DataFrame:
    """One row per row of ``world_points_of(grid, result)``, in its order: the keys, ``cov_xx .. cov_zz`` (world units squared),
    ``std_x, std_y, std_z``, ``std_major`` (root of the largest eigenvalue: the standard deviation along the worst direction),
    ``calib_share`` = tr cov_calib / tr cov (NaN without a calibration) and ``cov_status`` (0 no point, 1 ok, 2 not computable;
    the rows of 0 and 2, cells that ``xyz_gap`` filled among them, are NaN)."""
    s = np.flatnonzero(result.valid)
    f, j = s // max(grid.n_traj, 1), s % max(grid.n_traj, 1)
    rows, status = cov.cov[s], cov.cov_status[s]
    ok = status == COV_OK
    major = np.full(len(s), np.nan)
    if ok.any():
        major[ok] = np.sqrt(np.maximum(np.linalg.eigvalsh(full_matrices(rows[ok]))[:, -1], 0.0))
    share = np.full(len(s), np.nan)
    if cov.cov_calib is not None:
        calib = cov.cov_calib[s]
        share[ok] = (calib[ok][:, [0, 3, 5]].sum(axis=1)) / rows[ok][:, [0, 3, 5]].sum(axis=1)
    frame = {"sync_index": f + grid.sync_min, "object_id": grid.traj_object[j], "keypoint_id": grid.traj_keypoint[j]}
    frame.update({name: rows[:, i] for i, name in enumerate(COVARIANCE_COLUMNS[3:9])})
    with np.errstate(invalid="ignore"):
        frame.update({"std_x": np.sqrt(rows[:, 0]), "std_y": np.sqrt(rows[:, 3]), "std_z": np.sqrt(rows[:, 5])})
    frame.update({"std_major": major, "calib_share": share, "cov_status": status.astype(np.int64)})
    return pd.DataFrame(frame)


__all__ = ["COVARIANCE_COLUMNS", "CovarianceOptions", "DeviceUncertainTrajectorySolver", "TRAJ_UNCERTAINTY_SIGNATURES", "TrajCovOut", "TrajUncertainty",
           "TrajectoryCovariance", "UncertaintyTables", "covariance_frame", "full_matrices", "run_uncertain_call", "uncertainty_tables"]
