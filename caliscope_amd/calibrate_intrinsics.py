"""Intrinsic calibration of the cameras of a rig from their board views, all cameras in one call on the MI355X.

Host-side mirror of the reference's ``core/calibrate_intrinsics.py`` under the same names where it has them:

* :class:`IntrinsicCalibrationResult` and :func:`calibrate_intrinsics` (one camera: the reference's signature, errors and result);
* :func:`calibrate_camera_array_intrinsics`: every non-ignored camera of a :class:`CameraArray` in ONE device call, the
  ``matrix`` / ``distortions`` / ``error`` / ``grid_count`` fields set as ``run_intrinsic_calibration`` step 3 sets them.  With
  ``frames=None`` every frame with at least four corners is used (the reference sub-samples to about 30 frames because
  ``cv2.calibrateCamera`` cannot afford more); ``frames="select"`` runs the reference's frame selection for all cameras first
  (``caliscope_amd/frame_selector.py``, one more device call) and attaches each camera's coverage report;
* :class:`IntrinsicCalibrationReport`, :class:`IntrinsicCalibrationOutput` and :func:`run_intrinsic_calibration`: the reference's
  one-camera workflow, selection -> solve -> calibrated camera and report.

Where the work runs: the views are gathered with numpy (one sort of the rows); start poses (``k_pose_pnp`` with the start
intrinsics) and the whole Levenberg-Marquardt solve (``k_intrinsics``, one workgroup per camera) run on the device through
``cba_pose_intrinsics_batch`` (``csrc/intrinsic_math.h`` holds the arithmetic).  There is no CPU fallback: without the library or
a GPU the call raises ``BackendError``.  ``_solver`` replaces the device call (an object with ``intrinsics_batch``, as
:class:`DeviceIntrinsics`) — the CPU test-suite passes a g++ build of the same arithmetic.

Differences from cv2, on purpose: the result is the least-squares minimum of the pixel reprojection error, not cv2's bits (cv2 stops
after 30 iterations or a 2.2e-16 change); the fisheye model has no skew (``cv2.fisheye.calibrate`` estimates one unless told not
to; the camera model of this project has none); the fisheye start (f = max(w, h) / pi, c = (w/2 - 0.5, h/2 - 0.5)) is this project's
choice; views whose start pose cannot be found are left out and reported instead of failing the call.
"""

from __future__ import annotations

import ctypes as C
import logging
from copy import deepcopy
from dataclasses import dataclass, replace

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.frame_selector import IntrinsicCoverageReport, rig_cameras, select_calibration_frames, select_rig

logger = logging.getLogger(__name__)

MIN_CORNERS_PER_FRAME = 4  # reference calibrate_intrinsics.py:30
INTR_OK, INTR_TOO_FEW, INTR_FAILED = 0, 1, 2
_STATUS_NAME = {INTR_OK: "ok", INTR_TOO_FEW: "too few usable views", INTR_FAILED: "solve failed"}


class IntrinsicsDesc(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("cam_model", _lib.c_int32_p), ("cam_size", _lib.c_double_p), ("cam_start", _lib.c_double_p),
        ("n_views", C.c_int64), ("view_start", _lib.c_int64_p), ("view_cam", _lib.c_int32_p), ("obs_xy", _lib.c_double_p),
        ("obs_obj", _lib.c_double_p), ("float32_io", C.c_int32), ("max_iter", C.c_int32),
    ]


INTRINSICS_SIGNATURES = {
    "cba_pose_intrinsics_batch": (C.c_int, [C.POINTER(IntrinsicsDesc), C.c_int32, _lib.c_double_p, _lib.c_double_p, _lib.c_int32_p,
                                            _lib.c_int32_p, _lib.c_double_p, _lib.c_double_p, _lib.c_int32_p]),
}


class DeviceIntrinsics:
    """The device call ``cba_pose_intrinsics_batch`` on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def intrinsics_batch(self, cam_model, cam_size, cam_start, view_start, view_cam, obs_xy, obs_obj, float32_io=True, max_iter=0):
        """Returns ``(intr[n_cams, 9], rmse[n_cams], status[n_cams], iters[n_cams], pose[n_views, 12], view_rmse[n_views],
        view_status[n_views])``; ``cam_start`` may be None (default start values)."""
        lib = _lib.bind(_lib.load(), INTRINSICS_SIGNATURES)
        cam_model = np.ascontiguousarray(cam_model, dtype=np.int32)
        cam_size = np.ascontiguousarray(cam_size, dtype=np.float64).reshape(-1, 2)
        cam_start = None if cam_start is None else np.ascontiguousarray(cam_start, dtype=np.float64).reshape(-1, 9)
        view_start = np.ascontiguousarray(view_start, dtype=np.int64)
        view_cam = np.ascontiguousarray(view_cam, dtype=np.int32)
        obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
        obs_obj = np.ascontiguousarray(obs_obj, dtype=np.float64).reshape(-1, 3)
        n_cams, n_views = len(cam_model), len(view_start) - 1
        if len(cam_size) != n_cams or (cam_start is not None and len(cam_start) != n_cams) or len(view_cam) != n_views or \
                len(obs_xy) != int(view_start[-1]) or len(obs_obj) != int(view_start[-1]):
            raise ValueError("intrinsics_batch: array lengths do not match")
        intr, rmse = np.zeros((n_cams, 9)), np.zeros(n_cams)
        status, iters = np.zeros(n_cams, dtype=np.int32), np.zeros(n_cams, dtype=np.int32)
        pose, view_rmse, view_status = np.zeros((n_views, 12)), np.zeros(n_views), np.zeros(n_views, dtype=np.int32)
        desc = IntrinsicsDesc(n_cams=n_cams, cam_model=_lib.ptr(cam_model), cam_size=_lib.ptr(cam_size), cam_start=_lib.ptr(cam_start),
                              n_views=n_views, view_start=_lib.ptr(view_start), view_cam=_lib.ptr(view_cam), obs_xy=_lib.ptr(obs_xy),
                              obs_obj=_lib.ptr(obs_obj), float32_io=1 if float32_io else 0, max_iter=int(max_iter))
        rc = lib.cba_pose_intrinsics_batch(C.byref(desc), self.device_id, _lib.ptr(intr), _lib.ptr(rmse), _lib.ptr(status), _lib.ptr(iters),
                                           _lib.ptr(pose), _lib.ptr(view_rmse), _lib.ptr(view_status))
        _lib.check(lib, rc, "cba_pose_intrinsics_batch")
        return intr, rmse, status, iters, pose, view_rmse, view_status


@dataclass(frozen=True)
class IntrinsicCalibrationResult:
    """Result of the calibration of one camera (reference ``calibrate_intrinsics.py:33-50``): 3 x 3 camera matrix, distortion
    coefficients ((5,) k1 k2 p1 p2 k3, or (4,) k1..k4 for the fisheye model), RMS reprojection error in pixels as
    ``cv2.calibrateCamera`` defines it, and the number of frames that entered the solve."""

    camera_matrix: np.ndarray
    distortions: np.ndarray
    reprojection_error: float
    frames_used: int


@dataclass(frozen=True)
class CameraIntrinsicsReport:
    """What :func:`calibrate_camera_array_intrinsics` reports per camera: ``result`` (None unless ``status == 0``), the status
    (0 ok, 1 too few usable views, 2 solve failed), the number of linearisations, and per view handed to the solver — a view is
    one object in one frame, the key of the pose bootstrap — its ``sync_index``, ``object_id``, status (0 used, 1 too few corners,
    2 left out: no start pose) and RMS reprojection error in pixels.  ``coverage``: the camera's frame-selection report when the
    call selected the frames (``frames="select"``), else None."""

    result: IntrinsicCalibrationResult | None
    status: int
    iterations: int
    sync_index: np.ndarray
    view_status: np.ndarray
    view_rmse: np.ndarray
    object_id: np.ndarray | None = None
    coverage: IntrinsicCoverageReport | None = None


@dataclass(frozen=True)
class IntrinsicCalibrationReport:
    """How the intrinsic calibration of one camera was derived (reference ``calibrate_intrinsics.py:53-73``): RMSE on the calibration
    frames in pixels and their number, the selection's coverage fractions and orientation diversity, and the selected
    ``sync_index`` values."""

    rmse: float
    frames_used: int
    coverage_fraction: float
    edge_coverage_fraction: float
    corner_coverage_fraction: float
    orientation_sufficient: bool
    orientation_count: int
    selected_frames: tuple[int, ...]


@dataclass(frozen=True)
class IntrinsicCalibrationOutput:
    """The calibrated camera and its report, travelling together (reference ``calibrate_intrinsics.py:76-86``)."""

    camera: object
    report: IntrinsicCalibrationReport


def _gather_views(image_points, cam_ids, frames, by_object):
    """Views with at least MIN_CORNERS_PER_FRAME corners, in CSR form over cameras in ``cam_ids`` order.  A view is
    (cam_id, sync_index, object_id) with ``by_object`` — the key of the pose bootstrap (``pose_network.py``): every rigid object has
    its own ``obj_loc`` frame — and (cam_id, sync_index) without, as the reference's single-board ``calibrate_intrinsics`` groups.
    Rows without a finite pixel or ``obj_loc_x`` / ``obj_loc_y`` (tracker rows between board rows) are dropped, as the PnP bootstrap
    leaves them unsolved.  ``frames``: None (every frame) or ``{cam_id: iterable of sync_index}``."""
    df = image_points.df
    cam_all = df["cam_id"].to_numpy(dtype=np.int64)
    sync_all = df["sync_index"].to_numpy(dtype=np.int64)
    obj_all = df["object_id"].to_numpy(dtype=np.int64) if by_object and "object_id" in df.columns else np.zeros(len(df), dtype=np.int64)
    xy_all = np.column_stack([df["img_loc_x"].to_numpy(dtype=np.float64), df["img_loc_y"].to_numpy(dtype=np.float64)]).reshape(-1, 2)
    xyz_all = np.column_stack([df[c].to_numpy(dtype=np.float64) for c in ("obj_loc_x", "obj_loc_y", "obj_loc_z")]).reshape(-1, 3)
    xyz_all[:, 2] = np.nan_to_num(xyz_all[:, 2], nan=0.0)  # planar board: NaN z is 0 (reference :220)
    keep = np.isin(cam_all, cam_ids) & np.isfinite(xy_all).all(axis=1) & np.isfinite(xyz_all).all(axis=1)
    if frames is not None:
        sel = np.zeros(len(df), dtype=bool)
        for c in cam_ids:
            sel |= (cam_all == c) & np.isin(sync_all, np.asarray(list(frames.get(c, ())), dtype=np.int64))
        keep &= sel
    rows = np.flatnonzero(keep)
    index_of = {c: i for i, c in enumerate(cam_ids)}
    cam_idx = np.array([index_of[c] for c in cam_all[rows]], dtype=np.int64)
    sync, obj = sync_all[rows], obj_all[rows]
    order = np.lexsort((obj, sync, cam_idx))  # stable: rows of a view keep their order
    rows, cam_idx, sync, obj = rows[order], cam_idx[order], sync[order], obj[order]
    n = len(rows)
    brk = np.flatnonzero((np.diff(cam_idx) != 0) | (np.diff(sync) != 0) | (np.diff(obj) != 0)) + 1 if n else np.zeros(0, np.int64)
    starts = np.concatenate([[0], brk, [n]]).astype(np.int64) if n else np.zeros(1, np.int64)
    size = np.diff(starts)
    good = size >= MIN_CORNERS_PER_FRAME
    rows = rows[np.repeat(good, size)]
    first = starts[:-1][good]
    view_cam, view_sync, view_obj = cam_idx[first].astype(np.int32), sync[first], obj[first]
    view_start = np.concatenate([[0], np.cumsum(size[good])]).astype(np.int64)
    return view_start, view_cam, view_sync, view_obj, xy_all[rows], xyz_all[rows]


def _solve(image_points, cams, frames, float32_io, max_iter, _solver, by_object=True):
    """``cams``: list of (cam_id, (w, h), fisheye).  Returns {cam_id: CameraIntrinsicsReport}."""
    cam_ids = [c for c, _, _ in cams]
    view_start, view_cam, view_sync, view_obj, xy, xyz = _gather_views(image_points, cam_ids, frames, by_object)
    backend = _solver or DeviceIntrinsics()
    model = np.array([1 if fe else 0 for _, _, fe in cams], dtype=np.int32)
    size = np.array([[float(s[0]), float(s[1])] for _, s, _ in cams], dtype=np.float64)
    intr, rmse, status, iters, _, view_rmse, view_status = backend.intrinsics_batch(model, size, None, view_start, view_cam, xy, xyz, float32_io, max_iter)
    out = {}
    for i, (cam_id, _, fisheye) in enumerate(cams):
        mine = view_cam == i
        result = None
        if status[i] == INTR_OK:
            K = np.array([[intr[i, 0], 0.0, intr[i, 2]], [0.0, intr[i, 1], intr[i, 3]], [0.0, 0.0, 1.0]])
            result = IntrinsicCalibrationResult(K, intr[i, 4:8].copy() if fisheye else intr[i, 4:9].copy(), float(rmse[i]),
                                                int((view_status[mine] == 0).sum()))
            logger.info(f"Calibration complete for cam_id {cam_id}: error={result.reprojection_error:.4f}px, frames={result.frames_used}")
        else:
            logger.warning(f"Intrinsic calibration of cam_id {cam_id}: {_STATUS_NAME.get(int(status[i]), status[i])} ({int(mine.sum())} frames offered)")
        out[cam_id] = CameraIntrinsicsReport(result, int(status[i]), int(iters[i]), view_sync[mine].copy(), view_status[mine].copy(), view_rmse[mine].copy(),
                                             view_obj[mine].copy())
    return out


def calibrate_intrinsics(image_points, cam_id: int, image_size: tuple[int, int], selected_frames: list[int], *, fisheye: bool = False,
                         float32_io: bool = True, _solver=None) -> IntrinsicCalibrationResult:
    """Calibrate one camera from the frames ``selected_frames`` (the reference's function, ``calibrate_intrinsics.py:89-180``).
    ``ValueError`` when no selected frame of ``cam_id`` has at least four corners, or when the solve cannot run on those
    that do (fewer than three usable views, a singular system).  As in the reference all corners of a frame form one view (a
    single-board table); :func:`calibrate_camera_array_intrinsics` splits a frame by ``object_id``."""
    report = _solve(image_points, [(cam_id, image_size, fisheye)], {cam_id: list(selected_frames)}, float32_io, 0, _solver, by_object=False)[cam_id]
    if len(report.sync_index) == 0:
        raise ValueError(f"No valid calibration frames found for cam_id {cam_id}. Ensure frames have at least {MIN_CORNERS_PER_FRAME} corners each.")
    if report.result is None:
        raise ValueError(f"Intrinsic calibration of cam_id {cam_id} failed: {_STATUS_NAME.get(report.status, report.status)} "
                         f"({int((report.view_status == 0).sum())} of {len(report.sync_index)} frames usable).")
    return report.result


def run_intrinsic_calibration(camera, image_points, selection_result: IntrinsicCoverageReport | None = None, *, float32_io: bool = True,
                              _solver=None, _selector=None) -> IntrinsicCalibrationOutput:
    """The complete workflow for one camera (the reference's function, ``calibrate_intrinsics.py:233-308``): frame selection unless
    ``selection_result`` brings one, the solve on the selected frames, then the calibrated camera — a copy of ``camera`` with
    ``matrix``, ``distortions``, ``error`` and ``grid_count`` set — and the report.  ``ValueError`` when no frame is selected or the
    calibration fails.  ``_solver`` / ``_selector`` replace the two device calls."""
    cam_id = camera.cam_id
    if selection_result is None:
        selection_result = select_calibration_frames(image_points, cam_id, camera.size, float32_io=float32_io, _solver=_selector)
    if not selection_result.selected_frames:
        raise ValueError(f"No frames selected for calibration on cam_id {cam_id}")
    selected_frames = selection_result.selected_frames
    result = calibrate_intrinsics(image_points, cam_id, camera.size, selected_frames, fisheye=bool(camera.fisheye), float32_io=float32_io,
                                  _solver=_solver)
    calibrated = deepcopy(camera)
    calibrated.matrix = result.camera_matrix.copy()
    calibrated.distortions = result.distortions.copy()
    calibrated.error = result.reprojection_error
    calibrated.grid_count = result.frames_used
    report = IntrinsicCalibrationReport(
        rmse=result.reprojection_error, frames_used=result.frames_used, coverage_fraction=selection_result.coverage_fraction,
        edge_coverage_fraction=selection_result.edge_coverage_fraction, corner_coverage_fraction=selection_result.corner_coverage_fraction,
        orientation_sufficient=selection_result.orientation_sufficient, orientation_count=selection_result.orientation_count,
        selected_frames=tuple(selected_frames))
    logger.info(f"Calibration complete for cam_id {cam_id}: rmse={report.rmse:.3f}px, frames={report.frames_used}, coverage={report.coverage_fraction:.0%}")
    return IntrinsicCalibrationOutput(camera=calibrated, report=report)


def calibrate_camera_array_intrinsics(image_points, camera_array, frames=None, *, only_missing: bool = False, float32_io: bool = True,
                                      max_iter: int = 0, target_frame_count: int = 30, min_corners_per_frame: int = 6, min_orientations: int = 4,
                                      grid_size: int = 5, _solver=None, _selector=None):
    """Calibrate every non-ignored camera of ``camera_array`` (``only_missing``: only those without a matrix or distortion
    coefficients) in one device call.  A view is one object in one frame, (cam_id, sync_index, object_id) as in the pose
    bootstrap: sessions may hold several rigid objects, each with its own ``obj_loc`` frame.  ``frames=None``: every view with at
    least four corners; ``{cam_id: [sync_index, ...]}``
    selects frames per camera (a camera not named gets none); ``"select"`` runs :func:`caliscope_amd.frame_selector.select_rig` over the
    same cameras first (keywords ``target_frame_count``, ``min_corners_per_frame``, ``min_orientations``, ``grid_size``; ``_selector``
    replaces its device call), solves from the frames it chose and sets ``coverage`` in every report.  Returns ``(CameraArray, {cam_id: CameraIntrinsicsReport})``: a copy
    of the array in which every camera that solved carries ``matrix``, ``distortions``, ``error`` and ``grid_count``; a camera
    that did not is left as it was.  The input array is not touched."""
    out = deepcopy(camera_array)
    cams = [(cam_id, cam.size, bool(cam.fisheye)) for cam_id, cam in rig_cameras(out, only_missing)]
    if not cams:
        return out, {}
    coverage = None
    if isinstance(frames, str):
        if frames != "select":
            raise ValueError(f"frames must be None, a dict {{cam_id: sync_index values}} or \"select\", got {frames!r}")
        coverage, _, _ = select_rig(image_points, [(c, size) for c, size, _ in cams], target_frame_count=target_frame_count,
                                    min_corners_per_frame=min_corners_per_frame, min_orientations=min_orientations, grid_size=grid_size,
                                    float32_io=float32_io, by_object=True, _solver=_selector)
        frames = {c: rep.selected_frames for c, rep in coverage.items()}
    reports = _solve(image_points, cams, frames, float32_io, max_iter, _solver)
    if coverage is not None:
        reports = {c: replace(rep, coverage=coverage[c]) for c, rep in reports.items()}
    for cam_id, rep in reports.items():
        if rep.result is not None:
            cam = out.cameras[cam_id]
            cam.matrix = rep.result.camera_matrix.copy()
            cam.distortions = rep.result.distortions.copy()
            cam.error = rep.result.reprojection_error
            cam.grid_count = rep.result.frames_used
    return out, reports


__all__ = ["IntrinsicCalibrationResult", "CameraIntrinsicsReport", "IntrinsicCalibrationReport", "IntrinsicCalibrationOutput",
           "IntrinsicCoverageReport", "DeviceIntrinsics", "calibrate_intrinsics", "calibrate_camera_array_intrinsics",
           "run_intrinsic_calibration", "select_calibration_frames", "MIN_CORNERS_PER_FRAME"]
