"""Frame selection and coverage report for the intrinsic calibration, all cameras of a rig in one call on the MI355X.

Host-side mirror of the reference's ``core/frame_selector.py`` under the same names:

* :class:`IntrinsicCoverageReport` (the reference's nine fields) and :func:`select_calibration_frames` (one camera: the reference's
  signature and result);
* :func:`select_camera_array_frames`: every non-ignored camera of a :class:`CameraArray` in ONE device call.

The algorithm is the reference's.  Per frame: the grid cells its corners cover, five pose features (centroid, spread, aspect) and
the board orientation read off the homography board -> pixels.  Per camera: phase 1 takes one anchor per occupied 45 degree bin of
the tilt direction (the most tilted frame; Zhang's observability condition for the focal length wants at least four), phase 2 fills
the budget greedily by new cells (edge and corner cells weigh more) plus the distance in the pose features to the nearest frame
already taken; ties go to the lowest ``sync_index``.

Where the work runs: the rows are screened and put into CSR form with numpy (one lexsort, no per-frame Python); the per-frame
features (``k_frame_features``, one thread per frame) and both phases (``k_frame_select``, one workgroup per camera) run on the
device through ``cba_pose_select_frames`` (``csrc/frame_select_math.h`` holds the arithmetic); the four quality fractions of the
report are a few numpy lines on the returned masks and pose features.  There is no CPU fallback: without the library or a GPU the
call raises ``BackendError``.  ``_solver`` replaces the device call (an object with ``select_frames``, as
:class:`DeviceFrameSelection`) — the CPU test-suite passes a g++ build of the same arithmetic.

Differences from the reference, on purpose: the homography is the least-squares minimum of the pixel transfer error over all corners
handed in, not ``cv2.findHomography(..., RANSAC, 5.0)`` (board corners carry ids, so a wrong corner is a detector fault, not a
matching ambiguity; with no corner beyond the 5 px gate cv2's refined result is this same minimum) and the per-frame transfer RMSE
is returned so that a caller can screen frames; the in-plane rotation is the closed form of the polar factor instead of an SVD; rows
without a finite pixel or board coordinate are dropped first; in a frame that shows several rigid objects the homography runs over
the object with the most rows (lowest ``object_id`` on ties: each object has its own ``obj_loc`` frame) while coverage, pose
features and eligibility use all rows.
"""

from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from caliscope_amd import _lib

logger = logging.getLogger(__name__)

MAX_GRID_SIZE = 8  # the cell mask has 64 bits
NUM_TILT_DIRECTION_BINS = 8
HOMOG_OK, HOMOG_TOO_FEW, HOMOG_FAILED = 0, 1, 2


@dataclass(frozen=True)
class IntrinsicCoverageReport:
    """Coverage and selection result for the intrinsic calibration of one camera (reference ``frame_selector.py:71-94``):
    the selected ``sync_index`` values in selection order, the fractions of grid, edge and corner cells they cover, the mean
    variance of their pose features, whether at least ``min_orientations`` tilt-direction bins were seen and how many, and the
    number of eligible frames and of frames."""

    selected_frames: list[int]
    coverage_fraction: float
    edge_coverage_fraction: float
    corner_coverage_fraction: float
    pose_diversity: float
    orientation_sufficient: bool
    orientation_count: int
    eligible_frame_count: int
    total_frame_count: int


@dataclass
class FrameSelection:
    """What one ``select_frames`` call returns.  Per frame: ``cell_mask`` (uint64, bit row * grid_size + col), ``pose_features``
    [n, 5], ``orientation`` [n, 3] (tilt direction, tilt magnitude, in-plane rotation), ``homography_status`` (0 ok, 1 fewer than
    four corners, 2 fit failed) and ``homography_rmse`` (transfer RMSE in pixels).  Per camera: ``selected`` [n_cams, target_count]
    frame numbers within the camera in selection order (-1 beyond ``n_selected``), ``n_anchors``, ``bin_mask``, ``eligible``."""

    cell_mask: np.ndarray
    pose_features: np.ndarray
    orientation: np.ndarray
    homography_status: np.ndarray
    homography_rmse: np.ndarray
    selected: np.ndarray
    n_selected: np.ndarray
    n_anchors: np.ndarray
    bin_mask: np.ndarray
    eligible: np.ndarray

    @classmethod
    def empty(cls, n_cams: int, n_frames: int, target_count: int) -> "FrameSelection":
        i32 = np.int32
        return cls(np.zeros(n_frames, dtype=np.uint64), np.zeros((n_frames, 5)), np.zeros((n_frames, 3)), np.zeros(n_frames, dtype=i32),
                   np.zeros(n_frames), np.full((n_cams, target_count), -1, dtype=i32), np.zeros(n_cams, dtype=i32), np.zeros(n_cams, dtype=i32),
                   np.zeros(n_cams, dtype=i32), np.zeros(n_cams, dtype=i32))


def check_selection_arguments(cam_frame_start, cam_size, frame_start, obs_xy, obs_obj, homog_start, homog_count, grid_size, min_corners,
                              target_count):
    """The arrays of a ``select_frames`` call in the layout of ``cba_frame_select_desc``, after the checks the library makes
    (``ValueError``)."""
    if not 1 <= int(grid_size) <= MAX_GRID_SIZE:
        raise ValueError(f"grid_size must be 1..{MAX_GRID_SIZE} (the cell mask has 64 bits), got {grid_size}")
    if int(target_count) < 1:
        raise ValueError(f"target_frame_count must be at least 1, got {target_count}")
    if int(min_corners) < 0:
        raise ValueError(f"min_corners_per_frame must not be negative, got {min_corners}")
    a = SimpleNamespace(grid_size=int(grid_size), min_corners=int(min_corners), target_count=int(target_count))
    a.cam_frame_start = np.ascontiguousarray(cam_frame_start, dtype=np.int64)
    a.cam_size = np.ascontiguousarray(cam_size, dtype=np.float64).reshape(-1, 2)
    a.frame_start = np.ascontiguousarray(frame_start, dtype=np.int64)
    a.obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
    a.obs_obj = np.ascontiguousarray(obs_obj, dtype=np.float64).reshape(-1, 2)
    a.n_cams, a.n_frames = len(a.cam_frame_start) - 1, len(a.frame_start) - 1
    if a.n_cams < 0 or a.n_frames < 0 or len(a.cam_size) != a.n_cams or a.cam_frame_start[0] != 0 or a.frame_start[0] != 0 or \
            a.cam_frame_start[-1] != a.n_frames or len(a.obs_xy) != a.frame_start[-1] or len(a.obs_obj) != a.frame_start[-1]:
        raise ValueError("select_frames: array lengths do not match")
    if (np.diff(a.cam_frame_start) < 0).any() or (np.diff(a.frame_start) < 0).any():
        raise ValueError("select_frames: a CSR array decreases")
    if not (np.isfinite(a.cam_size).all() and (a.cam_size > 0).all()):
        raise ValueError("select_frames: a camera has no image size")
    if (homog_start is None) != (homog_count is None):
        raise ValueError("select_frames: homog_start and homog_count go together")
    a.homog_start = None if homog_start is None else np.ascontiguousarray(homog_start, dtype=np.int64)
    a.homog_count = None if homog_count is None else np.ascontiguousarray(homog_count, dtype=np.int32)
    if a.homog_start is not None:
        if len(a.homog_start) != a.n_frames or len(a.homog_count) != a.n_frames:
            raise ValueError("select_frames: array lengths do not match")
        if ((a.homog_count < 0) | (a.homog_start < a.frame_start[:-1]) | (a.homog_start + a.homog_count > a.frame_start[1:])).any():
            raise ValueError("select_frames: a homography subrange lies outside its frame")
    return a


class FrameSelectDesc(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("cam_frame_start", _lib.c_int64_p), ("cam_size", _lib.c_double_p), ("n_frames", C.c_int64),
        ("frame_start", _lib.c_int64_p), ("homog_start", _lib.c_int64_p), ("homog_count", _lib.c_int32_p), ("obs_xy", _lib.c_double_p),
        ("obs_obj", _lib.c_double_p), ("grid_size", C.c_int32), ("min_corners", C.c_int32), ("target_count", C.c_int32), ("float32_io", C.c_int32),
    ]


FRAME_SELECT_SIGNATURES = {
    "cba_pose_select_frames": (C.c_int, [C.POINTER(FrameSelectDesc), C.c_int32, _lib.c_uint64_p, _lib.c_double_p, _lib.c_double_p, _lib.c_int32_p,
                                         _lib.c_double_p, _lib.c_int32_p, _lib.c_int32_p, _lib.c_int32_p, _lib.c_int32_p, _lib.c_int32_p]),
}


# Kept for tests/test_frame_selection_gpu.py alone, which calls the library directly through these two names (the module itself
# uses _lib.bind / _lib.ptr): _ptr takes the element type that test passes and does not use it, the array's dtype decides.
def _load():
    return _lib.bind(_lib.load(), FRAME_SELECT_SIGNATURES)


def _ptr(a, ctype=None):
    return _lib.ptr(a)


class DeviceFrameSelection:
    """The device call ``cba_pose_select_frames`` on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def select_frames(self, cam_frame_start, cam_size, frame_start, obs_xy, obs_obj, homog_start=None, homog_count=None, *, grid_size=5,
                      min_corners=6, target_count=30, float32_io=True) -> FrameSelection:
        """Frames in CSR form over the rows, cameras in CSR form over the frames (``cba_frame_select_desc``); returns a
        :class:`FrameSelection`."""
        a = check_selection_arguments(cam_frame_start, cam_size, frame_start, obs_xy, obs_obj, homog_start, homog_count, grid_size, min_corners,
                                      target_count)
        lib = _lib.bind(_lib.load(), FRAME_SELECT_SIGNATURES)
        out = FrameSelection.empty(a.n_cams, a.n_frames, a.target_count)
        desc = FrameSelectDesc(n_cams=a.n_cams, cam_frame_start=_lib.ptr(a.cam_frame_start), cam_size=_lib.ptr(a.cam_size), n_frames=a.n_frames,
                               frame_start=_lib.ptr(a.frame_start), homog_start=_lib.ptr(a.homog_start),
                               homog_count=_lib.ptr(a.homog_count), obs_xy=_lib.ptr(a.obs_xy), obs_obj=_lib.ptr(a.obs_obj), grid_size=a.grid_size,
                               min_corners=a.min_corners, target_count=a.target_count, float32_io=1 if float32_io else 0)
        rc = lib.cba_pose_select_frames(C.byref(desc), self.device_id, _lib.ptr(out.cell_mask), _lib.ptr(out.pose_features), _lib.ptr(out.orientation),
                                        _lib.ptr(out.homography_status), _lib.ptr(out.homography_rmse), _lib.ptr(out.selected),
                                        _lib.ptr(out.n_selected), _lib.ptr(out.n_anchors), _lib.ptr(out.bin_mask),
                                        _lib.ptr(out.eligible))
        _lib.check(lib, rc, "cba_pose_select_frames")
        return out


@dataclass
class GatheredFrames:
    """The frames of the cameras ``cam_ids`` in CSR form: ``cam_frame_start`` over frames (ascending ``sync_index`` within a camera),
    ``frame_start`` over the kept rows, ``frame_sync`` per frame, the pixels and board x, y of the rows, and per frame the subrange
    the homography runs over (None: the whole frame)."""

    cam_frame_start: np.ndarray
    frame_start: np.ndarray
    frame_sync: np.ndarray
    obs_xy: np.ndarray
    obs_obj: np.ndarray
    homog_start: np.ndarray | None
    homog_count: np.ndarray | None


def gather_frames(image_points, cam_ids, by_object: bool) -> GatheredFrames:
    """Rows without a finite pixel or ``obj_loc_x`` / ``obj_loc_y`` are dropped (as ``calibrate_intrinsics._gather_views`` does); a
    frame is every remaining row of (cam_id, sync_index).  With ``by_object`` the rows of a frame are grouped by ``object_id`` and the
    homography subrange is the object with the most rows, the lowest ``object_id`` on ties."""
    df = image_points.df
    cam_all = df["cam_id"].to_numpy(dtype=np.int64)
    sync_all = df["sync_index"].to_numpy(dtype=np.int64)
    split = by_object and "object_id" in df.columns
    obj_all = df["object_id"].to_numpy(dtype=np.int64) if split else np.zeros(len(df), dtype=np.int64)
    xy_all = np.column_stack([df["img_loc_x"].to_numpy(dtype=np.float64), df["img_loc_y"].to_numpy(dtype=np.float64)]).reshape(-1, 2)
    board_all = np.column_stack([df["obj_loc_x"].to_numpy(dtype=np.float64), df["obj_loc_y"].to_numpy(dtype=np.float64)]).reshape(-1, 2)
    rows = np.flatnonzero(np.isin(cam_all, cam_ids) & np.isfinite(xy_all).all(axis=1) & np.isfinite(board_all).all(axis=1))
    ids = np.asarray(list(cam_ids), dtype=np.int64)
    by_id = np.argsort(ids, kind="stable")
    cam_idx = by_id[np.searchsorted(ids[by_id], cam_all[rows])] if len(ids) else np.zeros(0, dtype=np.int64)
    sync, obj = sync_all[rows], obj_all[rows]
    order = np.lexsort((obj, sync, cam_idx))  # stable: rows of an object keep their order
    rows, cam_idx, sync, obj = rows[order], cam_idx[order], sync[order], obj[order]
    n = len(rows)
    new_frame = np.ones(n, dtype=bool)
    new_frame[1:] = (np.diff(cam_idx) != 0) | (np.diff(sync) != 0)
    first = np.flatnonzero(new_frame)
    frame_start = np.concatenate([first, [n]]).astype(np.int64)
    cam_frame_start = np.searchsorted(cam_idx[first], np.arange(len(ids) + 1)).astype(np.int64)
    homog_start = homog_count = None
    if split and n:
        new_group = new_frame.copy()
        new_group[1:] |= np.diff(obj) != 0
        g_first = np.flatnonzero(new_group)
        g_size = np.diff(np.concatenate([g_first, [n]]))
        g_frame = np.searchsorted(first, g_first, side="right") - 1
        best = np.lexsort((g_first, -g_size, g_frame))  # per frame: the largest group first, the lowest object_id on ties
        lead = best[np.concatenate([[True], np.diff(g_frame[best]) != 0])]
        homog_start, homog_count = g_first[lead].astype(np.int64), g_size[lead].astype(np.int32)
    return GatheredFrames(cam_frame_start, frame_start, sync[first], xy_all[rows], board_all[rows], homog_start, homog_count)


def _popcount(v) -> int:
    return bin(int(v)).count("1")


def grid_masks(grid_size: int) -> tuple[int, int]:
    """Bit masks of the edge cells (border rows and columns) and of the four corner cells of the grid."""
    g = grid_size
    edge = sum(1 << (r * g + c) for r in range(g) for c in range(g) if r in (0, g - 1) or c in (0, g - 1))
    corner = (1 << 0) | (1 << (g - 1)) | (1 << ((g - 1) * g)) | (1 << ((g - 1) * g + g - 1))
    return edge, corner


def covered_cells(mask, grid_size: int) -> set[tuple[int, int]]:
    """The (row, col) cells of a cell mask, as the reference's ``CoveredCells``."""
    m = int(mask)
    return {(b // grid_size, b % grid_size) for b in range(grid_size * grid_size) if m >> b & 1}


def _empty_report(total: int) -> IntrinsicCoverageReport:
    return IntrinsicCoverageReport([], 0.0, 0.0, 0.0, 0.0, False, 0, 0, total)


def _report(masks, poses, sync, selected, n_anchors_bins, eligible, total, grid_size, min_orientations) -> IntrinsicCoverageReport:
    """The reference's ``_compute_quality_metrics`` on the masks and pose features of the selected frames."""
    if total == 0 or eligible == 0:
        return _empty_report(total)
    edge, corner = grid_masks(grid_size)
    covered = 0
    for m in masks[selected]:
        covered |= int(m)
    diversity = float(np.mean(np.var(poses[selected], axis=0))) if len(selected) > 1 else 0.0
    if len(selected) == 0:
        return IntrinsicCoverageReport([], 0.0, 0.0, 0.0, 0.0, n_anchors_bins >= min_orientations, n_anchors_bins, eligible, total)
    return IntrinsicCoverageReport(
        selected_frames=[int(s) for s in sync[selected]], coverage_fraction=_popcount(covered) / (grid_size * grid_size),
        edge_coverage_fraction=_popcount(covered & edge) / _popcount(edge), corner_coverage_fraction=_popcount(covered & corner) / _popcount(corner),
        pose_diversity=diversity, orientation_sufficient=n_anchors_bins >= min_orientations, orientation_count=n_anchors_bins,
        eligible_frame_count=eligible, total_frame_count=total)


def select_rig(image_points, cams, *, target_frame_count=30, min_corners_per_frame=6, min_orientations=4, grid_size=5, float32_io=True,
               by_object=True, _solver=None):
    """``cams``: list of (cam_id, (width, height)).  One ``select_frames`` call for all of them; returns ``({cam_id:
    IntrinsicCoverageReport}, GatheredFrames, FrameSelection)`` — the per-frame features behind the reports for callers that screen
    frames themselves."""
    if not 1 <= int(grid_size) <= MAX_GRID_SIZE:
        raise ValueError(f"grid_size must be 1..{MAX_GRID_SIZE} (the cell mask has 64 bits), got {grid_size}")
    if int(target_frame_count) < 1:
        raise ValueError(f"target_frame_count must be at least 1, got {target_frame_count}")
    cam_ids = [c for c, _ in cams]
    gathered = gather_frames(image_points, cam_ids, by_object)
    per_cam = np.diff(gathered.cam_frame_start)
    # no camera can yield more frames than it has: the device's selection table need not be wider
    target = int(min(int(target_frame_count), max(1, int(per_cam.max()) if len(per_cam) else 1)))
    size = np.array([[float(s[0]), float(s[1])] for _, s in cams], dtype=np.float64).reshape(-1, 2)
    backend = _solver or DeviceFrameSelection()
    sel = backend.select_frames(gathered.cam_frame_start, size, gathered.frame_start, gathered.obs_xy, gathered.obs_obj, gathered.homog_start,
                                gathered.homog_count, grid_size=int(grid_size), min_corners=int(min_corners_per_frame), target_count=target,
                                float32_io=bool(float32_io))
    reports = {}
    for i, cam_id in enumerate(cam_ids):
        a, b = int(gathered.cam_frame_start[i]), int(gathered.cam_frame_start[i + 1])
        chosen = sel.selected[i, :int(sel.n_selected[i])].astype(np.int64)
        reports[cam_id] = _report(sel.cell_mask[a:b], sel.pose_features[a:b], gathered.frame_sync[a:b], chosen, int(sel.n_anchors[i]),
                                  int(sel.eligible[i]), b - a, int(grid_size), int(min_orientations))
        r = reports[cam_id]
        logger.info(f"Frame selection for cam_id {cam_id}: {len(r.selected_frames)} of {r.eligible_frame_count} eligible frames, "
                    f"{r.orientation_count} tilt directions, coverage {r.coverage_fraction:.0%}")
    return reports, gathered, sel


def select_calibration_frames(image_points, cam_id: int, image_size: tuple[int, int], *, target_frame_count: int = 30,
                              min_corners_per_frame: int = 6, min_orientations: int = 4, grid_size: int = 5, float32_io: bool = True,
                              _solver=None) -> IntrinsicCoverageReport:
    """Select the frames for the intrinsic calibration of one camera (the reference's function, ``frame_selector.py:97-209``): at
    most ``target_frame_count`` frames with at least ``min_corners_per_frame`` corners, orientation anchors first, then greedy
    coverage.  A frame is all rows of (``cam_id``, ``sync_index``), and the homography runs over all of them, as in the reference
    (a single-board table); :func:`select_camera_array_frames` fits it to the largest object of a frame."""
    reports, _, _ = select_rig(image_points, [(cam_id, image_size)], target_frame_count=target_frame_count,
                               min_corners_per_frame=min_corners_per_frame, min_orientations=min_orientations, grid_size=grid_size,
                               float32_io=float32_io, by_object=False, _solver=_solver)
    return reports[cam_id]


def rig_cameras(camera_array, only_missing: bool):
    """(cam_id, CameraData) of every camera an intrinsic rig call covers: not ignored, and with ``only_missing`` without a matrix or
    distortion coefficients.  ``ValueError`` for one without a resolution."""
    cams = []
    for cam_id, cam in sorted(camera_array.cameras.items()):
        if cam.ignore or (only_missing and cam.matrix is not None and cam.distortions is not None):
            continue
        if cam.size is None:
            raise ValueError(f"Camera {cam_id} has no resolution data: intrinsic calibration starts from the image size.")
        cams.append((cam_id, cam))
    return cams


def select_camera_array_frames(image_points, camera_array, *, target_frame_count: int = 30, min_corners_per_frame: int = 6,
                               min_orientations: int = 4, grid_size: int = 5, float32_io: bool = True, only_missing: bool = False,
                               _solver=None) -> dict[int, IntrinsicCoverageReport]:
    """Frame selection and coverage report of every non-ignored camera of ``camera_array`` (``only_missing``: only those without a
    matrix or distortion coefficients) in one device call.  Coverage, pose features and eligibility use all rows of a frame; the
    homography uses the rows of the frame's object with the most rows (lowest ``object_id`` on ties), which on a single-board session
    is the whole frame."""
    cams = [(cam_id, cam.size) for cam_id, cam in rig_cameras(camera_array, only_missing)]
    if not cams:
        return {}
    reports, _, _ = select_rig(image_points, cams, target_frame_count=target_frame_count, min_corners_per_frame=min_corners_per_frame,
                               min_orientations=min_orientations, grid_size=grid_size, float32_io=float32_io, by_object=True, _solver=_solver)
    return reports


__all__ = ["IntrinsicCoverageReport", "FrameSelection", "DeviceFrameSelection", "select_calibration_frames", "select_camera_array_frames",
           "select_rig", "gather_frames", "covered_cells", "MAX_GRID_SIZE"]
