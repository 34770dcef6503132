"""The 3-D trajectories of a whole recording in one device call.

The reference's ``reconstruction/reconstruct_xyz.py`` runs ``ImagePoints.fill_gaps`` and ``ImagePoints.triangulate`` over the tracked
2-D landmarks of a recording, and its post-processing follows with ``WorldPoints.fill_gaps`` and ``WorldPoints.smooth``.  With the
host chain of this package every stage sorts or loops over the observation table and hands a pandas frame to the next one.  Here one
call, ``cba_reconstruct_trajectories`` (``include/caliscope_trajectory.h``, ``csrc/trajectory_math.h``, ``csrc/trajectory_lib.hip``),
does all four on one dense grid: frame ``f = sync_index - sync_min``, trajectory ``j`` = rank of ``(object_id, keypoint_id)``, camera
``c`` = rank of ``cam_id`` among the cameras of the table, slot ``s = f * n_traj + j``.  The host factorises the keys with numpy,
uploads the rows, and compacts the valid slots of the result into a :class:`WorldPoints` table sorted by
``(sync_index, object_id, keypoint_id)``.

Opt-in: ``ImagePoints.fill_gaps`` / ``triangulate`` and ``WorldPoints.fill_gaps`` / ``smooth`` stay as they are, and are what this
path is tested against.  Differences from that chain, all refusals: two rows of one ``(cam_id, sync_index, object_id, keypoint_id)``
(the chain feeds both to the DLT; the grid has one cell) and a negative ``sync_index`` raise ``ValueError``; static objects
(``static_object_ids``) are not supported.  A trajectory that would reach the filter with ``3 * order < n <= 3 * (order + 1)``
samples raises ``ValueError`` before anything is launched (scipy raises there in the host chain, after the work is done).

``refine=RefineOptions(...)`` makes ``cba_reconstruct_trajectories_refined`` instead (``caliscope_amd/trajectory_refinement.py``): the
same launches with the robust reprojection refinement of every point, and the rejection of contradicting views, between the
triangulation and the 3-D fill.  ``covariance=CovarianceOptions(...)`` makes ``cba_reconstruct_trajectories_uncertain``
(``caliscope_amd/trajectory_uncertainty.py``): either of the two with the 3-D covariance of every sample.  With it,
``smoother=SmootherOptions(...)`` makes ``cba_reconstruct_trajectories_smoothed`` (``caliscope_amd/trajectory_smoother.py``): the
covariance-weighted fixed-interval smoother behind the covariance, with positions, velocities and their covariances per frame.

There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.  ``_solver`` replaces the device call (an
object with ``reconstruct``, as :class:`DeviceTrajectorySolver`, and for ``refine`` with ``reconstruct_refined``, as
``DeviceRefinedTrajectorySolver``) — the CPU test-suite passes a g++ build of the same routines.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import pandas as pd

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError
from caliscope_amd.point_data import WORLD_POINT_COLUMNS, ImagePoints, WorldPoints

MAX_ORDER = 8


class TrajDesc(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_frames", C.c_int64), ("n_traj", C.c_int64), ("n_rows", C.c_int64),
                ("cam_model", _lib.c_int32_p), ("cam_intr", _lib.c_double_p), ("cam_P", _lib.c_double_p), ("cam_posed", _lib.c_uint8_p),
                ("row_cam", _lib.c_int32_p), ("row_slot", _lib.c_int64_p), ("row_xy", _lib.c_double_p), ("row_time", _lib.c_double_p),
                ("xy_gap", C.c_int32), ("xyz_gap", C.c_int32), ("float32_io", C.c_int32), ("filter_order", C.c_int32),
                ("filter_b", _lib.c_double_p), ("filter_a", _lib.c_double_p), ("filter_zi", _lib.c_double_p), ("memory_limit", C.c_int64)]


class TrajOut(C.Structure):
    _fields_ = [("xyz", _lib.c_double_p), ("valid", _lib.c_uint8_p), ("slot_time", _lib.c_double_p), ("frame_time", _lib.c_double_p),
                ("xy_filled", _lib.c_double_p), ("ft_filled", _lib.c_double_p)]


TRAJECTORY_SIGNATURES = {
    "cba_reconstruct_trajectories": (C.c_int, [C.POINTER(TrajDesc), C.c_int32, C.POINTER(TrajOut)]),
}


@dataclass(frozen=True)
class TrajectoryGrid:
    """A recording factorised onto the dense grid of ``cba_traj_desc``.  Rows are sorted by (camera, trajectory, frame)."""

    sync_min: int
    n_frames: int
    cam_ids: np.ndarray      # [n_cams] cam_id of camera c, ascending
    traj_object: np.ndarray  # [n_traj] object_id of trajectory j
    traj_keypoint: np.ndarray
    cam_posed: np.ndarray    # [n_cams] uint8
    cam_model: np.ndarray
    cam_intr: np.ndarray
    cam_P: np.ndarray
    row_cam: np.ndarray
    row_slot: np.ndarray
    row_xy: np.ndarray
    row_time: np.ndarray

    @property
    def n_cams(self) -> int:
        return len(self.cam_ids)

    @property
    def n_traj(self) -> int:
        return len(self.traj_object)

    @property
    def n_slots(self) -> int:
        return self.n_frames * self.n_traj


@dataclass(frozen=True)
class TrajectoryResult:
    """What one ``reconstruct`` call returns; the two grids are None unless they were asked for."""

    xyz: np.ndarray         # [n_slots, 3]
    valid: np.ndarray       # [n_slots] uint8: 0 nothing, 1 triangulated, 2 filled by xyz_gap
    slot_time: np.ndarray   # [n_slots]
    frame_time: np.ndarray  # [n_frames]
    xy_filled: np.ndarray | None = None  # [n_cams, n_slots, 2]
    ft_filled: np.ndarray | None = None  # [n_cams, n_slots]


def trajectory_grid(image_points: ImagePoints, camera_array) -> TrajectoryGrid:
    """Factorise the table (vectorised: ``np.unique`` and one stable argsort).  ``ValueError`` for a negative sync index, a pixel
    that is not finite and a duplicate row, each with the row named."""
    from caliscope_amd.triangulation import camera_tables

    df = image_points._df  # read only
    sync = df["sync_index"].to_numpy(dtype=np.int64)
    cam = df["cam_id"].to_numpy(dtype=np.int64)
    obj = df["object_id"].to_numpy(dtype=np.int64)
    kp = df["keypoint_id"].to_numpy(dtype=np.int64)
    x = df["img_loc_x"].to_numpy(dtype=np.float64)
    y = df["img_loc_y"].to_numpy(dtype=np.float64)
    ft = df["frame_time"].to_numpy(dtype=np.float64)
    sync_min = int(sync.min())
    if sync_min < 0:
        raise ValueError(f"reconstruct_trajectories: row {int(np.argmax(sync < 0))} has the negative sync_index {int(sync[np.argmax(sync < 0)])} "
                         f"(static objects are not supported by this call)")
    bad = ~(np.isfinite(x) & np.isfinite(y))
    if bad.any():
        raise ValueError(f"reconstruct_trajectories: row {int(np.argmax(bad))} has a pixel position that is not finite")
    n_frames = int(sync.max()) - sync_min + 1
    cam_ids, c = np.unique(cam, return_inverse=True)
    objects, oi = np.unique(obj, return_inverse=True)
    keypoints, ki = np.unique(kp, return_inverse=True)
    pairs, j = np.unique(oi.astype(np.int64) * len(keypoints) + ki, return_inverse=True)  # ascending in (object_id, keypoint_id)
    n_traj = len(pairs)
    f = sync - sync_min
    key = (c.astype(np.int64) * n_traj + j) * n_frames + f
    order = np.argsort(key, kind="stable")
    key = key[order]
    same = np.flatnonzero(key[1:] == key[:-1])
    if same.size:
        a, b = int(order[same[0]]), int(order[same[0] + 1])
        raise ValueError(f"reconstruct_trajectories: rows {a} and {b} are duplicates (cam_id {int(cam[a])}, sync_index {int(sync[a])}, object_id "
                         f"{int(obj[a])}, keypoint_id {int(kp[a])}): the grid holds one observation per camera, frame and landmark")
    posed = camera_array.posed_cam_id_to_index
    cam_posed = np.array([1 if int(cid) in posed else 0 for cid in cam_ids], dtype=np.uint8)
    model, intr, P = np.zeros(len(cam_ids), dtype=np.int32), np.zeros((len(cam_ids), 9)), np.zeros((len(cam_ids), 12))
    at = np.flatnonzero(cam_posed)
    if at.size:
        model[at], intr[at], P[at] = camera_tables(camera_array, [int(cam_ids[i]) for i in at])
    return TrajectoryGrid(sync_min=sync_min, n_frames=n_frames, cam_ids=cam_ids, traj_object=objects[pairs // len(keypoints)],
                          traj_keypoint=keypoints[pairs % len(keypoints)], cam_posed=cam_posed, cam_model=model, cam_intr=intr, cam_P=P,
                          row_cam=np.ascontiguousarray(c[order], dtype=np.int32), row_slot=np.ascontiguousarray((f * n_traj + j)[order], dtype=np.int64),
                          row_xy=np.ascontiguousarray(np.column_stack([x[order], y[order]])), row_time=np.ascontiguousarray(ft[order]))


def filter_coefficients(smooth):
    """``(order, b, a, zi)`` of ``smooth = (fps, cutoff_freq, order)``: the Butterworth low-pass of ``WorldPoints.smooth`` and the
    steady state ``filtfilt`` starts from; ``ValueError`` for an order outside 1..8."""
    from scipy.signal import butter, lfilter_zi

    fps, cutoff, order = smooth
    if int(order) != order or not 1 <= int(order) <= MAX_ORDER:
        raise ValueError(f"reconstruct_trajectories: filter order must be in 1..{MAX_ORDER}, got {order}")
    b, a = butter(int(order), cutoff, btype="low", fs=fps, output="ba")
    return int(order), np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(lfilter_zi(b, a))


def run_trajectory_call(call, grid: TrajectoryGrid, xy_gap: int, xyz_gap: int, filt, float32_io: bool, memory_limit: int, want_grids: bool, what: str,
                        last_error) -> TrajectoryResult:
    """Fill ``cba_traj_desc`` / ``cba_traj_out``, run ``call(desc_ref, out_ref) -> code`` and collect the result (shared by the device
    binding and the test harness).  A refusal of the input (``CBA_ERR_INVALID``, ``CBA_ERR_UNSUPPORTED``) is a ``ValueError`` with the
    library's message, anything else a ``BackendError``."""
    n_slots, n_cams = grid.n_slots, grid.n_cams
    xyz, valid = np.empty((n_slots, 3)), np.zeros(n_slots, dtype=np.uint8)
    slot_time, frame_time = np.empty(n_slots), np.empty(grid.n_frames)
    xy_filled = np.empty((n_cams, n_slots, 2)) if want_grids else None
    ft_filled = np.empty((n_cams, n_slots)) if want_grids else None
    order, b, a, zi = filt if filt is not None else (0, None, None, None)
    desc = TrajDesc(n_cams=n_cams, n_frames=grid.n_frames, n_traj=grid.n_traj, n_rows=len(grid.row_cam), cam_model=_lib.ptr(grid.cam_model),
                    cam_intr=_lib.ptr(grid.cam_intr), cam_P=_lib.ptr(grid.cam_P), cam_posed=_lib.ptr(grid.cam_posed),
                    row_cam=_lib.ptr(grid.row_cam), row_slot=_lib.ptr(grid.row_slot), row_xy=_lib.ptr(grid.row_xy),
                    row_time=_lib.ptr(grid.row_time), xy_gap=int(xy_gap), xyz_gap=int(xyz_gap), float32_io=1 if float32_io else 0,
                    filter_order=order, filter_b=_lib.ptr(b), filter_a=_lib.ptr(a), filter_zi=_lib.ptr(zi),
                    memory_limit=int(memory_limit))
    out = TrajOut(xyz=_lib.ptr(xyz), valid=_lib.ptr(valid), slot_time=_lib.ptr(slot_time), frame_time=_lib.ptr(frame_time),
                  xy_filled=_lib.ptr(xy_filled), ft_filled=_lib.ptr(ft_filled))
    rc = call(C.byref(desc), C.byref(out))
    if rc in (-1, -4):
        raise ValueError(last_error())
    if rc != 0:
        raise BackendError(f"{what} failed (code {rc}): {last_error()}")
    return TrajectoryResult(xyz=xyz, valid=valid, slot_time=slot_time, frame_time=frame_time, xy_filled=xy_filled, ft_filled=ft_filled)


class DeviceTrajectorySolver:
    """The device call ``cba_reconstruct_trajectories`` on ``device_id``.  ``memory_limit`` (bytes, 0: the free device memory) is what
    the buffers of a call are checked against."""

    def __init__(self, device_id: int = 0, memory_limit: int = 0):
        self.device_id = device_id
        self.memory_limit = memory_limit

    def reconstruct(self, grid: TrajectoryGrid, *, xy_gap=0, xyz_gap=0, filt=None, float32_io=True, want_grids=False) -> TrajectoryResult:
        lib = _lib.bind(_lib.load(), TRAJECTORY_SIGNATURES)
        return run_trajectory_call(lambda d, o: lib.cba_reconstruct_trajectories(d, self.device_id, o), grid, xy_gap, xyz_gap, filt, float32_io,
                                   self.memory_limit, want_grids, "cba_reconstruct_trajectories", lambda: _lib.last_error(lib))


def _empty() -> WorldPoints:
    return WorldPoints(pd.DataFrame(columns=list(WORLD_POINT_COLUMNS) + ["frame_time"]))


def world_points_of(grid: TrajectoryGrid, result: TrajectoryResult) -> WorldPoints:
    """The valid slots as a table sorted by (sync_index, object_id, keypoint_id) (slot order)."""
    s = np.flatnonzero(result.valid)
    f, j = s // max(grid.n_traj, 1), s % max(grid.n_traj, 1)
    return WorldPoints(pd.DataFrame({
        "sync_index": f + grid.sync_min, "object_id": grid.traj_object[j], "keypoint_id": grid.traj_keypoint[j],
        "x_coord": result.xyz[s, 0], "y_coord": result.xyz[s, 1], "z_coord": result.xyz[s, 2], "frame_time": result.slot_time[s],
    }))


def reconstruct_trajectories(image_points: ImagePoints, camera_array, *, xy_gap_fill: int = 3, xyz_gap_fill: int = 0, smooth=None,
                             float32_io: bool = True, device_id: int = 0, refine=None, return_quality: bool = False, covariance=None, smoother=None, _solver=None):
    """``image_points.fill_gaps(xy_gap_fill).triangulate(camera_array)``, then ``.fill_gaps(xyz_gap_fill)`` and, for
    ``smooth = (fps, cutoff_freq, order)``, ``.smooth(*smooth)`` — in one device call.  A gap of 0 skips that fill, ``smooth=None``
    the filter.  An empty table, or one without a posed camera, gives an empty table with the ``frame_time`` column.

    ``refine`` (a :class:`caliscope_amd.trajectory_refinement.RefineOptions`) makes the call that also refines every triangulated
    point by its robust reprojection error and drops contradicting views, before the 3-D fill and the filter; the table has the
    same columns.  ``return_quality=True`` (with ``refine`` only, else ``ValueError``) returns ``(WorldPoints, DataFrame)``, the frame
    row for row beside the table: its keys, ``n_views``, ``n_rejected``, ``reproj_rms_px``, ``reproj_max_px``, ``status`` and
    ``rejected_cam_ids``.  ``_solver`` then needs ``reconstruct_refined``.

    ``covariance`` (a :class:`caliscope_amd.trajectory_uncertainty.CovarianceOptions`) makes the call, plain or refined, that also
    computes the 3-D covariance of every sample from the pixel noise ``sigma_px`` and, with ``calibration``, from the covariance of
    the camera parameters; ``camera_array`` has to be the one that report was computed at.  The result then ends with a DataFrame row
    for row beside the table (after the quality frame when ``return_quality`` is set): the keys, ``cov_xx .. cov_zz``,
    ``std_x, std_y, std_z``, ``std_major``, ``calib_share`` and ``cov_status``.  The covariance is that of the sample before the 3-D
    fill and the filter (cells the fill adds: NaN, status 2).  ``_solver`` then needs ``reconstruct_uncertain``.

    ``smoother`` (a :class:`caliscope_amd.trajectory_smoother.SmootherOptions`) needs ``covariance`` and does the jobs of
    ``xyz_gap_fill`` and ``smooth`` itself, so it refuses both (``ValueError``).  The table and the frames before it are those of the
    call without it; the result then ends with one more DataFrame, ``smoothed_frame``'s: a row per measured sample and per frame
    of a hole of at most ``max_gap`` frames, with the smoothed position, the velocity, their covariances (the pixel-noise part; the
    sample's calibration term is passed through beside it) and ``nis``.  ``_solver`` then needs ``reconstruct_smoothed``."""
    if return_quality and refine is None:
        raise ValueError("reconstruct_trajectories: return_quality needs refine (the plain call computes no quality)")
    if smoother is not None:
        if covariance is None:
            raise ValueError("reconstruct_trajectories: smoother needs covariance (it weights every sample by its own covariance)")
        if int(xyz_gap_fill) != 0:
            raise ValueError(f"reconstruct_trajectories: smoother with xyz_gap_fill = {xyz_gap_fill}: the smoother fills the holes itself (max_gap)")
        if smooth is not None:
            raise ValueError("reconstruct_trajectories: smoother with smooth: one call smooths once, by the filter or by the smoother")
    filt = filter_coefficients(smooth) if smooth is not None else None
    if covariance is not None:
        return _reconstruct_uncertain(image_points, camera_array, int(xy_gap_fill), int(xyz_gap_fill), filt, float32_io, device_id, refine,
                                      return_quality, covariance, smoother, _solver)
    if refine is None:
        if len(image_points) == 0:
            return _empty()
        grid = trajectory_grid(image_points, camera_array)
        if not grid.cam_posed.any():
            return _empty()
        solver = _solver if _solver is not None else DeviceTrajectorySolver(device_id)
        result = solver.reconstruct(grid, xy_gap=int(xy_gap_fill), xyz_gap=int(xyz_gap_fill), filt=filt, float32_io=float32_io)
        return world_points_of(grid, result)
    from caliscope_amd import trajectory_refinement as TR

    TR.refine_struct(refine)  # (an unknown loss name is refused for an empty table too)
    grid = trajectory_grid(image_points, camera_array) if len(image_points) else None
    if grid is None or not grid.cam_posed.any():
        world, quality = _empty(), pd.DataFrame(columns=list(TR.QUALITY_COLUMNS))
    else:
        solver = _solver if _solver is not None else TR.DeviceRefinedTrajectorySolver(device_id)
        result, q = solver.reconstruct_refined(grid, refine, xy_gap=int(xy_gap_fill), xyz_gap=int(xyz_gap_fill), filt=filt, float32_io=float32_io)
        world, quality = world_points_of(grid, result), TR.quality_frame(grid, result, q)
    return (world, quality) if return_quality else world


def _reconstruct_uncertain(image_points, camera_array, xy_gap, xyz_gap, filt, float32_io, device_id, refine, return_quality, covariance, smoother,
                           _solver):
    """``reconstruct_trajectories`` with ``covariance``: ``(world[, quality], covariance frame[, smoothed frame])``."""
    from caliscope_amd import trajectory_refinement as TR
    from caliscope_amd import trajectory_smoother as TS
    from caliscope_amd import trajectory_uncertainty as TU

    if refine is not None:
        TR.refine_struct(refine)
    if smoother is not None:
        TS._fields(smoother)
    grid = trajectory_grid(image_points, camera_array) if len(image_points) else None
    smoothed = pd.DataFrame(columns=list(TS.SMOOTHED_COLUMNS))
    if grid is None or not grid.cam_posed.any():
        world, quality, frame = _empty(), pd.DataFrame(columns=list(TR.QUALITY_COLUMNS)), pd.DataFrame(columns=list(TU.COVARIANCE_COLUMNS))
    elif smoother is not None:
        solver = _solver if _solver is not None else TS.DeviceTrajectorySmoother(device_id)
        result, q, cov, sm = solver.reconstruct_smoothed(grid, covariance, smoother, refine, camera_array=camera_array, xy_gap=xy_gap, xyz_gap=xyz_gap,
                                                         filt=filt, float32_io=float32_io)
        world, frame, smoothed = world_points_of(grid, result), TU.covariance_frame(grid, result, cov), TS.smoothed_frame(grid, sm, cov.cov_calib)
        quality = TR.quality_frame(grid, result, q) if refine is not None else None
    else:
        solver = _solver if _solver is not None else TU.DeviceUncertainTrajectorySolver(device_id)
        result, q, cov = solver.reconstruct_uncertain(grid, covariance, refine, camera_array=camera_array, xy_gap=xy_gap, xyz_gap=xyz_gap, filt=filt,
                                                      float32_io=float32_io)
        world, frame = world_points_of(grid, result), TU.covariance_frame(grid, result, cov)
        quality = TR.quality_frame(grid, result, q) if refine is not None else None
    head = (world, quality, frame) if return_quality else (world, frame)
    return head + (smoothed,) if smoother is not None else head


def reconstruct_xyz(image_points: ImagePoints, camera_array, name: str, output_dir, xy_gap_fill: int = 3, **kw):
    """The reference's ``reconstruct_xyz`` use case: the trajectories of a recording written to ``output_dir / xyz_{name}.csv``
    (``WorldPoints.to_csv``).  Returns the path, or None when there are no 2-D points or nothing triangulates (no file then).
    With ``covariance=CovarianceOptions(...)`` the covariance frame goes to ``xyz_{name}_covariance.csv`` beside it, and with
    ``smoother=SmootherOptions(...)`` the smoothed frame to ``xyz_{name}_smoothed.csv``."""
    if len(image_points) == 0:
        return None
    world = reconstruct_trajectories(image_points, camera_array, xy_gap_fill=xy_gap_fill, **kw)
    frame, smoothed = None, None
    if kw.get("smoother") is not None:
        world, smoothed = world[:-1], world[-1]
    if kw.get("covariance") is not None:
        world, frame = world[0], world[-1]
    if len(world) == 0:
        return None
    path = Path(output_dir) / f"xyz_{name}.csv"
    world.to_csv(path)
    if frame is not None:
        frame.to_csv(Path(output_dir) / f"xyz_{name}_covariance.csv", index=False)
    if smoothed is not None:
        smoothed.to_csv(Path(output_dir) / f"xyz_{name}_smoothed.csv", index=False)
    return path


__all__ = ["DeviceTrajectorySolver", "TrajectoryGrid", "TrajectoryResult", "TRAJECTORY_SIGNATURES", "filter_coefficients", "reconstruct_trajectories",
           "reconstruct_xyz", "run_trajectory_call", "trajectory_grid", "world_points_of"]
