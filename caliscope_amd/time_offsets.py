"""Per-camera time offsets of a recording, and the observations as synchronous cameras would have made them.

Every stage after calibration takes the rows of one ``sync_index`` as exposed at one instant.  Unsynchronised USB cameras keep two
timing errors after the grouping: a constant latency of each camera, which the timestamps do not show, and the spread of
``frame_time`` inside a group, which they show and which nothing used.  At 2 m/s and 30 fps half a frame is 33 mm.
``estimate_time_offsets(image_points, camera_array, options)`` estimates the latency ``delta_c`` of every posed camera against a
reference camera, jointly with the 3-D points at the nominal frame times ``tau_f`` (``include/caliscope/time_offsets.h``, where the
model ``X(tau + s) = X + V s``, the rounds and their limits are stated; ``csrc/time_offset_math.h``; the ``k_sync_*`` kernels of
``csrc/time_offset_lib.hip``).  ``TimeOffsets.compensated(image_points)`` returns the table with every pixel moved to where its
camera would have seen the landmark at ``tau_f``, which ``reconstruct_trajectories`` (with ``refine``, ``covariance``,
``smoother``), ``adjust_skeleton`` and ``smooth_trajectories`` take unchanged.

Limits: no acceleration term (the model error of a row is ``a s^2 / 2``); one constant offset per camera, no clock drift; the
compensated pixels are measurements to the later stages, the uncertainty of the offsets does not enter their covariances; one
device; at most 64 posed cameras.  This call fills no holes and rounds nothing to float32.  There is no CPU fallback: without the
library or a GPU the call raises ``BackendError``.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError
from caliscope_amd.point_data import ImagePoints, WorldPoints
from caliscope_amd.reconstruction import TrajDesc, TrajectoryGrid, trajectory_grid

STATUS_NONE, STATUS_REFERENCE, STATUS_ESTIMATED, STATUS_AT_LIMIT, STATUS_UNDETERMINED = 0, 1, 2, 3, 4
MAX_CAMS = 64


@dataclass(frozen=True)
class TimeOffsetOptions:
    """``reference_cam``: the ``cam_id`` whose offset is 0 (None: the lowest posed ``cam_id`` with rows).  ``huber_px``: the Huber
    threshold of the reprojection error in pixels (None: linear loss).  ``max_offset``: the bound of ``|delta_c|`` in seconds (None:
    one median frame interval).  ``max_neighbour_gap``: how many frames away the neighbours of the velocity may lie.  ``min_rows``:
    a camera with fewer rows in moving slots is undetermined.  ``tol``: the rounds stop when no offset changed by more, seconds
    (None: 1e-6 of the median frame interval).  ``max_rounds``: the most rounds."""

    reference_cam: int | None = None
    huber_px: float | None = None
    max_offset: float | None = None
    max_neighbour_gap: int = 1
    min_rows: int = 30
    tol: float | None = None
    max_rounds: int = 10


class TimeOffsetOptionsStruct(C.Structure):
    _fields_ = [("reference_cam", C.c_int32), ("max_neighbour_gap", C.c_int32), ("min_rows", C.c_int32), ("max_rounds", C.c_int32),
                ("huber_px", C.c_double), ("max_offset", C.c_double), ("tol", C.c_double)]


class TimeOffsetOut(C.Structure):
    _fields_ = [("offsets", _lib.c_double_p), ("sigma", _lib.c_double_p), ("status", _lib.c_uint8_p), ("rms_before", _lib.c_double_p),
                ("rms_after", _lib.c_double_p), ("rows", _lib.c_int64_p), ("sigma0_px", _lib.c_double_p), ("rounds", _lib.c_int32_p),
                ("converged", _lib.c_uint8_p), ("xyz", _lib.c_double_p), ("valid", _lib.c_uint8_p), ("velocity", _lib.c_double_p),
                ("frame_time", _lib.c_double_p), ("row_xy", _lib.c_double_p), ("row_used", _lib.c_uint8_p)]


TIME_OFFSET_SIGNATURES = {
    "cba_estimate_time_offsets": (C.c_int, [C.POINTER(TrajDesc), C.POINTER(TimeOffsetOptionsStruct), C.c_int32, C.POINTER(TimeOffsetOut)]),
}


def options_struct(options: TimeOffsetOptions, grid: TrajectoryGrid | None) -> TimeOffsetOptionsStruct:
    """The options as the library takes them: None becomes the library's "default" (0, camera -1), a value that is given has to
    be a positive number; ``reference_cam`` is looked up among the cameras of the table.  ``ValueError`` names the field."""
    what = "estimate_time_offsets"
    out = {}
    for name in ("huber_px", "max_offset", "tol"):
        v = getattr(options, name)
        if v is None:
            out[name] = 0.0
            continue
        try:
            v = float(v)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"{what}: {name} is not a number: {exc}") from exc
        if not np.isfinite(v) or v <= 0.0:
            raise ValueError(f"{what}: {name} must be finite and positive, got {v}")
        out[name] = v
    for name in ("max_neighbour_gap", "min_rows", "max_rounds"):
        v = getattr(options, name)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{what}: {name} must be an integer of at least 1, got {v!r}")
        out[name] = int(v)
    ref = -1
    if options.reference_cam is not None:
        ids = [] if grid is None else [int(c) for c in grid.cam_ids]
        if int(options.reference_cam) not in ids:
            raise ValueError(f"{what}: reference camera {options.reference_cam} has no rows")
        ref = ids.index(int(options.reference_cam))
    return TimeOffsetOptionsStruct(reference_cam=ref, **out)


@dataclass(frozen=True)
class TimeOffsetResult:
    """What one call returns, on the grid: per camera of the grid, per slot, per frame and per row (in the grid's row order)."""

    offsets: np.ndarray     # [n_cams] seconds, NaN: status 0 or 4
    sigma: np.ndarray       # [n_cams]
    status: np.ndarray      # [n_cams] uint8
    rms_before: np.ndarray  # [n_cams] px
    rms_after: np.ndarray   # [n_cams]
    rows: np.ndarray        # [n_cams] int64
    sigma0_px: float
    rounds: int
    converged: bool
    xyz: np.ndarray         # [n_slots, 3]
    valid: np.ndarray       # [n_slots] uint8
    velocity: np.ndarray    # [n_slots, 3]
    frame_time: np.ndarray  # [n_frames]
    row_xy: np.ndarray      # [n_rows, 2]
    row_used: np.ndarray    # [n_rows] uint8


FIELDS = ("offsets", "sigma", "status", "rms_before", "rms_after", "rows", "xyz", "valid", "velocity", "frame_time", "row_xy", "row_used")


def run_time_offset_call(call, grid: TrajectoryGrid, options: TimeOffsetOptionsStruct, memory_limit: int, last_error,
                         what: str = "cba_estimate_time_offsets") -> TimeOffsetResult:
    """Fill ``cba_traj_desc`` / ``cba_time_offset_out``, run ``call(desc_ref, options_ref, out_ref) -> code`` and collect the result
    (shared by the device binding and the test harness).  A refusal of the input is a ``ValueError`` with the library's message,
    anything else a ``BackendError``."""
    n_slots, n_cams, n_rows = grid.n_slots, grid.n_cams, len(grid.row_cam)
    a = dict(offsets=np.full(n_cams, np.nan), sigma=np.full(n_cams, np.nan), status=np.zeros(n_cams, dtype=np.uint8),
             rms_before=np.full(n_cams, np.nan), rms_after=np.full(n_cams, np.nan), rows=np.zeros(n_cams, dtype=np.int64),
             sigma0_px=np.full(1, np.nan), rounds=np.zeros(1, dtype=np.int32), converged=np.zeros(1, dtype=np.uint8),
             xyz=np.full((n_slots, 3), np.nan), valid=np.zeros(n_slots, dtype=np.uint8), velocity=np.zeros((n_slots, 3)),
             frame_time=np.full(grid.n_frames, np.nan), row_xy=np.empty((n_rows, 2)), row_used=np.zeros(n_rows, dtype=np.uint8))
    desc = TrajDesc(n_cams=n_cams, n_frames=grid.n_frames, n_traj=grid.n_traj, n_rows=n_rows, cam_model=_lib.ptr(grid.cam_model),
                    cam_intr=_lib.ptr(grid.cam_intr), cam_P=_lib.ptr(grid.cam_P), cam_posed=_lib.ptr(grid.cam_posed), row_cam=_lib.ptr(grid.row_cam),
                    row_slot=_lib.ptr(grid.row_slot), row_xy=_lib.ptr(grid.row_xy), row_time=_lib.ptr(grid.row_time), xy_gap=0, xyz_gap=0, float32_io=0,
                    filter_order=0, filter_b=None, filter_a=None, filter_zi=None, memory_limit=int(memory_limit))
    out = TimeOffsetOut(**{name: _lib.ptr(a[name]) for name, _ in TimeOffsetOut._fields_})
    rc = call(C.byref(desc), C.byref(options), C.byref(out))
    if rc in (-1, -4):
        raise ValueError(last_error())
    if rc != 0:
        raise BackendError(f"{what} failed (code {rc}): {last_error()}")
    a["sigma0_px"], a["rounds"], a["converged"] = float(a["sigma0_px"][0]), int(a["rounds"][0]), bool(a["converged"][0])
    return TimeOffsetResult(**a)


class DeviceTimeOffsetSolver:
    """The device call ``cba_estimate_time_offsets`` on ``device_id``.  ``memory_limit`` (bytes, 0: the free device memory) is what the
    buffers of a call are checked against."""

    def __init__(self, device_id: int = 0, memory_limit: int = 0):
        self.device_id = device_id
        self.memory_limit = memory_limit

    def estimate(self, grid: TrajectoryGrid, options: TimeOffsetOptionsStruct) -> TimeOffsetResult:
        lib = _lib.bind(_lib.load(), TIME_OFFSET_SIGNATURES)
        return run_time_offset_call(lambda d, o, r: lib.cba_estimate_time_offsets(d, o, self.device_id, r), grid, options, self.memory_limit,
                                    lambda: _lib.last_error(lib))


_KEYS = ("cam_id", "sync_index", "object_id", "keypoint_id")


@dataclass(frozen=True)
class TimeOffsets:
    """``offsets``, ``sigma``, ``status``, ``rms_before``, ``rms_after``, ``rows``: dicts by ``cam_id`` (offsets and sigma in seconds,
    NaN for a camera that is unposed or undetermined; status ``STATUS_*``; RMS reprojection error in pixels at the synchronous start
    and at the end).  ``sigma0_px``: the a-posteriori pixel sigma.  ``world``: the trajectories at the nominal frame times, with
    ``frame_time`` as ``reconstruct_trajectories`` returns it."""

    offsets: dict
    sigma: dict
    status: dict
    rms_before: dict
    rms_after: dict
    rows: dict
    sigma0_px: float
    rounds: int
    converged: bool
    world: WorldPoints
    grid: TrajectoryGrid | None = field(default=None, repr=False)
    result: TimeOffsetResult | None = field(default=None, repr=False)

    def compensated(self, image_points: ImagePoints) -> ImagePoints:
        """The table the offsets were estimated from, with ``img_loc_x``, ``img_loc_y`` of every row in use replaced by the pixel its
        camera would have seen at the nominal frame time, and ``frame_time`` of every row set to that time; the rows that were not
        in use (an unposed camera, a slot without a point) keep their pixels.  ``ValueError`` for another table."""
        df = image_points.df
        if self.grid is None:
            if len(df):
                raise ValueError("TimeOffsets.compensated: not the table the offsets were estimated from (that one was empty)")
            return image_points
        g, r = self.grid, self.result
        if len(df) != len(g.row_cam):
            raise ValueError(f"TimeOffsets.compensated: the table has {len(df)} rows, the one the offsets were estimated from {len(g.row_cam)}")
        c = np.searchsorted(g.cam_ids, df["cam_id"].to_numpy(dtype=np.int64))
        f = df["sync_index"].to_numpy(dtype=np.int64) - g.sync_min
        keys = np.stack([g.traj_object, g.traj_keypoint], axis=1)
        table = {(int(o), int(k)): j for j, (o, k) in enumerate(keys)}
        try:
            j = np.array([table[(int(o), int(k))] for o, k in zip(df["object_id"], df["keypoint_id"])], dtype=np.int64)
        except KeyError as exc:
            raise ValueError(f"TimeOffsets.compensated: not the table the offsets were estimated from: no landmark {exc}") from exc
        ok = (c < len(g.cam_ids)) & (f >= 0) & (f < g.n_frames)
        key = (np.minimum(c, len(g.cam_ids) - 1) * g.n_traj + j) * g.n_frames + np.clip(f, 0, g.n_frames - 1)
        grid_key = (g.row_cam.astype(np.int64) * g.n_traj + g.row_slot % g.n_traj) * g.n_frames + g.row_slot // g.n_traj  # ascending
        at = np.searchsorted(grid_key, key)
        at = np.minimum(at, len(grid_key) - 1)
        if not ok.all() or not np.array_equal(grid_key[at], key) or not np.array_equal(g.cam_ids[np.minimum(c, len(g.cam_ids) - 1)], df["cam_id"]):
            raise ValueError("TimeOffsets.compensated: not the table the offsets were estimated from: a row has no cell of the grid")
        df["img_loc_x"] = r.row_xy[at, 0]
        df["img_loc_y"] = r.row_xy[at, 1]
        df["frame_time"] = r.frame_time[f]
        return ImagePoints(df)


def apply_time_offsets(image_points: ImagePoints, offsets) -> ImagePoints:
    """``frame_time + delta_c`` for every row of a camera with a finite offset (``offsets``: a dict by ``cam_id`` or a
    :class:`TimeOffsets`), nothing else: for users who run the sync mapping again on corrected times."""
    table = offsets.offsets if isinstance(offsets, TimeOffsets) else offsets
    df = image_points.df
    shift = np.array([table.get(int(c), np.nan) for c in df["cam_id"]], dtype=np.float64)
    df["frame_time"] = df["frame_time"].to_numpy(dtype=np.float64) + np.where(np.isfinite(shift), shift, 0.0)
    return ImagePoints(df)


def _by_cam(grid, values, cast):
    return {int(c): cast(v) for c, v in zip(grid.cam_ids, values)}


def time_offsets_of(grid: TrajectoryGrid, result: TimeOffsetResult) -> TimeOffsets:
    """The result of a call as the public object."""
    from caliscope_amd.reconstruction import TrajectoryResult, world_points_of

    slot_time = np.where(result.valid != 0, np.repeat(result.frame_time, grid.n_traj), np.nan)
    world = world_points_of(grid, TrajectoryResult(xyz=result.xyz, valid=result.valid, slot_time=slot_time, frame_time=result.frame_time))
    return TimeOffsets(offsets=_by_cam(grid, result.offsets, float), sigma=_by_cam(grid, result.sigma, float), status=_by_cam(grid, result.status, int),
                       rms_before=_by_cam(grid, result.rms_before, float), rms_after=_by_cam(grid, result.rms_after, float),
                       rows=_by_cam(grid, result.rows, int), sigma0_px=result.sigma0_px, rounds=result.rounds, converged=result.converged, world=world,
                       grid=grid, result=result)


def estimate_time_offsets(image_points: ImagePoints, camera_array, options: TimeOffsetOptions = TimeOffsetOptions(), *, device_id: int = 0,
                          memory_limit: int = 0, _solver=None) -> TimeOffsets:
    """Estimate the time offset of every posed camera of the table against the reference camera, with the trajectories at the nominal
    frame times.  The grid is that of ``reconstruct_trajectories`` (``reconstruction.trajectory_grid``).  An empty table gives an empty
    result.  ``ValueError``: options that are not positive numbers, a reference camera without rows or without a pose, a
    ``frame_time`` that is not finite, frames whose mean times do not increase, more than 64 posed cameras, buffers beyond
    ``memory_limit``, and what ``trajectory_grid`` refuses.  ``_solver`` replaces the device call (an object with ``estimate``, as
    :class:`DeviceTimeOffsetSolver`) — the CPU test-suite passes a g++ build of the same routines."""
    from caliscope_amd.reconstruction import _empty

    if len(image_points) == 0:
        options_struct(options, None)
        return TimeOffsets(offsets={}, sigma={}, status={}, rms_before={}, rms_after={}, rows={}, sigma0_px=float("nan"), rounds=0, converged=False,
                           world=_empty())
    grid = trajectory_grid(image_points, camera_array)
    opts = options_struct(options, grid)
    solver = _solver if _solver is not None else DeviceTimeOffsetSolver(device_id, memory_limit)
    return time_offsets_of(grid, solver.estimate(grid, opts))


__all__ = ["DeviceTimeOffsetSolver", "FIELDS", "MAX_CAMS", "STATUS_AT_LIMIT", "STATUS_ESTIMATED", "STATUS_NONE", "STATUS_REFERENCE", "STATUS_UNDETERMINED",
           "TIME_OFFSET_SIGNATURES", "TimeOffsetOptions", "TimeOffsetOptionsStruct", "TimeOffsetOut", "TimeOffsetResult", "TimeOffsets",
           "apply_time_offsets", "estimate_time_offsets", "options_struct", "run_time_offset_call", "time_offsets_of"]
