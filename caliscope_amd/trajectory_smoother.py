"""Covariance-weighted fixed-interval smoothing of reconstructed trajectories: position, velocity and their covariances per frame.

``reconstruct_trajectories(..., covariance=CovarianceOptions(...))`` gives every sample its 3 x 3 covariance; the Butterworth filter
(``smooth=``) does not use it, fills no hole, returns no velocity, and the covariance does not describe what it returns.  The
smoother here does: a Kalman filter forward and a modified Bryson-Frazier pass backward per trajectory under a white-noise-acceleration
model, the measurement noise of a sample its own covariance (``include/caliscope/trajectory_smoother.h``, where the model, the
recursion and its limits are stated; ``csrc/trajectory_smooth_math.h``; ``k_traj_smooth`` of ``csrc/trajectory_lib.hip``).  It gives
the exact posterior mean and covariance of position and velocity at every frame of a trajectory's span, inside holes too, and the
normalised innovation squared of every sample, whose mean is 3 when ``sigma_px`` and ``accel_density`` describe the data.

``reconstruct_trajectories(..., covariance=..., smoother=SmootherOptions(fps, accel_density))`` makes
``cba_reconstruct_trajectories_smoothed``: the uncertain call with one more kernel, and ``smoothed_frame``'s table as the last
element of its result.  ``smooth_trajectories(world, covariance_frame, options)`` runs the smoother alone
(``cba_smooth_trajectories``) on a table and its covariance frame, for instance an ``xyz_*.csv`` and its ``xyz_*_covariance.csv``.

Limits: the smoothed covariance is the pixel-noise part alone.  The calibration term is common to all frames, does not average out
and is not carried through time; ``cov_calib_*`` passes the sample's own through.  No innovation gating (``refine=`` rejects views
before the smoother), frames ``1 / fps`` apart, one device.  One thread per trajectory runs a serial recurrence: the kernel is bound
by latency, not by throughput.  There is no CPU fallback: without the library or a GPU the calls raise ``BackendError``.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import pandas as pd

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError
from caliscope_amd.reconstruction import TrajDesc, TrajOut
from caliscope_amd.trajectory_refinement import TrajQuality, TrajRefine
from caliscope_amd.trajectory_uncertainty import (COV_OK, TrajCovOut, TrajUncertainty, UncertaintyTables, full_matrices, run_uncertain_call,
                                                  uncertainty_tables)

SMOOTH_NONE, SMOOTH_MEASURED, SMOOTH_INTERPOLATED = 0, 1, 2
_COV = ("xx", "xy", "xz", "yy", "yz", "zz")


@dataclass(frozen=True)
class SmootherOptions:
    """``fps``: frames per second of the recording (consecutive ``sync_index`` are ``1 / fps`` apart).  ``accel_density``: the
    white-noise acceleration of the motion model in world units / s^1.5; the larger, the closer the result follows the samples.
    ``velocity_prior_std``: standard deviation of the velocity at a trajectory's first sample, world units / s.  ``max_gap``: an
    unmeasured frame gets a row when its hole is at most this many frames long."""

    fps: float
    accel_density: float
    velocity_prior_std: float = 10.0
    max_gap: int = 3


class TrajSmoother(C.Structure):
    _fields_ = [("fps", C.c_double), ("accel_density", C.c_double), ("velocity_prior_std", C.c_double), ("max_gap", C.c_int32)]


class SmoothDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int64), ("n_traj", C.c_int64), ("xyz", _lib.c_double_p), ("meas_cov", _lib.c_double_p), ("measured", _lib.c_uint8_p),
                ("fps", C.c_double), ("accel_density", C.c_double), ("velocity_prior_std", C.c_double), ("max_gap", C.c_int32),
                ("memory_limit", C.c_int64)]


class TrajSmoothOut(C.Structure):
    _fields_ = [("pos", _lib.c_double_p), ("vel", _lib.c_double_p), ("pos_cov", _lib.c_double_p), ("vel_cov", _lib.c_double_p), ("nis", _lib.c_double_p),
                ("status", _lib.c_uint8_p), ("meas_cov", _lib.c_double_p)]


TRAJ_SMOOTHER_SIGNATURES = {
    "cba_smooth_trajectories": (C.c_int, [C.POINTER(SmoothDesc), C.c_int32, C.POINTER(TrajSmoothOut)]),
    "cba_reconstruct_trajectories_smoothed": (C.c_int, [C.POINTER(TrajDesc), C.POINTER(TrajRefine), C.POINTER(TrajUncertainty), C.POINTER(TrajSmoother),
                                                        C.c_int32, C.POINTER(TrajOut), C.POINTER(TrajQuality), C.POINTER(TrajCovOut),
                                                        C.POINTER(TrajSmoothOut)]),
}


@dataclass(frozen=True)
class SmoothedTrajectories:
    """Per slot of the grid; covariance rows are xx xy xz yy yz zz.  Rows of ``status`` 0 are NaN, rows of 1 and 2 never."""

    pos: np.ndarray       # [n_slots, 3]
    vel: np.ndarray       # [n_slots, 3] world units / s
    pos_cov: np.ndarray   # [n_slots, 6]
    vel_cov: np.ndarray   # [n_slots, 6]
    nis: np.ndarray       # [n_slots] NaN at a trajectory's first sample and at unmeasured frames
    status: np.ndarray    # [n_slots] uint8: 0 nothing, 1 measured and smoothed, 2 interpolated
    meas_cov: np.ndarray | None = None  # [n_slots, 6] the R of the smoothed reconstruction (NaN where not measured); None for the stand-alone call


def _fields(options: SmootherOptions) -> dict:
    try:
        return dict(fps=float(options.fps), accel_density=float(options.accel_density), velocity_prior_std=float(options.velocity_prior_std),
                    max_gap=int(options.max_gap))
    except (AttributeError, TypeError, ValueError) as exc:
        raise ValueError(f"smoother options are not numbers: {exc}") from exc


def _outputs(n_slots: int, with_meas_cov: bool):
    out = SmoothedTrajectories(pos=np.full((n_slots, 3), np.nan), vel=np.full((n_slots, 3), np.nan), pos_cov=np.full((n_slots, 6), np.nan),
                               vel_cov=np.full((n_slots, 6), np.nan), nis=np.full(n_slots, np.nan), status=np.zeros(n_slots, dtype=np.uint8),
                               meas_cov=np.full((n_slots, 6), np.nan) if with_meas_cov else None)
    so = TrajSmoothOut(pos=_lib.ptr(out.pos), vel=_lib.ptr(out.vel), pos_cov=_lib.ptr(out.pos_cov), vel_cov=_lib.ptr(out.vel_cov), nis=_lib.ptr(out.nis),
                       status=_lib.ptr(out.status), meas_cov=_lib.ptr(out.meas_cov))
    return out, so


def run_smooth_call(call, n_frames: int, n_traj: int, xyz, meas_cov, measured, options: SmootherOptions, memory_limit: int, last_error,
                    what: str = "cba_smooth_trajectories") -> SmoothedTrajectories:
    """Fill ``cba_smooth_desc`` / ``cba_traj_smooth_out``, run ``call(desc_ref, out_ref) -> code`` and collect the result (shared by the
    device binding and the test harness).  A refusal of the input is a ``ValueError`` with the library's message."""
    n_slots = int(n_frames) * int(n_traj)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(n_slots, 3)
    meas_cov = np.ascontiguousarray(meas_cov, dtype=np.float64).reshape(n_slots, 6)
    measured = np.ascontiguousarray(measured, dtype=np.uint8).reshape(n_slots)
    out, so = _outputs(n_slots, False)
    desc = SmoothDesc(n_frames=int(n_frames), n_traj=int(n_traj), xyz=_lib.ptr(xyz), meas_cov=_lib.ptr(meas_cov), measured=_lib.ptr(measured),
                      memory_limit=int(memory_limit), **_fields(options))
    rc = call(C.byref(desc), C.byref(so))
    if rc in (-1, -4):
        raise ValueError(last_error())
    if rc != 0:
        raise BackendError(f"{what} failed (code {rc}): {last_error()}")
    return out


def run_smoothed_call(call, grid, tables: UncertaintyTables, options: SmootherOptions, refine, xy_gap: int, xyz_gap: int, filt, float32_io: bool,
                      memory_limit: int, want_grids: bool, last_error, what: str = "cba_reconstruct_trajectories_smoothed"):
    """``run_uncertain_call`` with the smoother's two structures: ``call(desc_ref, refine_ref, uncertainty_ref, smoother_ref, out_ref,
    quality_ref, cov_ref, smooth_ref) -> code``.  Returns ``(TrajectoryResult, TrajectoryQuality | None, TrajectoryCovariance,
    SmoothedTrajectories)``."""
    out, so = _outputs(grid.n_slots, True)
    sm = TrajSmoother(**_fields(options))
    result, quality, cov = run_uncertain_call(lambda d, r, u, o, q, c: call(d, r, u, C.byref(sm), o, q, c, C.byref(so)), grid, tables, refine, xy_gap,
                                              xyz_gap, filt, float32_io, memory_limit, want_grids, what, last_error)
    return result, quality, cov, out


class DeviceTrajectorySmoother:
    """The device calls ``cba_smooth_trajectories`` and ``cba_reconstruct_trajectories_smoothed`` on ``device_id``; ``memory_limit``
    (bytes, 0: the free device memory) is what the buffers of a call are checked against."""

    def __init__(self, device_id: int = 0, memory_limit: int = 0):
        self.device_id = device_id
        self.memory_limit = memory_limit

    def smooth(self, n_frames: int, n_traj: int, xyz, meas_cov, measured, options: SmootherOptions) -> SmoothedTrajectories:
        """The smoother alone on ``xyz [n_slots, 3]``, ``meas_cov [n_slots, 6]`` and ``measured [n_slots]`` (1: measured), slot
        ``s = f * n_traj + j``."""
        lib = _lib.bind(_lib.load(), TRAJ_SMOOTHER_SIGNATURES)
        return run_smooth_call(lambda d, o: lib.cba_smooth_trajectories(d, self.device_id, o), n_frames, n_traj, xyz, meas_cov, measured, options,
                               self.memory_limit, lambda: _lib.last_error(lib))

    def reconstruct_smoothed(self, grid, covariance, options: SmootherOptions, refine=None, *, camera_array=None, xy_gap=0, xyz_gap=0, filt=None,
                             float32_io=True, want_grids=False):
        """``(TrajectoryResult, TrajectoryQuality | None, TrajectoryCovariance, SmoothedTrajectories)``; ``covariance`` as the
        ``options`` of ``DeviceUncertainTrajectorySolver.reconstruct_uncertain``."""
        tables = covariance if isinstance(covariance, UncertaintyTables) else uncertainty_tables(grid, camera_array, covariance)
        lib = _lib.bind(_lib.load(), TRAJ_SMOOTHER_SIGNATURES)
        return run_smoothed_call(lambda d, r, u, m, o, q, c, s: lib.cba_reconstruct_trajectories_smoothed(d, r, u, m, self.device_id, o, q, c, s), grid,
                                 tables, options, refine, xy_gap, xyz_gap, filt, float32_io, self.memory_limit, want_grids, lambda: _lib.last_error(lib))


SMOOTHED_COLUMNS = ("sync_index", "object_id", "keypoint_id", "x", "y", "z", "vx", "vy", "vz", *(f"cov_{c}" for c in _COV), "std_x", "std_y", "std_z",
                    "std_major", *(f"vcov_{c}" for c in _COV), "nis", *(f"cov_calib_{c}" for c in _COV), "smooth_status")


def smoothed_frame(grid, smoothed: SmoothedTrajectories, cov_calib=None) -> pd.DataFrame:
    """One row per slot with a result (``smooth_status`` 1 or 2), in slot order (``sync_index``, then ``object_id``, ``keypoint_id``):
    the keys, the smoothed position ``x y z`` and velocity ``vx vy vz`` (world units / s), ``cov_xx .. cov_zz`` of the position with
    ``std_x, std_y, std_z`` and ``std_major`` (root of the largest eigenvalue), ``vcov_xx .. vcov_zz`` of the velocity, ``nis`` (NaN at
    a trajectory's first sample and in holes), ``cov_calib_xx .. cov_calib_zz`` and ``smooth_status``.  The covariances are the
    pixel-noise part; ``cov_calib`` (``[n_slots, 6]`` or None) is the calibration term of the samples, passed through as it is for
    status 1 and NaN for status 2.  ``grid`` needs ``sync_min``, ``n_traj``, ``traj_object`` and ``traj_keypoint``."""
    s = np.flatnonzero(smoothed.status)
    f, j = s // max(grid.n_traj, 1), s % max(grid.n_traj, 1)
    status = smoothed.status[s]
    pos_cov = smoothed.pos_cov[s]
    major = np.sqrt(np.maximum(np.linalg.eigvalsh(full_matrices(pos_cov))[:, -1], 0.0)) if len(s) else np.zeros(0)
    calib = np.full((len(s), 6), np.nan)
    if cov_calib is not None:
        calib[status == SMOOTH_MEASURED] = np.asarray(cov_calib)[s[status == SMOOTH_MEASURED]]
    frame = {"sync_index": f + grid.sync_min, "object_id": np.asarray(grid.traj_object)[j], "keypoint_id": np.asarray(grid.traj_keypoint)[j]}
    frame.update({name: smoothed.pos[s, i] for i, name in enumerate("xyz")})
    frame.update({f"v{name}": smoothed.vel[s, i] for i, name in enumerate("xyz")})
    frame.update({f"cov_{c}": pos_cov[:, i] for i, c in enumerate(_COV)})
    frame.update({"std_x": np.sqrt(pos_cov[:, 0]), "std_y": np.sqrt(pos_cov[:, 3]), "std_z": np.sqrt(pos_cov[:, 5]), "std_major": major})
    frame.update({f"vcov_{c}": smoothed.vel_cov[s, i] for i, c in enumerate(_COV)})
    frame["nis"] = smoothed.nis[s]
    frame.update({f"cov_calib_{c}": calib[:, i] for i, c in enumerate(_COV)})
    frame["smooth_status"] = status.astype(np.int64)
    return pd.DataFrame(frame, columns=list(SMOOTHED_COLUMNS))


@dataclass(frozen=True)
class _Keys:
    sync_min: int
    n_frames: int
    traj_object: np.ndarray
    traj_keypoint: np.ndarray

    @property
    def n_traj(self) -> int:
        return len(self.traj_object)


def smooth_trajectories(world, covariance_frame: pd.DataFrame, options: SmootherOptions, *, device_id: int = 0, _solver=None) -> pd.DataFrame:
    """The smoother alone on a table of 3-D points (``WorldPoints``) and the covariance frame that goes with it row for row, as
    ``reconstruct_trajectories(..., covariance=...)`` returns them and ``reconstruct_xyz`` writes them: measured are the rows with
    ``cov_status`` 1, their ``R`` the rows ``cov_xx .. cov_zz``.  That is the whole covariance of the frame: smooth a recording made
    with ``CovarianceOptions(calibration=None)`` (or one whose ``calib_share`` is small) to weight by the pixel noise alone.  The
    points must be those the covariance was computed for: no ``xyz_gap_fill``, no ``smooth``.  Returns ``smoothed_frame``'s table
    (``cov_calib_*`` is passed through from columns of that name when the frame has them).  ``ValueError``: tables of different
    length or keys, and what the library refuses.  ``_solver`` replaces the device call (an object with ``smooth``, as
    :class:`DeviceTrajectorySmoother`)."""
    _fields(options)
    df = world._df
    if len(df) != len(covariance_frame):
        raise ValueError(f"smooth_trajectories: the table has {len(df)} rows and the covariance frame {len(covariance_frame)}: they go row for row")
    sync, obj, kp = (df[c].to_numpy(dtype=np.int64) for c in ("sync_index", "object_id", "keypoint_id"))
    for name, mine in (("sync_index", sync), ("object_id", obj), ("keypoint_id", kp)):
        if not np.array_equal(mine, covariance_frame[name].to_numpy(dtype=np.int64)):
            raise ValueError(f"smooth_trajectories: the covariance frame is not that of the table: {name} differs")
    if len(df) == 0:
        return pd.DataFrame(columns=list(SMOOTHED_COLUMNS))
    if sync.min() < 0:
        raise ValueError(f"smooth_trajectories: row {int(np.argmax(sync < 0))} has a negative sync_index (static objects are not supported)")
    objects, oi = np.unique(obj, return_inverse=True)
    keypoints, ki = np.unique(kp, return_inverse=True)
    pairs, j = np.unique(oi.astype(np.int64) * len(keypoints) + ki, return_inverse=True)
    keys = _Keys(sync_min=int(sync.min()), n_frames=int(sync.max() - sync.min()) + 1, traj_object=objects[pairs // len(keypoints)],
                 traj_keypoint=keypoints[pairs % len(keypoints)])
    s = (sync - keys.sync_min) * keys.n_traj + j
    if len(np.unique(s)) != len(s):
        raise ValueError("smooth_trajectories: two rows of one (sync_index, object_id, keypoint_id)")
    n_slots = keys.n_frames * keys.n_traj
    xyz, meas_cov, measured = np.full((n_slots, 3), np.nan), np.full((n_slots, 6), np.nan), np.zeros(n_slots, dtype=np.uint8)
    xyz[s] = df[["x_coord", "y_coord", "z_coord"]].to_numpy(dtype=np.float64)
    meas_cov[s] = covariance_frame[[f"cov_{c}" for c in _COV]].to_numpy(dtype=np.float64)
    measured[s] = covariance_frame["cov_status"].to_numpy() == COV_OK
    calib = None
    if all(f"cov_calib_{c}" in covariance_frame for c in _COV):
        calib = np.full((n_slots, 6), np.nan)
        calib[s] = covariance_frame[[f"cov_calib_{c}" for c in _COV]].to_numpy(dtype=np.float64)
    solver = _solver if _solver is not None else DeviceTrajectorySmoother(device_id)
    return smoothed_frame(keys, solver.smooth(keys.n_frames, keys.n_traj, xyz, meas_cov, measured, options), calib)


__all__ = ["DeviceTrajectorySmoother", "SMOOTHED_COLUMNS", "SmoothDesc", "SmoothedTrajectories", "SmootherOptions", "TRAJ_SMOOTHER_SIGNATURES",
           "TrajSmoothOut", "TrajSmoother", "run_smooth_call", "run_smoothed_call", "smooth_trajectories", "smoothed_frame"]
