"""Adjustment of reconstructed trajectories to the constant segment lengths of a skeleton, frame by frame, weighted by covariance.

``reconstruct_trajectories(..., covariance=CovarianceOptions(...))`` gives every sample its 3 x 3 covariance, and every stage up to
there treats a landmark on its own.  The landmarks of one subject sit on a skeleton whose segments do not change length.
``adjust_skeleton(world, covariance_frame, skeleton, options)`` estimates the length of every segment of every subject over the
recording (an exact median, then a trimmed inverse-variance mean) and adjusts the measured points of every frame to them by
Levenberg-Marquardt on ``sum e^T R^-1 e + sum ((|Xa - Xb| - L) / sigma)^2``, one workgroup per (frame, subject)
(``include/caliscope/trajectory_skeleton.h``, where the mathematics and its limits are stated; ``csrc/trajectory_skeleton_math.h``;
``k_skel_length`` and ``k_skel_adjust`` of ``csrc/skeleton_lib.hip``).  It returns the table and the covariance frame that
``smooth_trajectories`` takes as they are: the adjustment uses the covariance across the points of a frame, the smoother the one
across time.

Limits: the cross-covariances between the points of a frame are not returned; no robust loss or gating on the segment rows
(``w_before`` reports a mistracked end, nothing removes it); no joint-angle limits; nothing through time; at most 54 landmarks in a
connected skeleton.  There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Mapping

import numpy as np
import pandas as pd

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError
from caliscope_amd.trajectory_uncertainty import COV_OK, COVARIANCE_COLUMNS, full_matrices

SLOT_NONE, SLOT_ADJUSTED, SLOT_INACTIVE, SLOT_FAILED = 0, 1, 2, 3
COMP_NONE, COMP_CONVERGED, COMP_MAX_ITER, COMP_FAILED = 0, 1, 2, 3
MAX_POINTS = 54
_COV = ("xx", "xy", "xz", "yy", "yz", "zz")


@dataclass(frozen=True)
class Skeleton:
    """``segments``: ``(name, keypoint_a, keypoint_b)`` triples, the keypoints as ``keypoint_id``."""

    segments: tuple

    def __post_init__(self):
        object.__setattr__(self, "segments", tuple((str(n), int(a), int(b)) for n, a, b in self.segments))
        names = [n for n, _, _ in self.segments]
        if len(set(names)) != len(names):
            raise ValueError("Skeleton: two segments of one name")

    @classmethod
    def from_wireframe_toml(cls, path, point_names: Mapping) -> "Skeleton":
        """A wireframe file: every table but ``points`` is a segment, its ``points = [A, B]`` landmark names (``color`` is ignored).
        ``point_names``: ``{keypoint_id: name}`` as a tracker has it, or ``{name: keypoint_id}``."""
        import tomli

        with open(Path(path), "rb") as fh:
            doc = tomli.load(fh)
        ids = {}
        for k, v in point_names.items():
            name, kp = (k, v) if isinstance(k, str) else (v, k)
            ids[str(name)] = int(kp)
        segments = []
        for name, spec in doc.items():
            if name == "points":
                continue
            if not isinstance(spec, dict) or len(spec.get("points", ())) != 2:
                raise ValueError(f"{path}: segment {name!r} needs points = [A, B]")
            for p in spec["points"]:
                if p not in ids:
                    raise ValueError(f"{path}: segment {name!r} names the landmark {p!r}, which point_names does not have")
            segments.append((name, ids[spec["points"][0]], ids[spec["points"][1]]))
        return cls(tuple(segments))


@dataclass(frozen=True)
class SkeletonOptions:
    """``length_sigma``: how rigid a segment is, world units: a number, or a mapping by segment name.  ``lengths``: a mapping
    ``(object_id, segment name) -> length`` of the lengths that are known; the others are estimated.  ``trim``: frames further than
    this many robust standard deviations from the median length do not enter the estimate.  ``max_iter``: factorisations per
    (frame, subject).  ``tol``: converged when the step is shorter than this in units of its own standard deviation."""

    length_sigma: object
    lengths: Mapping | None = None
    trim: float = 3.0
    max_iter: int = 30
    tol: float = 1e-9


class SkeletonDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int64), ("n_traj", C.c_int64), ("xyz", _lib.c_double_p), ("meas_cov", _lib.c_double_p), ("measured", _lib.c_uint8_p),
                ("n_seg", C.c_int64), ("seg_traj", _lib.c_int32_p), ("seg_length", _lib.c_double_p), ("seg_sigma", _lib.c_double_p),
                ("trim", C.c_double), ("max_iter", C.c_int32), ("tol", C.c_double), ("memory_limit", C.c_int64)]


class SkeletonOut(C.Structure):
    _fields_ = [("pos", _lib.c_double_p), ("pos_cov", _lib.c_double_p), ("status", _lib.c_uint8_p), ("length", _lib.c_double_p),
                ("med", _lib.c_double_p), ("mad", _lib.c_double_p), ("frames", _lib.c_int64_p), ("len_before", _lib.c_double_p),
                ("w_before", _lib.c_double_p), ("len_after", _lib.c_double_p), ("chi2", _lib.c_double_p), ("rows", _lib.c_int32_p),
                ("iterations", _lib.c_int32_p), ("comp_status", _lib.c_uint8_p)]


SKELETON_SIGNATURES = {
    "cba_skeleton_components": (C.c_int64, [C.POINTER(SkeletonDesc), _lib.c_int32_p]),
    "cba_adjust_skeleton": (C.c_int, [C.POINTER(SkeletonDesc), C.c_int32, C.POINTER(SkeletonOut)]),
}


@dataclass(frozen=True)
class AdjustedSkeleton:
    """Per slot of the grid (``pos`` .. ``status``), per segment (``length`` .. ``frames``), per (frame, segment) and per
    (frame, component); covariance rows are xx xy xz yy yz zz."""

    pos: np.ndarray          # [n_slots, 3]
    pos_cov: np.ndarray      # [n_slots, 6]
    status: np.ndarray       # [n_slots] uint8: 0 unmeasured, 1 adjusted, 2 measured with nothing active, 3 component failed
    length: np.ndarray       # [n_seg] the length in use
    med: np.ndarray          # [n_seg]
    mad: np.ndarray          # [n_seg]
    frames: np.ndarray       # [n_seg] int64
    len_before: np.ndarray   # [n_frames, n_seg] NaN where inactive
    w_before: np.ndarray     # [n_frames, n_seg]
    len_after: np.ndarray    # [n_frames, n_seg]
    chi2: np.ndarray         # [n_frames, n_comp]
    rows: np.ndarray         # [n_frames, n_comp] int32
    iterations: np.ndarray   # [n_frames, n_comp] int32
    comp_status: np.ndarray  # [n_frames, n_comp] uint8: 0 nothing active, 1 converged, 2 max_iter, 3 failed
    traj_comp: np.ndarray    # [n_traj] int32, -1: in no segment


def _segment_arrays(n_traj, seg_traj, seg_length, seg_sigma):
    seg_traj = np.ascontiguousarray(seg_traj, dtype=np.int32).reshape(-1, 2)
    n_seg = len(seg_traj)
    seg_length = np.ascontiguousarray(np.broadcast_to(np.asarray(seg_length, dtype=np.float64), (n_seg,)))
    seg_sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(seg_sigma, dtype=np.float64), (n_seg,)))
    return seg_traj, seg_length, seg_sigma


def skeleton_components(n_traj: int, seg_traj) -> tuple[int, np.ndarray]:
    """``(n_comp, traj_comp[n_traj])`` of ``cba_skeleton_components``: host code of the library, no device needed.  A refusal is a
    ``ValueError`` with the library's message."""
    lib = _lib.bind(_lib.load(), SKELETON_SIGNATURES)
    seg_traj = np.ascontiguousarray(seg_traj, dtype=np.int32).reshape(-1, 2)
    traj_comp = np.full(max(int(n_traj), 0), -1, dtype=np.int32)
    desc = SkeletonDesc(n_traj=int(n_traj), n_seg=len(seg_traj), seg_traj=_lib.ptr(seg_traj))
    n_comp = lib.cba_skeleton_components(C.byref(desc), _lib.ptr(traj_comp))
    if n_comp < 0:
        raise ValueError(_lib.last_error(lib))
    return int(n_comp), traj_comp


def run_skeleton_call(call, components, n_frames: int, n_traj: int, xyz, meas_cov, measured, seg_traj, seg_length, seg_sigma, trim: float,
                      max_iter: int, tol: float, memory_limit: int, last_error, what: str = "cba_adjust_skeleton") -> AdjustedSkeleton:
    """Fill ``cba_skeleton_desc`` / ``cba_skeleton_out``, run ``call(desc_ref, out_ref) -> code`` and collect the result (shared by the
    device binding and the test harness).  ``components(n_traj, seg_traj) -> (n_comp, traj_comp)`` sizes the outputs.  A refusal of
    the input is a ``ValueError`` with the library's message."""
    n_frames, n_traj = int(n_frames), int(n_traj)
    n_slots = n_frames * n_traj
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(n_slots, 3)
    meas_cov = np.ascontiguousarray(meas_cov, dtype=np.float64).reshape(n_slots, 6)
    measured = np.ascontiguousarray(measured, dtype=np.uint8).reshape(n_slots)
    seg_traj, seg_length, seg_sigma = _segment_arrays(n_traj, seg_traj, seg_length, seg_sigma)
    n_seg = len(seg_traj)
    n_comp, traj_comp = components(n_traj, seg_traj)
    out = AdjustedSkeleton(pos=np.full((n_slots, 3), np.nan), pos_cov=np.full((n_slots, 6), np.nan), status=np.zeros(n_slots, dtype=np.uint8),
                           length=np.full(n_seg, np.nan), med=np.full(n_seg, np.nan), mad=np.full(n_seg, np.nan), frames=np.zeros(n_seg, dtype=np.int64),
                           len_before=np.full((n_frames, n_seg), np.nan), w_before=np.full((n_frames, n_seg), np.nan),
                           len_after=np.full((n_frames, n_seg), np.nan), chi2=np.zeros((n_frames, n_comp)),
                           rows=np.zeros((n_frames, n_comp), dtype=np.int32), iterations=np.zeros((n_frames, n_comp), dtype=np.int32),
                           comp_status=np.zeros((n_frames, n_comp), dtype=np.uint8), traj_comp=traj_comp)
    so = SkeletonOut(**{name: _lib.ptr(getattr(out, name)) for name, _ in SkeletonOut._fields_})
    try:
        desc = SkeletonDesc(n_frames=n_frames, n_traj=n_traj, xyz=_lib.ptr(xyz), meas_cov=_lib.ptr(meas_cov), measured=_lib.ptr(measured), n_seg=n_seg,
                            seg_traj=_lib.ptr(seg_traj), seg_length=_lib.ptr(seg_length), seg_sigma=_lib.ptr(seg_sigma), trim=float(trim),
                            max_iter=int(max_iter), tol=float(tol), memory_limit=int(memory_limit))
    except (TypeError, ValueError) as exc:
        raise ValueError(f"skeleton options are not numbers: {exc}") from exc
    rc = call(C.byref(desc), C.byref(so))
    if rc in (-1, -4):
        raise ValueError(last_error())
    if rc != 0:
        raise BackendError(f"{what} failed (code {rc}): {last_error()}")
    return out


class DeviceSkeletonAdjuster:
    """The device call ``cba_adjust_skeleton`` on ``device_id``; ``memory_limit`` (bytes, 0: the free device memory) is what the
    buffers of a call are checked against."""

    def __init__(self, device_id: int = 0, memory_limit: int = 0):
        self.device_id = device_id
        self.memory_limit = memory_limit

    def adjust(self, n_frames: int, n_traj: int, xyz, meas_cov, measured, seg_traj, seg_length, seg_sigma, *, trim: float = 3.0, max_iter: int = 30,
               tol: float = 1e-9) -> AdjustedSkeleton:
        """``xyz [n_slots, 3]``, ``meas_cov [n_slots, 6]`` and ``measured [n_slots]`` (1: measured), slot ``s = f * n_traj + j``;
        ``seg_traj [n_seg, 2]`` trajectory indices, ``seg_length [n_seg]`` (NaN: estimated) and ``seg_sigma [n_seg]``."""
        lib = _lib.bind(_lib.load(), SKELETON_SIGNATURES)
        return run_skeleton_call(lambda d, o: lib.cba_adjust_skeleton(d, self.device_id, o), skeleton_components, n_frames, n_traj, xyz, meas_cov,
                                 measured, seg_traj, seg_length, seg_sigma, trim, max_iter, tol, self.memory_limit, lambda: _lib.last_error(lib))


SKELETON_COVARIANCE_COLUMNS = (*COVARIANCE_COLUMNS, "skeleton_status")
SEGMENT_COLUMNS = ("object_id", "segment", "keypoint_a", "keypoint_b", "length", "given", "sigma", "median", "mad", "frames")
ROW_COLUMNS = ("sync_index", "object_id", "segment", "len_before", "w_before", "len_after")
COMPONENT_COLUMNS = ("sync_index", "object_id", "keypoint_id", "chi2", "rows", "iterations", "status")


@dataclass(frozen=True)
class SkeletonResult:
    """``world``: the table with ``x y z`` replaced where ``skeleton_status`` is 1.  ``covariance_frame``: ``COVARIANCE_COLUMNS`` with
    ``cov_*`` and ``std_*`` of the adjusted rows recomputed, ``cov_status`` kept, and ``skeleton_status``; with ``world`` what
    ``smooth_trajectories`` takes.  ``segments``: one row per (``object_id``, segment): the length in use, whether it was given,
    its sigma, the median and the median absolute deviation of the measured lengths and the number of co-measured frames.  ``rows``:
    one row per (``sync_index``, ``object_id``, segment) where the segment is active: its length before, the standardised
    discrepancy ``w_before`` and its length after.  ``components``: one row per (``sync_index``, connected part of a subject's
    skeleton, named by ``object_id`` and its first ``keypoint_id``) with anything active: ``chi2`` and its expectation ``rows``,
    ``iterations`` and ``status`` (1 converged, 2 ``max_iter`` reached, 3 failed and passed through)."""

    world: object
    covariance_frame: pd.DataFrame
    segments: pd.DataFrame
    rows: pd.DataFrame
    components: pd.DataFrame


def adjust_skeleton(world, covariance_frame: pd.DataFrame, skeleton: Skeleton, options: SkeletonOptions, *, device_id: int = 0,
                    _solver=None) -> SkeletonResult:
    """Adjust a table of 3-D points (``WorldPoints``) and the covariance frame that goes with it row for row to ``skeleton``.  The
    grid is that of ``smooth_trajectories``: measured are the rows with ``cov_status`` 1, their ``R`` the rows ``cov_xx .. cov_zz``.
    Every segment is expanded once per ``object_id`` that has both keypoints: lengths are per subject.  ``ValueError``: tables of
    different length or keys, options that are not numbers, a segment name of ``length_sigma`` or ``lengths`` that the skeleton
    does not have, and what the library refuses.  ``_solver`` replaces the device call (an object with ``adjust``, as
    :class:`DeviceSkeletonAdjuster`)."""
    what = "adjust_skeleton"
    df = world._df
    if len(df) != len(covariance_frame):
        raise ValueError(f"{what}: the table has {len(df)} rows and the covariance frame {len(covariance_frame)}: they go row for row")
    sync, obj, kp = (df[c].to_numpy(dtype=np.int64) for c in ("sync_index", "object_id", "keypoint_id"))
    for name, mine in (("sync_index", sync), ("object_id", obj), ("keypoint_id", kp)):
        if not np.array_equal(mine, covariance_frame[name].to_numpy(dtype=np.int64)):
            raise ValueError(f"{what}: the covariance frame is not that of the table: {name} differs")
    names = [n for n, _, _ in skeleton.segments]
    sigma_of = options.length_sigma
    if isinstance(sigma_of, Mapping):
        unknown = set(sigma_of) - set(names)
        if unknown or set(names) - set(sigma_of):
            raise ValueError(f"{what}: length_sigma names {sorted(unknown)} beyond the skeleton and lacks {sorted(set(names) - set(sigma_of))}")
    for key in (options.lengths or {}):
        if len(key) != 2 or key[1] not in names:
            raise ValueError(f"{what}: lengths has the key {key!r}; keys are (object_id, segment name) of the skeleton")
    if len(df) and sync.min() < 0:
        raise ValueError(f"{what}: row {int(np.argmax(sync < 0))} has a negative sync_index (static objects are not supported)")
    objects, oi = np.unique(obj, return_inverse=True)
    keypoints, ki = np.unique(kp, return_inverse=True)
    pairs, j = np.unique(oi.astype(np.int64) * max(len(keypoints), 1) + ki, return_inverse=True)
    traj_object, traj_keypoint = objects[pairs // max(len(keypoints), 1)], keypoints[pairs % max(len(keypoints), 1)]
    n_traj = len(pairs)
    sync_min = int(sync.min()) if len(df) else 0
    n_frames = int(sync.max() - sync_min) + 1 if len(df) else 0
    s = (sync - sync_min) * n_traj + j
    if len(np.unique(s)) != len(s):
        raise ValueError(f"{what}: two rows of one (sync_index, object_id, keypoint_id)")
    n_slots = n_frames * n_traj
    xyz, meas_cov, measured = np.full((n_slots, 3), np.nan), np.full((n_slots, 6), np.nan), np.zeros(n_slots, dtype=np.uint8)
    xyz[s] = df[["x_coord", "y_coord", "z_coord"]].to_numpy(dtype=np.float64)
    meas_cov[s] = covariance_frame[[f"cov_{c}" for c in _COV]].to_numpy(dtype=np.float64)
    measured[s] = covariance_frame["cov_status"].to_numpy() == COV_OK
    # every segment once per subject that has both keypoints
    index = {(int(o), int(k)): t for t, (o, k) in enumerate(zip(traj_object, traj_keypoint))}
    seg_rows = []
    for o in objects:
        for name, a, b in skeleton.segments:
            if (int(o), a) in index and (int(o), b) in index:
                given = (options.lengths or {}).get((int(o), name), np.nan)
                sigma = sigma_of[name] if isinstance(sigma_of, Mapping) else sigma_of
                seg_rows.append((int(o), name, a, b, index[(int(o), a)], index[(int(o), b)], given, sigma))
    try:
        seg_traj = np.array([(r[4], r[5]) for r in seg_rows], dtype=np.int32).reshape(-1, 2)
        seg_length = np.array([float(r[6]) for r in seg_rows], dtype=np.float64)
        seg_sigma = np.array([float(r[7]) for r in seg_rows], dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"{what}: skeleton options are not numbers: {exc}") from exc
    solver = _solver if _solver is not None else DeviceSkeletonAdjuster(device_id)
    res = solver.adjust(n_frames, n_traj, xyz, meas_cov, measured, seg_traj, seg_length, seg_sigma, trim=options.trim, max_iter=options.max_iter,
                        tol=options.tol)

    status = res.status[s] if len(df) else np.zeros(0, dtype=np.uint8)
    adjusted = status == SLOT_ADJUSTED
    new_xyz = df[["x_coord", "y_coord", "z_coord"]].to_numpy(dtype=np.float64).copy()
    new_xyz[adjusted] = res.pos[s[adjusted]]
    frame = pd.DataFrame({c: covariance_frame[c].to_numpy().copy() for c in COVARIANCE_COLUMNS}, columns=list(COVARIANCE_COLUMNS))
    if adjusted.any():
        cov = res.pos_cov[s[adjusted]]
        for i, c in enumerate(_COV):
            frame.loc[adjusted, f"cov_{c}"] = cov[:, i]
        frame.loc[adjusted, "std_x"], frame.loc[adjusted, "std_y"], frame.loc[adjusted, "std_z"] = np.sqrt(cov[:, 0]), np.sqrt(cov[:, 3]), np.sqrt(cov[:, 5])
        frame.loc[adjusted, "std_major"] = np.sqrt(np.maximum(np.linalg.eigvalsh(full_matrices(cov))[:, -1], 0.0))
    frame["skeleton_status"] = status.astype(np.int64)

    segments = pd.DataFrame({"object_id": [r[0] for r in seg_rows], "segment": [r[1] for r in seg_rows], "keypoint_a": [r[2] for r in seg_rows],
                             "keypoint_b": [r[3] for r in seg_rows], "length": res.length, "given": ~np.isnan(seg_length), "sigma": seg_sigma,
                             "median": res.med, "mad": res.mad, "frames": res.frames}, columns=list(SEGMENT_COLUMNS))
    ff, ss = np.nonzero(~np.isnan(res.len_before))
    rows = pd.DataFrame({"sync_index": ff + sync_min, "object_id": segments["object_id"].to_numpy()[ss], "segment": segments["segment"].to_numpy()[ss],
                         "len_before": res.len_before[ff, ss], "w_before": res.w_before[ff, ss], "len_after": res.len_after[ff, ss]},
                        columns=list(ROW_COLUMNS))
    first = np.full(res.chi2.shape[1], -1, dtype=np.int64)  # a component is named by its first trajectory
    for t in range(n_traj - 1, -1, -1):
        if res.traj_comp[t] >= 0:
            first[res.traj_comp[t]] = t
    cf, ck = np.nonzero(res.comp_status)
    components = pd.DataFrame({"sync_index": cf + sync_min, "object_id": traj_object[first[ck]] if len(ck) else np.zeros(0, dtype=np.int64),
                               "keypoint_id": traj_keypoint[first[ck]] if len(ck) else np.zeros(0, dtype=np.int64), "chi2": res.chi2[cf, ck],
                               "rows": res.rows[cf, ck].astype(np.int64), "iterations": res.iterations[cf, ck].astype(np.int64),
                               "status": res.comp_status[cf, ck].astype(np.int64)}, columns=list(COMPONENT_COLUMNS))
    return SkeletonResult(world=world.with_points(new_xyz), covariance_frame=frame, segments=segments, rows=rows, components=components)


__all__ = ["AdjustedSkeleton", "COMPONENT_COLUMNS", "DeviceSkeletonAdjuster", "ROW_COLUMNS", "SEGMENT_COLUMNS", "SKELETON_COVARIANCE_COLUMNS",
           "SKELETON_SIGNATURES", "Skeleton", "SkeletonDesc", "SkeletonOptions", "SkeletonOut", "SkeletonResult", "adjust_skeleton", "run_skeleton_call",
           "skeleton_components"]
