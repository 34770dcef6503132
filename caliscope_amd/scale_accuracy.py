"""Scale accuracy of a calibrated volume in millimetres: how far the distances between triangulated corners of a rigid object
are from the object's own geometry — host-side mirror of the reference's ``core/scale_accuracy.py`` (same names, fields,
properties and errors).

Where the work runs: all pairwise distances of every (frame, object) group, tens of millions of pairs at the sizes this project
is built for, are one device call, ``cba_scale_errors`` (``csrc/scale_math.h``, ``csrc/scale_lib.hip``); the grouping that feeds it
is sorts and prefix sums in :meth:`caliscope_amd.capture_volume.CaptureVolume.compute_volumetric_scale_accuracy`.  There is no CPU
fallback: without the library or a GPU the call raises ``BackendError``.  ``_solver`` replaces the device call (an object with
``scale_errors``, as :class:`DeviceScaleErrors`) — the CPU test-suite passes a g++ build of the same arithmetic.

``compute_depth_ratios`` lives in :mod:`caliscope_amd.calibrate_extrinsics` and is importable from here as well, the path the
reference documents.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from functools import cached_property

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.point_data import STATIC_SYNC_INDEX

SCALE_NSTAT = 8
MAX_GROUP_ENTRIES = 32768  # SCALE_MAX_GROUP of csrc/scale_math.h: CBA_ERR_UNSUPPORTED beyond


def __getattr__(name):  # (calibrate_extrinsics imports capture_volume, which imports this module)
    if name == "compute_depth_ratios":
        from caliscope_amd.calibrate_extrinsics import compute_depth_ratios

        return compute_depth_ratios
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


@dataclass(frozen=True)
class FrameScaleError:
    """One rigid object in one frame; error = measured - true distance, so positive means the reconstruction is too large.
    Distances in millimetres unless the name says otherwise; ``centroid`` is the mean of the triangulated points."""

    sync_index: int
    object_id: int
    distance_rmse_mm: float
    distance_mean_signed_error_mm: float
    distance_max_error_mm: float
    n_corners: int
    n_distance_pairs: int
    n_cameras_contributing: int
    sum_squared_errors_m2: float
    sum_squared_relative_errors: float  # sum of (error / D_ref)^2, D_ref the largest true distance of the object
    centroid: tuple[float, float, float]


def _pooled(pairs_of_sums, factor):
    """{key: sqrt(sum / pairs) * factor} from (key, sum, pairs) triples, keys in order of first appearance, empty keys left out."""
    acc: dict = {}
    for key, s, m in pairs_of_sums:
        s0, m0 = acc.get(key, (0.0, 0))
        acc[key] = (s0 + s, m0 + m)
    return {key: float(np.sqrt(s / m) * factor) for key, (s, m) in acc.items() if m > 0}


@dataclass(frozen=True)
class VolumetricScaleReport:
    """Scale accuracy over many frames.  An empty report is a normal answer (no object geometry, nothing triangulated)."""

    frame_errors: tuple[FrameScaleError, ...]
    static_object_ids: frozenset[int] = frozenset()

    def _total(self, attr):
        return sum(getattr(fe, attr) for fe in self.frame_errors), sum(fe.n_distance_pairs for fe in self.frame_errors)

    @cached_property
    def pooled_rmse_mm(self) -> float:
        sse, pairs = self._total("sum_squared_errors_m2")
        return float(np.sqrt(sse / pairs) * 1000) if pairs else 0.0

    @cached_property
    def median_rmse_mm(self) -> float:
        return float(np.median([fe.distance_rmse_mm for fe in self.frame_errors])) if self.frame_errors else 0.0

    @cached_property
    def max_rmse_mm(self) -> float:
        return float(max(fe.distance_rmse_mm for fe in self.frame_errors)) if self.frame_errors else 0.0

    @cached_property
    def worst_frame(self) -> FrameScaleError | None:
        return max(self.frame_errors, key=lambda fe: fe.distance_rmse_mm) if self.frame_errors else None

    @cached_property
    def n_frames_sampled(self) -> int:
        return len(self.frame_errors)

    @cached_property
    def mean_signed_error_mm(self) -> float:
        """Bias over all pairs (per-frame means weighted by their pair counts)."""
        pairs = sum(fe.n_distance_pairs for fe in self.frame_errors)
        if not pairs:
            return 0.0
        return float(sum(fe.distance_mean_signed_error_mm * fe.n_distance_pairs for fe in self.frame_errors) / pairs)

    @cached_property
    def min_sync_index(self) -> int:
        return min(fe.sync_index for fe in self.frame_errors) if self.frame_errors else 0

    @cached_property
    def max_sync_index(self) -> int:
        return max(fe.sync_index for fe in self.frame_errors) if self.frame_errors else 0

    @cached_property
    def pooled_relative_rmse_pct(self) -> float:
        sse, pairs = self._total("sum_squared_relative_errors")
        return float(np.sqrt(sse / pairs) * 100) if pairs else 0.0

    @cached_property
    def per_frame_relative_rmse_pct(self) -> dict[int, float]:
        """By sync_index, entries at STATIC_SYNC_INDEX left out."""
        return _pooled(((fe.sync_index, fe.sum_squared_relative_errors, fe.n_distance_pairs) for fe in self.frame_errors
                        if fe.sync_index != STATIC_SYNC_INDEX), 100)

    @cached_property
    def per_frame_rmse_mm(self) -> dict[int, float]:
        return _pooled(((fe.sync_index, fe.sum_squared_errors_m2, fe.n_distance_pairs) for fe in self.frame_errors
                        if fe.sync_index != STATIC_SYNC_INDEX), 1000)

    @cached_property
    def per_object_relative_rmse_pct(self) -> dict[int, float]:
        return _pooled(((fe.object_id, fe.sum_squared_relative_errors, fe.n_distance_pairs) for fe in self.frame_errors), 100)

    @cached_property
    def split_relative_rmse_pct(self) -> tuple[float | None, float | None]:
        """(moving, static) by ``static_object_ids``; None for a side without pairs."""
        by_side = _pooled(((fe.object_id in self.static_object_ids, fe.sum_squared_relative_errors, fe.n_distance_pairs)
                           for fe in self.frame_errors), 100)
        return (by_side.get(False), by_side.get(True))

    @classmethod
    def empty(cls) -> "VolumetricScaleReport":
        return cls(frame_errors=())


def _checked(world_xyz, group_start, ent_world, ent_obj):
    world_xyz = np.ascontiguousarray(world_xyz, dtype=np.float64).reshape(-1, 3)
    group_start = np.ascontiguousarray(group_start, dtype=np.int64)
    ent_world = np.ascontiguousarray(ent_world, dtype=np.int64)
    ent_obj = np.ascontiguousarray(ent_obj, dtype=np.float64).reshape(-1, 3)
    if group_start.ndim != 1 or len(group_start) < 1 or len(ent_world) != len(ent_obj) or len(ent_world) < int(group_start[-1]):
        raise ValueError("scale_errors: array lengths do not match")
    return world_xyz, group_start, ent_world, ent_obj


class DeviceScaleErrors:
    """The device call ``cba_scale_errors`` on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def scale_errors(self, world_xyz, group_start, ent_world, ent_obj) -> np.ndarray:
        """``stats[n_groups, 8]``: sum err, sum err^2, max |err|, D_ref, centroid x y z, pair count, over all pairs of the entries
        ``group_start[g] .. group_start[g + 1]``; entry e pairs ``world_xyz[ent_world[e]]`` with ``ent_obj[e]``."""
        lib = _lib.load()
        world_xyz, group_start, ent_world, ent_obj = _checked(world_xyz, group_start, ent_world, ent_obj)
        n_groups = len(group_start) - 1
        stats = np.zeros((n_groups, SCALE_NSTAT))
        desc = _lib.ScaleDesc(n_world=len(world_xyz), world_xyz=_lib.ptr(world_xyz), n_groups=n_groups, group_start=_lib.ptr(group_start),
                              ent_world=_lib.ptr(ent_world), ent_obj=_lib.ptr(ent_obj))
        _lib.check(lib, lib.cba_scale_errors(C.byref(desc), self.device_id, _lib.ptr(stats)), "cba_scale_errors")
        return stats


def frame_errors_from_stats(stats, sync_index, object_id, n_corners, n_cameras) -> tuple[FrameScaleError, ...]:
    """The report entries of ``stats[n, 8]`` (rows with at least one pair) and their per-group labels, all columns at once."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, SCALE_NSTAT)
    m = stats[:, 7]
    dref = stats[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(dref > 0, stats[:, 1] / (dref * dref), 0.0)
    centroid = zip(stats[:, 4].tolist(), stats[:, 5].tolist(), stats[:, 6].tolist())
    return tuple(map(FrameScaleError, np.asarray(sync_index).tolist(), np.asarray(object_id).tolist(),
                     (np.sqrt(stats[:, 1] / m) * 1000).tolist(), (stats[:, 0] / m * 1000).tolist(), (stats[:, 2] * 1000).tolist(),
                     np.asarray(n_corners).tolist(), m.astype(np.int64).tolist(), np.asarray(n_cameras).tolist(), stats[:, 1].tolist(),
                     rel.tolist(), centroid))


def compute_frame_scale_error(world_points: np.ndarray, object_points: np.ndarray, sync_index: int, object_id: int,
                              n_cameras_contributing: int, _solver=None) -> FrameScaleError:
    """All pairwise distances of one object in one frame against its geometry (the reference's function; here a one-group call
    of the batch).  ``ValueError`` for mismatched shapes or fewer than two points."""
    if world_points.shape != object_points.shape:
        raise ValueError(f"Shape mismatch: world_points {world_points.shape} vs object_points {object_points.shape}")
    n = len(world_points)
    if n < 2:
        raise ValueError(f"Need at least 2 points to compute distances, got {n}")
    backend = _solver or DeviceScaleErrors()
    stats = backend.scale_errors(world_points, np.array([0, n], dtype=np.int64), np.arange(n, dtype=np.int64), object_points)
    return frame_errors_from_stats(stats, [int(sync_index)], [int(object_id)], [n], [int(n_cameras_contributing)])[0]


__all__ = ["FrameScaleError", "VolumetricScaleReport", "DeviceScaleErrors", "compute_frame_scale_error", "compute_depth_ratios",
           "frame_errors_from_stats", "MAX_GROUP_ENTRIES"]
