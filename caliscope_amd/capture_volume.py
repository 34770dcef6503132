"""``CaptureVolume.optimize()`` on the MI355X — host-side mirror of the reference's hot-path entry point.

Same public surface as the reference's ``core/capture_volume.py`` for the BA path:

* ``OptimizationStatus``                    <- ``capture_volume.py:45-67``
* ``CaptureVolume.optimize(ftol, max_nfev, verbose, strict, use_constraints, pixel_sigma, *,
  refine_intrinsics, loss, f_scale)``       <- ``:322-444`` (same kwargs, same defaults, immutable self,
  ``CalibrationError`` when ``strict`` and not converged)
* ``CaptureVolume.pixel_f_scale``           <- ``:141-148``
* ``CaptureVolume.reprojection_report``     <- ``:150-235`` (``overall_rmse = sqrt(mean(ex^2+ey^2))`` in pixels)
* ``CaptureVolume.filter_by_percentile_error`` (the stage between the product's passes,
  ``calibrate_extrinsics.py:244``)
* ``CaptureVolume.compute_volumetric_scale_accuracy``  <- ``:755-831`` (grouping by sorts and prefix sums, all pairwise distances
  in one device call, ``cba_scale_errors``)
* ``CaptureVolume.align_to_object`` / ``rotate`` / ``translate`` / ``scaled`` / ``oriented`` / ``grounded`` / ``centered``
  <- ``:833-1329`` (the frame and the metric scale of a solved volume; host work, O(points))

The marshalling of DataFrames into flat arrays follows ``:346-358`` but is vectorised (the reference uses a
Python list comprehension over every observation, and a Python loop to build ``img_to_obj_map``).  The solver
call goes through :func:`caliscope_amd.least_squares.least_squares`, i.e. the MI355X engine; a volume's
``ConstraintSet`` becomes the constraint rows of the solve (``_build_constraint_arrays`` <- ``:446-516``, weights
``(pixel_sigma / f_median) / sigma`` <- ``:373-383``), ``rigidity_report`` <- ``:532-605``.
"""

from __future__ import annotations

import logging
import warnings
from collections import Counter
from copy import deepcopy
from dataclasses import dataclass, field
from functools import cached_property

import numpy as np
import pandas as pd

from caliscope_amd.bundle_parameterization import BundleParameterization
from caliscope_amd.cameras import CameraArray
from caliscope_amd.engine import BAProblem
from caliscope_amd.exceptions import CalibrationError
from caliscope_amd.least_squares import least_squares
from caliscope_amd.constraints import ConstraintSet, ConstraintViolation, DistanceConstraint, RigidityReport
from caliscope_amd.point_data import STATIC_SYNC_INDEX, ImagePoints, WorldPoints
from caliscope_amd.engine import STATUS_REASONS
from caliscope_amd.alignment import SimilarityTransform, apply_similarity_transform, estimate_similarity_transform
from caliscope_amd.coordinate_frame import world_basis_from_up_and_forward
from caliscope_amd.scale_accuracy import DeviceScaleErrors, VolumetricScaleReport, frame_errors_from_stats
from caliscope_amd.scale_cues import CameraDistance, DepthObservation, SegmentLength

logger = logging.getLogger(__name__)

_KEY = ["sync_index", "object_id", "keypoint_id"]


@dataclass(frozen=True)
class OptimizationStatus:
    converged: bool
    termination_reason: str
    iterations: int  # number of residual evaluations (scipy's nfev)
    final_cost: float
    bound_warnings: tuple = ()


def _group_index(keys: np.ndarray):
    """``(unique_sorted_keys, inverse)`` like ``np.unique(keys, return_inverse=True)`` for integer keys.  Ids here
    (cameras, points, keypoints) are small and dense, so a presence table + prefix sum replaces the sort of every
    observation; widely spread keys fall back to ``np.unique``."""
    keys = np.asarray(keys, dtype=np.int64)
    if keys.size == 0:
        return keys, np.zeros(0, dtype=np.int64)
    lo, hi = int(keys.min()), int(keys.max())
    if hi - lo > 4 * keys.size + 1024:
        return np.unique(keys, return_inverse=True)
    shifted = keys - lo
    present = np.zeros(hi - lo + 1, dtype=bool)
    present[shifted] = True
    rank = np.cumsum(present, dtype=np.int64) - 1
    return np.flatnonzero(present) + lo, rank[shifted]


@dataclass(frozen=True)
class ReprojectionReport:
    overall_rmse: float
    by_camera: dict
    by_point: dict
    n_unmatched_observations: int
    unmatched_rate: float
    unmatched_by_camera: dict
    raw_errors: pd.DataFrame
    n_observations_matched: int
    n_observations_total: int
    n_cameras: int
    n_points: int


def pose_method(estimate_poses) -> str | None:
    """The pose-network method an ``estimate_poses`` value asks for: None (no estimation) for a false bool or None, "pnp" for a
    true bool (builtin or numpy), else the string itself if it is "pnp", "epipolar" or "auto"; anything else is ``ValueError``."""
    if estimate_poses is None or isinstance(estimate_poses, (bool, np.bool_)):
        return "pnp" if estimate_poses else None
    if isinstance(estimate_poses, str) and estimate_poses in ("pnp", "epipolar", "auto"):
        return estimate_poses
    raise ValueError(f"estimate_poses must be a bool, 'pnp', 'epipolar' or 'auto', got {estimate_poses!r}")


@dataclass(frozen=True)
class CaptureVolume:
    camera_array: CameraArray
    image_points: ImagePoints
    world_points: WorldPoints
    constraints: ConstraintSet | None = None
    img_to_obj_map: np.ndarray = field(init=False)
    _optimization_status: OptimizationStatus | None = field(default=None, compare=False)
    # optimize() changes coordinates only: the observation -> world-point map of the source volume stays valid (at 2M
    # observations rebuilding it is 30 % of the call)
    _known_map: np.ndarray | None = field(default=None, compare=False, repr=False)

    @property
    def optimization_status(self) -> OptimizationStatus | None:
        return self._optimization_status

    def __post_init__(self):
        known = self._known_map
        if known is not None and len(known) == len(self.image_points):
            object.__setattr__(self, "img_to_obj_map", known)
        else:
            object.__setattr__(self, "img_to_obj_map", self._compute_img_to_obj_map())
        object.__setattr__(self, "_known_map", None)
        n_img, n_world = len(self.image_points), len(self.world_points)
        if n_img == 0:
            raise ValueError("No image observations provided")
        if n_world == 0:
            raise ValueError("No world points provided")
        if len(self.camera_array.posed_cameras) == 0:
            raise ValueError("No posed cameras in array")
        n_matched = int(np.sum(self.img_to_obj_map >= 0))
        if n_matched == 0:
            raise ValueError("No image observations have corresponding world points")
        if n_matched < 2 * n_world:
            logger.warning(f"Suspicious geometry: {n_matched} matched observations for {n_world} world points. "
                           f"Expected at least {n_world * 2} for multi-view geometry.")
        if int(self.img_to_obj_map.max()) >= n_world:
            raise ValueError(f"obj_indices contains out-of-bounds index: {int(self.img_to_obj_map.max())} >= {n_world}")

    def _compute_img_to_obj_map(self) -> np.ndarray:
        """Row of ``world_points`` for every image observation, -1 when unmatched.  Observations of a static object look their
        point up at ``STATIC_SYNC_INDEX`` (reference :119-139, a left merge on (sync_index, object_id, keypoint_id) that keeps the LAST of duplicate
        world keys).  The three integer keys are folded into one and looked up in a dense table when their ranges are small (they are: frame
        numbers, a few objects, keypoint ids) — a fifth of the merge's time on 2M observations; spread-out keys take the merge."""
        wdf, idf = self.world_points._df, self.image_points._df
        static_ids = self.constraints.static_object_ids if self.constraints else frozenset()
        if len(wdf) and len(idf):
            w = [wdf[c].to_numpy() for c in _KEY]
            i = [idf[c].to_numpy() for c in _KEY]
            if static_ids:
                i[0] = np.where(np.isin(i[1], list(static_ids)), STATIC_SYNC_INDEX, i[0])
            lo = [min(int(a.min()), int(b.min())) for a, b in zip(w, i)]
            span = [max(int(a.max()), int(b.max())) - l + 1 for a, b, l in zip(w, i, lo)]
            if span[0] * span[1] * span[2] <= max(1 << 22, 16 * len(wdf)) and span[0] * span[1] * span[2] <= 1 << 25:  # (128 MB of int32 at most; wider key ranges take the merge)
                fold = lambda k: ((k[0] - lo[0]) * span[1] + (k[1] - lo[1])) * span[2] + (k[2] - lo[2])  # noqa: E731
                table = np.full(span[0] * span[1] * span[2], -1, dtype=np.int32)
                table[fold(w)] = np.arange(len(wdf), dtype=np.int32)  # (a repeated key keeps the last row written: numpy assigns in order)
                return table[fold(i)]
        return self._img_to_obj_map_by_merge(static_ids)

    def _img_to_obj_map_by_merge(self, static_ids) -> np.ndarray:
        world = self.world_points._df[_KEY].copy()
        world["world_idx"] = np.arange(len(world), dtype=np.int64)
        world = world.drop_duplicates(subset=_KEY, keep="last")
        keys = self.image_points._df[_KEY]
        if static_ids:
            keys = keys.copy()
            keys.loc[keys["object_id"].isin(list(static_ids)), "sync_index"] = STATIC_SYNC_INDEX
        merged = keys.merge(world, on=_KEY, how="left")
        return merged["world_idx"].fillna(-1).to_numpy(dtype=np.int32)

    # -- persistence (reference :237-267) -------------------------------------------------------------
    def save(self, directory) -> None:
        """Write ``camera_array.toml``, ``image_points.csv``, ``world_points.csv`` and, when the volume has one,
        ``constraints.toml`` (atomic writes).  As in the reference, ``optimization_status`` is not persisted."""
        from pathlib import Path

        directory = Path(directory)
        directory.mkdir(parents=True, exist_ok=True)
        self.camera_array.to_toml(directory / "camera_array.toml")
        self.image_points.to_csv(directory / "image_points.csv")
        self.world_points.to_csv(directory / "world_points.csv")
        if self.constraints is not None:
            self.constraints.to_toml(directory / "constraints.toml")

    @classmethod
    def load(cls, directory) -> "CaptureVolume":
        from pathlib import Path

        directory = Path(directory)
        con_path = directory / "constraints.toml"
        return cls(camera_array=CameraArray.from_toml(directory / "camera_array.toml"),
                   image_points=ImagePoints.from_csv(directory / "image_points.csv"),
                   world_points=WorldPoints.from_csv(directory / "world_points.csv"),
                   constraints=ConstraintSet.from_toml(con_path) if con_path.exists() else None)

    # -- marshalling (reference :346-358) ------------------------------------------------------------
    def _matched_arrays(self):
        col = self.image_points.arrays()
        index_of = self.camera_array.posed_cam_id_to_index
        # the volume is immutable apart from its camera array (a camera can be posed later): the arrays are kept per posed-camera set — optimize(),
        # the reprojection report and the filters of one volume marshal the same 2M rows (cfg4: 20 ms each time)
        key = tuple(sorted(index_of.items()))
        kept = getattr(self, "_matched_cache", None)
        if kept is not None and kept[0] == key:
            return kept[1]
        cam_id = col["cam_id"]
        # cam_id -> position among the posed cameras through a dense table (ids are small non-negative integers)
        lo = min(int(cam_id.min()), min(index_of, default=0)) if cam_id.size else 0
        hi = max(int(cam_id.max()), max(index_of, default=0)) if cam_id.size else 0
        if hi - lo < (1 << 20):
            table = np.full(hi - lo + 1, -1, dtype=np.int32)
            for cid, i in index_of.items():
                table[cid - lo] = i
            cam_idx = table[cam_id - lo]
        else:  # sparse ids: binary search in the sorted posed ids
            ids = np.array(sorted(index_of), dtype=np.int64)
            pos = np.array([index_of[c] for c in ids], dtype=np.int32)
            at = np.minimum(np.searchsorted(ids, cam_id), len(ids) - 1) if len(ids) else np.zeros(cam_id.shape, dtype=np.int64)
            cam_idx = np.where(ids[at] == cam_id, pos[at], -1).astype(np.int32) if len(ids) else np.full(cam_id.shape, -1, dtype=np.int32)
        mask = (self.img_to_obj_map >= 0) & (cam_idx >= 0)
        if mask.all():  # (the usual case after triangulation + filtering: nothing to select)
            camera_indices, obj_indices = cam_idx, self.img_to_obj_map.astype(np.int32)  # (a copy: the map itself stays writable)
            image_coords = np.empty((len(cam_idx), 2))
            image_coords[:, 0] = col["img_loc_x"]; image_coords[:, 1] = col["img_loc_y"]
        else:
            camera_indices = cam_idx[mask]
            image_coords = np.stack([col["img_loc_x"][mask], col["img_loc_y"][mask]], axis=1)
            obj_indices = self.img_to_obj_map[mask].astype(np.int32)
        for a in (mask, camera_indices, image_coords, obj_indices):
            a.setflags(write=False)  # shared between calls
        out = (mask, camera_indices, image_coords, obj_indices)
        object.__setattr__(self, "_matched_cache", (key, out))
        return out

    def pixel_f_scale(self, px: float = 1.0) -> float:
        focal = [cam.matrix[0, 0] for cam in self.camera_array.posed_cameras.values() if cam.matrix is not None]
        return px / float(np.median(focal))

    # -- the hot path ----------------------------------------------------------------------------------
    def optimize(
        self,
        ftol: float = 1e-8,
        max_nfev: int | None = None,
        verbose: int = 0,
        strict: bool = True,
        use_constraints: bool = True,
        pixel_sigma: float = 1.0,
        *,
        refine_intrinsics: bool = False,
        loss: str = "linear",
        f_scale: float = 1.0,
        _engine_factory=None,
    ) -> "CaptureVolume":
        """Bundle adjustment via pixel-space residuals, on the MI355X engine."""
        _, camera_indices, image_coords, obj_indices = self._matched_arrays()
        con_args = (None, None, None, None)
        if use_constraints and self.constraints is not None:
            arrays = self._build_constraint_arrays()
            if arrays is not None:
                groups_a, groups_b, distances, sigmas = arrays
                f_median = float(np.median([cam.matrix[0, 0] for cam in self.camera_array.posed_cameras.values()]))
                # residual units are normalised image coordinates (pixels / fx): a row is 1 when the distance is off
                # by one sigma scaled like a pixel_sigma reprojection error (reference :377-383)
                con_args = (groups_a, groups_b, distances, (pixel_sigma / f_median) / sigmas)
                logger.info(f"Adding {len(distances)} constraint rows (f_median={f_median:.0f}, pixel_sigma={pixel_sigma})")
        new_cameras = deepcopy(self.camera_array)
        par = BundleParameterization.from_camera_array(
            new_cameras, n_points=len(self.world_points), refine_intrinsics=refine_intrinsics
        )
        x0 = par.pack(new_cameras, self.world_points.points)
        logger.info(f"Beginning bundle adjustment on {len(image_coords)} observations")
        result = least_squares(
            None,
            x0,
            args=(par, camera_indices, image_coords, obj_indices, *con_args),
            jac=None,
            verbose=verbose,
            x_scale="jac",
            loss=loss,
            f_scale=f_scale,
            ftol=ftol,
            max_nfev=max_nfev,
            method="trf",
            bounds=par.bounds(),
            engine_factory=_engine_factory,
        )
        reason = STATUS_REASONS.get(result.status, f"unknown_{result.status}")
        converged = result.status in (1, 2, 3, 4)
        if strict and not converged:
            raise CalibrationError(
                f"Bundle adjustment did not converge: {reason}\n"
                f"Pass strict=False to suppress this error and inspect the result."
            )
        new_points = par.unpack_into(new_cameras, result.x)
        status = OptimizationStatus(
            converged=converged,
            termination_reason=reason,
            iterations=int(result.nfev),
            final_cost=float(result.cost),
            bound_warnings=par.bound_warnings(result.x),
        )
        out = CaptureVolume(
            camera_array=new_cameras,
            image_points=self.image_points,
            world_points=self.world_points.with_points(new_points),
            constraints=self.constraints,
            _optimization_status=status,
            _known_map=self.img_to_obj_map,
        )
        kept = getattr(self, "_constraint_cache", None)
        if kept is not None:  # same world-point keys, same constraint set
            object.__setattr__(out, "_constraint_cache", kept)
        return out

    # -- constraint rows (reference :446-605) ----------------------------------------------------------------
    def _constraint_blocks(self):
        """Per constraint that fires: ``(constraint, sync indices (n,), rows_a (n, 4), rows_b (n, 4))`` — four world-point rows per endpoint (a corner
        endpoint is its row four times) at every sync index at which all endpoint keypoints have a world point.  Static-static constraints fire once
        at ``STATIC_SYNC_INDEX``, mobile-mobile ones at every shared sync index, mixed ones never (reference ``_firing_sync_indices`` :518-530).
        The blocks depend on the KEYS of the world points and on the constraint set only, so they are built once per volume and handed to the
        volumes ``optimize()`` returns (same keys, new coordinates): on the reference's 4-camera session with its board they were 5 of the call's 7 ms."""
        kept = getattr(self, "_constraint_cache", None)
        if kept is not None:
            return kept
        con = self.constraints
        blocks = []
        if con is not None and (con.distances or con.centroid_distances):
            df = self.world_points._df
            order = np.lexsort((df["sync_index"].to_numpy(), df["keypoint_id"].to_numpy(), df["object_id"].to_numpy()))
            obj, kp, sync = (df[c].to_numpy()[order] for c in ("object_id", "keypoint_id", "sync_index"))
            # one slice of (sorted sync indices, world rows) per keypoint
            start = np.flatnonzero(np.r_[True, (obj[1:] != obj[:-1]) | (kp[1:] != kp[:-1])]) if len(obj) else np.array([], dtype=np.int64)
            end = np.r_[start[1:], len(obj)]
            table = {(int(obj[s]), int(kp[s])): (sync[s:e], order[s:e]) for s, e in zip(start, end)}
            static_ids = con.static_object_ids
            # One row table for the keypoints the constraints name: world row of (keypoint, sync index) or -1, over the sorted distinct sync indices.
            # A constraint fires where every endpoint has a row; all constraints of a kind are then ONE fancy-indexed comparison (an np.intersect1d
            # per endpoint pair was 1.6 of the 3.2 ms of a first optimize() on the reference's 4-camera session with its board).
            wanted = {(dc.object_id_a, dc.keypoint_id_a) for dc in con.distances} | {(dc.object_id_b, dc.keypoint_id_b) for dc in con.distances}
            wanted |= {(o, k) for cc in con.centroid_distances for o in (cc.object_id_a, cc.object_id_b) for k in range(4)}
            named = [key for key in wanted if key in table]
            usync = np.unique(np.concatenate([table[key][0] for key in named])) if named else np.array([], dtype=np.int64)
            row_of = {key: i for i, key in enumerate(named)}
            rowmat = np.full((len(named) + 1, len(usync)), -1, dtype=np.int64)  # last row: a keypoint without any world point
            for key, i in row_of.items():
                s_k, r_k = table[key]
                rowmat[i, np.searchsorted(usync, s_k)] = r_k  # (sorted by sync; of duplicate world keys the LAST row, as the reference's dict of rows keeps)
            is_static_col = usync == STATIC_SYNC_INDEX
            missing = len(named)

            def fire_all(constraints, endpoint_keys, split):
                """Append (constraint, syncs, rows_a, rows_b) for those of `constraints` that fire (`endpoint_keys(c)`: the keys of its endpoints;
                `split`: (instances, endpoints) world rows -> the two (instances, 4) row arrays)."""
                usable = [c for c in constraints if (c.object_id_a in static_ids) == (c.object_id_b in static_ids)]  # mixed static / mobile: never
                if not usable or not len(usync):
                    return
                idx = np.array([[row_of.get(key, missing) for key in endpoint_keys(c)] for c in usable], dtype=np.int64)  # (n, endpoints)
                rows = rowmat[idx]                                                                                          # (n, endpoints, syncs)
                static_c = np.array([c.object_id_a in static_ids for c in usable], dtype=bool)
                ok = (rows >= 0).all(axis=1) & (static_c[:, None] == is_static_col[None, :])
                ci, si = np.nonzero(ok)  # constraint-major, sync indices ascending inside a constraint: the order of the rows
                if not len(ci):
                    return
                rows_a, rows_b = split(rows[ci, :, si])
                syncs = usync[si]
                cut = np.searchsorted(ci, np.arange(len(usable) + 1)).tolist()
                for i, c in enumerate(usable):
                    if cut[i + 1] > cut[i]:
                        blocks.append((c, syncs[cut[i]:cut[i + 1]], rows_a[cut[i]:cut[i + 1]], rows_b[cut[i]:cut[i + 1]]))

            fire_all(con.distances, lambda c: ((c.object_id_a, c.keypoint_id_a), (c.object_id_b, c.keypoint_id_b)),
                     lambda r: (np.repeat(r[:, :1], 4, axis=1), np.repeat(r[:, 1:2], 4, axis=1)))
            fire_all(con.centroid_distances, lambda c: [(o, k) for o in (c.object_id_a, c.object_id_b) for k in range(4)], lambda r: (r[:, :4], r[:, 4:]))
        object.__setattr__(self, "_constraint_cache", blocks)
        return blocks

    def _constraint_instances(self):
        """``(constraint, sync_index, rows_a, rows_b)`` per instance, in the order of ``_build_constraint_arrays``'s rows."""
        for c, syncs, rows_a, rows_b in self._constraint_blocks():
            for i, si in enumerate(syncs):
                yield c, int(si), rows_a[i].tolist(), rows_b[i].tolist()

    def _build_constraint_arrays(self):
        """``(groups_a (n, 4) int32, groups_b (n, 4) int32, distances (n,), sigmas (n,))`` or None."""
        blocks = self._constraint_blocks()
        if not blocks:
            return None
        n = [len(b[1]) for b in blocks]
        return (np.concatenate([b[2] for b in blocks]).astype(np.int32), np.concatenate([b[3] for b in blocks]).astype(np.int32),
                np.repeat(np.array([b[0].distance for b in blocks], dtype=np.float64), n),
                np.repeat(np.array([b[0].sigma for b in blocks], dtype=np.float64), n))

    @property
    def unique_sync_indices(self) -> np.ndarray:
        """Sorted sync indices that have a world point (reference :933-941: the slider range of its viewers; STATIC_SYNC_INDEX included when
        static points exist, as there)."""
        return np.unique(self.world_points._df["sync_index"].to_numpy())

    def rigidity_report(self) -> RigidityReport:
        """Measured distance of every constraint instance with the current world points (no optimisation)."""
        xyz = self.world_points.points
        out = []
        for c, si, rows_a, rows_b in self._constraint_instances():
            actual = float(np.linalg.norm(xyz[rows_a].mean(axis=0) - xyz[rows_b].mean(axis=0)))
            if isinstance(c, DistanceConstraint):
                out.append(ConstraintViolation(c.object_id_a, c.keypoint_id_a, c.object_id_b, c.keypoint_id_b, si, c.distance, actual))
            else:
                out.append(ConstraintViolation(c.object_id_a, -1, c.object_id_b, -1, si, c.distance, actual, kind="centroid"))
        return RigidityReport(violations=tuple(out))

    # -- metric of record --------------------------------------------------------------------------------
    def _pixel_errors(self, camera_indices, image_coords, obj_indices, _engine_factory=None) -> np.ndarray:
        """(projected - observed) in pixels with the stored intrinsics/extrinsics, evaluated on the device:
        residuals are ``/fx_initial`` of a locked parameterization, so pixels = residual * fx."""
        par = BundleParameterization.from_camera_array(
            self.camera_array, n_points=len(self.world_points), refine_intrinsics=False
        )
        x = par.pack(self.camera_array, self.world_points.points)
        problem = BAProblem(par, camera_indices, image_coords, obj_indices)
        if _engine_factory is None:
            from caliscope_amd.hip_engine import HipEngine

            eng = HipEngine(problem, evaluation_only=True)  # the report needs residuals only: no Schur plan
        else:
            eng = _engine_factory(problem)
        try:
            r, _ = eng.residuals(x)
        finally:
            close = getattr(eng, "close", None)
            if close is not None:
                close()
        fx = np.array([b.fx_initial for b in par.blocks])[camera_indices]
        return r.reshape(-1, 2) * fx[:, None]

    def compute_reprojection_report(self, _engine_factory=None) -> ReprojectionReport:
        mask, camera_indices, image_coords, obj_indices = self._matched_arrays()
        n_total, n_matched = len(mask), int(mask.sum())
        if n_matched == 0:
            raise ValueError("No matched observations for reprojection error calculation")
        err = self._pixel_errors(camera_indices, image_coords, obj_indices, _engine_factory)
        sq = np.einsum("ij,ij->i", err, err)
        all_df = self.image_points._df
        # columns as arrays: a boolean-indexed DataFrame copy of 2M rows costs more than everything else in this function
        everything = n_matched == n_total  # (the usual case after triangulation and filtering: nothing to select)
        # (everything: to_numpy() hands out VIEWS of the ImagePoints table — copied, or writing to report.raw_errors would write through into the
        # table and the cached matched arrays)
        col = {c: (all_df[c].to_numpy().copy() if everything else all_df[c].to_numpy()[mask]) for c in ("sync_index", "cam_id", "object_id", "keypoint_id")}
        raw = pd.DataFrame(
            {
                "sync_index": col["sync_index"], "cam_id": col["cam_id"], "object_id": col["object_id"], "keypoint_id": col["keypoint_id"],
                "error_x": err[:, 0], "error_y": err[:, 1], "euclidean_error": np.sqrt(sq),
            },
            copy=False,  # (the arrays are this function's own: no need to copy them into consolidated blocks)
        )
        index_of = self.camera_array.posed_cam_id_to_index
        n_cam = len(index_of)
        cam_sum = np.bincount(camera_indices, weights=sq, minlength=n_cam)
        cam_cnt = np.bincount(camera_indices, minlength=n_cam)
        by_camera = {cid: 0.0 for cid in self.camera_array.posed_cameras}
        for cid, i in index_of.items():
            by_camera[cid] = float(np.sqrt(cam_sum[i] / cam_cnt[i])) if cam_cnt[i] else 0.0
        # RMS per (object_id, keypoint_id): one integer key, unique + bincount instead of a pandas group-by
        obj_id, kp_id = col["object_id"].astype(np.int64), col["keypoint_id"].astype(np.int64)
        kp_lo = int(kp_id.min()) if kp_id.size else 0
        span = int(kp_id.max()) - kp_lo + 1 if kp_id.size else 1
        keys, inv = _group_index(obj_id * span + (kp_id - kp_lo))
        mean_sq = np.bincount(inv, weights=sq, minlength=keys.size) / np.maximum(np.bincount(inv, minlength=keys.size), 1)
        by_point = dict(zip(zip((keys // span).tolist(), (keys % span + kp_lo).tolist()), np.sqrt(mean_sq).tolist()))
        cams_all, inv_all = _group_index(all_df["cam_id"].to_numpy())
        cams_ok, inv_ok = (cams_all, inv_all) if everything else _group_index(col["cam_id"])
        n_all, n_ok = np.bincount(inv_all, minlength=cams_all.size), np.bincount(inv_ok, minlength=cams_ok.size)
        total_by_cam, matched_by_cam = dict(zip(cams_all.tolist(), n_all.tolist())), dict(zip(cams_ok.tolist(), n_ok.tolist()))
        unmatched_by_camera = {
            int(c): int(total_by_cam.get(c, 0) - matched_by_cam.get(c, 0)) for c in self.camera_array.cameras
        }
        return ReprojectionReport(
            overall_rmse=float(np.sqrt(np.mean(sq))), by_camera=by_camera, by_point=by_point,
            n_unmatched_observations=n_total - n_matched, unmatched_rate=(n_total - n_matched) / n_total,
            unmatched_by_camera=unmatched_by_camera, raw_errors=raw, n_observations_matched=n_matched,
            n_observations_total=n_total, n_cameras=len(self.camera_array.posed_cameras), n_points=len(self.world_points),
        )

    @cached_property
    def reprojection_report(self) -> ReprojectionReport:
        return self.compute_reprojection_report()

    # -- outlier filtering between solver passes (reference capture_volume.py:607-753) ------------------
    def _filter_by_reprojection_thresholds(self, thresholds: dict, min_per_camera: int, _engine_factory=None, _report=None) -> "CaptureVolume":
        """Keep observations whose pixel error is <= their camera's threshold, but never fewer than
        ``min_per_camera`` per camera (the best ones are kept); world points left without any observation
        are pruned; the optimisation status is cleared."""
        report = _report if _report is not None else (self.compute_reprojection_report(_engine_factory) if _engine_factory else self.reprojection_report)
        raw = report.raw_errors
        err = raw["euclidean_error"].to_numpy()
        cam = raw["cam_id"].to_numpy()
        cams, inv = _group_index(cam)
        keep = err <= np.array([thresholds[int(c)] for c in cams], dtype=np.float64)[inv]
        kept_per_cam = np.bincount(inv, weights=keep, minlength=len(cams)).astype(np.int64)
        rows_per_cam = np.bincount(inv, minlength=len(cams))
        for k in np.flatnonzero((kept_per_cam < min_per_camera) & (kept_per_cam < rows_per_cam)):  # safety floor: rarely any
            idx = np.flatnonzero(inv == k)
            n_needed = min(min_per_camera, idx.size) - int(kept_per_cam[k])
            dropped = np.sort(err[idx][~keep[idx]])
            if dropped.size >= n_needed:
                keep[idx] = err[idx] <= dropped[n_needed - 1]
        mask, *_ = self._matched_arrays()
        keep_rows = np.zeros(len(mask), dtype=bool)  # like the reference's inner merge: unmatched rows go too
        keep_rows[np.flatnonzero(mask)[keep]] = True
        obj = self.img_to_obj_map[keep_rows]  # all >= 0: kept rows are matched rows
        seen = np.zeros(len(self.world_points), dtype=bool)
        seen[obj] = True
        # the surviving observations keep their world point, whose row number drops by the pruned rows before it: the new
        # volume gets its observation -> point map from the old one instead of a merge over every observation
        new_row = np.cumsum(seen, dtype=np.int64) - 1
        return CaptureVolume(self.camera_array, self.image_points.take(keep_rows), self.world_points.take(seen), self.constraints,
                             _known_map=new_row[obj].astype(np.int32))

    def filter_by_percentile_error(self, percentile: float, scope: str = "per_camera", min_per_camera: int = 10,
                                   _engine_factory=None) -> "CaptureVolume":
        """Remove the worst ``percentile`` percent of observations by reprojection error
        (``scope``: "per_camera" thresholds, the reference's default, or one "overall" threshold)."""
        if not (0 < percentile <= 100):
            raise ValueError(f"percentile must be between 0 and 100, got {percentile}")
        if min_per_camera < 1:
            raise ValueError(f"min_per_camera must be >= 1, got {min_per_camera}")
        if scope not in ("per_camera", "overall"):
            raise ValueError(f"scope must be 'per_camera' or 'overall', got {scope}")
        report = self.compute_reprojection_report(_engine_factory) if _engine_factory else self.reprojection_report
        raw = report.raw_errors
        keep_percentile = 100 - percentile
        if scope == "per_camera":
            # one stable sort by camera instead of a boolean selection over every observation per camera
            err, cam = raw["euclidean_error"].to_numpy(), raw["cam_id"].to_numpy()
            cams, inv = _group_index(cam)
            # numpy's stable sort of 16-bit keys is a radix sort
            order = np.argsort(inv.astype(np.int16) if cams.size < 32768 else inv, kind="stable")
            start = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=cams.size))[:-1]]).astype(np.int64)
            stop = np.append(start[1:], len(order))
            thresholds = {cam_id: float(np.inf) for cam_id in self.camera_array.posed_cameras}
            for c, a, b in zip(cams.tolist(), start.tolist(), stop.tolist()):
                if c in thresholds:
                    thresholds[c] = float(np.percentile(err[order[a:b]], keep_percentile))
        else:
            thr = float(np.percentile(raw["euclidean_error"], keep_percentile))
            thresholds = {cam_id: thr for cam_id in self.camera_array.posed_cameras}
        return self._filter_by_reprojection_thresholds(thresholds, min_per_camera, _engine_factory, _report=report)  # one report for both steps

    def filter_by_absolute_error(self, max_pixels: float, min_per_camera: int = 10, _engine_factory=None) -> "CaptureVolume":
        """Remove observations with a reprojection error above ``max_pixels`` (reference :687-707)."""
        if max_pixels <= 0:
            raise ValueError(f"max_pixels must be positive, got {max_pixels}")
        if min_per_camera < 1:
            raise ValueError(f"min_per_camera must be >= 1, got {min_per_camera}")
        thresholds = {cam_id: float(max_pixels) for cam_id in self.camera_array.posed_cameras}
        return self._filter_by_reprojection_thresholds(thresholds, min_per_camera, _engine_factory)

    # -- statistics and filter in one device call (caliscope_amd/reprojection_stats.py) -----------------------------------------
    def _reprojection_call(self, _solver, *, groups: bool, want_errors: bool, **how):
        """One ``reprojection_filter`` call on the matched observations with the stored (locked) intrinsics and extrinsics, as
        ``_pixel_errors`` evaluates them: ``(result, group keys or None, span of the keypoint ids, their lowest)``."""
        from caliscope_amd.reprojection_stats import DeviceReprojectionStats

        mask, camera_indices, image_coords, obj_indices = self._matched_arrays()
        if int(mask.sum()) == 0:
            raise ValueError("No matched observations for reprojection error calculation")
        par = BundleParameterization.from_camera_array(self.camera_array, n_points=len(self.world_points), refine_intrinsics=False)
        tabs = par.device_tables()
        x = par.pack(self.camera_array, self.world_points.points)
        poses = x[: par.n_camera_params].reshape(-1, 6)
        keys = obs_group = None
        span = kp_lo = 0
        if groups:  # one integer key per (object_id, keypoint_id), as compute_reprojection_report folds them
            all_df = self.image_points._df
            everything = bool(mask.all())
            obj_id = (all_df["object_id"].to_numpy() if everything else all_df["object_id"].to_numpy()[mask]).astype(np.int64)
            kp_id = (all_df["keypoint_id"].to_numpy() if everything else all_df["keypoint_id"].to_numpy()[mask]).astype(np.int64)
            kp_lo = int(kp_id.min())
            span = int(kp_id.max()) - kp_lo + 1
            keys, obs_group = _group_index(obj_id * span + (kp_id - kp_lo))
        backend = _solver or DeviceReprojectionStats()
        result = backend.reprojection_filter(tabs["cam_model"], tabs["cam_const"], poses, self.world_points.points, camera_indices, obj_indices, image_coords,
                                             obs_group=obs_group, n_groups=0 if keys is None else len(keys), want_errors=want_errors, **how)
        return result, keys, span, kp_lo

    def reprojection_summary(self, raw: bool = False, _solver=None):
        """The numbers of ``compute_reprojection_report`` from one device call: the pixel errors are summed per camera and per
        (object_id, keypoint_id) on the device and never come back, and no per-observation table is built, unless ``raw=True`` asks
        for one (``raw_errors`` with the report's columns).  ``_solver`` replaces the device call (tests)."""
        from caliscope_amd.reprojection_stats import ReprojectionSummary

        result, keys, span, kp_lo = self._reprojection_call(_solver, groups=True, want_errors=raw, mode="stats")
        mask, camera_indices, _, _ = self._matched_arrays()
        n_total, n_matched = len(mask), int(mask.sum())
        all_df = self.image_points._df
        everything = n_matched == n_total
        index_of = self.camera_array.posed_cam_id_to_index
        by_camera = {cid: 0.0 for cid in self.camera_array.posed_cameras}
        for cid, i in index_of.items():
            by_camera[cid] = float(np.sqrt(result.cam_sumsq[i] / result.cam_count[i])) if result.cam_count[i] else 0.0
        mean_sq = result.group_sumsq / np.maximum(result.group_count, 1)
        by_point = dict(zip(zip((keys // span).tolist(), (keys % span + kp_lo).tolist()), np.sqrt(mean_sq).tolist()))
        cam_all = all_df["cam_id"].to_numpy()
        cams_all, inv_all = _group_index(cam_all)
        cams_ok, inv_ok = (cams_all, inv_all) if everything else _group_index(cam_all[mask])
        n_all, n_ok = np.bincount(inv_all, minlength=cams_all.size), np.bincount(inv_ok, minlength=cams_ok.size)
        total_by_cam, matched_by_cam = dict(zip(cams_all.tolist(), n_all.tolist())), dict(zip(cams_ok.tolist(), n_ok.tolist()))
        unmatched_by_camera = {int(c): int(total_by_cam.get(c, 0) - matched_by_cam.get(c, 0)) for c in self.camera_array.cameras}
        raw_errors = None
        if raw:
            col = {c: (all_df[c].to_numpy().copy() if everything else all_df[c].to_numpy()[mask]) for c in ("sync_index", "cam_id", "object_id", "keypoint_id")}
            err_xy = result.err_xy if result.err_xy is not None else np.full((n_matched, 2), np.nan)  # (given errors carry no direction)
            raw_errors = pd.DataFrame({**col, "error_x": err_xy[:, 0], "error_y": err_xy[:, 1], "euclidean_error": result.err}, copy=False)
        return ReprojectionSummary(
            overall_rmse=float(np.sqrt(result.overall_sumsq / n_matched)), by_camera=by_camera, by_point=by_point,
            n_unmatched_observations=n_total - n_matched, unmatched_rate=(n_total - n_matched) / n_total, unmatched_by_camera=unmatched_by_camera,
            n_observations_matched=n_matched, n_observations_total=n_total, n_cameras=len(self.camera_array.posed_cameras),
            n_points=len(self.world_points), raw_errors=raw_errors,
        )

    def filter_outliers(self, percentile: float | None = None, *, max_pixels: float | None = None, scope: str = "per_camera", min_per_camera: int = 10,
                        _solver=None) -> "CaptureVolume":
        """``filter_by_percentile_error(percentile, scope, min_per_camera)`` or ``filter_by_absolute_error(max_pixels,
        min_per_camera)`` (exactly one of the two is given) with errors, thresholds, safety floor and keep mask from one device
        call; the volume is assembled from the mask as the host filters do (world points left without an observation are pruned,
        ``optimization_status`` is None).  The same rows survive as on the host path.  When an error is not finite the call is
        logged and the host filter's result is returned.  ``_solver`` replaces the device call (tests)."""
        if (percentile is None) == (max_pixels is None):
            raise ValueError("filter_outliers takes exactly one of percentile and max_pixels")
        if percentile is not None:
            if not (0 < percentile <= 100):
                raise ValueError(f"percentile must be between 0 and 100, got {percentile}")
        elif max_pixels <= 0:
            raise ValueError(f"max_pixels must be positive, got {max_pixels}")
        if min_per_camera < 1:
            raise ValueError(f"min_per_camera must be >= 1, got {min_per_camera}")
        if percentile is not None and scope not in ("per_camera", "overall"):
            raise ValueError(f"scope must be 'per_camera' or 'overall', got {scope}")
        mode = dict(mode="percentile", value=float(percentile), scope=scope) if percentile is not None else dict(mode="absolute", value=float(max_pixels))
        result, *_ = self._reprojection_call(_solver, groups=False, want_errors=False, min_per_camera=int(min_per_camera), **mode)
        if result.n_nonfinite:
            logger.warning(f"{result.n_nonfinite} reprojection errors are not finite: filtering on the host")
            if percentile is not None:
                return self.filter_by_percentile_error(percentile, scope=scope, min_per_camera=min_per_camera)
            return self.filter_by_absolute_error(max_pixels, min_per_camera=min_per_camera)
        keep = np.asarray(result.keep, dtype=bool)
        mask, *_ = self._matched_arrays()
        keep_rows = np.zeros(len(mask), dtype=bool)  # unmatched rows go too, as in the host filters
        keep_rows[np.flatnonzero(mask)[keep]] = True
        obj = self.img_to_obj_map[keep_rows]
        seen = np.zeros(len(self.world_points), dtype=bool)
        seen[obj] = True
        new_row = np.cumsum(seen, dtype=np.int64) - 1
        return CaptureVolume(self.camera_array, self.image_points.take(keep_rows), self.world_points.take(seen), self.constraints,
                             _known_map=new_row[obj].astype(np.int32))

    # -- parameter uncertainty (caliscope_amd/uncertainty.py; the reference has none) ----------------------------------------------
    def parameter_uncertainty(self, *, refine_intrinsics: bool = False, loss: str = "linear", f_scale: float | None = None,
                              include_constraints: bool = False, pixel_sigma: float = 1.0, _solver=None):
        """How well the matched observations determine every posed camera and every world point at the volume's current parameters
        (meaningful after ``optimize()`` with the same ``refine_intrinsics`` and ``loss``): an
        :class:`~caliscope_amd.uncertainty.UncertaintyReport` in the inner-constraint gauge from one device call.  ``f_scale`` is in
        residual units and defaults to ``pixel_f_scale()``.  World points with fewer than two matched observations take no part and
        have NaN rows in ``point_cov`` / ``point_std``.  A volume with constraints raises ``CalibrationError`` unless
        ``include_constraints=True``: then the rows of its ``ConstraintSet`` are rows of the adjustment, weighted
        ``(pixel_sigma / f_median) / sigma`` as ``optimize()`` weights them (meaningful after ``optimize()`` with the same
        ``pixel_sigma``).  They couple the points of a board and fix the scale: the report has ``gauge_dim == 6``, and a world point
        takes part if it has two matched observations or is named by a row.  ``_solver`` replaces the device call (tests)."""
        from caliscope_amd.uncertainty import DeviceUncertainty, build_report

        arrays = self._build_constraint_arrays() if include_constraints and self.constraints is not None else None
        par, args, used, _, _ = self._free_network_arguments("parameter_uncertainty", "covariance", refine_intrinsics,
                                                             constraint_groups=None if arrays is None else arrays[:2], allow_constraints=include_constraints)
        backend = _solver or DeviceUncertainty()
        f_scale = self.pixel_f_scale() if f_scale is None else float(f_scale)
        if arrays is None:
            result = backend.parameter_covariance(*args, loss=loss, f_scale=f_scale)
        else:
            groups_a, groups_b, distances, sigmas = arrays
            f_median = float(np.median([cam.matrix[0, 0] for cam in self.camera_array.posed_cameras.values()]))
            new_row = np.cumsum(used, dtype=np.int64) - 1  # the rows of the call: the world points that take part
            result = backend.parameter_covariance_constrained(*args, new_row[groups_a].astype(np.int32), new_row[groups_b].astype(np.int32), distances,
                                                              (pixel_sigma / f_median) / sigmas, loss=loss, f_scale=f_scale)
        if not used.all():  # back to the rows of world_points
            point_cov = np.full((len(self.world_points), 3, 3), np.nan)
            point_cov[used] = result.point_cov
            object.__setattr__(result, "point_cov", point_cov)
        return build_report(result, [blk.cam_id for blk in par.blocks], args[1], args[3])

    def _free_network_arguments(self, method: str, what: str, refine_intrinsics: bool, constraint_groups=None, allow_constraints: bool = False):
        """What ``parameter_uncertainty`` and ``observation_reliability`` hand their device call: ``(parameterisation, the eight
        positional arguments, used world points (mask), image-point row of every observation of the call, its world-point row)``.
        Matched observations of world points with at least two of them; a volume with constraints raises ``CalibrationError``
        unless ``allow_constraints``.  ``constraint_groups`` (groups_a, groups_b): a world point one of them names takes part too,
        whatever its observations."""
        if self.constraints is not None and not allow_constraints:
            hint = f"  {method}(include_constraints=True) keeps the rows in the adjustment."
            raise CalibrationError(f"{method} handles volumes without constraints: distance constraints couple points and fix the "
                                   f"scale of the gauge.  Build the volume without its ConstraintSet to get the reprojection-only {what}.{hint}")
        mask, camera_indices, image_coords, obj_indices = self._matched_arrays()
        if int(mask.sum()) == 0:
            raise ValueError(f"No matched observations for {method}")
        par = BundleParameterization.from_camera_array(self.camera_array, n_points=len(self.world_points), refine_intrinsics=refine_intrinsics)
        tabs = par.device_tables()
        x = par.pack(self.camera_array, self.world_points.points)
        cam_x = np.zeros((len(par.blocks), 9))
        for i, (blk, off) in enumerate(zip(par.blocks, par.camera_param_offsets)):
            cam_x[i, : blk.n_params] = x[off : off + blk.n_params]
        views = np.bincount(obj_indices, minlength=len(self.world_points))
        used = views >= 2
        if constraint_groups is not None:
            for grp in constraint_groups:
                used[np.asarray(grp).reshape(-1)] = True
        if not used.any():
            raise ValueError("No world point has two matched observations")
        new_row = np.cumsum(used, dtype=np.int64) - 1
        keep = used[obj_indices]
        args = (tabs["cam_model"], tabs["cam_n_params"], tabs["cam_const"], cam_x, self.world_points.points[used], camera_indices[keep],
                new_row[obj_indices[keep]].astype(np.int32), image_coords[keep])
        return par, args, used, np.flatnonzero(mask)[keep], obj_indices[keep]

    # -- reliability of the observations (caliscope_amd/reliability.py; the reference has a percentile cut only) ---------------------
    def observation_reliability(self, *, refine_intrinsics: bool = False, loss: str = "linear", f_scale: float | None = None, delta0: float = 4.13,
                                include_constraints: bool = False, pixel_sigma: float = 1.0, _solver=None):
        """How strongly the other observations control every matched observation at the volume's current parameters (meaningful after
        ``optimize()`` with the same ``refine_intrinsics`` and ``loss``), and how far its residual is from what the adjustment allows: a
        :class:`~caliscope_amd.reliability.ReliabilityReport` from one device call, aligned to the rows of ``image_points``.  Rows that
        take no part (unmatched, or on a world point with fewer than two matched observations) are NaN.  ``f_scale`` is in residual
        units and defaults to ``pixel_f_scale()``; ``delta0`` is the non-centrality behind ``mdb_px`` (4.13: Baarda's value for a
        significance of 0.1 % and a power of 80 %, a convention).  A volume with constraints raises ``CalibrationError`` unless
        ``include_constraints=True``: then the rows of its ``ConstraintSet`` are rows of the adjustment, weighted
        ``(pixel_sigma / f_median) / sigma`` as ``optimize()`` and ``parameter_uncertainty(include_constraints=True)`` weight them, a
        world point named by a row takes part whatever its observations, the report has ``gauge_dim == 6`` and its ``constraint_*``
        arrays judge every constraint instance (``_constraint_instances()``'s order).  Under a robust loss ``w`` is an approximation.
        ``_solver`` replaces the device call (tests)."""
        from caliscope_amd.reliability import DeviceReliability, build_report

        arrays = self._build_constraint_arrays() if include_constraints and self.constraints is not None else None
        par, args, used, rows, obs_world = self._free_network_arguments("observation_reliability", "reliability report", refine_intrinsics,
                                                                        constraint_groups=None if arrays is None else arrays[:2],
                                                                        allow_constraints=include_constraints)
        backend = _solver or DeviceReliability()
        f_scale = self.pixel_f_scale() if f_scale is None else float(f_scale)
        weights, instances = None, ()
        if arrays is None:
            result = backend.observation_reliability(*args, loss=loss, f_scale=f_scale)
        else:
            groups_a, groups_b, distances, sigmas = arrays
            f_median = float(np.median([cam.matrix[0, 0] for cam in self.camera_array.posed_cameras.values()]))
            new_row = np.cumsum(used, dtype=np.int64) - 1  # the rows of the call: the world points that take part
            weights = (pixel_sigma / f_median) / sigmas
            result = backend.observation_reliability_constrained(*args, new_row[groups_a].astype(np.int32), new_row[groups_b].astype(np.int32), distances,
                                                                 weights, loss=loss, f_scale=f_scale)
            instances = [(c, si) for c, si, _, _ in self._constraint_instances()]
        return build_report(result, rows, len(self.image_points._df), args[2][args[5], 0], [blk.cam_id for blk in par.blocks], args[5], obs_world,
                            len(self.world_points), delta0=delta0, constraint_weights=weights, constraint_instances=instances)

    def filter_by_w_test(self, alpha: float = 0.001, *, refine_intrinsics: bool = False, loss: str = "linear", f_scale: float | None = None,
                         include_constraints: bool = False, pixel_sigma: float = 1.0, _solver=None) -> "CaptureVolume":
        """One pass of data snooping (Baarda's w-test): the observations whose standardised residual contradicts the adjustment at the
        two-sided significance ``alpha`` go, judged by ``observation_reliability()`` at the volume's current parameters.  A blunder
        smears onto the other observations of its point, so per world point at most ONE observation is removed: the one with the
        largest ``|w|``, if that exceeds the critical value, and never if the point would be left with fewer than two matched views.
        Unlike ``filter_outliers`` nothing goes from a volume in which nothing is wrong beyond the share ``alpha`` predicts.  The
        volume is assembled from the row mask as ``filter_outliers`` assembles it (unmatched rows go, world points left without an
        observation are pruned, ``optimization_status`` is None).  For the next pass re-optimise the result and call again.
        ``include_constraints`` / ``pixel_sigma`` as in ``observation_reliability``: the observations are then judged in the adjustment
        with the distance rows; constraint rows are reported there and never removed here."""
        from caliscope_amd.reliability import critical_value, snooping_mask

        report = self.observation_reliability(refine_intrinsics=refine_intrinsics, loss=loss, f_scale=f_scale, include_constraints=include_constraints,
                                              pixel_sigma=pixel_sigma, _solver=_solver)
        mask, _, _, obj_indices = self._matched_arrays()
        views = np.bincount(obj_indices, minlength=len(self.world_points))
        keep = snooping_mask(report.max_abs_w[mask], obj_indices, views, critical_value(alpha))
        keep_rows = np.zeros(len(mask), dtype=bool)
        keep_rows[np.flatnonzero(mask)[keep]] = True
        obj = self.img_to_obj_map[keep_rows]
        seen = np.zeros(len(self.world_points), dtype=bool)
        seen[obj] = True
        new_row = np.cumsum(seen, dtype=np.int64) - 1
        return CaptureVolume(self.camera_array, self.image_points.take(keep_rows), self.world_points.take(seen), self.constraints,
                             _known_map=new_row[obj].astype(np.int32))

    # -- scale accuracy (reference :755-831) ---------------------------------------------------------------
    def _scale_groups(self):
        """The (frame, object) groups of the scale report as flat arrays, or None when no observation carries object geometry:
        ``(sync[g], object_id[g], n_cameras[g], n_corners[g], group_start[g + 1], ent_world[e], ent_obj[e, 3])``, groups sorted by
        (sync_index, object_id), only those with at least three joined rows.  What the reference does per group with a filter of the
        whole world table and a merge is here one sort of the image rows, one of the world keys and a binary search per distinct
        (group, keypoint)."""
        idf, wdf = self.image_points._df, self.world_points._df
        loc = [idf[c].to_numpy(dtype=np.float64) for c in ("obj_loc_x", "obj_loc_y", "obj_loc_z")]
        rows = np.flatnonzero(~(np.isnan(loc[0]) | np.isnan(loc[1])))
        if rows.size == 0:
            return None
        sync, obj, kp, cam = (idf[c].to_numpy()[rows] for c in ("sync_index", "object_id", "keypoint_id", "cam_id"))
        order = np.lexsort((obj, sync))  # stable: the rows of a group keep their table order
        rows, sync, obj, kp, cam = rows[order], sync[order], obj[order], kp[order], cam[order]
        new = np.r_[True, (sync[1:] != sync[:-1]) | (obj[1:] != obj[:-1])]
        gid = np.cumsum(new) - 1
        g_sync, g_obj = sync[new], obj[new]
        n_groups = len(g_sync)
        # distinct cameras of a group (all its rows, whether or not their keypoint has a world point)
        by_cam = np.lexsort((cam, gid))
        c2, g2 = cam[by_cam], gid[by_cam]
        n_cams = np.bincount(g2[np.r_[True, (c2[1:] != c2[:-1]) | (g2[1:] != g2[:-1])]], minlength=n_groups)
        # the object point of a keypoint: the group's first row of it
        by_kp = np.lexsort((kp, gid))
        k3, g3 = kp[by_kp], gid[by_kp]
        first = np.r_[True, (k3[1:] != k3[:-1]) | (g3[1:] != g3[:-1])]
        u_row, u_gid, u_kp = rows[by_kp][first], g3[first], k3[first]
        u_loc = np.column_stack([a[u_row] for a in loc])
        static_ids = self.constraints.static_object_ids if self.constraints else frozenset()
        g_world_sync = np.where(np.isin(g_obj, list(static_ids)), STATIC_SYNC_INDEX, g_sync) if static_ids else g_sync
        # world rows of every (group, keypoint): the three keys as ranks folded into one, duplicates of a world key all kept
        w_keys = [wdf[c].to_numpy() for c in _KEY]
        u_keys = [g_world_sync[u_gid], g_obj[u_gid], u_kp]
        w_fold, u_fold = np.zeros(len(wdf), dtype=np.int64), np.zeros(len(u_gid), dtype=np.int64)
        for w, u in zip(w_keys, u_keys):
            values = np.unique(np.concatenate([w, u]))
            w_fold = w_fold * len(values) + np.searchsorted(values, w)
            u_fold = u_fold * len(values) + np.searchsorted(values, u)
        w_order = np.argsort(w_fold, kind="stable")
        w_sorted = w_fold[w_order]
        lo, hi = np.searchsorted(w_sorted, u_fold, "left"), np.searchsorted(w_sorted, u_fold, "right")
        count = hi - lo
        e_u = np.repeat(np.arange(len(u_fold)), count)
        e_world = w_order[lo[e_u] + (np.arange(len(e_u)) - np.repeat(np.cumsum(count) - count, count))]
        e_gid, e_loc = u_gid[e_u], u_loc[e_u]
        # z: 0 for a group whose joined rows have none (a planar board), else rows without one are dropped
        z_missing = np.isnan(e_loc[:, 2])
        all_missing = np.bincount(e_gid, weights=z_missing, minlength=n_groups) == np.bincount(e_gid, minlength=n_groups)
        e_loc[all_missing[e_gid] & z_missing, 2] = 0.0
        keep = ~np.isnan(e_loc[:, 2])
        e_world, e_gid, e_loc = e_world[keep], e_gid[keep], e_loc[keep]
        size = np.bincount(e_gid, minlength=n_groups)
        good = size >= 3
        keep = good[e_gid]
        e_world, e_gid, e_loc = e_world[keep], e_gid[keep], e_loc[keep]
        in_table_order = np.lexsort((e_world, e_gid))  # (the left table of the reference's merge is the world table)
        group_start = np.concatenate([[0], np.cumsum(size[good])]).astype(np.int64)
        return (g_sync[good], g_obj[good], n_cams[good], size[good], group_start, e_world[in_table_order].astype(np.int64),
                np.ascontiguousarray(e_loc[in_table_order]))

    def compute_volumetric_scale_accuracy(self, *, _solver=None) -> VolumetricScaleReport:
        """Per (frame, rigid object): all pairwise distances of the triangulated corners against the object's own geometry
        (``obj_loc``), in millimetres; distances between different objects are never formed.  An empty report when no observation
        carries object geometry.  The distances are one device call (``cba_scale_errors``); ``_solver`` replaces it (tests)."""
        static_ids = self.constraints.static_object_ids if self.constraints else frozenset()
        groups = self._scale_groups()
        if groups is None:
            return VolumetricScaleReport.empty()
        g_sync, g_obj, n_cams, n_corners, group_start, ent_world, ent_obj = groups
        if len(g_sync) == 0:
            return VolumetricScaleReport(frame_errors=(), static_object_ids=static_ids)
        backend = _solver or DeviceScaleErrors()
        stats = backend.scale_errors(self.world_points.points, group_start, ent_world, ent_obj)
        return VolumetricScaleReport(frame_errors=frame_errors_from_stats(stats, g_sync, g_obj, n_corners, n_cams), static_object_ids=static_ids)

    # -- the frame and the scale of a solved volume (reference :833-1329) ------------------------------------
    def _transformed(self, transform: SimilarityTransform) -> "CaptureVolume":
        """This volume in another frame: new cameras and points, the same observations, constraints and optimisation status.
        Coordinates change, keys do not: the observation -> world-point map and the constraint rows are handed on."""
        cameras, points = apply_similarity_transform(self.camera_array, self.world_points, transform)
        out = CaptureVolume(camera_array=cameras, image_points=self.image_points, world_points=points, constraints=self.constraints,
                            _optimization_status=self._optimization_status, _known_map=self.img_to_obj_map)
        kept = getattr(self, "_constraint_cache", None)
        if kept is not None:
            object.__setattr__(out, "_constraint_cache", kept)
        return out

    def align_to_object(self, sync_index: int | None, object_id: int | None = None) -> "CaptureVolume":
        """Move the volume into the frame of one rigid object at one sync index (a rigid fit of its triangulated corners to their
        ``obj_loc``): origin and axes are the object's own.  ``object_id`` may be left out when the frame shows one object only.
        ``sync_index=None`` is for a static marker, whose world points sit at ``STATIC_SYNC_INDEX``."""
        idf, wdf = self.image_points._df, self.world_points._df
        static_ids = self.constraints.static_object_ids if self.constraints else frozenset()
        if sync_index is None:
            if object_id is None:
                raise ValueError("sync_index=None requires an explicit object_id")
            if object_id not in static_ids:
                raise ValueError(f"sync_index=None is only valid for static markers, but object_id={object_id} is not static")
        img_rows = np.flatnonzero(idf["sync_index"].to_numpy() == sync_index) if sync_index is not None else np.arange(len(idf))
        if img_rows.size == 0:
            raise ValueError(f"No image observations at sync_index={sync_index}")
        img_obj = idf["object_id"].to_numpy()[img_rows]
        if object_id is None:
            present = pd.unique(img_obj)
            if len(present) > 1:
                raise ValueError(f"Multiple markers present at sync_index {sync_index}; specify object_id (available: {sorted(present)})")
            object_id = int(present[0])
        world_si = STATIC_SYNC_INDEX if object_id in static_ids else (sync_index if sync_index is not None else 0)
        img_rows = img_rows[img_obj == object_id]
        world_rows = np.flatnonzero((wdf["sync_index"].to_numpy() == world_si) & (wdf["object_id"].to_numpy() == object_id))
        if img_rows.size == 0:
            raise ValueError(f"No image observations for object_id={object_id} at sync_index={sync_index}")
        if world_rows.size == 0:
            raise ValueError(f"No world points for object_id={object_id} at sync_index={world_si}")
        # object point of a keypoint: its first observation; world rows in table order, each with the object point of its keypoint
        kp_img = idf["keypoint_id"].to_numpy()[img_rows]
        kps, first = np.unique(kp_img, return_index=True)
        kp_world = wdf["keypoint_id"].to_numpy()[world_rows]
        at = np.minimum(np.searchsorted(kps, kp_world), len(kps) - 1)
        hit = kps[at] == kp_world
        src_rows, loc_rows = world_rows[hit], img_rows[first[at[hit]]]
        target = np.column_stack([idf[c].to_numpy(dtype=np.float64)[loc_rows] for c in ("obj_loc_x", "obj_loc_y", "obj_loc_z")]).reshape(-1, 3)
        if np.isnan(target[:, 2]).all():
            logger.info("obj_loc_z is all NaN, assuming planar board with z=0")
            target[:, 2] = 0.0
        valid = ~np.isnan(target).any(axis=1)
        if int(valid.sum()) < 3:
            raise ValueError(f"Need at least 3 valid correspondences for object_id={object_id}, got {int(valid.sum())}")
        source = self.world_points.points[src_rows[valid]]
        transform = estimate_similarity_transform(source, target[valid], rigid=True)
        logger.info(f"Estimated alignment: scale={transform.scale:.6f}, translation={transform.translation}, "
                    f"rotation_det={np.linalg.det(transform.rotation):.6f}")
        return self._transformed(transform)

    def rotate(self, axis: str, angle_degrees: float) -> "CaptureVolume":
        """Rotate the coordinate system about "x", "y" or "z" (right-hand rule, degrees); cameras and points move together."""
        if axis not in ("x", "y", "z"):
            raise ValueError(f"Invalid axis '{axis}'. Must be 'x', 'y', or 'z'")
        angle = np.radians(angle_degrees)
        c, s = np.cos(angle), np.sin(angle)
        k = "xyz".index(axis)
        a, b = (k + 1) % 3, (k + 2) % 3
        rotation = np.eye(3, dtype=np.float64)
        rotation[a, a], rotation[a, b], rotation[b, a], rotation[b, b] = c, -s, s, c
        return self._transformed(SimilarityTransform(rotation=rotation, translation=np.zeros(3, dtype=np.float64), scale=1.0))

    def translate(self, x: float = 0.0, y: float = 0.0, z: float = 0.0) -> "CaptureVolume":
        """Shift the coordinate system by (x, y, z) metres: added to every world point, the cameras carried along."""
        return self._transformed(SimilarityTransform(rotation=np.eye(3, dtype=np.float64), translation=np.array([x, y, z], dtype=np.float64), scale=1.0))

    def _anchor_cam_id(self) -> int:
        """The lowest posed cam_id: the camera that fixes yaw and the XY origin of a volume without a board."""
        posed = self.camera_array.posed_cameras
        if not posed:
            raise ValueError("No posed cameras; cannot anchor a shape-only volume.")
        return min(posed)

    def _camera_center(self, cam_id: int) -> np.ndarray:
        cam = self.camera_array.cameras[cam_id]
        if cam.rotation is None or cam.translation is None:
            raise ValueError(f"Camera {cam_id} has no pose; cannot compute its center.")
        return -cam.rotation.T @ cam.translation

    def scaled(self, *cues) -> "CaptureVolume":
        """Uniform scale from one or more metric cues (:mod:`caliscope_amd.scale_cues`).  One cue sets the scale exactly; several
        are combined by least squares weighted with their ``sigma_m``, and two whose implied scales differ by more than 2 sigma
        raise a ``warnings.warn``.  ``CameraDistance`` and ``SegmentLength`` are strict (``ValueError`` for a camera or keypoint that
        is not there); ``DepthObservation`` cues that cannot be resolved are skipped with one aggregated warning.  No cue, or none
        that resolves, is a ``ValueError``."""
        if not cues:
            raise ValueError("scaled() requires at least one cue; got none.")
        depth_cues = [cue for cue in cues if isinstance(cue, DepthObservation)]
        depth_outcome = iter(self._compile_depth_cues(depth_cues))
        compiled, skipped = [], []
        for cue in cues:
            if isinstance(cue, DepthObservation):
                outcome = next(depth_outcome)
                (skipped if isinstance(outcome, str) else compiled).append(outcome)
            else:
                compiled.append(self._compile_cue(cue))
        if skipped:
            breakdown = ", ".join(f"{count} {reason}" for reason, count in sorted(Counter(skipped).items()))
            warnings.warn(f"Skipped {len(skipped)} of {len(depth_cues)} depth cues as unresolvable ({breakdown}).", stacklevel=2)
        if not compiled:
            raise ValueError(f"All {len(cues)} scale cues were unresolvable; cannot determine scale.")
        d_arb, d_met, sigma = (np.array([c[k] for c in compiled], dtype=np.float64) for k in range(3))
        if len(compiled) == 1:
            scale = float(d_met[0] / d_arb[0])
        else:
            scale = float(np.sum(d_met * d_arb / sigma**2)) / float(np.sum(d_arb**2 / sigma**2))
            implied, sigma_scale = d_met / d_arb, sigma / d_arb
            two_sigma = 2.0 * np.hypot(sigma_scale[:, None], sigma_scale[None, :])
            apart = np.abs(implied[:, None] - implied[None, :]) > two_sigma
            for i, j in np.argwhere(np.triu(apart, 1)).tolist():  # (row-major: the order of the reference's double loop)
                warnings.warn(f"Scale cues {i} and {j} disagree: implied scales {implied[i]:.6g} vs {implied[j]:.6g} differ by more than "
                              f"2 sigma ({float(two_sigma[i, j]):.6g}).", stacklevel=2)
        return self._transformed(SimilarityTransform(rotation=np.eye(3, dtype=np.float64), translation=np.zeros(3, dtype=np.float64), scale=scale))

    def _compile_cue(self, cue) -> tuple[float, float, float]:
        """(distance in the volume's units, metres, sigma in metres) of a ``CameraDistance`` or ``SegmentLength``; ``ValueError``
        when it names something the volume does not have."""
        if isinstance(cue, CameraDistance):
            posed = self.camera_array.posed_cameras
            for cam_id in (cue.cam_a, cue.cam_b):
                if cam_id not in posed:
                    raise ValueError(f"CameraDistance references cam_id {cam_id}, which is not a posed camera.")
            d_arb = float(np.linalg.norm(self._camera_center(cue.cam_a) - self._camera_center(cue.cam_b)))
            if d_arb == 0.0:
                raise ValueError(f"Cameras {cue.cam_a} and {cue.cam_b} coincide; distance cue is degenerate.")
            return d_arb, float(cue.meters), float(cue.sigma_m)
        if isinstance(cue, SegmentLength):
            wdf = self.world_points._df
            coords = ["x_coord", "y_coord", "z_coord"]
            side_a = wdf[wdf["keypoint_id"] == cue.keypoint_id_a][["sync_index", "object_id", *coords]]
            side_b = wdf[wdf["keypoint_id"] == cue.keypoint_id_b][["sync_index", "object_id", *coords]]
            both = side_a.merge(side_b, on=["sync_index", "object_id"], suffixes=("_a", "_b"))
            if both.empty:
                raise ValueError(f"SegmentLength found no frame where both keypoints {cue.keypoint_id_a} and {cue.keypoint_id_b} are triangulated.")
            delta = both[[f"{c}_a" for c in coords]].to_numpy() - both[[f"{c}_b" for c in coords]].to_numpy()
            return float(np.median(np.linalg.norm(delta, axis=1))), float(cue.meters), float(cue.sigma_m)
        raise TypeError(f"Unknown scale cue type: {type(cue).__name__}")

    def _compile_depth_cues(self, cues) -> list:
        """Per ``DepthObservation``: (depth in the volume's units, metres, sigma) or the reason it cannot be used — "unposed camera",
        "no world point", "ambiguous match" (more than one world point of that keypoint at that sync index), "non-positive depth",
        tested in that order.  All cues are looked up in the world table with one sort of its (sync_index, keypoint_id) keys."""
        if not cues:
            return []
        wdf = self.world_points._df
        w_sync, w_kp = wdf["sync_index"].to_numpy(), wdf["keypoint_id"].to_numpy()
        c_sync = np.array([int(c.sync_index) for c in cues], dtype=np.int64)
        c_kp = np.array([int(c.keypoint_id) for c in cues], dtype=np.int64)
        kp_values = np.unique(np.concatenate([w_kp, c_kp]))
        sync_values = np.unique(np.concatenate([w_sync, c_sync]))
        w_fold = np.searchsorted(sync_values, w_sync) * len(kp_values) + np.searchsorted(kp_values, w_kp)
        c_fold = np.searchsorted(sync_values, c_sync) * len(kp_values) + np.searchsorted(kp_values, c_kp)
        order = np.argsort(w_fold, kind="stable")
        w_sorted = w_fold[order]
        lo = np.searchsorted(w_sorted, c_fold, "left")
        count = np.searchsorted(w_sorted, c_fold, "right") - lo
        row = order[np.minimum(lo, max(len(order) - 1, 0))] if len(order) else np.zeros(len(cues), dtype=np.int64)
        posed = self.camera_array.posed_cameras
        cam_ids = sorted(posed)
        index_of = {c: i for i, c in enumerate(cam_ids)}
        cam_idx = np.array([index_of.get(c.cam_id, -1) for c in cues], dtype=np.int64)
        z_row = np.array([posed[c].rotation[2] for c in cam_ids], dtype=np.float64).reshape(-1, 3)
        z_off = np.array([posed[c].translation[2] for c in cam_ids], dtype=np.float64)
        xyz = self.world_points.points[row] if len(order) else np.zeros((len(cues), 3))
        safe = np.maximum(cam_idx, 0)
        depth = (np.einsum("ij,ij->i", z_row[safe], xyz) + z_off[safe]) if cam_ids else np.zeros(len(cues))
        reason = np.select([cam_idx < 0, count == 0, count > 1, ~(depth > 0.0)], [1, 2, 3, 4], 0).tolist()
        names = (None, "unposed camera", "no world point", "ambiguous match", "non-positive depth")
        return [names[r] if r else (float(d), float(c.depth_m), float(c.sigma_m)) for r, d, c in zip(reason, depth.tolist(), cues)]

    def _compile_depth_cue(self, cue: DepthObservation):
        """One depth cue: ``(d_arbitrary, d_metric, sigma_m)`` or the reason it is skipped."""
        return self._compile_depth_cues([cue])[0]

    def oriented(self, up: dict) -> "CaptureVolume":
        """Rotate so that the vertical becomes +Z.  ``up``: cam_id -> that camera's up vector in its own frame; each is taken into
        the world (``R^T up``), their mean is the vertical.  Yaw: the optical axis of the anchor camera (lowest posed cam_id),
        projected onto the horizontal plane, becomes +Y.  Scale and origin stay.  The angle of every camera's vertical from the
        consensus and the largest angle between two of them are logged."""
        if not up:
            raise ValueError("oriented() requires at least one up vector.")
        world_ups = []
        for cam_id, up_cam in up.items():
            cam = self.camera_array.cameras.get(cam_id)
            if cam is None or cam.rotation is None:
                raise ValueError(f"oriented() references cam_id {cam_id}, which is not a posed camera.")
            world_ups.append(cam.rotation.T @ np.asarray(up_cam, dtype=np.float64))
        consensus = np.mean(np.stack(world_ups), axis=0)
        length = float(np.linalg.norm(consensus))
        if length < 1e-9:
            raise ValueError("Consensus up vector is degenerate (per-camera verticals cancel).")
        consensus = consensus / length
        units = np.stack([w / np.linalg.norm(w) for w in world_ups])
        from_consensus = np.degrees(np.arccos(np.clip(units @ consensus, -1.0, 1.0)))
        between = np.degrees(np.arccos(np.clip(units @ units.T, -1.0, 1.0)))[np.triu_indices(len(units), 1)]
        per_cam = ", ".join(f"cam {cam_id}: {deg:.2f}" for cam_id, deg in zip(up.keys(), from_consensus.tolist()))
        logger.info(f"Vertical agreement (deg from consensus): {per_cam}; max pairwise disagreement {float(between.max()) if between.size else 0.0:.2f}")
        forward = self.camera_array.cameras[self._anchor_cam_id()].rotation.T @ np.array([0.0, 0.0, 1.0])
        rotation = world_basis_from_up_and_forward(consensus, forward=forward)
        return self._transformed(SimilarityTransform(rotation=rotation, translation=np.zeros(3, dtype=np.float64), scale=1.0))

    def grounded(self, mode: str = "lowest_point", *, lowest_point_height_m: float = 0.0) -> "CaptureVolume":
        """Shift so that the floor is Z = 0 and the XY origin lies under the anchor camera.  The floor is the 1st percentile of the
        world Z taken as an order statistic (``method="lower"``: one stray low point does not bury it; the minimum on small sets),
        lifted by ``lowest_point_height_m`` when the lowest point is known to sit that far above the ground."""
        if mode != "lowest_point":
            raise ValueError(f"grounded() only supports mode='lowest_point', got {mode!r}.")
        floor = float(np.percentile(self.world_points._df["z_coord"].to_numpy(), 1.0, method="lower"))
        anchor = self._camera_center(self._anchor_cam_id())
        return self.translate(x=-anchor[0], y=-anchor[1], z=-floor + lowest_point_height_m)

    def centered(self) -> "CaptureVolume":
        """Shift so that the XY origin is the centroid of the posed cameras' centres; Z stays."""
        centers = np.array([self._camera_center(cam_id) for cam_id in self.camera_array.posed_cameras])
        xy = centers[:, :2].mean(axis=0)
        return self.translate(x=-xy[0], y=-xy[1])

    @classmethod
    def bootstrap(cls, image_points: ImagePoints, camera_array: CameraArray, constraints=None, *, estimate_poses: bool | str = False,
                  _triangulate=None, _pnp=None, _epi=None) -> "CaptureVolume":
        """Starting volume for ``optimize`` from 2-D observations (reference ``:268-320``): copy the cameras, triangulate
        every point seen by two or more posed cameras (on the device), keep the input untouched.

        ``estimate_poses=False`` (default): the poses the cameras already carry are used — a previous calibration, a rig
        description, another tool's estimate — and cameras that have observations but no pose raise ``CalibrationError``.
        ``estimate_poses=True``: the reference's order — copy the cameras, build the pose network from the board views
        (PnP per view on the device, :mod:`caliscope_amd.pose_network`), ``apply_to`` the copy (any pose a camera carried
        is replaced), then triangulate.  That needs object geometry (``obj_loc``).  ``estimate_poses="pnp"`` is the same.
        ``estimate_poses="epipolar"``: the pose network from 2-D correspondences alone (essential-matrix RANSAC per camera
        pair and resection against a scaffold cloud on the device, :mod:`caliscope_amd.epipolar_pose`; ``obj_loc`` is not
        read).  ``estimate_poses="auto"``: the reference's branching, PnP with object geometry and epipolar without.  Any
        other value raises ``ValueError``.  ``_pnp`` / ``_epi`` replace the device calls of the pose network (tests).
        Validation and errors otherwise follow the reference (``:288-307``)."""
        method = pose_method(estimate_poses)
        point_cams = set(int(c) for c in image_points.df["cam_id"].unique())
        missing = point_cams - set(camera_array.cameras)
        if missing:
            raise CalibrationError(f"ImagePoints reference cameras {missing} not in the CameraArray.")
        uncalibrated = [cid for cid, cam in camera_array.cameras.items() if cam.matrix is None or cam.distortions is None]
        if uncalibrated:
            raise CalibrationError(
                f"Cannot run extrinsic calibration -- cameras {uncalibrated} have no intrinsic calibration.\n\n"
                f"Run calibrate_intrinsics() for each camera first."
            )
        if method is not None:
            from caliscope_amd.pose_network import build_paired_pose_network, has_object_geometry

            if method == "pnp" and not has_object_geometry(image_points):
                raise CalibrationError(
                    "PnP pose estimation needs object geometry: obj_loc is all NaN in these observations. Use "
                    "estimate_poses='epipolar' or 'auto' for the essential-matrix (epipolar) bootstrap, supply board observations "
                    "with obj_loc, or cameras that already carry pose estimates."
                )
            cameras = deepcopy(camera_array)
            build_paired_pose_network(image_points, cameras, method=method, _pnp=_pnp, _epi=_epi).apply_to(cameras)
        else:
            unposed = sorted(cid for cid in point_cams
                             if not camera_array.cameras[cid].ignore
                             and (camera_array.cameras[cid].rotation is None or camera_array.cameras[cid].translation is None))
            if unposed:
                raise CalibrationError(
                    f"Cameras {unposed} have observations but no pose estimate. This backend refines poses; the initial pose "
                    f"network (PnP / essential matrix) is upstream of it: load a previous calibration or supply estimates."
                )
            cameras = deepcopy(camera_array)
        static_ids = constraints.static_object_ids if constraints else frozenset()
        triangulate = _triangulate or (lambda ip, cams, static: ip.triangulate(cams, static_object_ids=static))
        world_points = triangulate(image_points, cameras, static_ids)
        return cls(camera_array=cameras, image_points=image_points, world_points=world_points, constraints=constraints)

    @classmethod
    def from_arrays(cls, camera_array: CameraArray, camera_ids, image_coords, obj_indices, points_xyz) -> "CaptureVolume":
        """Build a volume from flat arrays (synthetic scenes): observation i is keypoint 0 of object
        ``obj_indices[i]`` at sync_index 0 — one world point per object."""
        obj_indices = np.asarray(obj_indices)
        n_pts = len(points_xyz)
        img = pd.DataFrame(
            {
                "sync_index": 0, "cam_id": np.asarray(camera_ids), "object_id": obj_indices, "keypoint_id": 0,
                "img_loc_x": np.asarray(image_coords)[:, 0], "img_loc_y": np.asarray(image_coords)[:, 1],
            }
        )
        pts = np.asarray(points_xyz, dtype=np.float64)
        world = pd.DataFrame(
            {"sync_index": 0, "object_id": np.arange(n_pts), "keypoint_id": 0, "x_coord": pts[:, 0], "y_coord": pts[:, 1], "z_coord": pts[:, 2]}
        )
        return cls(camera_array, ImagePoints(img), WorldPoints(world))
