"""The solver stages of the reference's extrinsic-calibration use case, on the MI355X engine.

``calibrate_extrinsics`` (reference ``core/calibrate_extrinsics.py:44-261``) is a nine-stage pipeline; stage 3 (the pose
bootstrap) runs here with ``estimate_poses``: ``True`` for board sessions (PnP per view on the device,
``caliscope_amd/pose_network.py``), ``"epipolar"`` / ``"auto"`` for sessions without object geometry (essential-matrix RANSAC on
the device, ``caliscope_amd/epipolar_pose.py``).
Stage 4 (static-marker guard, :146-196) and stages 5-9 — the part that calls the solver three times with a filter in
between — are mirrored here, on a volume that is already bootstrapped (a dropped marker's rows are removed from
the volume instead of re-running the bootstrap).  :func:`calibrate_extrinsics` keeps the reference's entry point and its
input guards (stages 1-2, :70-143) for cameras that already carry pose estimates; stage 3 is then only the
triangulation (``CaptureVolume.bootstrap``):

  4  static-marker guard: drop a static marker whose intra-marker rigidity RMSE exceeds 25 % of its size    (:146-196)
  5  ``optimize(refine_intrinsics=False)``                          linear loss, reach the basin        (:206)
     depth-ratio gate: refine intrinsics only if every camera sees p95(z)/p5(z) >= 2.0                  (:215-226)
  6  ``optimize(refine=effective, loss="soft_l1", f_scale=1px, max_nfev=2000, ftol=1e-4, strict=False)`` (:230-238)
  7  ``filter_by_percentile_error(filter_percentile)``              per-camera, worst 2.5 %             (:244)
  8  ``optimize(refine_intrinsics=effective)``                      linear loss on the clean data       (:250)
  9  ``CalibrationRun``                                             intrinsic estimates vs anchors      (:255-316)

Cancellation is checked between stages only, as in the reference (``InterruptedError``); progress percentages
are the reference's (40, 55, 75, 90, 100).
"""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Callable

import numpy as np

from caliscope_amd.bundle_parameterization import IntrinsicEstimate
from caliscope_amd.capture_volume import CaptureVolume, pose_method
from caliscope_amd.point_data import STATIC_SYNC_INDEX

logger = logging.getLogger(__name__)

MIN_DEPTH_RATIO_FOR_INTRINSIC_REFINEMENT = 2.0  # reference calibrate_extrinsics.py:32


@dataclass(frozen=True)
class CalibrationRun:
    capture_volume: CaptureVolume
    intrinsic_estimates: tuple[IntrinsicEstimate, ...]
    synthesized_cam_ids: frozenset = frozenset()
    dropped_static_markers: tuple = ()
    intrinsic_refinement_gated: bool = False


def compute_depth_ratios(capture_volume: CaptureVolume) -> dict[int, float]:
    """Per camera p95(z)/p5(z) of the moving world points in that camera's frame (reference
    ``core/scale_accuracy.py:210-234``); NaN for a camera with fewer than two positive depths."""
    world = capture_volume.world_points._df
    moving = world[world["sync_index"] != STATIC_SYNC_INDEX]
    cams = capture_volume.camera_array.posed_cameras
    if moving.empty:
        return {cam_id: float("nan") for cam_id in cams}
    pts = moving[["x_coord", "y_coord", "z_coord"]].to_numpy()
    out = {}
    for cam_id, cam in cams.items():
        z = pts @ np.asarray(cam.rotation)[2] + float(np.asarray(cam.translation).ravel()[2])
        z = z[z > 0]
        out[cam_id] = float(np.percentile(z, 95) / np.percentile(z, 5)) if z.size >= 2 else float("nan")
    return out


def _intrinsic_estimates(capture_volume: CaptureVolume, anchors: dict) -> tuple:
    out = []
    for cam_id, cam in capture_volume.camera_array.posed_cameras.items():
        if cam_id in anchors and cam.matrix is not None and cam.distortions is not None:
            f0, k10, k20 = anchors[cam_id]
            d = np.asarray(cam.distortions).ravel()
            out.append(IntrinsicEstimate(cam_id, float(cam.matrix[0, 0]), float(d[0]), float(d[1]), f0, k10, k20))
    return tuple(out)


def refresh_run(previous: CalibrationRun, capture_volume: CaptureVolume) -> CalibrationRun:
    """Rebuild the run around a re-optimised volume (reference :263-283): the initial anchors, synthesised cameras, dropped
    markers and the gate flag are kept, the recovered intrinsics are read again."""
    anchors = {e.cam_id: (e.f_initial, e.k1_initial, e.k2_initial) for e in previous.intrinsic_estimates}
    return CalibrationRun(capture_volume, _intrinsic_estimates(capture_volume, anchors), previous.synthesized_cam_ids,
                          previous.dropped_static_markers, previous.intrinsic_refinement_gated)


def apply_static_marker_guard(capture_volume: CaptureVolume) -> tuple[CaptureVolume, tuple[int, ...]]:
    """Stage 4: a "static" marker that moved during the recording shows up as a non-rigid set of triangulated corners.
    Markers whose intra-marker rigidity RMSE exceeds 25 % of their largest corner distance are dropped: their
    observations, world points and every constraint that names them (reference :146-186)."""
    from caliscope_amd.constraints import ConstraintSet, RigidityReport
    from caliscope_amd.point_data import ImagePoints, WorldPoints

    con = capture_volume.constraints
    if con is None or not con.static_object_ids:
        return capture_volume, ()
    intra = tuple(v for v in capture_volume.rigidity_report().violations if v.object_id_a == v.object_id_b)
    rmse = RigidityReport(violations=intra).per_object_rmse_mm
    dropped = []
    for obj in sorted(con.static_object_ids):
        size_mm = 1000.0 * max((d.distance for d in con.distances if d.object_id_a == obj and d.object_id_b == obj), default=0.0)
        if size_mm > 0 and rmse.get(obj, 0.0) > 0.25 * size_mm:
            logger.warning(f"Dropping static marker {obj}: rigidity RMSE {rmse[obj]:.1f}mm > 25% of max intra-distance {size_mm:.1f}mm")
            dropped.append(obj)
    if not dropped:
        return capture_volume, ()
    gone = set(dropped)
    img = capture_volume.image_points.df
    world = capture_volume.world_points.df
    kept = ConstraintSet(
        distances=tuple(d for d in con.distances if d.object_id_a not in gone and d.object_id_b not in gone),
        static_object_ids=con.static_object_ids - frozenset(gone),
        centroid_distances=tuple(c for c in con.centroid_distances if c.object_id_a not in gone and c.object_id_b not in gone),
        point_remaps=con.point_remaps,
    )
    vol = CaptureVolume(capture_volume.camera_array, ImagePoints(img[~img["object_id"].isin(gone)].reset_index(drop=True)),
                        WorldPoints(world[~world["object_id"].isin(gone)].reset_index(drop=True)), kept)
    return vol, tuple(dropped)


def _validate_two_sided_extraction(image_points, thickness_m: float) -> None:
    """The identity scheme of a two-sided board is frozen into the extraction (object 1 = back face, ``obj_loc_z`` =
    thickness) while the constraints are compiled from the current configuration: a mismatch would silently drop every
    cross-face row, so it is an error (reference :328-370)."""
    from caliscope_amd.exceptions import CalibrationError

    df = image_points.df
    observed = {int(o) for o in df["object_id"].unique()}
    expected = {0, 1} if thickness_m > 0 else {0}
    if observed != expected:
        if thickness_m > 0 and 1 not in observed:
            detail = ("board thickness is set but the extraction has no back-face observations (object_id 1): re-extract, or "
                      "set thickness to 0 if only one face was filmed.")
        elif thickness_m == 0 and 1 in observed:
            detail = ("the extraction contains back-face observations (object_id 1) but board thickness is 0: re-extract, or "
                      "restore the thickness the extraction was made with.")
        else:
            detail = "re-extract with the current board configuration."
        raise CalibrationError(f"Extraction/config identity mismatch: observed object_ids {sorted(observed)}, configured "
                               f"thickness implies {sorted(expected)} — {detail}")
    if thickness_m > 0:
        extracted = float(df.loc[df["object_id"] == 1, "obj_loc_z"].iloc[0])
        if abs(extracted - thickness_m) > 1e-9:
            raise CalibrationError(f"Board thickness changed since extraction: extraction carries back-face obj_loc "
                                   f"z={extracted * 100:.2f}cm but configured thickness is {thickness_m * 100:.2f}cm. Re-extract, "
                                   f"or restore the original thickness.")


def _count_firing_cross_face_rows(world_df, distances) -> int:
    """Cross-object distance rows whose two endpoints are triangulated at one common sync index at least — the join
    ``_build_constraint_arrays`` performs (reference :373-391), on integer keys instead of per-row Python sets."""
    cross = [d for d in distances if d.object_id_a != d.object_id_b]
    if not cross or len(world_df) == 0:
        return 0
    triples = set(zip(world_df["object_id"].astype(int).tolist(), world_df["keypoint_id"].astype(int).tolist(),
                      world_df["sync_index"].astype(int).tolist()))
    by_point: dict = {}
    for o, k, s in triples:
        by_point.setdefault((o, k), set()).add(s)
    return sum(1 for d in cross if by_point.get((d.object_id_a, d.keypoint_id_a), set()) & by_point.get((d.object_id_b, d.keypoint_id_b), set()))


MAX_PLAUSIBLE_INTRINSIC_RMSE = 0.005   # of max(width, height): 9.6 px at 1920; board corners are detected to a fraction of a pixel
PLAUSIBLE_FOCAL_RANGE = (0.1, 10.0)    # of max(width, height): fields of view from ~6 to ~157 degrees


def _plausible_intrinsics(cam, report) -> str | None:
    """Why the calibrated intrinsics of ``cam`` are not taken over (None: they are).  A least-squares minimum can be a wrong one
    (views that are not rigid, a mislabelled object): its reprojection error or its focal length then give it away."""
    m = float(max(cam.size))
    res = report.result
    if not res.reprojection_error <= MAX_PLAUSIBLE_INTRINSIC_RMSE * m:
        return f"reprojection RMSE {res.reprojection_error:.1f} px exceeds {MAX_PLAUSIBLE_INTRINSIC_RMSE * m:.1f} px"
    for f in (res.camera_matrix[0, 0], res.camera_matrix[1, 1]):
        if not PLAUSIBLE_FOCAL_RANGE[0] * m <= f <= PLAUSIBLE_FOCAL_RANGE[1] * m:
            return f"focal length {f:.0f} px is outside [{PLAUSIBLE_FOCAL_RANGE[0] * m:.0f}, {PLAUSIBLE_FOCAL_RANGE[1] * m:.0f}]"
    return None


def _estimate_missing_intrinsics(image_points, cameras, _intr) -> dict:
    """``estimate_intrinsics=True``: ``{cam_id: (matrix, distortions, error, grid_count)}`` of the non-ignored cameras without
    intrinsics that the board views calibrate (whatever pose bootstrap follows: the views carry ``obj_loc``).  Without object
    geometry there is nothing to calibrate against: the existing error of ``calibrate_extrinsics``.  A camera whose calibration
    does not solve, or solves to an implausible minimum, is left without intrinsics (the caller then falls back to blind defaults)."""
    from caliscope_amd.calibrate_intrinsics import calibrate_camera_array_intrinsics
    from caliscope_amd.exceptions import CalibrationError

    missing = sorted(c.cam_id for c in cameras.cameras.values() if not c.ignore and (c.matrix is None or c.distortions is None))
    if not missing:
        return {}
    df = image_points.df
    if bool(df[["obj_loc_x", "obj_loc_y", "obj_loc_z"]].isna().all().all()):
        raise CalibrationError(
            f"Epipolar bootstrap requires calibrated intrinsics, but cameras {missing} have none and fell back to "
            f"blind defaults (f=width/2). Without object geometry there is no anchor to absorb the focal-length error: "
            f"supply real intrinsics first, then re-run extrinsic calibration."
        )
    calibrated, reports = calibrate_camera_array_intrinsics(image_points, cameras, only_missing=True, _solver=_intr)
    out = {}
    for cam_id in missing:
        if reports[cam_id].result is None:
            logger.warning(f"Camera {cam_id}: intrinsic calibration from the board views did not solve; falling back to blind defaults")
            continue
        why = _plausible_intrinsics(calibrated.cameras[cam_id], reports[cam_id])
        if why is not None:
            logger.warning(f"Camera {cam_id}: intrinsic calibration from the board views rejected ({why}); falling back to blind defaults")
            continue
        cam = calibrated.cameras[cam_id]
        out[cam_id] = (cam.matrix, cam.distortions, cam.error, cam.grid_count)
    return out


def _apply_estimated_intrinsics(cameras, estimated: dict) -> None:
    for cam_id, (matrix, distortions, error, grid_count) in estimated.items():
        cam = cameras.cameras[cam_id]
        cam.matrix, cam.distortions, cam.error, cam.grid_count = matrix.copy(), distortions.copy(), error, grid_count


def calibrate_extrinsics(
    image_points,
    camera_array,
    constraints,
    *,
    refine_intrinsics: bool = True,
    filter_percentile: float = 2.5,
    cancellation_token=None,
    progress: Callable[[int, str], None] | None = None,
    estimate_poses: bool | str = False,
    estimate_intrinsics: bool = False,
    device_filter: bool = False,
    _engine_factory=None,
    _triangulate=None,
    _pnp=None,
    _epi=None,
    _intr=None,
) -> CalibrationRun:
    """The reference's entry point (``calibrate_extrinsics.py:44-261``, same arguments, progress marks and errors): blind
    intrinsics for uncalibrated cameras, the extraction guards, the bootstrap (triangulation on the device; with
    ``estimate_poses=True`` first the pose network from the board views, as the reference always does; ``"epipolar"`` / ``"auto"``
    as ``CaptureVolume.bootstrap`` takes them), static-marker guard, the three solver passes with the filter in between.
    ``estimate_poses=False`` needs cameras that carry pose estimates.  ``estimate_intrinsics=True``: cameras without intrinsics are
    calibrated from the session's board views on the device (``caliscope_amd/calibrate_intrinsics.py``, all of them in one call)
    instead of receiving blind defaults, which also makes fisheye cameras without intrinsics usable; they are not listed in
    ``synthesized_cam_ids``.  A camera whose calibration does not solve, or ends at an implausible minimum (reprojection RMSE above
    0.5 % of the image size, focal length outside 0.1 ... 10 image sizes), falls back to the blind defaults and is listed.
    ``device_filter=True``: the outlier filter between the passes is ``CaptureVolume.filter_outliers`` (errors, thresholds and keep mask
    in one device call) instead of ``filter_by_percentile_error``; the same observations survive."""
    from copy import deepcopy

    from caliscope_amd.exceptions import CalibrationError

    def report(pct, msg):
        if progress is not None:
            progress(pct, msg)

    def check_cancelled():
        if cancellation_token is not None and getattr(cancellation_token, "is_cancelled", False):
            raise InterruptedError("Calibration cancelled")

    report(5, "Preparing cameras")
    cameras = deepcopy(camera_array)
    synthesized = set()
    estimated = {}
    if estimate_intrinsics:
        estimated = _estimate_missing_intrinsics(image_points, cameras, _intr)
        _apply_estimated_intrinsics(cameras, estimated)
    for cam in cameras.cameras.values():
        if not cam.ignore and (cam.matrix is None or cam.distortions is None):
            synthesized.add(cam.cam_id)
            cam.synthesize_default_intrinsics()
    df = image_points.df
    method = pose_method(estimate_poses)
    no_geometry = bool(df[["obj_loc_x", "obj_loc_y", "obj_loc_z"]].isna().all().all())
    # the essential-matrix path has no obj_loc anchor to absorb a focal-length error: gate on the path that will run
    if synthesized and (no_geometry or method == "epipolar"):
        raise CalibrationError(
            f"Epipolar bootstrap requires calibrated intrinsics, but cameras {sorted(synthesized)} have none and fell back to "
            f"blind defaults (f=width/2). Without object geometry there is no anchor to absorb the focal-length error: "
            f"supply real intrinsics first, then re-run extrinsic calibration."
        )
    anchors = {}
    for cam in cameras.cameras.values():
        if not cam.ignore and cam.matrix is not None and cam.distortions is not None:
            d = np.asarray(cam.distortions).ravel()
            anchors[cam.cam_id] = (float(cam.matrix[0, 0]), float(d[0]), float(d[1]))
    if constraints is not None and constraints.back_face_thickness_m is not None:
        _validate_two_sided_extraction(image_points, constraints.back_face_thickness_m)
    if constraints is not None:
        image_points = constraints.remap_image_points(image_points)
    check_cancelled()

    report(15, "Bootstrapping poses")
    volume = CaptureVolume.bootstrap(image_points, cameras, constraints=constraints, estimate_poses=estimate_poses, _triangulate=_triangulate,
                                     _pnp=_pnp, _epi=_epi)
    if constraints is not None and (constraints.back_face_thickness_m or 0) > 0:
        firing = _count_firing_cross_face_rows(volume.world_points.df, constraints.distances)
        total = sum(1 for d in constraints.distances if d.object_id_a != d.object_id_b)
        logger.info(f"Cross-face constraints firing: {firing}/{total} rows across all sync indices")
        if firing == 0:
            raise CalibrationError(
                "No cross-face constraint fires: no sync index has both the front and the mirrored face triangulated (each "
                "face needs >= 2 cameras simultaneously). The front-viewing and back-viewing camera groups have no rigid "
                "link, so calibration would be arbitrary."
            )
    check_cancelled()
    # static-marker guard as the reference runs it (:146-203): decide on the first triangulation, then START AGAIN without the dropped markers —
    # fresh copies of the caller's cameras, the 20 % progress mark, a second bootstrap (the reference's pose network could change without the bad
    # marker; here the poses are the caller's, so the second triangulation only loses the marker's points) — pinned against the reference's own
    # run of this function with the heavy calls scripted (tests/golden/reference_host/driver_03.npz)
    guarded, dropped = apply_static_marker_guard(volume)
    if dropped:
        report(20, "Re-bootstrapping after dropping markers")
        cameras = deepcopy(camera_array)
        _apply_estimated_intrinsics(cameras, estimated)
        for cam in cameras.cameras.values():
            if not cam.ignore and cam.cam_id in synthesized:
                cam.synthesize_default_intrinsics()
        # (with estimate_poses the pose network is rebuilt without the dropped markers' views, as the reference does)
        volume = CaptureVolume.bootstrap(guarded.image_points, cameras, constraints=guarded.constraints, estimate_poses=estimate_poses,
                                         _triangulate=_triangulate, _pnp=_pnp, _epi=_epi)
    check_cancelled()
    run = refine_calibration(volume, refine_intrinsics=refine_intrinsics, filter_percentile=filter_percentile,
                             cancellation_token=cancellation_token, progress=progress, device_filter=device_filter,
                             _engine_factory=_engine_factory, _guard=False)
    estimates = _intrinsic_estimates(run.capture_volume, anchors)
    return CalibrationRun(run.capture_volume, estimates, frozenset(synthesized), tuple(dropped), run.intrinsic_refinement_gated)


def refine_calibration(
    capture_volume: CaptureVolume,
    *,
    refine_intrinsics: bool = True,
    filter_percentile: float = 2.5,
    cancellation_token=None,
    progress: Callable[[int, str], None] | None = None,
    device_filter: bool = False,
    _engine_factory=None,
    _guard: bool = True,
) -> CalibrationRun:
    """Stages 5-9 of ``calibrate_extrinsics`` on a bootstrapped volume (``_guard=False``: the caller has run the static-marker guard;
    ``device_filter=True``: stage 7 is ``filter_outliers``, one device call, instead of ``filter_by_percentile_error``)."""

    def check_cancelled():
        if cancellation_token is not None and getattr(cancellation_token, "is_cancelled", False):
            raise InterruptedError("Extrinsic calibration cancelled")

    def report(pct, msg):
        if progress is not None:
            progress(pct, msg)

    anchors = {}
    for cam_id, cam in capture_volume.camera_array.posed_cameras.items():
        if cam.matrix is not None and cam.distortions is not None and not cam.fisheye:
            d = np.asarray(cam.distortions).ravel()
            anchors[cam_id] = (float(cam.matrix[0, 0]), float(d[0]), float(d[1]))

    kw = {} if _engine_factory is None else {"_engine_factory": _engine_factory}
    check_cancelled()
    dropped = ()
    if _guard:
        capture_volume, dropped = apply_static_marker_guard(capture_volume)
    check_cancelled()
    report(40, "Optimizing")
    cv = capture_volume.optimize(refine_intrinsics=False, **kw)
    check_cancelled()

    ratios = compute_depth_ratios(cv)
    effective = bool(refine_intrinsics and ratios and all(r >= MIN_DEPTH_RATIO_FOR_INTRINSIC_REFINEMENT for r in ratios.values()))
    gated = bool(refine_intrinsics and not effective)
    if gated:
        logger.warning(f"Intrinsic refinement requested but gated off (need every camera >= "
                       f"{MIN_DEPTH_RATIO_FOR_INTRINSIC_REFINEMENT}). Per-camera depth ratios: {ratios}")

    report(55, "Robust refinement")
    cv = cv.optimize(refine_intrinsics=effective, loss="soft_l1", f_scale=cv.pixel_f_scale(px=1.0), max_nfev=2000,
                     ftol=1e-4, strict=False, **kw)
    check_cancelled()

    report(75, "Filtering outliers")
    cv = cv.filter_outliers(filter_percentile) if device_filter else cv.filter_by_percentile_error(filter_percentile, **kw)
    check_cancelled()

    report(90, "Re-optimizing")
    cv = cv.optimize(refine_intrinsics=effective, **kw)

    report(100, "Optimization complete")
    return CalibrationRun(cv, _intrinsic_estimates(cv, anchors), dropped_static_markers=dropped, intrinsic_refinement_gated=gated)
