"""Scale report and anchoring of a volume on the CPU: against the reference's own outputs (tests/golden/anchoring, written by
tests/golden/make_anchoring_fixtures.py), the algebra of the transforms, and the arithmetic and lane-to-pair mapping of
cba_scale_errors in its g++ build (tests/scale_native.py) against scipy and an ``np.longdouble`` evaluation.

The bounds on the statistics are derived in tests/scale_scenes.py."""
import json
import logging
import warnings
from dataclasses import FrozenInstanceError
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from scipy.spatial.distance import pdist

from caliscope_amd.alignment import SimilarityTransform, apply_similarity_transform, estimate_similarity_transform
from caliscope_amd.cameras import CameraArray, CameraData
from caliscope_amd.capture_volume import CaptureVolume
from caliscope_amd.constraints import ConstraintSet
from caliscope_amd.coordinate_frame import world_basis_from_up_and_forward
from caliscope_amd.exceptions import BackendError
from caliscope_amd.point_data import STATIC_SYNC_INDEX, ImagePoints, WorldPoints
from caliscope_amd.scale_accuracy import (DeviceScaleErrors, FrameScaleError, VolumetricScaleReport, compute_frame_scale_error)
from caliscope_amd.scale_cues import CameraDistance, DepthObservation, SegmentLength
from tests import scale_native
from tests.scale_scenes import U, assert_stats, derived_bounds, noisy_group, reference_stats, uniform_scale_scene

GOLDEN = Path(__file__).parent / "golden" / "anchoring"
CASES = sorted(GOLDEN.glob("anchor_*.npz"))
WORLD_COLS = ["sync_index", "object_id", "keypoint_id", "x_coord", "y_coord", "z_coord"]
IMG_COLS = ["sync_index", "cam_id", "object_id", "keypoint_id", "img_loc_x", "img_loc_y", "obj_loc_x", "obj_loc_y", "obj_loc_z"]
CUES = {"CameraDistance": CameraDistance, "SegmentLength": SegmentLength, "DepthObservation": DepthObservation}
HARNESS = scale_native.HarnessScaleErrors()


# ---- fixtures ----------------------------------------------------------------------------------------------------------------

def load_volume(z):
    world = pd.DataFrame(z["world"], columns=WORLD_COLS).astype({c: "int64" for c in WORLD_COLS[:3]})
    image = pd.DataFrame(z["image"], columns=IMG_COLS).astype({c: "int64" for c in IMG_COLS[:4]})
    K = np.array([[400.0, 0.0, 200.0], [0.0, 400.0, 200.0], [0.0, 0.0, 1.0]])
    cams = {}
    for c, R, t in zip(z["cam_ids"].tolist(), z["cam_R"], z["cam_t"]):
        posed = not np.isnan(R).any()
        cams[c] = CameraData(cam_id=c, size=(400, 400), matrix=K.copy(), distortions=np.zeros(5), rotation=R.copy() if posed else None,
                             translation=t.copy() if posed else None, error=0.1 * c, grid_count=c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CaptureVolume(CameraArray(cams), ImagePoints(image), WorldPoints(world), ConstraintSet((), frozenset(z["static"].tolist())))


@pytest.fixture(scope="module", params=CASES, ids=lambda p: p.stem)
def case(request):
    z = np.load(request.param)
    return z, load_volume(z)


def close(a, b, what=""):
    """1e-12 max(1, |value|): the figure of the reference-host fixture tests for rotation entries."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern"
    ok = ~np.isnan(b)
    assert np.all(np.abs(a[ok] - b[ok]) <= 1e-12 * np.maximum(1.0, np.abs(b[ok]))), f"{what}: off by {np.abs(a[ok] - b[ok]).max():.3e}"


def poses(vol, cam_ids):
    cams = vol.camera_array.cameras
    return (np.array([np.full((3, 3), np.nan) if cams[c].rotation is None else cams[c].rotation for c in cam_ids]),
            np.array([np.full(3, np.nan) if cams[c].translation is None else cams[c].translation for c in cam_ids]))


def test_fixtures_are_there():
    assert len(CASES) == 8


def test_scale_report_matches_the_reference(case):
    z, vol = case
    ref = z["frame_errors"]
    rep = vol.compute_volumetric_scale_accuracy(_solver=HARNESS)
    assert rep.static_object_ids == frozenset(z["report_static"].tolist())
    got = rep.frame_errors
    # integer fields, group order, cameras: exactly the reference's
    assert [(fe.sync_index, fe.object_id, fe.n_corners, fe.n_distance_pairs, fe.n_cameras_contributing) for fe in got] == \
        [tuple(int(v) for v in row[[0, 1, 5, 6, 7]]) for row in ref]
    assert all(type(getattr(fe, f)) is int for fe in got for f in ("sync_index", "object_id", "n_corners", "n_distance_pairs", "n_cameras_contributing"))
    # floats: within the bounds, evaluated on the joined rows (whose keys the exact fields above have just pinned)
    _, _, _, _, group_start, ent_world, ent_obj = vol._scale_groups()
    xyz = vol.world_points.points
    for g, (fe, row) in enumerate(zip(got, ref)):
        a, b = group_start[g], group_start[g + 1]
        stats, bounds, _ = reference_stats(xyz[ent_world[a:b]], ent_obj[a:b])
        tol = derived_bounds(stats, bounds)
        for k, name in ((2, "distance_rmse_mm"), (3, "distance_mean_signed_error_mm"), (4, "distance_max_error_mm"), (8, "sum_squared_errors_m2"),
                        (9, "sum_squared_relative_errors")):
            assert abs(getattr(fe, name) - row[k]) <= tol[name], f"group {g} {name}: {getattr(fe, name)!r} vs {row[k]!r}, bound {tol[name]:.3e}"
        assert np.all(np.abs(np.array(fe.centroid) - row[10:13]) <= tol["centroid"]), f"group {g} centroid"
        assert type(fe.centroid) is tuple and all(type(v) is float for v in fe.centroid)
    # the report's own properties, on the reference's entries (so that they are compared exactly)
    theirs = VolumetricScaleReport(tuple(FrameScaleError(int(r[0]), int(r[1]), r[2], r[3], r[4], int(r[5]), int(r[6]), int(r[7]), r[8], r[9], tuple(r[10:13]))
                                         for r in ref), frozenset(z["report_static"].tolist()))
    s = z["report_scalars"]
    split = theirs.split_relative_rmse_pct
    worst = theirs.worst_frame
    mine = [theirs.pooled_rmse_mm, theirs.median_rmse_mm, theirs.max_rmse_mm, theirs.n_frames_sampled, theirs.mean_signed_error_mm, theirs.min_sync_index,
            theirs.max_sync_index, theirs.pooled_relative_rmse_pct, *(np.nan if v is None else v for v in split),
            worst.sync_index if worst else -99, worst.object_id if worst else -99]
    np.testing.assert_allclose(mine, s, rtol=4 * U * max(len(ref), 1), atol=0, equal_nan=True)
    for name in ("per_frame_relative_rmse_pct", "per_frame_rmse_mm", "per_object_relative_rmse_pct"):
        d = getattr(theirs, name)
        assert list(d) == z[name][:, 0].astype(np.int64).tolist(), name
        np.testing.assert_allclose(list(d.values()), z[name][:, 1], rtol=4 * U * max(len(ref), 1), atol=0)
        assert STATIC_SYNC_INDEX not in d or name.startswith("per_object")


def run_op(vol, op):
    a = op["args"]
    name = op["op"]
    if name == "align_to_object":
        return vol.align_to_object(a["sync_index"], a["object_id"])
    if name == "rotate":
        return vol.rotate(a["axis"], a["angle_degrees"])
    if name == "translate":
        return vol.translate(**a)
    if name == "scaled":
        return vol.scaled(*[CUES[r[0]](*r[1:]) for r in a["cues"]])
    if name == "oriented":
        return vol.oriented({int(c): np.array(v) for c, v in a["up"]})
    if name == "grounded":
        return vol.grounded(a["mode"], lowest_point_height_m=a["lowest_point_height_m"])
    if name == "centered":
        return vol.centered()
    if name == "chain":
        return vol.scaled(*[CUES[r[0]](*r[1:]) for r in a["cues"]]).oriented({int(c): np.array(v) for c, v in a["up"]}).grounded().centered()
    raise AssertionError(name)


def test_operations_match_the_reference(case):
    z, vol = case
    cam_ids = z["cam_ids"].tolist()
    xyz0, (R0, t0) = vol.world_points.points, poses(vol, cam_ids)
    ops = json.loads(str(z["ops"]))
    assert len(ops) >= 40
    for k, op in enumerate(ops):
        what = f"op {k} {op['op']} {op['args']}"
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            if op["error"] is not None:
                with pytest.raises(Exception) as exc:
                    run_op(vol, op)
                assert [type(exc.value).__name__, str(exc.value)] == op["error"], what
                new = None
            else:
                new = run_op(vol, op)
        assert [str(w.message) for w in caught] == op["warnings"], what
        if new is None:
            continue
        key = op["key"]
        close(new.world_points.points, z[key + "_xyz"], what + " xyz")
        R, t = poses(new, cam_ids)
        close(R, z[key + "_R"], what + " R")
        close(t, z[key + "_t"], what + " t")
        # a new volume around the same observations, constraints, status and map; every other camera field kept
        assert new is not vol and new.image_points is vol.image_points and new.constraints is vol.constraints
        assert new.optimization_status is vol.optimization_status and np.array_equal(new.img_to_obj_map, vol.img_to_obj_map)
        assert np.array_equal(new.world_points._df[WORLD_COLS[:3]].to_numpy(), vol.world_points._df[WORLD_COLS[:3]].to_numpy())
        for c in cam_ids:
            cam, old = new.camera_array.cameras[c], vol.camera_array.cameras[c]
            assert (cam.error, cam.grid_count, cam.size, cam.ignore, cam.fisheye, cam.rotation_count, cam.exposure) == \
                (old.error, old.grid_count, old.size, old.ignore, old.fisheye, old.rotation_count, old.exposure)
            assert np.array_equal(cam.matrix, old.matrix) and np.array_equal(cam.distortions, old.distortions)
    # the inputs are untouched
    assert np.array_equal(vol.world_points.points, xyz0)
    R1, t1 = poses(vol, cam_ids)
    assert np.array_equal(R1, R0, equal_nan=True) and np.array_equal(t1, t0, equal_nan=True)


def test_depth_cue_outcomes_one_by_one(case):
    """`_compile_depth_cue` (one cue) says what the batch said inside scaled(): every skip reason the generator found is met."""
    z, vol = case
    seen = set()
    for op in json.loads(str(z["ops"])):
        if op["op"] != "scaled":
            continue
        for r in op["args"]["cues"]:
            if r[0] == "DepthObservation":
                out = vol._compile_depth_cue(DepthObservation(*r[1:]))
                seen.add(out if isinstance(out, str) else "ok")
    assert seen == set(z["depth_outcomes"].tolist())


def test_estimate_similarity_transform_matches_the_reference(case):
    z, _ = case
    for k, rec in enumerate(json.loads(str(z["est"]))):
        src, dst = z[f"est{k}_src"], z[f"est{k}_dst"]
        if rec["error"] is not None:
            with pytest.raises(Exception) as exc:
                estimate_similarity_transform(src, dst, rigid=rec["rigid"])
            assert [type(exc.value).__name__, str(exc.value)] == rec["error"]
            continue
        tr = estimate_similarity_transform(src, dst, rigid=rec["rigid"])
        close(tr.rotation, z[f"est{k}_R"], f"est {k} R")
        close(tr.translation, z[f"est{k}_t"], f"est {k} t")
        close(tr.scale, z[f"est{k}_s"], f"est {k} s")
        close(tr.inverse.matrix, z[f"est{k}_inv"], f"est {k} inverse")
        assert np.linalg.det(tr.rotation) > 0


# ---- messages of the small classes ---------------------------------------------------------------------------------------------

def test_similarity_transform_validation():
    eye, zero = np.eye(3), np.zeros(3)
    with pytest.raises(ValueError, match=r"Rotation must be 3x3, got \(2, 2\)"):
        SimilarityTransform(np.eye(2), zero, 1.0)
    with pytest.raises(ValueError, match=r"Rotation must be proper \(det=\+1\), got det=-1.000000"):
        SimilarityTransform(np.diag([1.0, 1.0, -1.0]), zero, 1.0)
    with pytest.raises(ValueError, match="Rotation matrix must be orthogonal"):
        SimilarityTransform(np.array([[1.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), zero, 1.0)
    with pytest.raises(ValueError, match=r"Translation must be 3-vector, got \(2,\)"):
        SimilarityTransform(eye, np.zeros(2), 1.0)
    with pytest.raises(ValueError, match="Scale must be positive, got 0.0"):
        SimilarityTransform(eye, zero, 0.0)
    with pytest.raises(ValueError, match=r"Points must be Nx3 array, got shape \(3,\)"):
        SimilarityTransform(eye, zero, 1.0).apply(np.zeros(3))
    with pytest.raises(ValueError, match="Point arrays must have same shape"):
        estimate_similarity_transform(np.zeros((3, 3)), np.zeros((4, 3)))
    with pytest.raises(ValueError, match=r"Points must be 3D \(Nx3\), got shape \(4, 2\)"):
        estimate_similarity_transform(np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="Input points cannot contain NaN values"):
        estimate_similarity_transform(np.full((4, 3), np.nan), np.zeros((4, 3)))
    with pytest.raises(FrozenInstanceError):
        SimilarityTransform(eye, zero, 1.0).scale = 2.0


def test_cue_defaults_and_basis():
    assert CameraDistance(0, 1, 2.0).sigma_m == 0.01 and SegmentLength(0, 1, 2.0).sigma_m == 0.02 and DepthObservation(0, 1, 2, 3.0).sigma_m == 0.1
    R = world_basis_from_up_and_forward([0.0, -2.0, 0.0], forward=[0.0, 0.3, 1.0])
    np.testing.assert_allclose(R, [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]], atol=1e-15)
    with pytest.raises(ValueError, match="forward points along gravity"):
        world_basis_from_up_and_forward([0.0, 0.0, 1.0], forward=[0.0, 0.0, -3.0])


def test_compute_frame_scale_error_errors_and_backend():
    with pytest.raises(ValueError, match=r"Shape mismatch: world_points \(3, 3\) vs object_points \(4, 3\)"):
        compute_frame_scale_error(np.zeros((3, 3)), np.zeros((4, 3)), 0, 0, 1, _solver=HARNESS)
    with pytest.raises(ValueError, match="Need at least 2 points to compute distances, got 1"):
        compute_frame_scale_error(np.zeros((1, 3)), np.zeros((1, 3)), 0, 0, 1, _solver=HARNESS)
    rng = np.random.default_rng(5)
    obj = rng.normal(size=(7, 3))
    world = 1.01 * obj + 0.5
    fe = compute_frame_scale_error(world, obj, 4, 9, 3, _solver=HARNESS)
    stats, bounds, err = reference_stats(world, obj)
    tol = derived_bounds(stats, bounds)
    assert (fe.sync_index, fe.object_id, fe.n_corners, fe.n_distance_pairs, fe.n_cameras_contributing) == (4, 9, 7, 21, 3)
    assert abs(fe.distance_rmse_mm - 1000 * np.sqrt(np.mean(err ** 2))) <= tol["distance_rmse_mm"]
    assert abs(fe.distance_mean_signed_error_mm - 1000 * err.mean()) <= tol["distance_mean_signed_error_mm"]
    assert abs(fe.sum_squared_relative_errors - (err ** 2).sum() / pdist(obj).max() ** 2) <= tol["sum_squared_relative_errors"]
    from caliscope_amd.calibrate_extrinsics import compute_depth_ratios
    from caliscope_amd import scale_accuracy

    assert scale_accuracy.compute_depth_ratios is compute_depth_ratios
    empty = VolumetricScaleReport.empty()
    assert empty.frame_errors == () and empty.pooled_rmse_mm == 0.0 and empty.worst_frame is None and empty.split_relative_rmse_pct == (None, None)
    assert empty.per_frame_rmse_mm == {} and empty.min_sync_index == 0 and empty.n_frames_sampled == 0 and empty.median_rmse_mm == 0.0


def test_library_checks_its_input_and_has_no_cpu_fallback():
    """The host side of cba_scale_errors in the built library: input errors name the position; without a device a valid call is
    BackendError (CBA_ERR_NO_DEVICE), never a number."""
    from caliscope_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    dev = DeviceScaleErrors()
    world, obj = np.zeros((5, 3)), np.zeros((4, 3))
    with pytest.raises(BackendError, match=r"code -1\).*entry 2: world row 5 out of range \[0, 5\)"):
        dev.scale_errors(world, [0, 4], [0, 1, 5, 2], obj)
    with pytest.raises(BackendError, match=r"code -1\).*entry 0: world row -1 out of range"):
        dev.scale_errors(world, [0, 4], [-1, 1, 3, 2], obj)
    with pytest.raises(BackendError, match=r"code -1\).*group_start decreases at group 1"):
        dev.scale_errors(world, [0, 3, 2, 4], [0, 1, 3, 2], obj)
    limit = scale_native.constants()["max_group"]
    assert limit >= 4096
    n = limit + 1
    with pytest.raises(BackendError, match=rf"code -4\).*group 1 has {n} entries; at most {limit} are supported"):
        dev.scale_errors(world, [0, 2, 2 + n], np.zeros(2 + n, dtype=np.int64), np.zeros((2 + n, 3)))
    assert dev.scale_errors(world, [0], [], np.zeros((0, 3))).shape == (0, 8)  # no group: no launch, no device needed
    if lib.cba_device_count() <= 0:
        with pytest.raises(BackendError, match="no HIP device"):
            dev.scale_errors(world, [0, 4], [0, 1, 3, 2], obj)
        with pytest.raises(BackendError):
            compute_frame_scale_error(np.zeros((3, 3)), np.ones((3, 3)), 0, 0, 1)
    # the harness applies the same checks (they are one function, scale_plan)
    with pytest.raises(scale_native.HarnessError, match=r"code -1: .*entry 2: world row 5 out of range"):
        HARNESS.scale_errors(world, [0, 4], [0, 1, 5, 2], obj)
    with pytest.raises(scale_native.HarnessError, match="code -4"):
        HARNESS.scale_errors(world, [0, 2, 2 + n], np.zeros(2 + n, dtype=np.int64), np.zeros((2 + n, 3)))


def test_host_half_in_a_build_without_device_code():
    """The entry point (input checks and binning, plain C++ in csrc/cba_solve.cpp) is part of every build of the C ABI; the CPU test
    build of tests/test_cpu_abi.py has no device code, so there a bad call is refused with the same messages and a valid one is
    CBA_ERR_UNSUPPORTED, never a number.  (Its own interpreter: this process has loaded the real library.)"""
    import os
    import subprocess
    import sys
    import textwrap

    from tests.native_build import CSRC, INCLUDE, NATIVE, ROOT as root, compile_native

    out = compile_native(NATIVE / "cpu_library.cpp", CSRC / "cba_solve.cpp", flags=("-pthread",), include=(INCLUDE,))
    body = """
        import json
        import numpy as np
        from caliscope_amd.exceptions import BackendError
        from caliscope_amd.scale_accuracy import DeviceScaleErrors
        dev, said = DeviceScaleErrors(), []
        for start, ent in (([0, 4], [0, 1, 5, 2]), ([0, 3, 2, 4], [0, 1, 3, 2]), ([0, 4], [0, 1, 3, 2])):
            try:
                dev.scale_errors(np.zeros((5, 3)), start, ent, np.zeros((4, 3)))
                said.append("returned")
            except BackendError as e:
                said.append(str(e))
        print(json.dumps(said))
    """
    proc = subprocess.run([sys.executable, "-c", textwrap.dedent(body)], env=dict(os.environ, CALISCOPE_BA_LIB=str(out), PYTHONPATH=str(root)), cwd=root,
                          capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-2000:]
    said = json.loads(proc.stdout.strip().splitlines()[-1])
    assert "code -1" in said[0] and "entry 2: world row 5 out of range [0, 5)" in said[0]
    assert "code -1" in said[1] and "group_start decreases at group 1" in said[1]
    assert "code -4" in said[2] and "no device kernels" in said[2]


def test_report_without_object_geometry_is_empty(case):
    z, vol = case
    image = vol.image_points.df
    image[["obj_loc_x", "obj_loc_y", "obj_loc_z"]] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bare = CaptureVolume(vol.camera_array, ImagePoints(image), vol.world_points, vol.constraints)
    rep = bare.compute_volumetric_scale_accuracy(_solver=None)  # returns before any device call
    assert rep.frame_errors == () and rep.static_object_ids == frozenset()


# ---- algebra -----------------------------------------------------------------------------------------------------------------

def project(vol):
    """Normalised image coordinates of every world point in every posed camera (a pinhole without a lens is enough here: what a
    similarity may not change is X_cam up to scale)."""
    X = vol.world_points.points
    out = []
    for c, cam in sorted(vol.camera_array.posed_cameras.items()):
        Xc = X @ cam.rotation.T + cam.translation
        out.append(Xc[:, :2] / Xc[:, 2:3])
    return np.array(out)


def test_similarity_leaves_every_projection_unchanged(case):
    _, vol = case
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    tr = SimilarityTransform(q if np.linalg.det(q) > 0 else -q, rng.normal(size=3), 2.7)
    cams, pts = apply_similarity_transform(vol.camera_array, vol.world_points, tr)
    moved = CaptureVolume(cams, vol.image_points, pts, vol.constraints, _known_map=vol.img_to_obj_map)
    before, after = project(vol), project(moved)
    assert np.abs(after - before).max() <= 1e-9 * max(1.0, np.abs(before).max())  # depths of a few units, coordinates up to ~1e2
    for cam in cams.cameras.values():
        if cam.rotation is not None:
            np.testing.assert_allclose(cam.rotation @ cam.rotation.T, np.eye(3), atol=1e-14)  # the scale did not get into the rotation
    # inverse undoes apply
    back_c, back_p = apply_similarity_transform(cams, pts, tr.inverse)
    np.testing.assert_allclose(back_p.points, vol.world_points.points, atol=1e-12)
    for c, cam in back_c.cameras.items():
        old = vol.camera_array.cameras[c]
        if old.rotation is None:
            assert cam.rotation is None and cam.translation is None
        else:
            np.testing.assert_allclose(cam.rotation, old.rotation, atol=1e-13)
            np.testing.assert_allclose(cam.translation, old.translation, atol=1e-12)
    np.testing.assert_allclose(tr.inverse.apply(tr.apply(vol.world_points.points)), vol.world_points.points, atol=1e-12)
    np.testing.assert_allclose(tr.matrix @ tr.inverse.matrix, np.eye(4), atol=1e-14)


def test_reprojection_residuals_survive_a_similarity():
    """The same property through the project's own residual code (`_pixel_errors` with an injected engine: the oracle's projection,
    lens distortion included)."""
    from oracle.engine import OracleEngine
    from oracle.residuals import joint_residuals
    from tests.scenario_scenes import moving_board_volume

    def factory(problem):
        eng = OracleEngine(problem.parameterization, problem.camera_indices, problem.image_coords, problem.obj_indices,
                           loss=problem.loss, f_scale=problem.f_scale, constraints=problem.constraint_args())

        def residuals(x):
            r = joint_residuals(x, problem.parameterization, problem.camera_indices, problem.image_coords, problem.obj_indices)
            return r, 0.5 * float(r @ r)

        eng.residuals = residuals
        return eng

    vol, _ = moving_board_volume()
    _, ci, uv, oi = vol._matched_arrays()
    before = vol._pixel_errors(ci, uv, oi, _engine_factory=factory)
    moved = vol.rotate("y", 33.0).translate(0.3, -1.0, 2.0).scaled(CameraDistance(*sorted(vol.camera_array.posed_cameras)[:2], 7.0))
    after = moved._pixel_errors(ci, uv, oi, _engine_factory=factory)
    assert np.abs(before).max() > 1e-3  # (a perturbed start: there are residuals to keep)
    assert np.abs(after - before).max() < 1e-9


def test_align_puts_the_board_at_its_obj_loc(case):
    z, vol = case
    done = 0
    for op in json.loads(str(z["ops"])):
        if op["op"] != "align_to_object" or op["error"] is not None or op["args"]["sync_index"] is None or op["args"]["object_id"] is None:
            continue
        si, o = op["args"]["sync_index"], op["args"]["object_id"]
        new = vol.align_to_object(si, o)
        rep = new.compute_volumetric_scale_accuracy(_solver=HARNESS)
        _, g_obj, _, _, group_start, ent_world, ent_obj = new._scale_groups()
        g = [k for k, fe in enumerate(rep.frame_errors) if (fe.sync_index, fe.object_id) == (si, o)]
        if not g:
            continue
        a, b = group_start[g[0]], group_start[g[0] + 1]
        resid = new.world_points.points[ent_world[a:b]] - ent_obj[a:b]
        # a rigid fit: the residual is the board's own noise (2 mm per coordinate, 0.2 % scale on 0.5 m, now and then an obj_loc 1 cm off)
        assert np.abs(resid).max() < 0.03
        rows = vol.image_points._df[(vol.image_points._df["sync_index"] == si) & (vol.image_points._df["object_id"] == o)]
        if not rows["obj_loc_x"].isna().any():  # (else the fit, which takes a keypoint's first row NaN or not, may have used fewer corners than the report)
            assert np.abs(resid.mean(axis=0)).max() < 1e-12, "the centroids of a least-squares rigid fit coincide"
        done += 1
    assert done or not len(z["frame_errors"])


def test_scaled_grounded_centered_do_what_they_say(case):
    _, vol = case
    posed = sorted(vol.camera_array.posed_cameras)
    a, b = posed[0], posed[-1]
    new = vol.scaled(CameraDistance(a, b, 3.25))
    assert abs(np.linalg.norm(new._camera_center(a) - new._camera_center(b)) - 3.25) < 1e-12
    two = vol.scaled(CameraDistance(a, b, 3.25), CameraDistance(a, b, 3.25, 0.5))
    np.testing.assert_allclose(two.world_points.points, new.world_points.points, rtol=1e-14, atol=0)
    g = vol.grounded()
    zs = g.world_points.points[:, 2]
    assert abs(np.percentile(zs, 1.0, method="lower")) < 1e-12 and np.abs(g._camera_center(posed[0])[:2]).max() < 1e-12
    assert abs(np.percentile(vol.grounded(lowest_point_height_m=0.07).world_points.points[:, 2], 1.0, method="lower") - 0.07) < 1e-12
    gc = g.centered()
    centres = np.array([gc._camera_center(c) for c in posed])
    assert np.abs(centres[:, :2].mean(axis=0)).max() < 1e-12
    assert abs(np.percentile(gc.world_points.points[:, 2], 1.0, method="lower")) < 1e-12
    # oriented: the vertical handed in becomes +Z, the anchor's optical axis has no X component
    up_world = np.array([0.2, -1.0, 0.1])
    o = vol.oriented({c: vol.camera_array.cameras[c].rotation @ up_world for c in posed})
    for c in posed:
        np.testing.assert_allclose(o.camera_array.cameras[c].rotation.T @ (vol.camera_array.cameras[c].rotation @ up_world) / np.linalg.norm(up_world),
                                   [0.0, 0.0, 1.0], atol=1e-12)
    forward = o.camera_array.cameras[posed[0]].rotation.T @ np.array([0.0, 0.0, 1.0])
    assert abs(forward[0]) < 1e-12 and forward[1] > 0


def test_oriented_logs_the_agreement(case, caplog):
    _, vol = case
    posed = sorted(vol.camera_array.posed_cameras)
    with caplog.at_level(logging.INFO, logger="caliscope_amd.capture_volume"):
        vol.oriented({c: vol.camera_array.cameras[c].rotation @ np.array([0.0, 0.0, 1.0]) for c in posed})
    assert any("Vertical agreement (deg from consensus): " + ", ".join(f"cam {c}: 0.00" for c in posed) + "; max pairwise disagreement 0.00" in r.message
               for r in caplog.records)


# ---- header edges: the mapping and the arithmetic of the g++ build -----------------------------------------------------------------

C = scale_native.constants()
THRESHOLDS = sorted({C["small_max"], C["small_max"] + 1, C["lds_small"], C["lds_small"] + 1, C["lds_large"], C["lds_large"] + 1})
EDGE_SIZES = sorted({2, 3, 4, 11, 12, 64, 65, 257, 600, 4096, *THRESHOLDS})


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_every_pair_is_visited_exactly_once(n):
    stride = C["block"]
    hits = np.zeros((n, n), dtype=np.int32)
    total = 0
    for lane in range(stride):
        i, j = scale_native.lane_pairs(n, lane, stride)
        assert np.all(i < j) and np.all(i >= 0) and np.all(j < n)
        lin = i.astype(np.int64) * n - i.astype(np.int64) * (i + 1) // 2 + (j - i - 1)  # row-major pair number
        assert np.array_equal(lin, lane + stride * np.arange(len(i))), f"lane {lane} does not take pairs {lane}, {lane} + {stride}, .."
        np.add.at(hits, (i, j), 1)
        total += len(i)
    assert total == n * (n - 1) // 2 and np.array_equal(hits, np.triu(np.ones((n, n), dtype=np.int32), 1))


@pytest.fixture(scope="module")
def edge_call():
    """One call with a group of every edge size (and of 0 and 1 entries), shuffled; the harness result and the groups."""
    rng = np.random.default_rng(77)
    sizes = [0, 1] + EDGE_SIZES
    order = rng.permutation(len(sizes))
    sizes = [sizes[k] for k in order]
    groups = [noisy_group(rng, n, 0.05 + 0.4 * (k % 3), (0.0, 0.002, 0.2)[k % 3]) for k, n in enumerate(sizes)]
    world = np.concatenate([g[0] for g in groups])
    perm = rng.permutation(len(world))  # entries point into a shuffled world table
    inv = np.argsort(perm)
    group_start = np.concatenate([[0], np.cumsum(sizes)])
    stats = HARNESS.scale_errors(world[perm], group_start, inv, np.concatenate([g[1] for g in groups]))
    return sizes, groups, stats, HARNESS.bins.copy()


def test_edge_groups_take_the_path_the_header_states(edge_call):
    sizes, _, _, bins = edge_call
    want = [0 if n <= C["small_max"] else 1 if n <= C["lds_small"] else 2 if n <= C["lds_large"] else 3 for n in sizes]
    assert bins.tolist() == want and set(want) == {0, 1, 2, 3}


def test_edge_statistics_against_pdist_and_longdouble(edge_call):
    sizes, groups, stats, _ = edge_call
    for n, (world, obj), got in zip(sizes, groups, stats):
        if n < 2:
            assert np.array_equal(got, np.zeros(8))
            continue
        want, bounds, _ = reference_stats(world, obj)
        assert_stats(got, want, bounds, f"n = {n} vs pdist")
        if n <= 600:
            want, bounds, _ = reference_stats(world, obj, np.longdouble)
            assert_stats(got, want, bounds, f"n = {n} vs longdouble")


UNIFORM_SIZES = (3, 12, 65, 257, 600, 2049)


@pytest.fixture(scope="module")
def uniform_scenes():
    rng = np.random.default_rng(123)
    return {n: uniform_scale_scene(rng, n) for n in UNIFORM_SIZES}


@pytest.mark.parametrize("n", UNIFORM_SIZES)
def test_uniform_scale_scene_shows_a_dropped_or_doubled_pair(uniform_scenes, n):
    world, obj = uniform_scenes[n]
    want, bounds, err = reference_stats(world, obj, np.longdouble if n <= 600 else np.float64)
    assert float(err.min()) > 10 * bounds["s1"], "the scene cannot show a missing pair"  # from the reference alone
    got = HARNESS.scale_errors(world, [0, n], np.arange(n), obj)[0]
    assert_stats(got, want, bounds, f"uniform n = {n}")
    fe = compute_frame_scale_error(world, obj, 0, 0, 1, _solver=HARNESS)
    assert abs(fe.distance_mean_signed_error_mm - 1000 * float(err.mean())) <= derived_bounds(want.astype(np.float64), bounds)["distance_mean_signed_error_mm"]
