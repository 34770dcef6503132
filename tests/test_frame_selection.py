"""Frame selection on the g++ build of csrc/frame_select_math.h (tests/frame_select_native.py): against the reference's own selector
(fixtures of tests/golden/frame_selection), the workflow on top of it through the `_solver` hooks, argument errors and the
multi-object rule."""
import dataclasses

import numpy as np
import pandas as pd
import pytest

from caliscope_amd import frame_selector as FS
from caliscope_amd.calibrate_intrinsics import (CameraIntrinsicsReport, IntrinsicCalibrationOutput, IntrinsicCalibrationReport,
                                                calibrate_camera_array_intrinsics, calibrate_intrinsics, run_intrinsic_calibration)
from caliscope_amd.cameras import CameraArray, CameraData
from caliscope_amd.frame_selector import IntrinsicCoverageReport, select_calibration_frames, select_camera_array_frames
from caliscope_amd.point_data import ImagePoints
from tests import frame_select_fixtures as F
from tests import intrinsic_scenes as S
from tests.frame_select_native import HarnessFrameSelection, homography
from tests.intrinsic_native import HarnessIntrinsics

SEL = HarnessFrameSelection()
INTR = HarnessIntrinsics()
NOISE_FREE_TOL = 10 * 5.7e-13  # the bound of tests/test_intrinsic_calibration.py on noise-free scenes (10 x what scipy leaves)


def test_the_reference_selector_fixtures(capsys):
    """Every fixture case through select_rig on the g++ build: selection identical in order, counts, orientation count and flag
    equal, covered cells equal as sets, the three coverage fractions equal, pose features and pose_diversity within 1e-12 *
    max(1, |value|), orientation features within ten times the difference between the generator's two solves of every homography.
    Measured: the two solves differ by at most 1.7e-12 (tilt direction, rad), 1.2e-14 (tilt magnitude) and 1.1e-13 (in-plane
    rotation, rad), so the bounds are 1.7e-11, 1.2e-13 and 1.1e-12; the g++ build's worst distances are printed below and recorded
    in INTEGRATION.md section 3d."""
    bound = F.orientation_bound()
    worst = np.zeros(3)
    with capsys.disabled():
        for i, fx in enumerate(F.cases()):
            assert float(fx["min_margin"]) >= F.MARGIN_FLOOR  # (exact ties of twin frames are left out of it by the generator)
            report, gathered, sel = F.run_case(fx, SEL)
            assert isinstance(report, IntrinsicCoverageReport)
            w = F.compare(fx, report, gathered.frame_sync, sel.cell_mask, sel.pose_features, sel.orientation, bound, label=f"sel_{i:02d}")
            worst = np.maximum(worst, w)
            print(f"sel_{i:02d}: {len(report.selected_frames)} selected of {report.eligible_frame_count} / {report.total_frame_count}, "
                  f"{report.orientation_count} bins, orientation distance to the reference {w}")
        print(f"orientation: worst distance {worst}, bound {bound}")


def test_select_calibration_frames_has_the_reference_signature_and_result():
    fx = F.load(0)
    ip = ImagePoints(F.dataframe(fx))
    rep = select_calibration_frames(ip, int(fx["cam_id"]), (1280, 720), _solver=SEL)
    assert [f.name for f in dataclasses.fields(IntrinsicCoverageReport)] == [
        "selected_frames", "coverage_fraction", "edge_coverage_fraction", "corner_coverage_fraction", "pose_diversity", "orientation_sufficient",
        "orientation_count", "eligible_frame_count", "total_frame_count"]
    assert rep.selected_frames == fx["selected_frames"].tolist() and all(isinstance(s, int) for s in rep.selected_frames)
    with pytest.raises(dataclasses.FrozenInstanceError):
        rep.orientation_count = 0
    # min_orientations only moves the flag
    strict = select_calibration_frames(ip, int(fx["cam_id"]), (1280, 720), min_orientations=9, _solver=SEL)
    assert strict.selected_frames == rep.selected_frames and rep.orientation_sufficient and not strict.orientation_sufficient
    # the empty reports (reference frame_selector.py:139-166)
    assert select_calibration_frames(ip, 99, (1280, 720), _solver=SEL) == IntrinsicCoverageReport([], 0.0, 0.0, 0.0, 0.0, False, 0, 0, 0)
    few = select_calibration_frames(ip, int(fx["cam_id"]), (1280, 720), min_corners_per_frame=25, _solver=SEL)
    assert few == IntrinsicCoverageReport([], 0.0, 0.0, 0.0, 0.0, False, 0, 0, 70)
    # float32_io off: the same frames on this scene (every margin is far above float32 rounding of the inputs), features differ
    wide = select_calibration_frames(ip, int(fx["cam_id"]), (1280, 720), float32_io=False, _solver=SEL)
    assert wide.selected_frames == rep.selected_frames


def test_rows_without_geometry_are_dropped_and_frames_are_counted_after_it():
    fx = F.load(7)
    df = F.dataframe(fx)
    extra = df.iloc[:6].copy()
    extra["sync_index"] = 5000  # a frame of tracker rows only: no board coordinates
    extra[["obj_loc_x", "obj_loc_y"]] = np.nan
    holes = df.iloc[6:9].copy()
    holes["keypoint_id"] += 500
    holes["img_loc_x"] = np.inf  # rows without a finite pixel inside a good frame
    both = pd.concat([df, extra, holes], ignore_index=True)
    a = select_calibration_frames(ImagePoints(df), int(fx["cam_id"]), (1280, 720), _solver=SEL)
    b = select_calibration_frames(ImagePoints(both), int(fx["cam_id"]), (1280, 720), _solver=SEL)
    assert a == b and a.total_frame_count == 24


def test_argument_errors():
    fx = F.load(7)
    ip = ImagePoints(F.dataframe(fx))
    cam = int(fx["cam_id"])
    for bad in (0, 9):
        with pytest.raises(ValueError, match="grid_size"):
            select_calibration_frames(ip, cam, (1280, 720), grid_size=bad, _solver=SEL)
        with pytest.raises(ValueError, match="grid_size"):
            SEL.select_frames([0, 0], [[1280.0, 720.0]], [0], np.zeros((0, 2)), np.zeros((0, 2)), grid_size=bad)
    with pytest.raises(ValueError, match="target_frame_count"):
        select_calibration_frames(ip, cam, (1280, 720), target_frame_count=0, _solver=SEL)
    arr = CameraArray({cam: CameraData(cam_id=cam, size=None)})
    with pytest.raises(ValueError, match="resolution"):
        select_camera_array_frames(ip, arr, _solver=SEL)
    with pytest.raises(ValueError, match="resolution"):
        calibrate_camera_array_intrinsics(ip, arr, "select", _solver=INTR, _selector=SEL)
    with pytest.raises(ValueError, match="frames must be"):
        calibrate_camera_array_intrinsics(ip, CameraArray({cam: CameraData(cam_id=cam, size=(1280, 720))}), "all", _solver=INTR, _selector=SEL)
    with pytest.raises(ValueError, match="subrange"):
        SEL.select_frames([0, 1], [[1280.0, 720.0]], [0, 4], np.zeros((4, 2)), np.zeros((4, 2)), [2], [3])
    with pytest.raises(ValueError, match="decreases"):
        SEL.select_frames([0, 2], [[1280.0, 720.0]], [0, 4, 3], np.zeros((3, 2)), np.zeros((3, 2)))


def test_rig_call_equals_the_single_camera_calls():
    """select_camera_array_frames: the default-argument fixture cases as cameras of one rig (0 to 300 frames, one with a single
    frame); an ignored camera and, with only_missing, a calibrated one are left out."""
    ip, cams, fxs = F.default_rig()
    arr = CameraArray({c: CameraData(cam_id=c, size=size) for c, size in cams})
    arr.cameras[50] = CameraData(cam_id=50, size=(1280, 720), ignore=True)
    arr.cameras[51] = CameraData(cam_id=51, size=(1280, 720), matrix=np.eye(3), distortions=np.zeros(5))
    reports = select_camera_array_frames(ip, arr, only_missing=True, _solver=SEL)
    assert set(reports) == {c for c, _ in cams}
    for (c, _), fx in zip(cams, fxs):
        if fx is None:
            assert reports[c].total_frame_count == 1 and reports[c].eligible_frame_count == 1 and len(reports[c].selected_frames) == 1
            assert reports[c].pose_diversity == 0.0
        else:
            assert reports[c].selected_frames == fx["selected_frames"].tolist(), c
            assert reports[c].orientation_count == int(fx["orientation_count"]) and reports[c].total_frame_count == int(fx["total_frame_count"])
    assert set(select_camera_array_frames(ip, arr, _solver=SEL)) == {c for c, _ in cams} | {51}


def test_two_boards_in_one_frame():
    """The multi-object rule: the homography of a frame runs over its object with the most rows (lowest object_id on ties), coverage
    and pose features over all rows."""
    fx = F.load(0)
    df = F.dataframe(fx)
    cam = int(fx["cam_id"])
    small = df[df["keypoint_id"] < 8].copy()  # a second, smaller board with its own obj_loc frame, seen elsewhere in the image
    small["object_id"] = 1
    small["img_loc_x"] = 1280.0 - small["img_loc_x"] * 0.5
    small["img_loc_y"] = 720.0 - small["img_loc_y"] * 0.5
    small["obj_loc_x"] = small["obj_loc_y"] * 3.0 + 1.0
    both = pd.concat([small, df], ignore_index=True)  # (the smaller board's rows first: the order must not matter)
    size = [(cam, (1280, 720))]
    _, g2, s2 = FS.select_rig(ImagePoints(both), size, by_object=True, _solver=SEL)
    _, g1, s1 = FS.select_rig(ImagePoints(df), size, by_object=True, _solver=SEL)
    _, g0, s0 = FS.select_rig(ImagePoints(small), size, by_object=True, _solver=SEL)
    assert np.array_equal(g2.frame_sync, g1.frame_sync) and g2.homog_count.tolist() == np.diff(g1.frame_start).tolist()
    assert np.array_equal(s2.orientation, s1.orientation) and np.array_equal(s2.homography_rmse, s1.homography_rmse)
    at = np.searchsorted(g1.frame_sync, g0.frame_sync)
    assert np.array_equal(s2.cell_mask[at], s1.cell_mask[at] | s0.cell_mask) and (s2.cell_mask[at] != s1.cell_mask[at]).any()
    assert not np.array_equal(s2.pose_features, s1.pose_features)
    # a tie in size goes to the lowest object_id
    twin = df.copy()
    twin["object_id"] = 2
    twin["obj_loc_x"] = -twin["obj_loc_x"]
    _, g3, s3 = FS.select_rig(ImagePoints(pd.concat([twin, df], ignore_index=True)), size, by_object=True, _solver=SEL)
    assert np.array_equal(s3.orientation, s1.orientation)
    # without by_object (the reference's single-board reading) the fit runs over every row of the frame
    _, g4, s4 = FS.select_rig(ImagePoints(both), size, by_object=False, _solver=SEL)
    assert g4.homog_start is None and not np.array_equal(s4.orientation, s1.orientation)


def test_homography_closed_forms_and_degenerate_frames():
    """The fit recovers an exact homography (also a mirrored one: det A < 0, where the in-plane rotation is that of the reflection
    the reference's U Vt gives), and fails cleanly on collinear corners, on corners at one pixel and on fewer than four."""
    rng = np.random.default_rng(3)
    obj = np.array([[c * 0.04, r * 0.04] for r in range(4) for c in range(6)])
    X = (obj - obj.min(0)) / (obj.max(0) - obj.min(0))
    for Ht in (np.array([[900.0, 50.0, 300.0], [-30.0, 1000.0, 200.0], [0.2, -0.1, 1.0]]),
               np.array([[-700.0, 90.0, 900.0], [60.0, 650.0, 100.0], [-0.05, 0.3, 1.0]])):
        p = np.c_[X, np.ones(len(X))] @ Ht.T
        uv = p[:, :2] / p[:, 2:]
        st, H, o, rmse = homography(obj, uv, float32_io=False)
        assert st == 0 and np.abs(H - Ht).max() <= 1e-9 * np.abs(Ht).max() and rmse < 1e-9
        U, _, Vt = np.linalg.svd(Ht[:2, :2])
        R = U @ Vt
        want = np.array([np.arctan2(Ht[2, 1], Ht[2, 0]) % (2 * np.pi), np.hypot(Ht[2, 0], Ht[2, 1]), np.arctan2(R[1, 0], R[0, 0]) % (2 * np.pi)])
        assert F.circular(o[0], want[0]) < 1e-9 and abs(o[1] - want[1]) < 1e-9 and F.circular(o[2], want[2]) < 1e-9
        noisy = uv + rng.normal(0, 0.3, uv.shape)
        st, H, o, rmse = homography(obj, noisy, float32_io=True)
        assert st == 0 and 0.1 < rmse < 0.5
    line = np.column_stack([np.linspace(0, 1, 8), np.linspace(0, 1, 8) * 0.5])
    for bad_obj, bad_uv, want in ((line, line * 300 + 50, 2), (obj, np.full((len(obj), 2), 123.0), 2), (obj[:3], uv[:3], 1),
                                  (np.full((6, 2), 0.5), uv[:6], 2)):
        st, H, o, rmse = homography(bad_obj, bad_uv)
        assert st == want and not H.any() and not o.any() and rmse == 0.0


# ---- the workflow on top ----------------------------------------------------------------------------------------------------------

def test_run_intrinsic_calibration_selects_then_solves():
    sc = S.camera_scene(61, n_views=45, noise=0.3)
    ip = S.scene_image_points([sc], cam_ids=[4])
    camera = CameraData(cam_id=4, size=S.SIZE)
    out = run_intrinsic_calibration(camera, ip, _solver=INTR, _selector=SEL)
    assert isinstance(out, IntrinsicCalibrationOutput) and isinstance(out.report, IntrinsicCalibrationReport)
    sel = select_calibration_frames(ip, 4, S.SIZE, _solver=SEL)
    assert 0 < len(sel.selected_frames) <= 30 and out.report.selected_frames == tuple(sel.selected_frames)
    direct = calibrate_intrinsics(ip, 4, S.SIZE, sel.selected_frames, _solver=INTR)
    assert np.array_equal(out.camera.matrix, direct.camera_matrix) and np.array_equal(out.camera.distortions, direct.distortions)
    assert out.camera.error == direct.reprojection_error == out.report.rmse and out.camera.grid_count == direct.frames_used == out.report.frames_used
    assert out.report.frames_used == len(sel.selected_frames)
    assert (out.report.coverage_fraction, out.report.edge_coverage_fraction, out.report.corner_coverage_fraction, out.report.orientation_sufficient,
            out.report.orientation_count) == (sel.coverage_fraction, sel.edge_coverage_fraction, sel.corner_coverage_fraction,
                                              sel.orientation_sufficient, sel.orientation_count)
    assert camera.matrix is None and camera.grid_count is None and out.camera is not camera  # the input is not touched
    # a selection brought along is used as it is
    mine = dataclasses.replace(sel, selected_frames=sel.selected_frames[:12])
    assert run_intrinsic_calibration(camera, ip, mine, _solver=INTR, _selector=None).report.frames_used == 12
    with pytest.raises(ValueError, match="No frames selected"):
        run_intrinsic_calibration(CameraData(cam_id=9, size=S.SIZE), ip, _solver=INTR, _selector=SEL)


def test_rig_calibration_with_selection_and_without():
    scenes = [S.camera_scene(71, n_views=40, noise=0.0), S.camera_scene(72, n_views=36, fisheye=True, noise=0.0), S.camera_scene(73, n_views=2, noise=0.3)]
    ip = S.scene_image_points(scenes, cam_ids=[0, 1, 2])
    arr = CameraArray({0: CameraData(cam_id=0, size=S.SIZE), 1: CameraData(cam_id=1, size=S.SIZE, fisheye=True), 2: CameraData(cam_id=2, size=S.SIZE)})
    out, reports = calibrate_camera_array_intrinsics(ip, arr, "select", float32_io=False, _solver=INTR, _selector=SEL)
    cover = select_camera_array_frames(ip, arr, float32_io=False, _solver=SEL)
    for c in (0, 1):
        rep = reports[c]
        assert isinstance(rep, CameraIntrinsicsReport) and rep.coverage == cover[c] and rep.status == 0
        assert rep.sync_index.tolist() == sorted(cover[c].selected_frames) and len(rep.sync_index) <= 30  # the selected frames are the ones solved
        assert out.cameras[c].grid_count == rep.result.frames_used == len(cover[c].selected_frames)
        got = np.zeros(9)
        got[:4] = [out.cameras[c].matrix[0, 0], out.cameras[c].matrix[1, 1], out.cameras[c].matrix[0, 2], out.cameras[c].matrix[1, 2]]
        got[4:4 + len(out.cameras[c].distortions)] = out.cameras[c].distortions
        assert np.abs(got - scenes[c].truth9).max() <= NOISE_FREE_TOL, (c, np.abs(got - scenes[c].truth9).max())
    assert reports[2].status == 1 and reports[2].coverage == cover[2] and out.cameras[2].matrix is None
    # selection keywords reach the selector
    _, r5 = calibrate_camera_array_intrinsics(ip, arr, "select", target_frame_count=5, grid_size=3, float32_io=False, _solver=INTR, _selector=SEL)
    assert len(r5[0].sync_index) == 5 and r5[0].coverage == select_camera_array_frames(ip, arr, target_frame_count=5, grid_size=3, float32_io=False,
                                                                                       _solver=SEL)[0]
    # frames=None and frames={...}: as before, bit for bit, and no coverage
    for frames in (None, {0: list(range(10)), 1: range(12)}):
        a, ra = calibrate_camera_array_intrinsics(ip, arr, frames, _solver=INTR)
        model, size, vstart, vcam, xy, obj = S.pack([dataclasses.replace(s, views=s.views[:{0: 10, 1: 12, 2: 2}[i]] if frames else s.views)
                                                     for i, s in enumerate(scenes)])
        intr, rmse, status, *_ = INTR.intrinsics_batch(model, size, None, vstart, vcam, xy, obj, True, 0)
        for c in (0, 1):
            assert ra[c].coverage is None and status[c] == 0 and a.cameras[c].error == rmse[c]
            assert np.array_equal(np.array([a.cameras[c].matrix[0, 0], a.cameras[c].matrix[1, 1], a.cameras[c].matrix[0, 2], a.cameras[c].matrix[1, 2]]), intr[c, :4])
        assert ra[2].coverage is None and ra[2].status == 1
