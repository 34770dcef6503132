"""Intrinsic calibration on the g++ build of csrc/intrinsic_math.h (tests/intrinsic_native.py): the Jacobian, the solve against
the scipy yardstick of tests/intrinsic_scenes.py, the edges, and the Python layer through its `_solver` hook."""
import inspect

import numpy as np
import pytest

from caliscope_amd.calibrate_intrinsics import (CameraIntrinsicsReport, IntrinsicCalibrationResult, calibrate_camera_array_intrinsics,
                                                calibrate_intrinsics)
from caliscope_amd.cameras import CameraArray, CameraData, rvec_to_matrix
from oracle.camera_model import project_fisheye, project_pinhole, rodrigues, rotation_to_rvec
from tests import intrinsic_scenes as S
from tests.intrinsic_native import HarnessIntrinsics, point, start_intrinsics

H = HarnessIntrinsics()

# Tolerances, set from the yardstick's own error as the issue prescribes (10 x what scipy leaves), never from the code under test.
# Measured on the scenes of these tests (figures in the docstrings of the tests that use them):
NOISE_FREE_TOL = 10 * 5.7e-13   # scipy's largest |intrinsics - truth| on the noise-free scenes, from either start
NOISY_TOL = 10 * 7.9e-7         # scipy's largest |intrinsics(start = truth) - intrinsics(cold start)| on the noisy scenes
COST_REL = 1e-8                 # final cost <= yardstick cost * (1 + COST_REL): the bound smoke() holds the BA solver to


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _views_of(scene, keep, f32):
    return [((_f32(scene.views[i][0]), _f32(scene.views[i][1])) if f32 else (scene.views[i][0], scene.views[i][1])) for i in keep]


def _solve(scenes, f32, **kw):
    model, size, vstart, vcam, xy, obj = S.pack(scenes)
    intr, rmse, status, iters, pose, vrmse, vstat = H.intrinsics_batch(model, size, kw.get("start"), vstart, vcam, xy, obj, f32, kw.get("max_iter", 0))
    assert np.isfinite(intr).all() and np.isfinite(rmse).all() and np.isfinite(pose).all() and np.isfinite(vrmse).all()
    return dict(intr=intr, rmse=rmse, status=status, iters=iters, pose=pose, vrmse=vrmse, vstat=vstat, vcam=vcam, vstart=vstart)


def _against_yardstick(scenes, f32, label):
    """Harness against scipy from two starts, camera by camera; returns (max |h - ya|, max |ya - yb|, max relative cost excess)."""
    out = _solve(scenes, f32)
    start, pose0, _ = S.cold_start_poses(scenes, f32)
    worst_h = worst_y = worst_c = 0.0
    for c, sc in enumerate(scenes):
        assert out["status"][c] == 0, (label, c, out["status"])
        mine = np.flatnonzero(out["vcam"] == c)
        keep = np.flatnonzero(out["vstat"][mine] == 0)
        views = _views_of(sc, keep, f32)
        n = sum(len(X) for X, _ in views)
        ya, ssq_a, _, ra = S.yardstick(views, sc.fisheye, sc.truth9, S.truth_poses(sc, keep))
        yb, ssq_b, _, rb = S.yardstick(views, sc.fisheye, start[c], pose0[mine][keep])
        ssq_h = out["rmse"][c] ** 2 * n
        ssq_y = min(ssq_a, ssq_b)
        d_h, d_y = np.abs(out["intr"][c] - ya).max(), np.abs(ya - yb).max()
        print(f"{label} cam {c} {'fisheye' if sc.fisheye else 'pinhole'} views {len(keep)}/{len(mine)} iters {out['iters'][c]} rmse {out['rmse'][c]:.6f} "
              f"cost/yardstick - 1 = {ssq_h / ssq_y - 1:.2e}  |harness - yardstick| {d_h:.2e}  |yardstick(truth) - yardstick(cold)| {d_y:.2e}  "
              f"nfev {ra.nfev}/{rb.nfev}  f error {abs(out['intr'][c][0] - sc.intr[0]) / sc.intr[0]:.2e}")
        assert ssq_h <= ssq_y * (1.0 + COST_REL), (label, c, ssq_h, ssq_y)
        worst_h, worst_y, worst_c = max(worst_h, d_h), max(worst_y, d_y), max(worst_c, ssq_h / ssq_y - 1)
    return worst_h, worst_y, worst_c, out


# ---- 1. Jacobian and residual ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1])
def test_jacobian_matches_central_differences_and_residual_matches_the_oracle(model):
    """All NI + 6 columns against central differences of the header's own residual, per column relative 1e-6 (the reference's
    Jacobian test tolerance); the residual against oracle.camera_model at 1e-12 relative."""
    rng = np.random.default_rng(4 + model)
    ni = 8 if model else 9
    for trial in range(20):
        intr = np.concatenate([[620.0, 615.0, 950.0, 545.0], S.FISHEYE_D]) if model else np.concatenate([*S.PINHOLE_TRUTH])
        intr = intr * (1 + 0.05 * rng.normal(size=ni))
        rv, t = rng.normal(0, 0.4, 3), np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(0.5, 1.5)])
        R = rodrigues(rv)
        X = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05)])
        u = rng.uniform(0, 1000, 2)
        front, e, J = point(model, intr, R, t, X, u)
        assert front
        K = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1.0]])
        ref = (project_fisheye if model else project_pinhole)(X[None], rv, t, K, intr[4:])[0][0] - u
        assert np.abs(e - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (e, ref)

        def resid(dw, dt, di):
            return point(model, intr + di, rvec_to_matrix(dw) @ R, t + dt, X, u)[1]

        for col in range(6 + ni):
            # steps: the pose columns are non-linear (h = 1e-6: truncation ~h^2); the residual is linear in every intrinsic, so those
            # columns take large steps.  The floor is what rounding of a ~2000 px residual leaves of a central difference.
            h = 1e-6 if col < 6 else (1e-2 if col < 10 else 1e-4)
            d = np.zeros(6 + ni)
            d[col] = h
            num = (resid(d[:3], d[3:6], d[6:]) - resid(-d[:3], -d[3:6], -d[6:])) / (2 * h)
            floor = 8 * np.finfo(float).eps * 2000.0 / h
            assert np.abs(J[:, col] - num).max() <= 1e-6 * np.abs(num).max() + floor, (model, trial, col, J[:, col], num)


# ---- 2. noise-free scenes from the cold start -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fisheye", [False, True])
def test_noise_free_scenes_recover_the_truth(fisheye, capsys):
    """Three scenes per model, float32_io off, cold start.  Measured: scipy's yardstick leaves at most 5.7e-13 (absolute, largest
    entry: the focal lengths and the principal point, ~1e3 px, i.e. a few ulp) from either start; the tolerance is 10 x that,
    5.7e-12.  The g++ build leaves at most 6.9e-13 on the same scenes."""
    worst = 0.0
    with capsys.disabled():
        for seed in range(3):
            sc = S.camera_scene(seed, fisheye=fisheye, noise=0.0)
            out = _solve([sc], False)
            keep = np.flatnonzero(out["vstat"] == 0)
            views = _views_of(sc, keep, False)
            start, pose0, _ = S.cold_start_poses([sc], False)
            ya = S.yardstick(views, fisheye, sc.truth9, S.truth_poses(sc, keep))[0]
            yb = S.yardstick(views, fisheye, start[0], pose0[keep])[0]
            left = max(np.abs(ya - sc.truth9).max(), np.abs(yb - sc.truth9).max())
            err = np.abs(out["intr"][0] - sc.truth9).max()
            print(f"noise-free {'fisheye' if fisheye else 'pinhole'} seed {seed}: status {out['status'][0]} iters {out['iters'][0]} views {len(keep)} "
                  f"|harness - truth| {err:.2e}  yardstick leaves {left:.2e}  rmse {out['rmse'][0]:.2e}")
            assert out["status"][0] == 0 and left <= NOISE_FREE_TOL / 10 * 1.0001
            worst = max(worst, err)
    assert worst <= NOISE_FREE_TOL, worst


# ---- 3. noisy scenes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fisheye", [False, True])
def test_noisy_scenes_reach_the_yardstick_minimum(fisheye, capsys):
    """The probe's recipe (30 views, 0.3 px noise, float32_io on), three seeds per model; fisheye also at f = 430 and 860.
    Measured: the yardstick's two starts (ground truth, cold start) end within 7.9e-7 of each other (largest entry), so the
    tolerance is 7.9e-6; the g++ build lies within 4.5e-7 of the yardstick and its cost within 1e-13 relative of scipy's."""
    with capsys.disabled():
        scenes = [S.camera_scene(seed, fisheye=fisheye, noise=0.3) for seed in range(3)]
        if fisheye:
            scenes += [S.camera_scene(7, fisheye=True, noise=0.3, intr=S.fisheye_truth(430.0)[0], dist=S.FISHEYE_D),
                       S.camera_scene(8, fisheye=True, noise=0.3, intr=S.fisheye_truth(860.0)[0], dist=S.FISHEYE_D)]
        worst_h, worst_y, _, out = _against_yardstick(scenes, True, "noisy")
    assert worst_y <= NOISY_TOL / 10 * 1.0001, worst_y   # the yardstick itself is as good as when the tolerance was set
    assert worst_h <= NOISY_TOL, worst_h
    for c, sc in enumerate(scenes):
        assert abs(out["intr"][c][0] - sc.intr[0]) <= 0.01 * sc.intr[0]


def test_rig_of_six_cameras_in_one_call(capsys):
    """Six cameras, both models, different true intrinsics, 3 to 240 views, one call.  Same bounds as the single-camera scenes;
    every camera also equals its own solo call bit for bit (cameras do not interact).  Measured: the g++ build within 4.4e-7 of the
    yardstick, the yardstick's two starts within 3.5e-6 of each other (the 3-view camera), costs within 2e-14 relative.  NOISY_TOL
    stays the 7.9e-6 set on the single-camera scenes: it is the stricter choice (2.3 x the yardstick's own spread here, not 10 x),
    which is why the yardstick's spread is printed and not asserted in this test."""
    with capsys.disabled():
        scenes = S.rig_scenes()
        worst_h, worst_y, _, out = _against_yardstick(scenes, True, "rig")
    assert worst_h <= NOISY_TOL, (worst_h, worst_y)
    solo = _solve([scenes[3]], True)
    assert np.array_equal(solo["intr"][0], out["intr"][3]) and solo["rmse"][0] == out["rmse"][3]


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------
def _with_views(scene, views):
    return S.CameraScene(scene.fisheye, scene.size, scene.intr, scene.dist, list(views))


def test_edges_too_few_views_short_collinear_and_empty():
    base = S.camera_scene(21, n_views=12, noise=0.3)
    # a camera with 2 views: TOO_FEW by the counts, start intrinsics and rmse 0 come back
    two = _solve([_with_views(base, base.views[:2])], True)
    assert two["status"][0] == 1 and two["rmse"][0] == 0.0
    assert np.array_equal(two["intr"][0], start_intrinsics(0, *base.size))
    # a view with 3 corners and a collinear view (one board row) among healthy ones: both left out, the camera solves, and the
    # result is the yardstick's on the views that remain
    X, uv, rv, t = base.views[0]
    short = (X[:3], uv[:3], rv, t)
    Xl, uvl, rvl, tl = base.views[1]
    row = np.flatnonzero(np.isclose(Xl[:, 1], Xl[0, 1]))
    line = (Xl[row], uvl[row], rvl, tl)
    assert len(row) >= 4
    mixed = _with_views(base, [short, line] + base.views[2:])
    out = _solve([mixed], True)
    assert out["status"][0] == 0 and out["vstat"][0] == 1 and out["vstat"][1] == 2 and (out["vstat"][2:] == 0).all()
    assert out["vrmse"][0] == 0.0 and out["vrmse"][1] == 0.0 and (out["vrmse"][2:] > 0).all()
    eye = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    assert np.array_equal(out["pose"][0], eye) and np.array_equal(out["pose"][1], eye)
    keep = np.arange(2, len(mixed.views))
    ya, ssq, _, _ = S.yardstick(_views_of(mixed, keep, True), False, mixed.truth9, S.truth_poses(mixed, keep))
    n = sum(len(mixed.views[i][0]) for i in keep)
    assert np.abs(out["intr"][0] - ya).max() <= NOISY_TOL and out["rmse"][0] ** 2 * n <= ssq * (1 + COST_REL)
    # all corners of all views on one image row (fy and cy cannot be told apart): no result, never NaN (_solve checks finiteness)
    flat = _with_views(base, [(X, np.column_stack([uv[:, 0], np.full(len(uv), 500.0)]), rv, t) for X, uv, rv, t in base.views])
    deg = _solve([flat], True)
    assert deg["status"][0] in (1, 2) and deg["rmse"][0] == 0.0 and np.array_equal(deg["intr"][0], start_intrinsics(0, *base.size))
    # a camera without any view beside healthy ones
    healthy = S.camera_scene(22, n_views=8, fisheye=True, noise=0.3)
    trio = _solve([base, _with_views(base, []), healthy], True)
    assert trio["status"].tolist() == [0, 1, 0]
    assert np.array_equal(trio["intr"][0], _solve([base], True)["intr"][0]) and np.array_equal(trio["intr"][2], _solve([healthy], True)["intr"][0])
    # no views at all
    none = _solve([_with_views(base, [])], True)
    assert none["status"][0] == 1


def test_float32_io_on_and_off_and_nan_z():
    sc = S.camera_scene(23, n_views=15, noise=0.3)
    keep = np.arange(len(sc.views))
    for f32 in (True, False):
        out = _solve([sc], f32)
        assert out["status"][0] == 0 and (out["vstat"] == 0).all()
        ya, ssq, rm, _ = S.yardstick(_views_of(sc, keep, f32), False, sc.truth9, S.truth_poses(sc, keep))
        assert np.abs(out["intr"][0] - ya).max() <= NOISY_TOL and abs(out["rmse"][0] - rm) <= 1e-9
    on, off = _solve([sc], True), _solve([sc], False)
    assert not np.array_equal(on["intr"], off["intr"]) and np.abs(on["intr"] - off["intr"]).max() < 1e-2  # float32 pixels: ~6e-5 px
    # NaN obj_loc_z is read as 0
    nan = _with_views(sc, [(np.column_stack([X[:, :2], np.full(len(X), np.nan)]), uv, rv, t) for X, uv, rv, t in sc.views])
    model, size, vstart, vcam, xy, obj = S.pack([nan])
    res = H.intrinsics_batch(model, size, None, vstart, vcam, xy, obj, True, 0)
    assert np.array_equal(res[0], on["intr"]) and np.array_equal(res[4], on["pose"])
    # caller's start values are used when given
    own = _solve([sc], True, start=np.array([sc.truth9]))
    assert own["status"][0] == 0 and np.abs(own["intr"] - on["intr"]).max() <= NOISY_TOL


# ---- 5. the Python layer ---------------------------------------------------------------------------------------------------------------
def test_calibrate_intrinsics_has_the_reference_signature_and_result():
    sig = inspect.signature(calibrate_intrinsics)
    names = list(sig.parameters)
    assert names[:5] == ["image_points", "cam_id", "image_size", "selected_frames", "fisheye"]
    assert sig.parameters["fisheye"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["fisheye"].default is False
    sc = S.camera_scene(31, n_views=10, noise=0.3)
    ip = S.scene_image_points([sc], cam_ids=[4])
    df = ip.df.copy()
    df.loc[df["sync_index"] % 2 == 0, "obj_loc_z"] = np.nan  # planar board: z may be NaN
    ip = type(ip)(df)
    res = calibrate_intrinsics(ip, 4, sc.size, list(range(10)), _solver=H)
    assert isinstance(res, IntrinsicCalibrationResult) and res.frames_used == 10
    assert res.camera_matrix.shape == (3, 3) and res.distortions.shape == (5,) and res.camera_matrix[0, 1] == 0.0 and res.camera_matrix[2, 2] == 1.0
    direct = _solve([sc], True)
    assert res.camera_matrix[0, 0] == direct["intr"][0, 0] and res.reprojection_error == direct["rmse"][0]
    assert abs(res.camera_matrix[0, 0] - sc.intr[0]) < 0.01 * sc.intr[0]
    sub = calibrate_intrinsics(ip, 4, sc.size, [0, 2, 4, 6, 99], _solver=H)
    assert sub.frames_used == 4
    fe = S.camera_scene(32, n_views=10, fisheye=True, noise=0.3)
    rf = calibrate_intrinsics(S.scene_image_points([fe]), 0, fe.size, list(range(10)), fisheye=True, _solver=H)
    assert rf.distortions.shape == (4,) and abs(rf.camera_matrix[0, 0] - fe.intr[0]) < 0.01 * fe.intr[0]
    with pytest.raises(ValueError, match="No valid calibration frames"):
        calibrate_intrinsics(ip, 4, sc.size, [500, 501], _solver=H)
    with pytest.raises(ValueError, match="No valid calibration frames"):
        calibrate_intrinsics(ip, 9, sc.size, list(range(10)), _solver=H)
    short = type(ip)(df.groupby("sync_index").head(3).reset_index(drop=True))
    with pytest.raises(ValueError, match="No valid calibration frames"):
        calibrate_intrinsics(short, 4, sc.size, list(range(10)), _solver=H)
    with pytest.raises(ValueError, match="failed"):
        calibrate_intrinsics(ip, 4, sc.size, [0, 1], _solver=H)


def test_calibrate_camera_array_intrinsics_fills_a_copy():
    scenes = [S.camera_scene(41, n_views=8, noise=0.3), S.camera_scene(42, n_views=9, fisheye=True, noise=0.3), S.camera_scene(43, n_views=2, noise=0.3)]
    ip = S.scene_image_points(scenes, cam_ids=[0, 1, 2])
    known = np.array([[1000.0, 0, 900.0], [0, 1000.0, 500.0], [0, 0, 1.0]])
    arr = CameraArray({0: CameraData(cam_id=0, size=S.SIZE), 1: CameraData(cam_id=1, size=S.SIZE, fisheye=True), 2: CameraData(cam_id=2, size=S.SIZE),
                       3: CameraData(cam_id=3, size=S.SIZE, ignore=True), 5: CameraData(cam_id=5, size=S.SIZE, matrix=known.copy(), distortions=np.zeros(5))})
    out, reports = calibrate_camera_array_intrinsics(ip, arr, only_missing=True, _solver=H)
    assert all(cam.matrix is None and cam.distortions is None and cam.error is None and cam.grid_count is None for c, cam in arr.cameras.items() if c != 5)
    assert set(reports) == {0, 1, 2} and all(isinstance(r, CameraIntrinsicsReport) for r in reports.values())
    direct = _solve(scenes, True)
    for c in (0, 1):
        cam, rep = out.cameras[c], reports[c]
        assert rep.status == 0 and cam.matrix[0, 0] == direct["intr"][c, 0] and cam.error == direct["rmse"][c] == rep.result.reprojection_error
        assert cam.grid_count == len(scenes[c].views) == rep.result.frames_used and len(cam.distortions) == (4 if c else 5)
        assert rep.sync_index.tolist() == list(range(len(scenes[c].views))) and (rep.view_rmse > 0).all() and (rep.view_status == 0).all()
    assert reports[2].status == 1 and reports[2].result is None and out.cameras[2].matrix is None
    assert out.cameras[3].matrix is None and np.array_equal(out.cameras[5].matrix, known)
    # a frame selection per camera
    sel, rs = calibrate_camera_array_intrinsics(ip, arr, {0: [0, 1, 2, 3, 4], 1: range(9)}, only_missing=True, _solver=H)
    assert sel.cameras[0].grid_count == 5 and sel.cameras[1].grid_count == 9 and rs[2].status == 1 and len(rs[2].sync_index) == 0
    # without only_missing the calibrated camera is solved again (it has no views here: left as it was)
    again, ra = calibrate_camera_array_intrinsics(ip, arr, _solver=H)
    assert set(ra) == {0, 1, 2, 5} and ra[5].status == 1 and np.array_equal(again.cameras[5].matrix, known)


def test_calibrate_extrinsics_keyword_default_is_identical_and_true_replaces_blind_defaults():
    from caliscope_amd.calibrate_extrinsics import calibrate_extrinsics
    from caliscope_amd.exceptions import CalibrationError
    from tests.test_stage_driver import _board_session, _engine_kwargs

    image_points, cameras, constraints, truth = _board_session()
    kw = _engine_kwargs("numpy")
    a = calibrate_extrinsics(image_points, cameras, constraints, **kw)
    b = calibrate_extrinsics(image_points, cameras, constraints, estimate_intrinsics=False, **kw)
    assert a.synthesized_cam_ids == b.synthesized_cam_ids and a.intrinsic_estimates == b.intrinsic_estimates
    for c, cam in a.capture_volume.camera_array.cameras.items():
        other = b.capture_volume.camera_array.cameras[c]
        assert np.array_equal(cam.matrix, other.matrix) and np.array_equal(cam.distortions, other.distortions)
        assert np.array_equal(cam.rotation, other.rotation) and np.array_equal(cam.translation, other.translation)
    cols = ["x_coord", "y_coord", "z_coord"]
    assert np.array_equal(a.capture_volume.world_points.df[cols].to_numpy(), b.capture_volume.world_points.df[cols].to_numpy())

    image_points, stripped, constraints, truth = _board_session(strip=True)
    run = calibrate_extrinsics(image_points, stripped, constraints, estimate_intrinsics=True, _intr=H, **kw)
    assert run.synthesized_cam_ids == frozenset() and run.capture_volume.optimization_status.converged
    assert all(cam.matrix is None for cam in stripped.cameras.values())
    assert len(run.intrinsic_estimates) == len(stripped.cameras)
    for est in run.intrinsic_estimates:
        f_true = truth["cameras"].cameras[est.cam_id].matrix[0, 0]
        assert abs(est.f_initial - f_true) < 0.01 * f_true and est.f_initial != 960.0, (est.cam_id, est.f_initial, f_true)
        assert abs(est.f_recovered - f_true) < 0.01 * f_true
    # a fisheye camera without intrinsics is refused without the keyword (with it: tests/test_intrinsic_calibration_gpu.py)
    fish = _board_session(strip=True)[1]
    fish.cameras[min(fish.cameras)].fisheye = True
    with pytest.raises(CalibrationError, match="fisheye"):
        calibrate_extrinsics(image_points, fish, constraints, **kw)
    # sessions without object geometry raise the existing error
    nogeo = image_points.df.copy()
    nogeo[["obj_loc_x", "obj_loc_y", "obj_loc_z"]] = np.nan
    with pytest.raises(CalibrationError, match="requires calibrated intrinsics"):
        calibrate_extrinsics(type(image_points)(nogeo), stripped, None, estimate_intrinsics=True, _intr=H, **kw)


def _two_object_session(n_frames=20):
    """One camera that sees two boards in every frame, each with its own obj_loc frame and pose; tracker rows without obj_loc between."""
    import pandas as pd

    from caliscope_amd.point_data import ImagePoints

    a, b = S.camera_scene(51, n_views=n_frames, noise=0.3), S.camera_scene(52, n_views=n_frames, noise=0.3)
    da, db = S.scene_image_points([a]).df.copy(), S.scene_image_points([b]).df.copy()
    db["object_id"] = 1
    body = da.iloc[::7].copy()
    body["object_id"], body[["obj_loc_x", "obj_loc_y", "obj_loc_z"]] = 30, np.nan
    return a, ImagePoints(pd.concat([da, body, db], ignore_index=True)), ImagePoints(da)


def test_views_are_split_by_object_and_rows_without_geometry_are_dropped():
    """Two rigid objects in one frame are two views (the key of the pose bootstrap), never one fused "board"; rows without obj_loc
    do not reach the solver."""
    scene, both, alone = _two_object_session()
    arr = CameraArray({0: CameraData(cam_id=0, size=S.SIZE)})
    out2, rep2 = calibrate_camera_array_intrinsics(both, arr, _solver=H)
    out1, rep1 = calibrate_camera_array_intrinsics(alone, arr, _solver=H)
    r2, r1 = rep2[0], rep1[0]
    assert r1.status == 0 and r2.status == 0
    assert len(r2.sync_index) == 40 and sorted(set(r2.object_id.tolist())) == [0, 1] and (r2.view_status == 0).all()
    assert out2.cameras[0].grid_count == 40 and out1.cameras[0].grid_count == 20
    f_true = scene.intr[0]
    assert abs(out2.cameras[0].matrix[0, 0] - f_true) < 0.01 * f_true and out2.cameras[0].error < 0.5, (out2.cameras[0].matrix, out2.cameras[0].error)
    # twice the views of the same camera: closer to the truth than 1 %, and to the one-object result
    assert abs(out2.cameras[0].matrix[0, 0] - out1.cameras[0].matrix[0, 0]) < 0.01 * f_true
    # the reference-named single-camera function keeps the reference's grouping (all corners of a frame), for single-board tables
    res = calibrate_intrinsics(alone, 0, S.SIZE, list(range(20)), _solver=H)
    assert res.camera_matrix[0, 0] == out1.cameras[0].matrix[0, 0] and res.frames_used == 20


def test_implausible_minimum_is_not_taken_over():
    """A mislabelled session (two boards under one object_id) still "solves": the gate of calibrate_extrinsics sends such a camera to
    the blind defaults instead of applying a 270 px minimum."""
    from caliscope_amd.calibrate_extrinsics import _estimate_missing_intrinsics, _plausible_intrinsics

    scene, both, alone = _two_object_session()
    fused = both.df[both.df["object_id"] != 30].copy()
    fused["object_id"] = 0
    arr = CameraArray({0: CameraData(cam_id=0, size=S.SIZE)})
    out, rep = calibrate_camera_array_intrinsics(type(both)(fused), arr, _solver=H)
    if rep[0].result is not None:
        assert _plausible_intrinsics(out.cameras[0], rep[0]) is not None, (out.cameras[0].matrix, out.cameras[0].error)
    assert _estimate_missing_intrinsics(type(both)(fused), arr, H) == {}
    good = _estimate_missing_intrinsics(both, arr, H)  # (whatever pose bootstrap follows, "epipolar" included: the views carry obj_loc)
    assert set(good) == {0} and abs(good[0][0][0, 0] - scene.intr[0]) < 0.01 * scene.intr[0] and good[0][2] < 0.5
    assert arr.cameras[0].matrix is None
