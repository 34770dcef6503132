"""The pose bootstrap on the MI355X: cba_pose_pnp_batch / cba_pose_pair_rmse against the g++ build of the same arithmetic and
numpy, and CaptureVolume.bootstrap / calibrate_extrinsics with estimate_poses=True from unposed cameras."""
import numpy as np
import pandas as pd
import pytest

from caliscope_amd.cameras import CameraArray, CameraData, rvec_to_matrix
from caliscope_amd.capture_volume import CaptureVolume
from caliscope_amd.exceptions import CalibrationError
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.pose_network import DevicePnP
from caliscope_amd.synthetic import WEBCAM_SIZE, project_pinhole_bc5, ring_camera_array
from tests.pnp_native import HarnessPnP
from tests.scenario_scenes import keyed_errors, two_sided_board_session

pytestmark = pytest.mark.gpu


def _unposed(cameras):
    return CameraArray({c: CameraData(cam_id=c, size=cam.size, matrix=None if cam.matrix is None else cam.matrix.copy(),
                                      distortions=None if cam.distortions is None else cam.distortions.copy(), fisheye=cam.fisheye)
                        for c, cam in cameras.cameras.items()})


def ring_board_session(n_cams=6, n_frames=40, rows=6, cols=9, spacing=0.04, noise_px=0.5, seed=11):
    """Ring cameras around a planar board (object 0 at z = 0) that tilts and drifts through the volume."""
    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams, radius=1.5, target=(0.0, 0.0, 0.5))
    grid = np.array([[c * spacing, r * spacing, 0.0] for r in range(rows) for c in range(cols)])
    off = grid.mean(axis=0)
    w, h = WEBCAM_SIZE
    out, truth = [], {}
    for f in range(n_frames):
        s = f / max(n_frames - 1, 1)
        R = rvec_to_matrix(np.array([0.0, 0.0, 2 * np.pi * s])) @ rvec_to_matrix(np.array([np.pi / 2 + 0.3 * np.sin(4 * s), 0.0, 0.0]))
        X = (grid - off) @ R.T + np.array([0.2 * np.cos(3 * s), 0.2 * np.sin(2 * s), 0.5 + 0.1 * np.sin(5 * s)])
        for c, cam in sorted(cams.cameras.items()):
            K = cam.matrix
            p, z = project_pinhole_bc5(X, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
            ok = (z > 0.1) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)
            if ok.sum() < 8 or abs(float(R[:, 2] @ (-cam.rotation.T @ cam.translation - X.mean(0)))) < 0.3:
                continue
            p = p + rng.normal(0, noise_px, p.shape)
            for k in np.flatnonzero(ok):
                out.append(dict(sync_index=f, cam_id=c, object_id=0, keypoint_id=int(k), img_loc_x=p[k, 0], img_loc_y=p[k, 1],
                                obj_loc_x=grid[k, 0], obj_loc_y=grid[k, 1], obj_loc_z=0.0))
                truth[(f, 0, int(k))] = X[k]
    return ImagePoints(pd.DataFrame(out)), cams, dict(cameras=cams, points=truth)


def _views(seed=3, n_views=300):
    """Random board views (planar at z = 0 / z = const, non-planar, too few, degenerate) in the CSR form of the batch call."""
    rng = np.random.default_rng(seed)
    sizes, obj, xy, cam = [], [], [], []
    intr = np.array([[1400.0, 1390.0, 960.0, 540.0, 0.1, -0.2, 0.001, 0.002, 0.05], [900.0, 900.0, 640.0, 360.0, 0.05, 0.01, 0.02, -0.01, 0.0]])
    for v in range(n_views):
        kind = v % 5
        # (views of 8+ points: with fewer, the pose moves by ~1e-9 for a one-ulp change of the data, and the device's sin / cos
        # are not the host's to the last bit)
        n = 3 if v % 10 == 7 else int(rng.integers(8, 60))
        if kind == 3:
            P = rng.uniform(-0.2, 0.2, (n, 3))
        else:
            P = np.column_stack([rng.uniform(0, 0.3, (n, 2)), np.full(n, 0.006 * (kind == 1))])
        if kind == 4:
            P[:, 1] = 0.0  # collinear
        R = rvec_to_matrix(rng.normal(0, 0.5, 3))
        t = np.array([0.0, 0.0, 1.5]) - R @ P.mean(0)
        Xc = P @ R.T + t
        uv = Xc[:, :2] / Xc[:, 2:] + rng.normal(0, 5e-4, (n, 2))
        c = v % 2
        K = intr[c]
        # (the batch undistorts: feed it pixels through the distortion model of its camera)
        px, _ = project_pinhole_bc5(np.column_stack([uv, np.ones(n)]), np.eye(3), np.zeros(3), K[0], K[1], K[2], K[3], K[4:9])
        sizes.append(n); obj.append(P); xy.append(px); cam.append(c)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return start, np.array(cam, np.int32), np.zeros(2, np.int32), intr, np.concatenate(xy), np.concatenate(obj)


def test_pnp_batch_matches_cpu_build():
    args = _views()
    dev = DevicePnP().pnp_batch(*args, 4, True)
    cpu = HarnessPnP().pnp_batch(*args, 4, True)
    pose_d, rmse_d, st_d, und_d = dev
    pose_c, rmse_c, st_c, und_c = cpu
    assert np.array_equal(st_d, st_c)
    assert {0, 1, 2} <= set(st_d.tolist())
    np.testing.assert_allclose(und_d, und_c, rtol=0, atol=1e-12)
    ok = st_d == 0
    np.testing.assert_allclose(pose_d[ok], pose_c[ok], rtol=0, atol=1e-12 * max(1.0, np.abs(pose_c[ok]).max()))
    np.testing.assert_allclose(rmse_d, rmse_c, rtol=1e-9, atol=1e-12)
    assert np.isfinite(pose_d).all() and np.isfinite(rmse_d).all()
    assert np.array_equal(pose_d[~ok], np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), ((~ok).sum(), 1)))


def _numpy_pair_rmse(rt, a, b):
    R, t = rt[:9].reshape(3, 3), rt[9:]
    P1, P2 = np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([R, t[:, None]])
    err = []
    for (xa, ya), (xb, yb) in zip(a, b):
        A = np.stack([xa * P1[2] - P1[0], ya * P1[2] - P1[1], xb * P2[2] - P2[0], yb * P2[2] - P2[1]])
        X = np.linalg.svd(A)[2][-1]
        X = X[:3] / X[3]
        pb = R @ X + t
        err += [(xa - X[0] / X[2]) ** 2 + (ya - X[1] / X[2]) ** 2, (xb - pb[0] / pb[2]) ** 2 + (yb - pb[1] / pb[2]) ** 2]
    return np.sqrt(np.mean(err))


def test_pair_rmse_matches_numpy_dlt_and_is_deterministic():
    rng = np.random.default_rng(8)
    poses, A, B, sizes = [], [], [], []
    for m in (4, 5, 63, 64, 65, 257, 1000, 3):
        R = rvec_to_matrix(rng.normal(0, 0.4, 3))
        t = np.array([0.8, 0.05, 0.1]) + rng.normal(0, 0.05, 3)
        X = rng.uniform(-0.3, 0.3, (m, 3)) + [0, 0, 2.0]
        a = X[:, :2] / X[:, 2:] + rng.normal(0, 1e-3, (m, 2))
        Xb = X @ R.T + t
        b = Xb[:, :2] / Xb[:, 2:] + rng.normal(0, 1e-3, (m, 2))
        poses.append(np.concatenate([R.ravel(), t])); A.append(a); B.append(b); sizes.append(m)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    args = (np.stack(poses), start, np.concatenate(A), np.concatenate(B))
    rmse, count = DevicePnP().pair_rmse(*args)
    assert count.tolist() == sizes
    for p in range(len(sizes)):
        assert abs(rmse[p] - _numpy_pair_rmse(poses[p], A[p], B[p])) < 1e-10
    again, _ = DevicePnP().pair_rmse(*args)
    assert np.array_equal(rmse, again)


def test_real_session_bootstrap_reaches_the_stored_pose_minimum(golden_dir):
    """tests/golden/post_optimization with every pose removed: the estimated start converges to the same minimum as the
    stored poses."""
    d = golden_dir / "post_optimization"
    stored = CameraArray.from_toml(d / "camera_array.toml")
    ip = ImagePoints.from_csv(d / "xy_CHARUCO.csv")
    ref = CaptureVolume.bootstrap(ip, stored).optimize(ftol=1e-12)
    est = CaptureVolume.bootstrap(ip, _unposed(stored), estimate_poses=True).optimize(ftol=1e-12)
    assert set(est.camera_array.posed_cameras) == set(stored.posed_cameras)
    r_ref, r_est = ref.reprojection_report.overall_rmse, est.reprojection_report.overall_rmse
    assert abs(r_ref - r_est) < 1e-6, (r_ref, r_est)
    wdf = ref.world_points.df
    truth = dict(cameras=ref.camera_array, points={k: p for k, p in zip(zip(wdf.sync_index, wdf.object_id, wdf.keypoint_id),
                                                                   wdf[["x_coord", "y_coord", "z_coord"]].to_numpy())})
    trans, rot, rmse = keyed_errors(est, truth)
    assert trans < 1e-6 and np.radians(rot) < 1e-6 and rmse < 1e-6, (trans, rot, rmse)


@pytest.mark.parametrize("scene", ["two_sided", "ring_board"])
def test_calibrate_extrinsics_from_unposed_cameras(scene):
    from caliscope_amd.calibrate_extrinsics import calibrate_extrinsics

    if scene == "two_sided":
        ip, cams, constraints, truth = two_sided_board_session(n_cams=8, radius=1.2, n_frames=30, thickness=0.006)
    else:
        ip, cams, truth = ring_board_session()
        constraints = None
    run = calibrate_extrinsics(ip, _unposed(cams), constraints, refine_intrinsics=False, estimate_poses=True)
    vol = run.capture_volume
    assert vol.optimization_status.converged and set(vol.camera_array.posed_cameras) == set(cams.cameras)
    trans, rot, _ = keyed_errors(vol, truth)
    assert rot < 0.5 and trans < 0.005, (trans, rot)


def test_blind_intrinsics_run_on_the_pnp_path():
    from caliscope_amd.calibrate_extrinsics import calibrate_extrinsics

    ip, cams, _ = ring_board_session()
    blind = CameraArray({c: CameraData(cam_id=c, size=cam.size) for c, cam in cams.cameras.items()})
    run = calibrate_extrinsics(ip, blind, None, refine_intrinsics=True, estimate_poses=True)
    assert run.synthesized_cam_ids == frozenset(cams.cameras)
    assert set(run.capture_volume.camera_array.posed_cameras) == set(cams.cameras)
    assert run.capture_volume.optimization_status is not None


def test_edge_cases_isolated_camera_no_geometry_and_repeatability():
    ip, cams, _ = ring_board_session(n_cams=5)
    df = ip.df.copy()
    lone = df[df["cam_id"] == 0].copy()
    lone["cam_id"], lone["sync_index"] = 9, lone["sync_index"] + 10_000
    cams9 = _unposed(cams)
    cams9.cameras[9] = CameraData(cam_id=9, size=cams.cameras[0].size, matrix=cams.cameras[0].matrix.copy(),
                                  distortions=cams.cameras[0].distortions.copy())
    ip9 = ImagePoints(pd.concat([df, lone], ignore_index=True))
    vol = CaptureVolume.bootstrap(ip9, cams9, estimate_poses=True)
    assert 9 in vol.camera_array.unposed_cameras and set(vol.camera_array.posed_cameras) == set(cams.cameras)
    assert vol.optimize().optimization_status.converged  # the solve runs on the posed cameras

    nan = df.copy()
    nan[["obj_loc_x", "obj_loc_y", "obj_loc_z"]] = np.nan
    with pytest.raises(CalibrationError, match="essential-matrix"):
        CaptureVolume.bootstrap(ImagePoints(nan), _unposed(cams), estimate_poses=True)

    a = CaptureVolume.bootstrap(ip, _unposed(cams), estimate_poses=True)
    b = CaptureVolume.bootstrap(ip, _unposed(cams), estimate_poses=True)
    for c in cams.cameras:
        assert np.array_equal(a.camera_array.cameras[c].rotation, b.camera_array.cameras[c].rotation)
        assert np.array_equal(a.camera_array.cameras[c].translation, b.camera_array.cameras[c].translation)


def test_pnp_batch_without_the_undistorted_points(monkeypatch):
    """undistorted_out is optional in the C ABI (the wrapper always asks for it): a call without it returns the same poses, RMSE and
    statuses bit for bit, which stand against the g++ build as in test_pnp_batch_matches_cpu_build.  Twelve views of two cameras."""
    from caliscope_amd.pose_network import POSE_SIGNATURES
    from tests.helpers import null_outputs

    args = _views(n_views=12)
    full = DevicePnP().pnp_batch(*args, 4, True)
    cpu = HarnessPnP().pnp_batch(*args, 4, True)
    null_outputs(monkeypatch, POSE_SIGNATURES, "cba_pose_pnp_batch", drop={3})
    pose, rmse, status, und = DevicePnP().pnp_batch(*args, 4, True)
    assert not und.any() and full[3].any()  # nothing was copied back
    assert np.array_equal(pose, full[0]) and np.array_equal(rmse, full[1]) and np.array_equal(status, full[2])
    assert np.array_equal(status, cpu[2]) and {0, 1} <= set(status.tolist())
    ok = status == 0
    np.testing.assert_allclose(pose[ok], cpu[0][ok], rtol=0, atol=1e-12 * max(1.0, np.abs(cpu[0][ok]).max()))
    np.testing.assert_allclose(rmse, cpu[1], rtol=1e-9, atol=1e-12)
