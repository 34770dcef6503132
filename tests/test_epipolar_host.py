"""The epipolar bootstrap's host stages on the CPU: caliscope_amd.epipolar_pose driven through its `_epi` hook (the g++ build of
epipolar_math.h), CaptureVolume.bootstrap(estimate_poses="auto" | "epipolar") through the `_triangulate` hook, and the gates."""
import numpy as np
import pandas as pd
import pytest

from caliscope_amd.cameras import CameraArray, CameraData
from caliscope_amd.capture_volume import CaptureVolume
from caliscope_amd.epipolar_pose import build_epipolar_pose_network, pair_correspondences, pooled_correspondences, recover_pair_pose
from caliscope_amd.exceptions import CalibrationError
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.pose_network import build_paired_pose_network
from tests.epipolar_native import HarnessEpipolar
from tests.epipolar_scenes import constellation_session, unposed
from tests.scenario_scenes import keyed_errors
from tests.test_pose_bootstrap_cpu import _posed_triangulate


def test_pooled_correspondences_matches_and_drops_nan():
    df_a = pd.DataFrame({"sync_index": [0, 0, 1, 2], "cam_id": [0, 0, 0, 0], "object_id": [0, 0, 0, 0], "keypoint_id": [1, 2, 1, 1],
                         "img_loc_x": [10.0, 20.0, 11.0, np.nan], "img_loc_y": [10.0, 20.0, 11.0, 40.0]})
    df_b = pd.DataFrame({"sync_index": [0, 0, 1, 2], "cam_id": [1, 1, 1, 1], "object_id": [0, 0, 0, 0], "keypoint_id": [1, 2, 3, 1],
                         "img_loc_x": [110.0, 120.0, 130.0, 140.0], "img_loc_y": [110.0, 120.0, 130.0, 140.0]})
    keys, pix_a, pix_b = pooled_correspondences(df_a, df_b)
    assert {(int(o), int(k), int(s)) for o, k, s in keys} == {(0, 1, 0), (0, 2, 0)}
    assert np.isfinite(pix_a).all() and np.isfinite(pix_b).all()
    np.testing.assert_array_equal(pix_b[np.argsort(keys[:, 1])], [[110.0, 110.0], [120.0, 120.0]])


def test_batched_correspondences_equal_the_per_pair_merge():
    ip, _, _ = constellation_session(n_cams=4, n_frames=6, dropout=0.2)
    df = ip.df
    arr = lambda c: df[c].to_numpy(dtype=np.int64)  # noqa: E731
    pairs, start, ra, rb, _ = pair_correspondences(arr("cam_id"), arr("sync_index"), arr("object_id"), arr("keypoint_id"))
    assert pairs == sorted(pairs) and len(pairs) == 6
    for p, (a, b) in enumerate(pairs):
        keys, pa, pb = pooled_correspondences(df[df.cam_id == a], df[df.cam_id == b])
        s, e = start[p], start[p + 1]
        got = sorted(zip(df.keypoint_id.to_numpy()[ra[s:e]], df.sync_index.to_numpy()[ra[s:e]], df.img_loc_x.to_numpy()[rb[s:e]]))
        ref = sorted(zip(keys[:, 1], keys[:, 2], pb[:, 0]))
        assert got == ref


def test_recover_pair_pose_exact():
    """The reference unit test: noiseless pixels of a 300-point cloud, K with f = 1600."""
    from caliscope_amd.cameras import rvec_to_matrix

    rng = np.random.default_rng(0)
    X = rng.uniform([-0.5, -0.5, 4.0], [0.5, 0.5, 6.0], size=(300, 3))
    K = np.array([[1600.0, 0, 960.0], [0, 1600.0, 540.0], [0, 0, 1.0]])
    cam_a = CameraData(cam_id=0, size=(1920, 1080), matrix=K, distortions=np.zeros(5))
    cam_b = CameraData(cam_id=1, size=(1920, 1080), matrix=K, distortions=np.zeros(5))
    R, t = rvec_to_matrix(np.array([0.05, 0.35, -0.1])), np.array([1.2, 0.1, 0.3])
    proj = lambda P: (P[:, :2] / P[:, 2:]) * 1600.0 + [960.0, 540.0]  # noqa: E731
    pose = recover_pair_pose(proj(X), proj(X @ R.T + t), camera_a=cam_a, camera_b=cam_b, _epi=HarnessEpipolar())
    np.testing.assert_allclose(pose["rotation"], R, atol=1e-8)
    np.testing.assert_allclose(pose["translation"], t / np.linalg.norm(t), atol=1e-8)
    assert pose["conditioning"] > 0.9 and pose["n_inliers"] == 300 and pose["cheirality_inliers"] == 300
    assert len(pose["inlier_index"]) == 300 and pose["norm_a"].shape == (300, 2)


def test_cpu_end_to_end_bootstrap_auto():
    ip, cams, truth = constellation_session(n_cams=4, n_frames=30)
    assert ip.df[["obj_loc_x", "obj_loc_y", "obj_loc_z"]].isna().all().all()
    vol = CaptureVolume.bootstrap(ip, unposed(cams), estimate_poses="auto", _triangulate=_posed_triangulate, _epi=HarnessEpipolar())
    assert set(vol.camera_array.posed_cameras) == set(cams.cameras)
    trans, rot, _ = keyed_errors(vol, truth)
    assert rot < 1.0 and trans < 0.03, (trans, rot)


def test_epipolar_network_poses_gapped_camera_ids():
    ip, cams, _ = constellation_session(n_cams=3, n_frames=30, cam_ids=[1, 2, 5])
    net = build_paired_pose_network(ip, unposed(cams), method="epipolar", _epi=HarnessEpipolar())
    target = unposed(cams)
    net.apply_to(target)
    assert set(target.posed_cameras) == {1, 2, 5}


def test_gates():
    ip, cams, _ = constellation_session(n_cams=2, n_frames=20)
    df = ip.df
    disjoint = df[((df.cam_id == 0) & (df.sync_index < 10)) | ((df.cam_id == 1) & (df.sync_index >= 10))].reset_index(drop=True)
    with pytest.raises(CalibrationError, match="overlap"):
        CaptureVolume.bootstrap(ImagePoints(disjoint), unposed(cams), estimate_poses="epipolar", _epi=HarnessEpipolar())
    one = df[df.cam_id == 0].reset_index(drop=True)
    with pytest.raises(CalibrationError, match="at least 2 cameras"):
        build_epipolar_pose_network(ImagePoints(one), unposed(cams), _epi=HarnessEpipolar())
    for bad in ("essential", 2, 1.0, "PNP"):
        with pytest.raises(ValueError, match="estimate_poses"):
            CaptureVolume.bootstrap(ip, unposed(cams), estimate_poses=bad, _epi=HarnessEpipolar())
    with pytest.raises(ValueError, match="method"):
        build_paired_pose_network(ip, unposed(cams), method="essential")
    for legacy in (True, "pnp"):
        with pytest.raises(CalibrationError, match="essential-matrix"):
            CaptureVolume.bootstrap(ip, unposed(cams), estimate_poses=legacy, _epi=HarnessEpipolar())
    with pytest.raises(ValueError, match="obj_loc"):
        build_paired_pose_network(ip, unposed(cams))


def test_run_to_run_identical():
    ip, cams, _ = constellation_session(n_cams=3, n_frames=20)
    a, b = unposed(cams), unposed(cams)
    build_paired_pose_network(ip, a, method="auto", _epi=HarnessEpipolar()).apply_to(a)
    build_paired_pose_network(ip, b, method="auto", _epi=HarnessEpipolar()).apply_to(b)
    for c in cams.cameras:
        assert np.array_equal(a.cameras[c].rotation, b.cameras[c].rotation)
        assert np.array_equal(a.cameras[c].translation, b.cameras[c].translation)
    assert isinstance(a, CameraArray)


def test_estimate_poses_values_and_the_intrinsics_gate():
    from caliscope_amd.calibrate_extrinsics import calibrate_extrinsics
    from caliscope_amd.capture_volume import pose_method

    assert pose_method(False) is None and pose_method(None) is None and pose_method(np.False_) is None
    assert pose_method(True) == "pnp" and pose_method(np.True_) == "pnp"
    assert [pose_method(m) for m in ("pnp", "epipolar", "auto")] == ["pnp", "epipolar", "auto"]
    # estimate_poses="epipolar" ignores obj_loc: blind f = width / 2 intrinsics are refused even when obj_loc is present
    ip, cams, _ = constellation_session(n_cams=2, n_frames=5, with_obj_loc=True)
    blind = CameraArray({c: CameraData(cam_id=c, size=cam.size) for c, cam in cams.cameras.items()})
    with pytest.raises(CalibrationError, match="requires calibrated intrinsics"):
        calibrate_extrinsics(ip, blind, None, estimate_poses="epipolar", _epi=HarnessEpipolar())
