"""The pose bootstrap end to end on the CPU: caliscope_amd.pose_network driven through its `_pnp` hook (the g++ build of
pnp_math.h) and CaptureVolume.bootstrap(estimate_poses=True) through the `_triangulate` hook — no optimisation."""
import numpy as np
import pandas as pd
import pytest

from caliscope_amd.cameras import CameraArray, CameraData
from caliscope_amd.capture_volume import CaptureVolume
from caliscope_amd.exceptions import CalibrationError
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.pose_network import PairedPoseNetwork, PoseNetworkBuilder, StereoPair
from oracle.scene import default_ring_scene_rows
from tests.pnp_native import HarnessPnP
from tests.scenario_scenes import pose_errors
from tests.test_stage_driver import _oracle_triangulate


def _posed_triangulate(image_points, cameras, static_ids):
    """The oracle triangulation on the posed cameras (the device path skips unposed ones the same way)."""
    posed = CameraArray(dict(cameras.posed_cameras))
    df = image_points.df
    return _oracle_triangulate(ImagePoints(df[df["cam_id"].isin(list(posed.cameras))].reset_index(drop=True)), posed, static_ids)


def _ring_session(golden_dir):
    _, cams, world_by_frame = default_ring_scene_rows(pixel_noise_sigma=0.5, random_seed=42)
    df = pd.read_csv(golden_dir / "default_ring_baseline" / "image_points_noisy.csv")
    truth_cams, unposed = {}, {}
    for cam_id, (R, t, K, dist, size) in enumerate(cams):
        truth_cams[cam_id] = CameraData(cam_id=cam_id, size=tuple(size), matrix=np.asarray(K, float), distortions=np.asarray(dist, float),
                                        rotation=np.asarray(R, float), translation=np.asarray(t, float).ravel())
        unposed[cam_id] = CameraData(cam_id=cam_id, size=tuple(size), matrix=np.asarray(K, float), distortions=np.asarray(dist, float))
    return ImagePoints(df), CameraArray(unposed), CameraArray(truth_cams), np.asarray(world_by_frame)


def test_bootstrap_estimates_poses_of_the_ring_session(golden_dir):
    image_points, cameras, truth_cams, world = _ring_session(golden_dir)
    assert not cameras.posed_cameras
    with pytest.raises(CalibrationError, match="no pose estimate"):
        CaptureVolume.bootstrap(image_points, cameras, _triangulate=_oracle_triangulate)
    vol = CaptureVolume.bootstrap(image_points, cameras, estimate_poses=True, _triangulate=_oracle_triangulate, _pnp=HarnessPnP())
    assert not cameras.posed_cameras  # the input stays untouched
    assert set(vol.camera_array.posed_cameras) == {0, 1, 2, 3}
    wdf = vol.world_points.df
    truth_points = world[wdf["sync_index"].to_numpy(), wdf["keypoint_id"].to_numpy()]
    trans, rot = pose_errors(vol, {"cameras": truth_cams, "points": truth_points})
    assert trans < 0.02 and rot < 1.0, (trans, rot)


def test_builder_states_and_reference_names(golden_dir):
    image_points, cameras, _, _ = _ring_session(golden_dir)
    b = PoseNetworkBuilder(cameras, image_points, _pnp=HarnessPnP())
    assert b.state == "initialized"
    with pytest.raises(RuntimeError):
        b.estimate_relative_poses()
    b.estimate_camera_to_object_poses()
    assert b.state == "camera_poses_estimated"
    poses = b._camera_to_object_poses.as_dict()
    assert len(poses) > 0 and all(np.isfinite(R).all() and np.isfinite(t).all() for R, t, _ in poses.values())
    net = b.estimate_relative_poses().filter_outliers().build()
    assert b.state == "built" and isinstance(net, PairedPoseNetwork)
    p = net.get_pair(0, 1)
    assert isinstance(p, StereoPair) and p.pair == (0, 1) and np.isfinite(p.error_score)
    back = p.inverted()
    assert back.pair == (1, 0) and np.allclose(p.link(back).transformation, np.eye(4), atol=1e-12)
    # every pair of the four cameras is in the graph, both directions
    assert all(net.get_pair(a, c) is not None for a in range(4) for c in range(4) if a != c)


def test_no_object_geometry_raises(golden_dir):
    image_points, cameras, _, _ = _ring_session(golden_dir)
    df = image_points.df.copy()
    df[["obj_loc_x", "obj_loc_y", "obj_loc_z"]] = np.nan
    with pytest.raises(CalibrationError, match="essential-matrix"):
        CaptureVolume.bootstrap(ImagePoints(df), cameras, estimate_poses=True, _triangulate=_oracle_triangulate, _pnp=HarnessPnP())


def test_isolated_camera_stays_unposed(golden_dir):
    """A camera that never shares a (sync_index, object_id) with another stays unposed; the others are posed."""
    image_points, cameras, _, _ = _ring_session(golden_dir)
    df = image_points.df.copy()
    extra = df[df["cam_id"] == 0].copy()
    extra["cam_id"] = 7
    extra["sync_index"] = extra["sync_index"] + 1000
    df = pd.concat([df, extra], ignore_index=True)
    cams = dict(cameras.cameras)
    cams[7] = CameraData(cam_id=7, size=cams[0].size, matrix=cams[0].matrix.copy(), distortions=cams[0].distortions.copy())
    vol = CaptureVolume.bootstrap(ImagePoints(df), CameraArray(cams), estimate_poses=True, _triangulate=_posed_triangulate, _pnp=HarnessPnP())
    assert set(vol.camera_array.posed_cameras) == {0, 1, 2, 3}
    assert 7 in vol.camera_array.unposed_cameras
