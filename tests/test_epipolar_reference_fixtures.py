"""The epipolar bootstrap's host stages against the reference's own builder (tests/golden/make_epipolar_fixtures.py): on the same
scripted solver results (tests/epipolar_script.py), caliscope_amd.epipolar_pose must score the scaffold candidates as the reference
does, reject the twisted pair that ranks first by cheirality, count the camera with < 50 cloud points as a failure, package the
same anchor-relative pairs and pose the same rig.  Also triangulate_scaffold and resection_camera on the g++ harness."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import caliscope_amd.epipolar_pose as ep
from caliscope_amd.cameras import CameraArray, CameraData, rvec_to_matrix
from caliscope_amd.point_data import ImagePoints
from tests import epipolar_script as S
from tests.epipolar_native import HarnessEpipolar

FIXTURES = sorted((Path(__file__).parent / "golden" / "epipolar").glob("epi_*.npz"))


def _cams():
    return CameraArray({c: CameraData(cam_id=c, size=(1280, 720), matrix=S.K.copy(), distortions=np.zeros(5)) for c in range(S.N_CAMS)})


@pytest.mark.parametrize("path", FIXTURES, ids=[p.stem for p in FIXTURES])
def test_same_choices_as_the_reference(path, monkeypatch):
    fx = np.load(path)
    df = pd.DataFrame(fx["df_int"], columns=["sync_index", "cam_id", "object_id", "keypoint_id"])
    df["img_loc_x"], df["img_loc_y"] = fx["df_xy"][:, 0], fx["df_xy"][:, 1]
    df["obj_loc_x"] = df["obj_loc_y"] = df["obj_loc_z"] = np.nan
    poses = {c: (fx["true_R"][c], fx["true_t"][c]) for c in range(S.N_CAMS)}
    captured = {}
    finish = ep.estimate_pnp_paired_pose_network

    def finish_rec(aggregated, common, _pnp=None):
        captured.update(aggregated)
        return finish(aggregated, common, _pnp=_pnp)

    monkeypatch.setattr(ep, "estimate_pnp_paired_pose_network", finish_rec)
    report = {}
    cams = _cams()
    net = ep.build_epipolar_pose_network(ImagePoints(df), cams, report=report, _epi=S.ScriptedEpipolar(df, poses, range(S.N_CAMS)))
    net.apply_to(cams)

    ref = fx["scores"]
    got = np.array([s for s in report["scores"]], dtype=np.float64)
    assert got.shape == ref.shape[:1] + (5,)
    np.testing.assert_array_equal(got[:, [0, 1, 2, 4]], ref[:, [0, 1, 2, 4]])  # candidate order, failures, -cheirality
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-7, atol=1e-12)  # worst median third-view error
    assert tuple(report["scaffold"]) == tuple(fx["scaffold"])
    assert tuple(got[0, :2]) in S.TWISTED and tuple(report["scaffold"]) not in S.TWISTED  # ranked first, lost on the third views
    assert sorted(captured) == [tuple(p) for p in fx["agg_keys"]]
    for p, R, t in zip(fx["agg_keys"], fx["agg_R"], fx["agg_t"]):
        np.testing.assert_allclose(captured[tuple(p)].rotation, R, atol=1e-8)
        np.testing.assert_allclose(captured[tuple(p)].translation, t, atol=1e-8)
    posed = np.array([cams.cameras[c].rotation is not None for c in range(S.N_CAMS)])
    assert np.array_equal(posed, fx["posed"]) and not posed[S.SHORT_CAM]
    for c in np.flatnonzero(posed):
        np.testing.assert_allclose(cams.cameras[c].rotation, fx["out_R"][c], atol=1e-8)
        np.testing.assert_allclose(np.ravel(cams.cameras[c].translation), fx["out_t"][c], atol=1e-8)


def test_fixtures_present():
    assert len(FIXTURES) == 3


def _two_view_scene(n=200, seed=1):
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-1, 1, (n, 2)), rng.uniform(4, 6, n)])
    R, t = rvec_to_matrix(np.array([0.05, 0.3, -0.1])), np.array([1.0, 0.1, 0.2])
    K = np.array([[1000.0, 0, 640.0], [0, 1000.0, 360.0], [0, 0, 1.0]])
    px = lambda P: P[:, :2] / P[:, 2:] * 1000.0 + [640.0, 360.0]  # noqa: E731
    cam = lambda c: CameraData(cam_id=c, size=(1280, 720), matrix=K, distortions=np.zeros(5))  # noqa: E731
    return X, R, t, px, cam


def test_triangulate_scaffold_and_resection_camera():
    X, R, t, px, cam = _two_view_scene()
    n = len(X)
    pose = ep.recover_pair_pose(px(X), px(X @ R.T + t), camera_a=cam(0), camera_b=cam(1), _epi=HarnessEpipolar())
    keys = np.column_stack([np.zeros(n, np.int64), np.arange(n), np.full(n, 7)])
    cloud = ep.triangulate_scaffold(pose, keys)
    assert len(cloud) == n
    scale = 1.0 / np.linalg.norm(t)
    for i in (0, 17, n - 1):
        np.testing.assert_allclose(cloud[(0, i, 7)], X[i] * scale, atol=1e-9)
    # a third camera at a known pose sees the points (rows shuffled, some keys absent from the cloud)
    R3, t3 = rvec_to_matrix(np.array([-0.1, -0.3, 0.05])), np.array([-1.2, 0.0, 0.4])
    rng = np.random.default_rng(2)
    order = rng.permutation(n + 20)
    kp = np.concatenate([np.arange(n), n + np.arange(20)])[order]
    Xall = np.vstack([X, X[:20] + 0.1])[order]
    p3 = px(Xall @ R3.T + t3)
    df3 = pd.DataFrame({"sync_index": 7, "cam_id": 3, "object_id": 0, "keypoint_id": kp, "img_loc_x": p3[:, 0], "img_loc_y": p3[:, 1]})
    Rr, tr, m, med = ep.resection_camera(cloud, df3, cam(3), _epi=HarnessEpipolar())
    assert m == n
    np.testing.assert_allclose(Rr, R3, atol=1e-8)
    np.testing.assert_allclose(tr, t3 * scale, atol=1e-8)
    assert med < 1e-9
    with pytest.raises(ValueError, match="cloud points"):
        ep.resection_camera(cloud, df3[df3.keypoint_id < 40], cam(3), _epi=HarnessEpipolar())
