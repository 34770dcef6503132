"""The host stages of caliscope_amd.pose_network against the reference's own outputs (tests/golden/pose_network/, made by
tests/golden/make_pose_network_fixtures.py): relative poses, IQR rejection, aggregation, the bridged graph and the anchored
camera array — runs without a GPU."""
from pathlib import Path

import numpy as np
import pytest

from caliscope_amd.cameras import CameraArray, CameraData
from caliscope_amd.pose_network import (
    PairedPoseNetwork, StereoPair, ViewPoses, aggregate_poses, compute_relative_poses, reject_outliers,
)

CASES = sorted((Path(__file__).parent / "golden" / "pose_network").glob("pnet_*.npz"))


def _cameras(z):
    return CameraArray({int(c): CameraData(cam_id=int(c), size=(640, 480), ignore=bool(ig)) for c, ig in zip(z["cams"], z["ignore"])})


def _stages(z):
    k = z["in_keys"]
    vp = ViewPoses(k[:, 0], k[:, 1], k[:, 2], z["in_R"], z["in_t"], z["in_rmse"])
    rel = compute_relative_poses(vp, _cameras(z))
    kept = reject_outliers(rel)
    agg = aggregate_poses(rel, kept)
    return rel, kept, agg


def test_fixtures_present():
    assert len(CASES) == 6


@pytest.mark.parametrize("path", CASES, ids=lambda p: p.stem)
def test_relative_poses_and_outlier_rejection_match_the_reference(path):
    z = np.load(path)
    rel, kept, _ = _stages(z)
    got = np.column_stack([rel.cam_a, rel.cam_b, rel.sync_index, rel.object_id]).reshape(-1, 4)
    order = np.lexsort(got.T[::-1])
    assert np.array_equal(got[order], z["rel_keys"])
    np.testing.assert_allclose(rel.rotation[order], z["rel_R"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(rel.translation[order], z["rel_t"], rtol=0, atol=1e-12)
    kept_rows = np.concatenate([idx for idx in kept.values()]) if kept else np.zeros(0, np.int64)
    kept_keys = sorted(map(tuple, got[kept_rows].tolist()))
    assert kept_keys == sorted(map(tuple, z["kept"].tolist()))


@pytest.mark.parametrize("path", CASES, ids=lambda p: p.stem)
def test_aggregation_graph_and_anchor_match_the_reference(path):
    z = np.load(path)
    _, _, agg = _stages(z)
    assert sorted(agg) == [tuple(p) for p in z["agg_keys"].tolist()]
    for i, p in enumerate(map(tuple, z["agg_keys"].tolist())):
        np.testing.assert_allclose(agg[p].rotation, z["agg_R"][i], rtol=0, atol=1e-12)
        np.testing.assert_allclose(agg[p].translation, z["agg_t"][i], rtol=0, atol=1e-12)
    # the graph from the reference's aggregated pairs with the injected error scores
    raw = {tuple(p): StereoPair(int(p[0]), int(p[1]), float(e), t, R)
           for p, e, R, t in zip(z["agg_keys"].tolist(), z["errors"], z["agg_R"], z["agg_t"])}
    net = PairedPoseNetwork.from_raw_estimates(raw)
    assert sorted(net._pairs) == [tuple(p) for p in z["net_keys"].tolist()]
    for i, p in enumerate(map(tuple, z["net_keys"].tolist())):
        sp = net.get_pair(*p)
        np.testing.assert_allclose(sp.rotation, z["net_R"][i], rtol=0, atol=1e-12)
        np.testing.assert_allclose(sp.translation, z["net_t"][i], rtol=0, atol=1e-12)
        assert abs(sp.error_score - z["net_err"][i]) <= 1e-12
    cams = _cameras(z)
    net.apply_to(cams)
    posed = np.array([cams.cameras[int(c)].rotation is not None for c in z["cams"]])
    assert np.array_equal(posed, z["posed"])
    anchor = [int(c) for c in z["cams"] if posed[c] and np.array_equal(cams.cameras[int(c)].rotation, np.eye(3))
              and not np.any(cams.cameras[int(c)].translation)]
    assert anchor == z["anchor"].tolist()
    for c in np.flatnonzero(posed):
        np.testing.assert_allclose(cams.cameras[int(c)].rotation, z["out_R"][c], rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.ravel(cams.cameras[int(c)].translation), z["out_t"][c], rtol=0, atol=1e-12)
