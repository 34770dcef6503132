"""cba_scale_errors on the MI355X: kernel edges against the g++ build and pdist, the static-marker pattern at 100 000 groups, input
errors, and the two steps after a solve end to end (align_to_object + scale report on a board session, scaled() on a 2-D-only one).
The bounds are those of tests/scale_scenes.py; nothing here is measured on the code under test.  Observed on an MI355X: the device
and the g++ build agree bit for bit in all eight numbers of every edge group, on every path (the test prints it and asks for the
bounds only); ring board session: 40 report entries, pooled RMSE 0.424 mm, reprojection RMSE unchanged by align_to_object to the
printed digits; 2-D-only session: camera distances within 1.11 mm of the truth after scaled()."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist

from caliscope_amd.exceptions import BackendError
from caliscope_amd.scale_accuracy import DeviceScaleErrors
from caliscope_amd.scale_cues import CameraDistance
from tests import scale_native
from tests.scale_scenes import assert_stats, derived_bounds, noisy_group, reference_stats, stat_bounds, uniform_scale_scene

pytestmark = pytest.mark.gpu

C = scale_native.constants()
THRESHOLDS = [C["small_max"], C["small_max"] + 1, C["lds_small"], C["lds_small"] + 1, C["lds_large"], C["lds_large"] + 1]
EDGE_SIZES = sorted({0, 1, 2, 3, 4, 11, 12, 64, 65, 256, 257, 600, 2049, 4096, *THRESHOLDS})
UNIFORM_SIZES = (3, 12, 65, 257, 600, 2049)
DEVICE, HARNESS = DeviceScaleErrors(), scale_native.HarnessScaleErrors()


def packed(groups, rng):
    """One call's arrays from (world, obj) groups: entries point into a shuffled world table."""
    sizes = [len(g[0]) for g in groups]
    world = np.concatenate([g[0] for g in groups]).reshape(-1, 3)
    perm = rng.permutation(len(world))
    return world[perm], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.argsort(perm).astype(np.int64), np.concatenate([g[1] for g in groups]).reshape(-1, 3)


@pytest.fixture(scope="module")
def edge_call():
    rng = np.random.default_rng(2024)
    sizes = [EDGE_SIZES[k] for k in rng.permutation(len(EDGE_SIZES))]  # shuffled: the bins interleave
    groups = [noisy_group(rng, n, 0.05 + 0.4 * (k % 3), (0.0, 0.002, 0.2)[k % 3]) for k, n in enumerate(sizes)]
    args = packed(groups, rng)
    return sizes, groups, args, DEVICE.scale_errors(*args), HARNESS.scale_errors(*args), HARNESS.bins.copy()


def test_kernel_edges_against_the_cpu_build(edge_call, capsys):
    sizes, groups, _, dev, cpu, bins = edge_call
    assert set(bins.tolist()) == {0, 1, 2, 3}, "every path runs in this call"
    equal = {0: True, 1: True, 2: True, 3: True}
    for n, (world, obj), d, c, b in zip(sizes, groups, dev, cpu, bins.tolist()):
        if n < 2:
            assert np.array_equal(d, np.zeros(8)) and np.array_equal(c, np.zeros(8))
            continue
        _, bounds, _ = reference_stats(world, obj)
        assert_stats(d, c, bounds, f"n = {n}, device vs g++ build")
        equal[b] &= bool(np.array_equal(d, c))
    with capsys.disabled():
        print(f"cba_scale_errors device vs g++ build, bit-equal per path (thread / stage 128 / stage 1024 / unstaged): {equal}; "
              f"max|err| and D_ref bit-equal in every group: {bool(np.array_equal(dev[:, 2:4], cpu[:, 2:4]))}")


def test_kernel_edges_against_pdist(edge_call):
    sizes, groups, _, dev, _, _ = edge_call
    for n, (world, obj), d in zip(sizes, groups, dev):
        if n >= 2:
            want, bounds, _ = reference_stats(world, obj)
            assert_stats(d, want, bounds, f"n = {n}, device vs pdist")


def test_uniform_scale_scenes_on_the_device():
    rng = np.random.default_rng(123)
    groups = [uniform_scale_scene(rng, n) for n in UNIFORM_SIZES]
    refs = [reference_stats(w, o, np.longdouble if len(w) <= 600 else np.float64) for w, o in groups]
    for (want, bounds, err), n in zip(refs, UNIFORM_SIZES):
        assert float(err.min()) > 10 * bounds["s1"], f"n = {n}: the scene cannot show a missing pair"
    dev = DEVICE.scale_errors(*packed(groups, rng))
    for (want, bounds, _), d, n in zip(refs, dev, UNIFORM_SIZES):
        assert_stats(d, want, bounds, f"uniform n = {n}")


def test_two_calls_return_the_same_bits(edge_call):
    _, _, args, dev, _, _ = edge_call
    assert np.array_equal(DEVICE.scale_errors(*args), dev)


def test_many_small_groups_sharing_world_rows():
    """100 000 groups of 3 to 5 entries over 40 world rows (a few static markers seen in every frame), one group whose entries all
    point at the same row: measured distances 0, err = -d_true."""
    rng = np.random.default_rng(9)
    n_groups, n_world = 100_000, 40
    world = rng.normal(size=(n_world, 3))
    sizes = rng.integers(3, 6, n_groups)
    group_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ent_world = rng.integers(0, n_world, group_start[-1]).astype(np.int64)
    same = 77_777
    ent_world[group_start[same]:group_start[same + 1]] = 5
    ent_obj = world[ent_world] * 0.999 + rng.normal(size=(len(ent_world), 3)) * 0.002
    dev = DEVICE.scale_errors(world, group_start, ent_world, ent_obj)
    for s in (3, 4, 5):
        g = np.flatnonzero(sizes == s)
        idx = group_start[g][:, None] + np.arange(s)[None, :]
        w, o = world[ent_world[idx]], ent_obj[idx]                      # (groups, s, 3)
        i, j = np.triu_indices(s, 1)
        dm, dt = np.sqrt(((w[:, i] - w[:, j]) ** 2).sum(axis=2)), np.sqrt(((o[:, i] - o[:, j]) ** 2).sum(axis=2))
        err = dm - dt
        m = len(i)
        L = np.maximum(dm.max(axis=1), dt.max(axis=1))
        b = stat_bounds(L, m, np.abs(err).sum(axis=1), (err * err).sum(axis=1), s, np.abs(w).max(axis=(1, 2)))
        got = dev[g]
        assert np.all(got[:, 7] == m)
        assert np.all(np.abs(got[:, 0] - err.sum(axis=1)) <= b["s1"]) and np.all(np.abs(got[:, 1] - (err * err).sum(axis=1)) <= b["s2"])
        assert np.all(np.abs(got[:, 2] - np.abs(err).max(axis=1)) <= b["mx"]) and np.all(np.abs(got[:, 3] - dt.max(axis=1)) <= b["dref"])
        assert np.all(np.abs(got[:, 4:7] - w.mean(axis=1)) <= b["centroid"][:, None])
    a, b = group_start[same], group_start[same + 1]
    want, bounds, err = reference_stats(world[ent_world[a:b]], ent_obj[a:b])
    assert np.array_equal(err, -pdist(ent_obj[a:b])) and np.all(err < 0)
    assert_stats(dev[same], want, bounds, "all entries on one world row")
    assert dev[same, 0] < 0 and dev[same, 2] == dev[same, 3]  # every measured distance is 0: the largest |err| is the largest true distance


def test_errors_name_the_position_and_the_library_goes_on():
    world, obj = np.random.default_rng(1).normal(size=(6, 3)), np.random.default_rng(2).normal(size=(4, 3))
    with pytest.raises(BackendError, match=r"code -1\).*entry 2: world row 6 out of range \[0, 6\)"):
        DEVICE.scale_errors(world, [0, 4], [0, 1, 6, 2], obj)
    with pytest.raises(BackendError, match=r"code -1\).*group_start decreases at group 1"):
        DEVICE.scale_errors(world, [0, 3, 2, 4], [0, 1, 3, 2], obj)
    n = C["max_group"] + 1
    with pytest.raises(BackendError, match=rf"code -4\).*group 0 has {n} entries; at most {C['max_group']} are supported"):
        DEVICE.scale_errors(world, [0, n], np.zeros(n, dtype=np.int64), np.zeros((n, 3)))
    got = DEVICE.scale_errors(world, [0, 4], [0, 1, 3, 2], obj)
    want, bounds, _ = reference_stats(world[[0, 1, 3, 2]], obj)
    assert_stats(got[0], want, bounds, "a valid call after the refused ones")
    assert DEVICE.scale_errors(world, [0], [], np.zeros((0, 3))).shape == (0, 8)


def _camera_distances(cams):
    ids = sorted(cams.posed_cameras)
    centres = np.array([cams.cameras[c].position for c in ids])
    return ids, np.linalg.norm(centres[:, None, :] - centres[None, :, :], axis=2)


def test_board_session_end_to_end(capsys):
    """6 cameras, 40 frames of a 9 x 6 board: calibrate_extrinsics(estimate_poses=True) -> align_to_object(mid frame) -> scale report."""
    from caliscope_amd.calibrate_extrinsics import calibrate_extrinsics
    from tests import intrinsic_scenes as S
    from tests.epipolar_scenes import unposed

    ip, cams = S.ring_board_session()
    vol = calibrate_extrinsics(ip, unposed(cams), None, estimate_poses=True).capture_volume
    frames = np.sort(vol.world_points._df["sync_index"].unique())
    aligned = vol.align_to_object(int(frames[len(frames) // 2]))
    before, after = vol.compute_reprojection_report().overall_rmse, aligned.compute_reprojection_report().overall_rmse
    assert abs(after - before) < 1e-9, (before, after)
    rep = aligned.compute_volumetric_scale_accuracy()
    cpu = aligned.compute_volumetric_scale_accuracy(_solver=HARNESS)
    # one entry per (frame, board) with at least three triangulated corners
    counts = aligned.world_points._df.groupby(["sync_index", "object_id"]).size()
    assert [(fe.sync_index, fe.object_id) for fe in rep.frame_errors] == [k for k, n in counts.items() if n >= 3]
    assert [fe.n_corners for fe in rep.frame_errors] == [int(n) for n in counts if n >= 3]
    _, _, _, _, group_start, ent_world, ent_obj = aligned._scale_groups()
    xyz = aligned.world_points.points
    for g, (d, c) in enumerate(zip(rep.frame_errors, cpu.frame_errors)):
        a, b = group_start[g], group_start[g + 1]
        stats, bounds, _ = reference_stats(xyz[ent_world[a:b]], ent_obj[a:b])
        tol = derived_bounds(stats, bounds)
        assert (d.sync_index, d.object_id, d.n_corners, d.n_distance_pairs, d.n_cameras_contributing) == \
            (c.sync_index, c.object_id, c.n_corners, c.n_distance_pairs, c.n_cameras_contributing)
        for name in ("distance_rmse_mm", "distance_mean_signed_error_mm", "distance_max_error_mm", "sum_squared_errors_m2", "sum_squared_relative_errors"):
            assert abs(getattr(d, name) - getattr(c, name)) <= tol[name], (g, name)
        assert np.all(np.abs(np.array(d.centroid) - np.array(c.centroid)) <= tol["centroid"])
    assert np.isfinite(rep.pooled_rmse_mm) and rep.pooled_rmse_mm > 0
    with capsys.disabled():
        print(f"ring board session: {len(rep.frame_errors)} report entries, pooled RMSE {rep.pooled_rmse_mm:.3f} mm, relative {rep.pooled_relative_rmse_pct:.3f} %, "
              f"bias {rep.mean_signed_error_mm:+.3f} mm; reprojection RMSE {before:.6f} px before and {after:.6f} px after align_to_object")


def test_two_d_only_session_gets_its_metres_from_one_camera_distance(capsys):
    """The same session without object geometry: estimate_poses="epipolar" leaves scale arbitrary; scaled(CameraDistance) with the true
    distance of the two cameras farthest apart brings every camera-centre distance to the truth, within the position tolerance
    tests/test_epipolar_bootstrap_gpu.py asks of its aligned poses (0.010 m, its box sessions)."""
    import pandas as pd

    from caliscope_amd.calibrate_extrinsics import calibrate_extrinsics
    from caliscope_amd.point_data import ImagePoints
    from tests import intrinsic_scenes as S
    from tests.epipolar_scenes import unposed

    ip, cams = S.ring_board_session()
    flat = ip.df
    flat[["obj_loc_x", "obj_loc_y", "obj_loc_z"]] = np.nan
    vol = calibrate_extrinsics(ImagePoints(pd.DataFrame(flat)), unposed(cams), None, refine_intrinsics=False, estimate_poses="epipolar").capture_volume
    assert set(vol.camera_array.posed_cameras) == set(cams.cameras)
    assert vol.compute_volumetric_scale_accuracy().frame_errors == ()  # no object geometry: an empty report, no device call
    ids, true = _camera_distances(cams)
    i, j = np.unravel_index(np.argmax(true), true.shape)
    metric = vol.scaled(CameraDistance(ids[i], ids[j], float(true[i, j])))
    got_ids, got = _camera_distances(metric.camera_array)
    assert got_ids == ids
    with capsys.disabled():
        print(f"2-D-only ring session: camera distances off by at most {np.abs(got - true).max() * 1000:.2f} mm after scaled(); "
              f"scale applied {got[i, j] / _camera_distances(vol.camera_array)[1][i, j]:.6f}")
    assert abs(got[i, j] - true[i, j]) < 1e-12
    assert np.abs(got - true).max() < 0.010
