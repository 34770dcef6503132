"""The pose-bootstrap kernels of pose_lib.hip at their shape edges on the MI355X (scenes: tests/pose_edge_scenes.py, whose properties
tests/test_pose_edge_scenes.py checks on the g++ build).  Every call is compared with

  * the g++ build of the same arithmetic: statuses, winners, counts and flags equal; pose to 1e-9, undistorted points equal bit for bit,
    conditioning and err to rtol 1e-6, xyz to 1e-9, PnP pose to 1e-12 x scale, PnP rmse to rtol 1e-9 (the project's figures for these
    quantities).  A pair or job with an item within relative 1e-6 of its gate at the CPU build's pose may be decided differently by
    the two builds and is left out of the comparison: at most one per call, named in the message (the scenes have none on the CPU
    build);
  * plain numpy in np.longdouble from the returned pose alone (tests.pose_edge_scenes.check_*): Sampson distances give the flags and
    n_inliers, reprojection errors give err and n_inliers, the SVD two-view point gives xyz, flag 2 and n_cheiral;
  * ground truth, with limits of twice what the CPU build achieves on the same scene (tests/test_pose_edge_scenes.py holds the CPU
    figures and asserts them);

and run twice: the outputs are bit-identical.

Limits taken from measurements on the CPU build:
  xyz against the SVD point     CPU build 6.4e-13 relative (limit there 6.5e-13), device limit 6.5e-12
  mixed essential scene, n_hyp >= 128, pairs of 127 and up: rotation 0.144 deg, direction 0.332 deg (CPU limits 0.15 / 0.34), device 0.30 / 0.68
  tail scenes: essential 0.013 / 0.0152 deg (CPU limits 0.014 / 0.016), device 0.028 / 0.032; resection 0.0131 deg / 8.6e-5
    (0.014 / 1.0e-4), device 0.028 / 2.0e-4
  many resection jobs: 0.282 deg / 0.01047 (0.29 / 0.0105), device 0.58 / 0.021
  many essential pairs (exact correspondences): 4.35e-6 / 1.21e-6 deg (4.4e-6 / 1.3e-6), device 8.8e-6 / 2.6e-6
  resection edges, n_hyp 100 and 200: 0.0926 deg / 0.00309 (0.093 / 0.0031), device 0.186 / 0.0062
  PnP views of 8 points and up: 6.95 deg / 0.0269 (7.0 / 0.027), device 14.0 / 0.054
"""
import numpy as np
import pytest

from caliscope_amd.epipolar_pose import DeviceEpipolar
from caliscope_amd.pose_network import DevicePnP
from tests import pose_edge_scenes as S
from tests import test_pose_edge_scenes as CPU
from tests.epipolar_native import HarnessEpipolar, essential_counts, resect_counts
from tests.pnp_native import HarnessPnP

pytestmark = pytest.mark.gpu

XYZ_DEVICE_REL = 10.0 * CPU.XYZ_CPU_REL


def _bit_identical(a, b, keys):
    for k in keys:
        assert np.array_equal(np.nan_to_num(a[k]), np.nan_to_num(b[k])) and np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k


ESS_KEYS = ("pose", "status", "n_inliers", "n_cheiral", "conditioning", "winner", "flag", "xyz", "undistorted")
RES_KEYS = ("pose", "status", "n_inliers", "winner", "err")


def _skip_of(on_gate, what):
    assert len(on_gate) <= 1, f"{what} on the gate at the CPU build's pose: {on_gate} (at most one may be left out)"
    return set(on_gate)


def _essential_matches_cpu(args, dev, cpu, on_gate=None, values=True):
    """`values=False`: statuses, winners, counts, flags and undistorted points only (the poses, conditioning and points are then
    compared by a test of their own)."""
    assert np.array_equal(dev["undistorted"], cpu["undistorted"])  # (plain arithmetic without contraction in both builds: equal bits)
    skip = _skip_of(S.pairs_on_the_gate(args, cpu) if on_gate is None else on_gate, "pairs")
    keep = np.array([p not in skip for p in range(len(cpu["status"]))], dtype=bool)
    assert np.array_equal(dev["status"][keep], cpu["status"][keep]), (dev["status"], cpu["status"])
    assert np.array_equal(dev["winner"][keep], cpu["winner"][keep]), np.flatnonzero(dev["winner"] != cpu["winner"])
    assert np.array_equal(dev["n_inliers"][keep], cpu["n_inliers"][keep]), (dev["n_inliers"], cpu["n_inliers"])
    assert np.array_equal(dev["n_cheiral"][keep], cpu["n_cheiral"][keep]), (dev["n_cheiral"], cpu["n_cheiral"])
    item = np.repeat(keep, np.diff(args[4]))
    assert np.array_equal(dev["flag"][item], cpu["flag"][item]), np.flatnonzero(dev["flag"] != cpu["flag"])
    if values:
        np.testing.assert_allclose(dev["pose"][keep], cpu["pose"][keep], rtol=0, atol=1e-9)
        np.testing.assert_allclose(dev["conditioning"][keep], cpu["conditioning"][keep], rtol=1e-6, atol=0)
        np.testing.assert_allclose(dev["xyz"][item], cpu["xyz"][item], rtol=0, atol=1e-9, equal_nan=True)


def _resection_matches_cpu(args, dev, cpu, on_gate=None):
    skip = _skip_of(S.jobs_on_the_gate(args, cpu) if on_gate is None else on_gate, "jobs")
    keep = np.array([j not in skip for j in range(len(cpu["status"]))], dtype=bool)
    assert np.array_equal(dev["status"][keep], cpu["status"][keep]), (dev["status"], cpu["status"])
    assert np.array_equal(dev["winner"][keep], cpu["winner"][keep]), np.flatnonzero(dev["winner"] != cpu["winner"])
    assert np.array_equal(dev["n_inliers"][keep], cpu["n_inliers"][keep]), (dev["n_inliers"], cpu["n_inliers"])
    np.testing.assert_allclose(dev["pose"][keep], cpu["pose"][keep], rtol=0, atol=1e-9)
    item = np.repeat(keep, np.diff(args[0]))
    np.testing.assert_allclose(dev["err"][item], cpu["err"][item], rtol=1e-6, atol=0, equal_nan=True)


@pytest.mark.parametrize("float32_io", [False, True])
@pytest.mark.parametrize("n_hyp", S.MIXED_N_HYP)
def test_essential_batch_mixed_sizes(n_hyp, float32_io):
    """Pairs of 0 to 5117 correspondences in one call (one to five k_score tiles, small jobs leaving the tile loop next to a large
    one), too-few and failed pairs next to good ones, three cameras of both models, n_hyp on both sides of a wave, SCORE_CHUNK and
    REFINE_BLOCK; then the undistort-only call."""
    sc = S.mixed_essential_scene()
    args = sc["args"]
    dev = DeviceEpipolar().essential_batch(*args, n_hyp, S.MIXED_SEED, float32_io)
    cpu = HarnessEpipolar().essential_batch(*args, n_hyp, S.MIXED_SEED, float32_io)
    _essential_matches_cpu(args, dev, cpu, values=False)
    assert (dev["status"][sc["too_few"]] == 1).all() and (dev["status"][sc["failed"]] == 2).all() and (dev["winner"][sc["too_few"]] == -1).all()
    left_out, items, worst = S.check_essential_outputs(args, dev)  # (also: the pairs without status 0 hold identity, zeros and NaN)
    assert left_out <= 1e-3 * items and worst <= XYZ_DEVICE_REL, (left_out, worst)
    if n_hyp >= CPU.MIXED_TRUTH_MIN_HYP:
        errs = np.array([S.motion_errors(dev["pose"][p], sc["pairs"][p]["R"], sc["pairs"][p]["t"], unit=True) for p in sc["good"]])
        assert errs[:, 0].max() <= 2 * CPU.MIXED_CPU_ROT_DEG and errs[:, 1].max() <= 2 * CPU.MIXED_CPU_DIR_DEG, errs.max(axis=0)
    _bit_identical(dev, DeviceEpipolar().essential_batch(*args, n_hyp, S.MIXED_SEED, float32_io), ESS_KEYS)
    # n_pairs = 0, n_obs > 0: the product's undistort-only call
    empty = np.zeros(0, dtype=np.int64)
    only = DeviceEpipolar().essential_batch(args[0], args[1], args[2], args[3], np.zeros(1, dtype=np.int64), empty, empty, np.zeros(0), n_hyp,
                                            S.MIXED_SEED, float32_io)
    assert np.array_equal(only["undistorted"], dev["undistorted"]) and len(only["status"]) == 0


IDEAL_CAMERA = (np.zeros(1, dtype=np.int32), np.array([[1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]))


@pytest.mark.parametrize("float32_io", [False, True])
@pytest.mark.parametrize("n_hyp", S.MIXED_N_HYP)
def test_essential_batch_mixed_sizes_values_match_cpu_build(n_hyp, float32_io):
    """Pose to 1e-9, conditioning to rtol 1e-6 and xyz to 1e-9 against the CPU build, from pixels.

    With float32_io = 0 this failed while undistort_one called the maths library's tan and was compiled with contraction on the
    device: the undistorted points of a fisheye camera differed from the g++ build's in the last bit (3.3e-16), and the refinement
    amplified that to 2.9e-9 in the pose (n_hyp 63, the pair of 128 between two fisheye views; limit 1e-9) and 1.2e-7 in xyz (n_hyp
    128; limit 1e-9), because epi_refine accepts a step when the cost falls and its last step of 3.2e-9 changes a cost of 1.2e-5 by
    1.6e-19, the rounding of the sum.  (The g++ build alone moved by the same 2.9e-9 when every pixel moved by one ulp.)  With
    tan_portable and no contraction in undistort_one both builds return the same undistorted bits and the same poses."""
    sc = S.mixed_essential_scene()
    args = sc["args"]
    dev = DeviceEpipolar().essential_batch(*args, n_hyp, S.MIXED_SEED, float32_io)
    cpu = HarnessEpipolar().essential_batch(*args, n_hyp, S.MIXED_SEED, float32_io)
    _essential_matches_cpu(args, dev, cpu)


@pytest.mark.parametrize("n_hyp", S.MIXED_N_HYP)
def test_essential_batch_mixed_sizes_from_equal_points(n_hyp):
    """float32_io = 0 with both builds starting from the same undistorted points: the device's own, passed again as the pixels of an
    ideal camera (f = 1, c = 0, no distortion: undistortion returns them unchanged).  Everything downstream of k_epi_undistort at the
    project's limits, pose, conditioning and xyz included."""
    sc = S.mixed_essential_scene()
    args = sc["args"]
    und = DeviceEpipolar().essential_batch(*args, n_hyp, S.MIXED_SEED, False)["undistorted"]
    same = IDEAL_CAMERA + (und, np.zeros(len(und), dtype=np.int32)) + args[4:]
    dev = DeviceEpipolar().essential_batch(*same, n_hyp, S.MIXED_SEED, False)
    cpu = HarnessEpipolar().essential_batch(*same, n_hyp, S.MIXED_SEED, False)
    assert np.array_equal(dev["undistorted"], und) and np.array_equal(cpu["undistorted"], und)
    _essential_matches_cpu(same, dev, cpu)
    assert set(dev["status"].tolist()) == {0, 1, 2}


def test_essential_tail_decides():
    """k_score<true> over two tiles: motion A has the majority inside the first tile, motion B overall.  A count that lost the second
    tile would elect A's hypothesis."""
    sc = S.tail_essential_scene()
    a, is_a = sc["args"], sc["is_a"]
    dev = DeviceEpipolar().essential_batch(*a, sc["n_hyp"], sc["seed"])
    cpu = HarnessEpipolar().essential_batch(*a, sc["n_hyp"], sc["seed"])
    counts_of = lambda items: essential_counts(cpu["undistorted"], a[5], a[6], 0, S.TAIL_N, S.ESS_THR, sc["n_hyp"], sc["seed"], 0, items)  # noqa: E731
    whole, first = counts_of(np.arange(S.TAIL_N)), counts_of(np.arange(S.TILE))
    assert dev["status"][0] == 0 and dev["winner"][0] == whole.argmax() != first.argmax(), (dev["winner"], whole.argmax(), first.argmax())
    _essential_matches_cpu(a, dev, cpu)
    rot, dirn = S.motion_errors(dev["pose"][0], *S.MOTION_B, unit=True)
    assert rot <= 2 * CPU.TAIL_ESS_CPU[0] and dirn <= 2 * CPU.TAIL_ESS_CPU[1], (rot, dirn)
    assert dev["n_inliers"][0] >= 0.9 * (~is_a).sum() and dev["flag"][is_a].sum() < 0.1 * is_a.sum()
    left_out, _, worst = S.check_essential_outputs(a, dev)
    assert left_out == 0 and worst <= XYZ_DEVICE_REL, (left_out, worst)
    _bit_identical(dev, DeviceEpipolar().essential_batch(*a, sc["n_hyp"], sc["seed"]), ESS_KEYS)


def test_resection_tail_decides():
    """The same for k_score<false>."""
    sc = S.tail_resection_scene()
    a, is_a = sc["args"], sc["is_a"]
    dev = DeviceEpipolar().resect_batch(*a, sc["n_hyp"], sc["min_points"], sc["seed"])
    cpu = HarnessEpipolar().resect_batch(*a, sc["n_hyp"], sc["min_points"], sc["seed"])
    counts_of = lambda items: resect_counts(a[1], a[2], 0, S.TAIL_N, S.RES_THR, sc["n_hyp"], sc["seed"], 0, items)  # noqa: E731
    whole, first = counts_of(np.arange(S.TAIL_N)), counts_of(np.arange(S.TILE))
    assert dev["status"][0] == 0 and dev["winner"][0] == whole.argmax() != first.argmax(), (dev["winner"], whole.argmax(), first.argmax())
    _resection_matches_cpu(a, dev, cpu)
    rot, dt = S.motion_errors(dev["pose"][0], *S.RES_MOTION_B)
    assert rot <= 2 * CPU.TAIL_RES_CPU[0] and dt <= 2 * CPU.TAIL_RES_CPU[1], (rot, dt)
    assert dev["n_inliers"][0] >= 0.9 * (~is_a).sum()
    assert S.check_resection_outputs(a, dev, sc["min_points"])[0] == 0
    _bit_identical(dev, DeviceEpipolar().resect_batch(*a, sc["n_hyp"], sc["min_points"], sc["seed"]), RES_KEYS)


def test_resection_many_small_jobs():
    """More jobs than the grid's y extent: k_score's `j += gridDim.y` loop.  The jobs past 65535 have results, not zeros."""
    sc = S.many_resection_jobs()
    a = sc["args"]
    dev = DeviceEpipolar().resect_batch(*a, sc["n_hyp"], sc["min_points"], sc["seed"])
    cpu = HarnessEpipolar().resect_batch(*a, sc["n_hyp"], sc["min_points"], sc["seed"])
    on_gate = np.flatnonzero(np.add.reduceat(S.many_resection_ld(a, cpu)[2].astype(np.int64), a[0][:-1])).tolist()
    _resection_matches_cpu(a, dev, cpu, on_gate)
    ok = dev["status"] == 0
    assert ok[S.GRID_Y_MAX:].mean() > 0.97 and (dev["n_inliers"][ok] >= S.RES_SAMPLE).all()
    err, n_inl, band = S.many_resection_ld(a, dev)
    assert band.sum() == 0 and np.array_equal(n_inl, dev["n_inliers"])
    np.testing.assert_allclose(dev["err"], err, rtol=0, atol=1e-12)
    rot, dt = S.motion_errors_many(dev["pose"][ok], sc["R"][ok], sc["t"][ok])
    assert rot.max() <= 2 * CPU.MANY_RES_CPU[0] and dt.max() <= 2 * CPU.MANY_RES_CPU[1], (rot.max(), dt.max())
    _bit_identical(dev, DeviceEpipolar().resect_batch(*a, sc["n_hyp"], sc["min_points"], sc["seed"]), RES_KEYS)


def test_essential_many_small_pairs():
    sc = S.many_essential_pairs()
    a = sc["args"]
    dev = DeviceEpipolar().essential_batch(*a, sc["n_hyp"], sc["seed"])
    cpu = HarnessEpipolar().essential_batch(*a, sc["n_hyp"], sc["seed"])
    on_gate = np.flatnonzero(np.add.reduceat(S.many_essential_counts_ld(a, cpu)[1].astype(np.int64), a[4][:-1])).tolist()
    _essential_matches_cpu(a, dev, cpu, on_gate)
    ok = dev["status"] == 0
    assert ok.mean() > 0.9999 and ok[S.GRID_Y_MAX:].all()
    n_inl, band = S.many_essential_counts_ld(a, dev)
    assert band.sum() == 0 and np.array_equal(n_inl, dev["n_inliers"]) and np.array_equal(n_inl[ok], np.diff(a[4])[ok])
    rot, dirn = S.motion_errors_many(dev["pose"][ok], sc["R"][ok], sc["t"][ok], unit=True)
    assert rot.max() <= 2 * CPU.MANY_ESS_CPU[0] and dirn.max() <= 2 * CPU.MANY_ESS_CPU[1], (rot.max(), dirn.max())
    sample = np.concatenate([np.arange(200), np.arange(S.GRID_Y_MAX - 100, S.GRID_Y_MAX + 100), np.arange(len(ok) - 200, len(ok))])
    left_out, _, worst = S.check_essential_outputs(a, dev, pairs=sample)
    assert left_out == 0 and worst <= XYZ_DEVICE_REL, worst
    _bit_identical(dev, DeviceEpipolar().essential_batch(*a, sc["n_hyp"], sc["seed"]), ESS_KEYS)


@pytest.mark.parametrize("n_hyp", S.RES_N_HYP)
def test_resection_edges(n_hyp):
    """Jobs of 5 to 3077 points in one call: below RES_SAMPLE, between it and min_points, at min_points, around one tile, several
    tiles, coincident points, random points."""
    sc = S.resection_edge_scene()
    a = sc["args"]
    dev = DeviceEpipolar().resect_batch(*a, n_hyp, sc["min_points"], sc["seed"])
    cpu = HarnessEpipolar().resect_batch(*a, n_hyp, sc["min_points"], sc["seed"])
    _resection_matches_cpu(a, dev, cpu)
    assert (dev["status"][sc["too_few"]] == 1).all() and (dev["status"][sc["failed"]] == 2).all()
    assert S.check_resection_outputs(a, dev, sc["min_points"])[0] == 0
    if n_hyp >= 100:
        assert (dev["status"][sc["good"]] == 0).all()
        errs = np.array([S.motion_errors(dev["pose"][j], *sc["truth"][j]) for j in sc["good"]])
        assert errs[:, 0].max() <= 2 * CPU.RES_CPU[0] and errs[:, 1].max() <= 2 * CPU.RES_CPU[1], errs.max(axis=0)
    _bit_identical(dev, DeviceEpipolar().resect_batch(*a, n_hyp, sc["min_points"], sc["seed"]), RES_KEYS)


@pytest.mark.parametrize("float32_io", [False, True])
@pytest.mark.parametrize("min_points", [4, 6])
@pytest.mark.parametrize("n_views", S.PNP_VIEW_COUNTS)
def test_pnp_batch_edges(n_views, min_points, float32_io):
    """1, 63, 64, 65 and 1000 views over two pinhole cameras and a fisheye camera, an empty view, planar views of 5 points, one view
    of 5000 points among views of 8 to 60 (the host's sort by count), float32_io off and on.  Poses are compared with the CPU
    build on the views of 8 points and up: with fewer, a one-ulp change of the data moves the pose by about 1e-9
    (tests/test_pose_bootstrap_gpu.py), and there the status, the undistorted points and the rmse of the returned pose are checked."""
    sc = CPU.pnp_case(n_views)
    dev = DevicePnP().pnp_batch(*sc["args"], min_points, float32_io)
    cpu = HarnessPnP().pnp_batch(*sc["args"], min_points, float32_io)
    (pose_d, rmse_d, st_d, und_d), (pose_c, rmse_c, st_c, und_c) = dev, cpu
    assert np.array_equal(st_d, st_c)
    assert np.array_equal(und_d, und_c)  # (as in the essential call)
    big = (st_d == 0) & (sc["sizes"] >= 8)
    np.testing.assert_allclose(rmse_d[big], rmse_c[big], rtol=1e-9, atol=0)
    S.check_pnp_outputs(sc, dev, float32_io)
    errs = np.array([S.motion_errors(pose_d[v], *sc["truth"][v]) for v in np.flatnonzero(big)])
    assert errs[:, 0].max() <= 2 * CPU.PNP_CPU[0] and errs[:, 1].max() <= 2 * CPU.PNP_CPU[1], errs.max(axis=0)
    again = DevicePnP().pnp_batch(*sc["args"], min_points, float32_io)
    for x, y in zip(dev, again):
        assert np.array_equal(x, y)


def _pnp_poses_match(sc, dev, cpu):
    (pose_d, _, st_d, _), (pose_c, _, st_c, _) = dev, cpu
    assert np.array_equal(st_d, st_c)
    big = (st_d == 0) & (sc["sizes"] >= 8)
    np.testing.assert_allclose(pose_d[big], pose_c[big], rtol=0, atol=1e-12 * max(1.0, np.abs(pose_c[big]).max()))


@pytest.mark.parametrize("float32_io", [False, True])
@pytest.mark.parametrize("min_points", [4, 6])
@pytest.mark.parametrize("n_views", S.PNP_VIEW_COUNTS)
def test_pnp_batch_edges_poses_match_cpu_build(n_views, min_points, float32_io):
    """PnP pose to 1e-12 x scale against the CPU build, from pixels, on the views of 8 points and up.

    With float32_io = 0 and 1000 views this failed before undistort_one returned the same bits in both builds: view 566 (13 points, the
    fisheye camera) was 8.0e-9 off (limit 1.7e-12), the other 598 views compared held.  Now the largest difference is 6.7e-16."""
    sc = CPU.pnp_case(n_views)
    _pnp_poses_match(sc, DevicePnP().pnp_batch(*sc["args"], min_points, float32_io), HarnessPnP().pnp_batch(*sc["args"], min_points, float32_io))


@pytest.mark.parametrize("min_points", [4, 6])
def test_pnp_batch_from_equal_points(min_points):
    """1000 views, float32_io = 0, both builds starting from the device's own undistorted points (passed as the pixels of an ideal
    camera)."""
    sc = CPU.pnp_case(max(S.PNP_VIEW_COUNTS))
    start, _, _, _, _, obj = sc["args"]
    und = DevicePnP().pnp_batch(*sc["args"], min_points, False)[3]
    same = (start, np.zeros(len(start) - 1, dtype=np.int32)) + IDEAL_CAMERA + (und, obj)
    dev, cpu = DevicePnP().pnp_batch(*same, min_points, False), HarnessPnP().pnp_batch(*same, min_points, False)
    assert np.array_equal(dev[3], und) and np.array_equal(cpu[3], und)
    _pnp_poses_match(sc, dev, cpu)
    np.testing.assert_allclose(dev[1], cpu[1], rtol=1e-9, atol=0)


def test_pair_rmse_edges():
    """Empty pairs (first and last of the call) and pairs of PAIR_BLOCK - 1, PAIR_BLOCK, PAIR_BLOCK + 1 observations."""
    sc = S.pair_rmse_scene()
    rmse, count = DevicePnP().pair_rmse(*sc["args"])
    rmse_c, count_c = HarnessPnP().pair_rmse(*sc["args"])
    assert count.tolist() == list(S.PAIR_SIZES) == count_c.tolist()
    np.testing.assert_allclose(rmse, rmse_c, rtol=1e-9, atol=0)
    for p, m in enumerate(S.PAIR_SIZES):
        assert abs(rmse[p] - S.numpy_pair_rmse(sc["args"][0][p], sc["A"][p], sc["B"][p])) < 1e-10
        assert m > 0 or rmse[p] == 0.0
    again, _ = DevicePnP().pair_rmse(*sc["args"])
    assert np.array_equal(rmse, again)
