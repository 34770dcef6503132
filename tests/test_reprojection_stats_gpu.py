"""cba_reprojection_filter on the device (csrc/report_lib.hip): the errors against the oracle and the existing evaluation, the sums
against bincount, thresholds / keep mask / kept counts against a sort-based brute force and the g++ harness at every edge of the
kernels' paths, the reference's filter fixtures, agreement of CaptureVolume.filter_outliers with the host filters, and the driver."""
import numpy as np
import pandas as pd
import pytest

from caliscope_amd.exceptions import BackendError
from caliscope_amd.reprojection_stats import DeviceReprojectionStats
from tests import report_native as N
from tests.helpers import aligned_difference, small_problem

pytestmark = pytest.mark.gpu

EXACT = ("cam_count", "group_count", "n_nonfinite", "cam_threshold", "keep", "cam_kept", "n_floor_cams")


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def _check_sums(got, cam, n_cams, group=None, n_groups=0):
    """Counts exact; every sum of squares against bincount over the device's own err within 2 n 2^-53 relative, n the count of that
    destination (both sides add n non-negative terms in some order)."""
    sq = got.err * got.err
    cnt = np.bincount(cam, minlength=n_cams)
    assert np.array_equal(got.cam_count, cnt)
    want = np.bincount(cam, weights=sq, minlength=n_cams)
    assert np.all(np.abs(got.cam_sumsq - want) <= 2 * cnt * 2.0**-53 * want), np.max(np.abs(got.cam_sumsq - want) / np.maximum(want, 1e-300))
    assert abs(got.overall_sumsq - sq.sum()) <= 2 * len(sq) * 2.0**-53 * sq.sum()
    if group is not None:
        gcnt = np.bincount(group, minlength=n_groups)
        assert np.array_equal(got.group_count, gcnt)
        gwant = np.bincount(group, weights=sq, minlength=n_groups)
        assert np.all(np.abs(got.group_sumsq - gwant) <= 2 * gcnt * 2.0**-53 * gwant)


def _check_filter(err, cam, n_cams, mode, value, scope="per_camera", floor=10, group=None, n_groups=0):
    """The device on given errors against the brute force and against the harness: thresholds, keep and counts bit for bit."""
    got = N.filter_with_given_errors(DeviceReprojectionStats(), err, cam, n_cams, mode, value, scope, floor, obs_group=group, n_groups=n_groups)
    assert np.array_equal(_bits(got.err), _bits(np.asarray(err) + 0.0)) and got.err_xy is None and got.n_nonfinite == 0
    thr, keep, kept, n_floor = N.brute_force_filter(got.err, cam, n_cams, mode, value, scope, floor)
    assert np.array_equal(_bits(got.cam_threshold), _bits(thr)), (got.cam_threshold, thr)
    assert np.array_equal(got.keep, keep) and np.array_equal(got.cam_kept, kept) and got.n_floor_cams == n_floor
    host = N.filter_with_given_errors(N.HarnessReprojectionStats(), err, cam, n_cams, mode, value, scope, floor, obs_group=group, n_groups=n_groups)
    for name in EXACT:
        a, b = getattr(got, name), getattr(host, name)
        assert np.array_equal(_bits(a), _bits(b)) if name == "cam_threshold" else np.array_equal(a, b), name
    _check_sums(got, cam, n_cams, group, n_groups)
    return got


# ---- errors -----------------------------------------------------------------------------------------------------------------------------

def _projection_case(kind):
    from caliscope_amd.bundle_parameterization import BundleParameterization
    from caliscope_amd.capture_volume import CaptureVolume

    if kind == "pinhole":
        sc, par, x = small_problem(n_cams=6, n_points=300, k=4)  # 1200 observations: two workgroups
        cameras, points, cam, uv, obj = sc.cameras_init, sc.points_init, sc.camera_indices, sc.image_coords, sc.obj_indices
    else:
        from tests.test_oracle_pins import _mixed_arrays

        cameras, points, uv, cam, obj = _mixed_arrays()
        cam, obj = cam.astype(np.int32), obj.astype(np.int32)
        par = BundleParameterization.from_camera_array(cameras, n_points=len(points), refine_intrinsics=False)
        x = par.pack(cameras, points)
    vol = CaptureVolume.from_arrays(cameras, cam, uv, obj, points)
    return vol, par, x, points, cam, uv, obj


@pytest.mark.parametrize("kind", ["pinhole", "mixed_fisheye_pinhole"])
def test_errors_equal_the_oracle_and_the_existing_evaluation(kind):
    from oracle.residuals import joint_residuals

    vol, par, x, points, cam, uv, obj = _projection_case(kind)
    tabs = par.device_tables()
    group = (obj % 5).astype(np.int32)
    got = DeviceReprojectionStats().reprojection_filter(tabs["cam_model"], tabs["cam_const"], x[: par.n_camera_params].reshape(-1, 6), points, cam, obj, uv,
                                                        obs_group=group, n_groups=5)
    fx = np.array([b.fx_initial for b in par.blocks])[cam]
    want = joint_residuals(x, par, cam, uv, obj).reshape(-1, 2) * fx[:, None]
    assert _rel(got.err_xy, want) < 1e-12
    assert _rel(got.err_xy, vol._pixel_errors(cam, uv, obj)) < 1e-12
    assert _rel(got.err, np.sqrt(np.einsum("ij,ij->i", got.err_xy, got.err_xy))) < 1e-15 and got.keep is None and got.n_nonfinite == 0
    _check_sums(got, cam, len(par.blocks), group, 5)
    host = N.HarnessReprojectionStats().reprojection_filter(tabs["cam_model"], tabs["cam_const"], x[: par.n_camera_params].reshape(-1, 6), points, cam, obj,
                                                            uv, obs_group=group, n_groups=5)
    assert _rel(got.err_xy, host.err_xy) < 1e-12
    summary = vol.reprojection_summary()
    report = vol.compute_reprojection_report()
    assert summary.overall_rmse == pytest.approx(report.overall_rmse, rel=1e-12) and summary.raw_errors is None
    assert summary.by_camera.keys() == report.by_camera.keys() and summary.by_point.keys() == report.by_point.keys()
    assert all(summary.by_camera[c] == pytest.approx(v, rel=1e-12) for c, v in report.by_camera.items())
    assert all(summary.by_point[c] == pytest.approx(v, rel=1e-12) for c, v in report.by_point.items())


def test_camera_table_beyond_the_lds_and_exact_projections():
    """More cameras than the error kernel keeps in LDS (the table read through the vector cache), and observations that are the exact
    projections of their points: err == 0.0 everywhere... up to the rounding of the projection; given zeros are exactly zero."""
    from oracle.residuals import joint_residuals

    k = N.constants()
    sc, par, x = small_problem(n_cams=k["lds_cams"] + 1, n_points=200, k=6)
    tabs = par.device_tables()
    cam, uv, obj = sc.camera_indices, sc.image_coords, sc.obj_indices
    got = DeviceReprojectionStats().reprojection_filter(tabs["cam_model"], tabs["cam_const"], x[: par.n_camera_params].reshape(-1, 6), sc.points_init, cam, obj, uv)
    fx = np.array([b.fx_initial for b in par.blocks])[cam]
    assert _rel(got.err_xy, joint_residuals(x, par, cam, uv, obj).reshape(-1, 2) * fx[:, None]) < 1e-12
    _check_sums(got, cam, len(par.blocks))
    zero = _check_filter(np.zeros(700), (np.arange(700) % 3).astype(np.int32), 3, "percentile", 2.5)
    assert zero.keep.all() and np.all(zero.cam_threshold == 0.0) and zero.n_floor_cams == 0


# ---- edges of the select, the mask and the floor ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_obs", ["one", "tile-1", "tile", "tile+1", 4097])
def test_observation_counts_at_the_tile_edges(n_obs):
    tile = N.constants()["tile"]
    n = {"one": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}.get(n_obs, n_obs)
    err, cam = N.random_errors(n, 3 if n > 3 else 1, seed=n)
    n_cams = 3 if n > 3 else 1
    _check_filter(err, cam, n_cams, "percentile", 2.5)
    _check_filter(err, cam, n_cams, "percentile", 2.5, scope="overall")
    _check_filter(err, cam, n_cams, "absolute", 1.5)


def _camera_counts():
    q = N.constants()["lds_queries"]
    # two queries per camera in the percentile round, one per camera in the floor round: both capacities
    return sorted({1, 2, q // 2 - 1, q // 2, q // 2 + 1, q - 1, q, q + 1, 200, 1000})


@pytest.mark.parametrize("n_cams", _camera_counts())
def test_camera_counts_at_the_lds_query_capacity(n_cams):
    err, cam = N.random_errors(20 * n_cams if n_cams >= 200 else 3000, n_cams, seed=n_cams)
    _check_filter(err, cam, n_cams, "percentile", 2.5)
    got = _check_filter(err, cam, n_cams, "percentile", 30.0, floor=10**6)  # every camera that drops a row is below this floor: one floor query each
    assert got.n_floor_cams >= min(n_cams, 100) // 2 and got.keep.all()


def test_more_cameras_and_groups_than_the_lds_partials_hold():
    k = N.constants()
    n_cams = n_groups = k["lds_sums"] + 1
    err, cam = N.random_errors(6000, n_cams, seed=5)
    group = ((np.arange(6000) * 7) % n_groups).astype(np.int32)
    _check_filter(err, cam, n_cams, "percentile", 10.0, floor=2, group=group, n_groups=n_groups)
    _check_filter(err, cam % 4, 4, "absolute", 1.0, group=np.zeros(6000, dtype=np.int32), n_groups=1)  # one group: every row on one sum


def test_sparse_and_tied_cameras():
    """Cameras with 0, 1 and 2 rows, a camera whose errors are all equal, percentile 100 and 1e-3."""
    rng = np.random.default_rng(3)
    cam = np.concatenate([np.full(1, 1), np.full(2, 2), np.full(500, 3), np.full(900, 4)]).astype(np.int32)  # camera 0 and 5: no rows
    err = rng.gamma(2.0, 0.3, len(cam))
    err[cam == 3] = 0.7321
    order = rng.permutation(len(cam))
    err, cam = err[order], cam[order]
    for value in (2.5, 100.0, 1e-3, 50.0):
        for scope in ("per_camera", "overall"):
            got = _check_filter(err, cam, 6, "percentile", value, scope=scope, floor=10)
            if scope == "per_camera":
                assert np.isinf(got.cam_threshold[[0, 5]]).all() and got.cam_kept[3] == 500
    _check_filter(err, cam, 6, "absolute", 0.5, floor=3)


def test_floors():
    """A floor above a camera's row count, three cameras below the floor in one call, a tie at the top-up value."""
    rng = np.random.default_rng(9)
    cam = np.concatenate([np.full(5, 0), np.full(40, 1), np.full(60, 2), np.full(2000, 3)]).astype(np.int32)
    err = rng.gamma(2.0, 0.3, len(cam)) + 2.0
    err[cam == 3] -= 1.9
    one = np.flatnonzero(cam == 1)
    err[one[:30]] = 2.25  # camera 1: its 10th smallest error is one of thirty equal ones
    err[one[30:]] = 9.0
    order = rng.permutation(len(cam))
    err, cam = err[order], cam[order]
    got = _check_filter(err, cam, 4, "absolute", 1.0, floor=10)  # cameras 0, 1, 2 keep nothing at 1.0 px
    assert got.n_floor_cams == 3 and got.cam_kept.tolist()[:3] == [5, 30, 10] and got.cam_threshold[1] == 2.25
    got = _check_filter(err, cam, 4, "percentile", 99.9, scope="overall", floor=10)  # the overall threshold leaves camera 3 two or three rows
    assert got.n_floor_cams == 4
    _check_filter(err, cam, 4, "percentile", 60.0, floor=50)


# ---- the reference's fixtures and the host path -----------------------------------------------------------------------------------------------

def test_filter_fixtures_through_the_device():
    runs = weaker = 0
    for path in N.FILTER_FIXTURES:
        r, w = N.run_filter_fixture(path, lambda err: DeviceReprojectionStats(err_in=err))
        runs, weaker = runs + r, weaker + w
    assert runs == 54 and weaker <= 18, (runs, weaker)


def test_filter_outliers_equals_the_host_filters():
    """8 cameras / 5 000 points / 40 000 observations, 5 % outliers: the host filters on the device's own errors (a report in the
    cached slot, as the fixture test does) and filter_outliers return identical tables and maps."""
    from caliscope_amd.capture_volume import CaptureVolume, ReprojectionReport
    from caliscope_amd.synthetic import make_scene

    sc = make_scene(n_cams=8, n_points=5000, n_obs=40000, outliers=0.05)
    vol = CaptureVolume.from_arrays(sc.cameras_init, sc.camera_indices, sc.image_coords, sc.obj_indices, sc.points_init)
    summary = vol.reprojection_summary(raw=True)
    raw = summary.raw_errors
    assert len(raw) == 40000 and list(raw.columns) == ["sync_index", "cam_id", "object_id", "keypoint_id", "error_x", "error_y", "euclidean_error"]
    vol.__dict__["reprojection_report"] = ReprojectionReport(
        overall_rmse=summary.overall_rmse, by_camera=summary.by_camera, by_point=summary.by_point, n_unmatched_observations=0, unmatched_rate=0.0,
        unmatched_by_camera=summary.unmatched_by_camera, raw_errors=raw, n_observations_matched=40000, n_observations_total=40000, n_cameras=8, n_points=5000)
    solver = DeviceReprojectionStats(err_in=raw["euclidean_error"].to_numpy())
    pairs = [(vol.filter_by_percentile_error(2.5), vol.filter_outliers(2.5, _solver=solver)),
             (vol.filter_by_percentile_error(5.0, scope="overall", min_per_camera=4900), vol.filter_outliers(5.0, scope="overall", min_per_camera=4900, _solver=solver)),
             (vol.filter_by_absolute_error(2.0), vol.filter_outliers(max_pixels=2.0, _solver=solver)),
             (vol.filter_by_percentile_error(2.5), vol.filter_outliers(2.5))]  # the last one projects on the device again: same errors, same rows
    for host, dev in pairs:
        assert len(dev.image_points) < 40000 and dev.optimization_status is None
        pd.testing.assert_frame_equal(host.image_points.df, dev.image_points.df)
        pd.testing.assert_frame_equal(host.world_points.df, dev.world_points.df)
        assert np.array_equal(host.img_to_obj_map, dev.img_to_obj_map)


def test_driver_with_the_device_filter():
    """calibrate_extrinsics(device_filter=True) on the board session of tests/test_stage_driver.py: the same observations survive
    as with the host filter, and the poses agree as two runs of one bounded solve do (tests/test_gpu_parity.py: aligned positions
    and angles within 1e-4; the atomics of the solves before the filter differ from run to run)."""
    from caliscope_amd.bundle_parameterization import BundleParameterization
    from caliscope_amd.calibrate_extrinsics import calibrate_extrinsics
    from tests.test_stage_driver import _board_session

    image_points, cameras, constraints, _ = _board_session()
    host = calibrate_extrinsics(image_points, cameras, constraints).capture_volume
    dev = calibrate_extrinsics(image_points, cameras, constraints, device_filter=True).capture_volume
    assert dev.optimization_status.converged and len(dev.image_points) < len(image_points)
    pd.testing.assert_frame_equal(host.image_points.df, dev.image_points.df)
    keys = ["sync_index", "object_id", "keypoint_id"]
    assert np.array_equal(host.world_points.df[keys].to_numpy(), dev.world_points.df[keys].to_numpy())
    par = BundleParameterization.from_camera_array(host.camera_array, n_points=len(host.world_points), refine_intrinsics=False)
    pos, ang, _ = aligned_difference(par, par.pack(dev.camera_array, dev.world_points.points), par.pack(host.camera_array, host.world_points.points))
    assert pos < 1e-4 and ang < 1e-4, (pos, ang)


# ---- refusal and repeatability ---------------------------------------------------------------------------------------------------------------

def test_a_bad_index_is_refused_and_the_next_call_succeeds():
    err, cam = N.random_errors(3000, 5, seed=2)
    bad = cam.copy()
    bad[2999] = 5
    messages = []
    for solver in (DeviceReprojectionStats(), N.HarnessReprojectionStats()):
        with pytest.raises(BackendError) as exc:
            N.filter_with_given_errors(solver, err, bad, 5, "percentile", 2.5)
        messages.append(str(exc.value))
    assert messages[0] == messages[1] and "observation 2999: camera 5 out of range [0, 5)" in messages[0]
    e = err.copy()
    e[7] = np.nan
    with pytest.raises(BackendError, match="observation 7: error nan"):
        N.filter_with_given_errors(DeviceReprojectionStats(), e, cam, 5, "percentile", 2.5)
    group = (np.arange(3000) % 11).astype(np.int32)
    a = _check_filter(err, cam, 5, "percentile", 2.5, group=group, n_groups=11)
    b = N.filter_with_given_errors(DeviceReprojectionStats(), err, cam, 5, "percentile", 2.5, obs_group=group, n_groups=11)
    for name in EXACT:  # two identical calls: the same bytes
        assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes(), name
    empty = N.filter_with_given_errors(DeviceReprojectionStats(), np.zeros(0), np.zeros(0, dtype=np.int32), 3, "percentile", 2.5)
    assert np.all(np.isinf(empty.cam_threshold)) and empty.cam_kept.tolist() == [0, 0, 0] and empty.n_floor_cams == 0


def test_non_finite_projection_falls_back_to_the_host_filter(caplog):
    """A world point at infinity: the call counts its observations and does not filter; filter_outliers logs it and returns
    what the host filter returns (or raises what it raises)."""
    from caliscope_amd.capture_volume import CaptureVolume

    sc, par, x = small_problem(n_cams=4, n_points=100, k=3)
    points = sc.points_init.copy()
    points[int(sc.obj_indices[0])] = np.inf  # (the tables refuse NaN coordinates)
    tabs = par.device_tables()
    got = DeviceReprojectionStats().reprojection_filter(tabs["cam_model"], tabs["cam_const"], x[: par.n_camera_params].reshape(-1, 6), points, sc.camera_indices,
                                                        sc.obj_indices, sc.image_coords, mode="percentile", value=2.5)
    assert got.n_nonfinite == 3 and got.keep is None and got.cam_threshold is None
    vol = CaptureVolume.from_arrays(sc.cameras_init, sc.camera_indices, sc.image_coords, sc.obj_indices, points)
    outcome = []
    for call in (lambda: vol.filter_by_percentile_error(2.5), lambda: vol.filter_outliers(2.5)):
        try:
            outcome.append(call().image_points.df)
        except Exception as exc:  # noqa: BLE001  (whatever the host filter does with such errors is what the new path must do)
            outcome.append((type(exc), str(exc)))
    if isinstance(outcome[0], tuple):
        assert outcome[0] == outcome[1]
    else:
        pd.testing.assert_frame_equal(outcome[0], outcome[1])
    assert "not finite" in caplog.text


def test_a_filter_call_that_does_not_ask_for_the_mask(monkeypatch):
    """keep of cba_report_out is optional (the wrapper always asks for it in a filter call): without it the thresholds, the kept counts
    and the floor count come back as in a full call, which stand against the harness bit for bit as in _check_filter.  Two cameras,
    forty rows, one of them under the floor."""
    from caliscope_amd.reprojection_stats import REPORT_SIGNATURES
    from tests.helpers import null_outputs

    rng = np.random.default_rng(12)
    err, cam = rng.gamma(2.0, 0.5, 40), np.r_[np.zeros(28, np.int32), np.ones(12, np.int32)]
    full = _check_filter(err, cam, 2, "percentile", 60.0, floor=10)
    assert full.n_floor_cams == 1 and full.keep.any()
    null_outputs(monkeypatch, REPORT_SIGNATURES, "cba_reprojection_filter", fields=("keep",))
    got = N.filter_with_given_errors(DeviceReprojectionStats(), err, cam, 2, "percentile", 60.0, "per_camera", 10)
    assert not got.keep.any()  # nothing was copied back
    assert np.array_equal(_bits(got.cam_threshold), _bits(full.cam_threshold)) and np.array_equal(got.cam_kept, full.cam_kept)
    assert got.n_floor_cams == full.n_floor_cams and np.array_equal(_bits(got.err), _bits(full.err))
