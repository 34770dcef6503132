"""Reprojection statistics and outlier filter (caliscope_amd/reprojection_stats.py, csrc/report_math.h) on the CPU: the percentile
interpolation against numpy, the radix select against a sort, CaptureVolume.filter_outliers and reprojection_summary on the
reference's own fixtures through the g++ build of the select, mask and floor logic, and the argument checks."""
import warnings

import numpy as np
import pytest

from caliscope_amd.exceptions import BackendError
from tests import report_native as N


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_constants_are_consistent():
    k = N.constants()
    assert k["radix"] == 1 << k["digit_bits"] and k["passes"] * k["digit_bits"] == 64
    assert k["tile"] % k["block"] == 0 and k["lds_queries"] >= 2


def test_percentile_equals_numpy_bit_for_bit():
    """numpy.percentile(x, 100 - p), default method, restated as two order statistics and one interpolation whose product is rounded
    before it is added: 12 000 random cases and the edges (n = 1, n = 2, p = 100 (q = 0), q -> 100, all-equal arrays, a == b across
    the rank)."""
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(12_000):
        n = int(rng.integers(1, 60))
        scale = 10.0 ** rng.integers(-8, 8)
        x = rng.gamma(2.0, 0.3, n) * scale
        if rng.random() < 0.2:
            x[rng.integers(0, n, n)] = x[rng.integers(0, n, n)]  # ties
        cases.append((x, float(rng.uniform(1e-6, 100.0))))
    for n in (1, 2, 3, 5, 101):
        x = rng.gamma(2.0, 0.3, n)
        cases += [(x, 100.0), (x, 1e-12), (x, 50.0), (x, 2.5), (np.full(n, x[0]), 2.5), (np.full(n, 0.0), 37.0)]
    tied = np.array([0.1, 0.7, 0.7, 0.7, 0.7, 3.0])
    cases += [(tied, p) for p in (10.0, 30.0, 50.0, 60.0, 80.0)]
    assert len(cases) >= 10_000
    for x, p in cases:
        want = np.percentile(x, 100 - p)
        got = N.percentile(x, p)
        assert _bits(got) == _bits(want), (len(x), p, got, want)
        lo, hi, g = N.rank_plan(len(x), p)
        s = np.sort(x)
        assert _bits(N.harness().rh_interpolate(s[lo], s[hi], g)) == _bits(want)


def test_select_equals_the_sort_bit_for_bit():
    """np.sort(x)[rank] for ranks 0, 1, n-2, n-1 and a middle one: arrays with 0.0 and subnormals, values that differ in the lowest
    digit only, long runs of ties that straddle the rank, and more rows than one tile."""
    rng = np.random.default_rng(11)
    tile = N.constants()["tile"]
    tiny = np.array([0.0, 5e-324, 1e-320, 2.2250738585072014e-308, 0.0, 5e-324, 1.0, 3e-310])
    base = np.float64(1.2345).view(np.uint64)
    low_digit = (base + rng.permutation(300).astype(np.uint64)).view(np.float64)  # neighbours in the last byte and one carry beyond
    ties = np.concatenate([np.full(500, 0.25), np.full(700, 0.5), rng.random(40), np.full(300, 0.75)])
    big = np.concatenate([rng.gamma(2.0, 0.3, 2 * tile + 1), tiny, [0.0] * 10])
    for x in (tiny, np.concatenate([tiny, rng.random(5) * 1e-300]), low_digit, rng.permutation(ties), big, np.array([3.0]), np.array([2.0, 1.0])):
        s = np.sort(x)
        n = len(x)
        for rank in sorted({0, min(1, n - 1), max(n - 2, 0), n - 1, n // 2, min(499, n - 1), min(500, n - 1), min(1199, n - 1), min(1200, n - 1)}):
            assert _bits(N.select(x, rank)) == _bits(s[rank]), (n, rank)
    assert _bits(N.select(np.array([-0.0, 1.0]), 0)) == _bits(0.0)  # the sign bit of a zero is not part of the key


@pytest.mark.parametrize("mode,value,scope", [("percentile", 2.5, "per_camera"), ("percentile", 2.5, "overall"), ("percentile", 100.0, "per_camera"),
                                              ("percentile", 1e-3, "per_camera"), ("absolute", 1.0, "per_camera")])
def test_harness_filter_equals_the_brute_force(mode, value, scope):
    k = N.constants()
    for n_obs, n_cams, floor in ((1, 1, 10), (k["tile"] + 1, 2, 10), (4097, k["lds_queries"] // 2 + 1, 10), (4000, 200, 25), (300, k["lds_queries"] + 1, 12)):
        err, cam = N.random_errors(n_obs, n_cams, seed=n_obs + n_cams)
        got = N.filter_with_given_errors(N.HarnessReprojectionStats(), err, cam, n_cams, mode, value, scope, floor)
        thr, keep, kept, n_floor = N.brute_force_filter(err, cam, n_cams, mode, value, scope, floor)
        assert np.array_equal(_bits(got.cam_threshold), _bits(thr)) and np.array_equal(got.keep, keep)
        assert np.array_equal(got.cam_kept, kept) and got.n_floor_cams == n_floor
        assert np.array_equal(got.cam_count, np.bincount(cam, minlength=n_cams)) and got.n_nonfinite == 0


def test_filter_fixtures_through_filter_outliers():
    """All 54 runs of the six filter fixtures, the stored errors as err_in: equal to the reference row for row except in the runs
    where the fixture says two cameras were below the floor (18 of them; tests/test_reference_host_fixtures.py says why)."""
    assert len(N.FILTER_FIXTURES) == 6
    runs = weaker = 0
    for path in N.FILTER_FIXTURES:
        r, w = N.run_filter_fixture(path, lambda err: N.HarnessReprojectionStats(err_in=err))
        runs, weaker = runs + r, weaker + w
    assert runs == 54 and weaker <= 18, (runs, weaker)


@pytest.mark.parametrize("path", N.REPORT_FIXTURES, ids=lambda p: p.stem)
def test_report_fixtures_through_reprojection_summary(path):
    """The bookkeeping of tests/test_reference_host_fixtures.py::test_report_bookkeeping_equals_the_reference_s_own_output for the
    fields the summary has, with the stored pixel errors in the place of the projection."""
    from caliscope_amd.cameras import CameraArray, CameraData
    from caliscope_amd.capture_volume import CaptureVolume
    from caliscope_amd.constraints import ConstraintSet
    from caliscope_amd.point_data import ImagePoints, WorldPoints

    ref = np.load(path)
    wdf, idf = N.fixture_tables(ref)
    K = np.array([[400.0, 0.0, 200.0], [0.0, 400.0, 200.0], [0.0, 0.0, 1.0]])

    def cam(c, posed=True, ignore=False):
        return CameraData(cam_id=c, size=(400, 400), matrix=K.copy(), distortions=np.zeros(5), ignore=ignore,
                          rotation=np.eye(3) if posed else None, translation=np.array([0.1 * c, 0.0, 0.0]) if posed else None)

    cams = CameraArray({0: cam(0), 1: cam(1), 5: cam(5, posed=False), 9: cam(9, ignore=True), 12: cam(12)})
    static = frozenset(int(o) for o in ref["static_ids"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vol = CaptureVolume(cams, ImagePoints(idf), WorldPoints(wdf), ConstraintSet((), static) if static else None)
    solver = N.HarnessReprojectionStats(pixel_errors=ref["errors"])
    rep = vol.reprojection_summary(_solver=solver)
    assert rep.raw_errors is None and solver.calls == 1
    assert rep.overall_rmse == pytest.approx(float(ref["overall_rmse"]), rel=1e-14)
    mine = np.array(sorted(rep.by_camera.items()), dtype=np.float64).reshape(-1, 2)
    assert np.array_equal(mine[:, 0], ref["by_camera"][:, 0]) and np.allclose(mine[:, 1], ref["by_camera"][:, 1], rtol=1e-14, atol=0)
    mine = np.array(sorted((o, k, v) for (o, k), v in rep.by_point.items()), dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(mine[:, :2], ref["by_point"][:, :2]) and np.allclose(mine[:, 2], ref["by_point"][:, 2], rtol=1e-14, atol=0)
    assert rep.n_unmatched_observations == int(ref["n_unmatched"]) and rep.unmatched_rate == pytest.approx(float(ref["unmatched_rate"]), rel=1e-15)
    assert np.array_equal(np.array(sorted(rep.unmatched_by_camera.items()), dtype=np.int64).reshape(-1, 2), ref["unmatched_by_camera"])
    assert [rep.n_observations_matched, rep.n_observations_total, rep.n_cameras, rep.n_points] == ref["counts"].tolist()
    full = vol.reprojection_summary(raw=True, _solver=solver)
    assert list(full.raw_errors.columns) == [str(c) for c in ref["raw_columns"]]
    got = full.raw_errors.to_numpy(dtype=np.float64)
    assert np.array_equal(got[:, :6], ref["raw_errors"][:, :6]) and np.allclose(got[:, 6], ref["raw_errors"][:, 6], rtol=1e-15, atol=0)


def _small_volume():
    from caliscope_amd.capture_volume import CaptureVolume
    from caliscope_amd.synthetic import make_scene

    sc = make_scene(n_cams=4, n_points=100, n_obs=300)
    return CaptureVolume.from_arrays(sc.cameras_init, sc.camera_indices, sc.image_coords, sc.obj_indices, sc.points_init)


def test_filter_outliers_refuses_what_the_host_filters_refuse():
    vol = _small_volume()
    solver = N.HarnessReprojectionStats()
    for bad in (0, -1.0, 100.5):
        with pytest.raises(ValueError, match=f"percentile must be between 0 and 100, got {bad}"):
            vol.filter_outliers(bad, _solver=solver)
    with pytest.raises(ValueError, match="scope must be 'per_camera' or 'overall', got each"):
        vol.filter_outliers(2.5, scope="each", _solver=solver)
    with pytest.raises(ValueError, match="min_per_camera must be >= 1, got 0"):
        vol.filter_outliers(2.5, min_per_camera=0, _solver=solver)
    with pytest.raises(ValueError, match="min_per_camera must be >= 1, got 0"):
        vol.filter_outliers(max_pixels=1.0, min_per_camera=0, _solver=solver)
    with pytest.raises(ValueError, match="max_pixels must be positive, got -2.0"):
        vol.filter_outliers(max_pixels=-2.0, _solver=solver)
    with pytest.raises(ValueError, match="exactly one of percentile and max_pixels"):
        vol.filter_outliers(_solver=solver)
    with pytest.raises(ValueError, match="exactly one of percentile and max_pixels"):
        vol.filter_outliers(2.5, max_pixels=1.0, _solver=solver)
    assert solver.calls == 0
    # the same texts as the two host filters
    for call, new in ((lambda: vol.filter_by_percentile_error(0), lambda: vol.filter_outliers(0, _solver=solver)),
                      (lambda: vol.filter_by_percentile_error(2.5, scope="each"), lambda: vol.filter_outliers(2.5, scope="each", _solver=solver)),
                      (lambda: vol.filter_by_absolute_error(-2.0), lambda: vol.filter_outliers(max_pixels=-2.0, _solver=solver))):
        with pytest.raises(ValueError) as old:
            call()
        with pytest.raises(ValueError) as now:
            new()
        assert str(old.value) == str(now.value)


def test_the_library_s_checks_name_the_observation():
    err, cam = N.random_errors(50, 3, seed=1)
    solver = N.HarnessReprojectionStats()
    bad = cam.copy()
    bad[17] = 3
    with pytest.raises(BackendError, match=r"observation 17: camera 3 out of range \[0, 3\)"):
        N.filter_with_given_errors(solver, err, bad, 3, "percentile", 2.5)
    for value, shown in ((-1.0, "-1.0"), (np.nan, "nan"), (np.inf, "inf")):
        e = err.copy()
        e[31] = value
        with pytest.raises(BackendError, match=f"observation 31: error {shown}.* is not a finite non-negative number"):
            N.filter_with_given_errors(solver, e, cam, 3, "percentile", 2.5)
    group = np.zeros(50, dtype=np.int32)
    group[9] = 4
    with pytest.raises(BackendError, match=r"observation 9: group 4 out of range \[0, 4\)"):
        N.filter_with_given_errors(solver, err, cam, 3, "stats", 0.0, obs_group=group, n_groups=4)
    model, const, pose, points = N.placeholder_cameras(3)
    pt = np.zeros(50, dtype=np.int32)
    pt[5] = 1
    with pytest.raises(BackendError, match=r"observation 5: point 1 out of range \[0, 1\)"):
        solver.reprojection_filter(model, const, pose, points, cam, pt, np.zeros((50, 2)))
    with pytest.raises(ValueError, match="differ in length"):
        solver.reprojection_filter(model, const, pose, points, cam, pt[:-1], np.zeros((50, 2)))
    got = N.filter_with_given_errors(solver, err, cam, 3, "percentile", 2.5)  # the next call succeeds
    assert got.keep.sum() == got.cam_kept.sum()
    empty = N.filter_with_given_errors(solver, np.zeros(0), np.zeros(0, dtype=np.int32), 3, "percentile", 2.5)
    assert np.all(np.isinf(empty.cam_threshold)) and empty.cam_kept.tolist() == [0, 0, 0] and empty.n_floor_cams == 0


def test_the_symbol_is_in_its_own_header_and_bound_by_its_own_module():
    from pathlib import Path

    from caliscope_amd import _lib
    from caliscope_amd import reprojection_stats as RS

    root = Path(__file__).resolve().parent.parent
    assert "cba_reprojection_filter" in (root / "include" / "caliscope_report.h").read_text()
    assert "cba_reprojection_filter" not in (root / "include" / "caliscope_ba.h").read_text()
    assert list(RS.REPORT_SIGNATURES) == ["cba_reprojection_filter"] and "cba_reprojection_filter" not in _lib.SIGNATURES


def test_harness_projection_equals_the_oracle():
    """The projection path of the harness (ba_math.h compiled by g++): err_xy = oracle residuals times fx, sums against bincount."""
    from caliscope_amd.bundle_parameterization import BundleParameterization
    from caliscope_amd.synthetic import make_scene
    from oracle.residuals import joint_residuals

    sc = make_scene(n_cams=4, n_points=100, n_obs=300)
    par = BundleParameterization.from_camera_array(sc.cameras_init, n_points=100, refine_intrinsics=False)
    x = par.pack(sc.cameras_init, sc.points_init)
    tabs = par.device_tables()
    group = (sc.obj_indices % 7).astype(np.int32)
    got = N.HarnessReprojectionStats().reprojection_filter(tabs["cam_model"], tabs["cam_const"], x[: par.n_camera_params].reshape(-1, 6), sc.points_init,
                                                           sc.camera_indices, sc.obj_indices, sc.image_coords, obs_group=group, n_groups=7)
    fx = np.array([b.fx_initial for b in par.blocks])[sc.camera_indices]
    want = joint_residuals(x, par, sc.camera_indices, sc.image_coords, sc.obj_indices).reshape(-1, 2) * fx[:, None]
    assert np.max(np.abs(got.err_xy - want)) <= 1e-12 * np.max(np.abs(want))
    sq = got.err**2
    assert np.allclose(got.cam_sumsq, np.bincount(sc.camera_indices, weights=sq, minlength=4), rtol=2 * 300 * 2.0**-53, atol=0)
    assert np.allclose(got.group_sumsq, np.bincount(group, weights=sq, minlength=7), rtol=2 * 300 * 2.0**-53, atol=0)
    assert np.array_equal(got.group_count, np.bincount(group, minlength=7)) and got.keep is None
