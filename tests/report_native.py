"""g++ build of caliscope_amd/csrc/report_math.h (tests/native/report_harness.cpp), a `_solver` hook for
CaptureVolume.reprojection_summary / filter_outliers that runs on it, and the brute force and the tables the reprojection-statistics
tests share."""
from __future__ import annotations

import ctypes as C
import functools
from pathlib import Path

import numpy as np

from caliscope_amd.reprojection_stats import ReportDesc, ReportOut, check_reprojection_arguments, run_reprojection_call
from tests.native_build import CSRC, NATIVE, load_native

I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)
F64 = C.POINTER(C.c_double)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "report_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.rh_last_error.restype = C.c_char_p
    lib.rh_constants.restype = None
    lib.rh_constants.argtypes = [I32]
    lib.rh_interpolate.restype = C.c_double
    lib.rh_interpolate.argtypes = [C.c_double, C.c_double, C.c_double]
    lib.rh_rank_plan.restype = None
    lib.rh_rank_plan.argtypes = [C.c_int64, C.c_double, I64, F64]
    lib.rh_select.restype = C.c_double
    lib.rh_select.argtypes = [F64, C.c_int64, C.c_int64]
    lib.rh_percentile.restype = C.c_double
    lib.rh_percentile.argtypes = [F64, C.c_int64, C.c_double]
    lib.rh_reprojection_filter.restype = C.c_int
    lib.rh_reprojection_filter.argtypes = [C.POINTER(ReportDesc), C.POINTER(ReportOut)]
    return lib


def constants() -> dict:
    out = np.zeros(8, dtype=np.int32)
    harness().rh_constants(out.ctypes.data_as(I32))
    return dict(zip(("digit_bits", "radix", "passes", "block", "tile", "lds_queries", "lds_cams", "lds_sums"), out.tolist()))


def rank_plan(n: int, percentile: float):
    """(lo, hi, g) of numpy.percentile(x[n], 100 - percentile)."""
    lo_hi, g = np.zeros(2, dtype=np.int64), C.c_double()
    harness().rh_rank_plan(n, percentile, lo_hi.ctypes.data_as(I64), C.byref(g))
    return int(lo_hi[0]), int(lo_hi[1]), g.value


def select(x, rank: int) -> float:
    x = np.ascontiguousarray(x, dtype=np.float64)
    return harness().rh_select(x.ctypes.data_as(F64), len(x), rank)


def percentile(x, removed_percent: float) -> float:
    """numpy.percentile(x, 100 - removed_percent) by the select and the interpolation of report_math.h."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return harness().rh_percentile(x.ctypes.data_as(F64), len(x), removed_percent)


class HarnessReprojectionStats:
    """The `_solver` hook on the g++ build: same arguments, checks, result and error type as
    caliscope_amd.reprojection_stats.DeviceReprojectionStats.  `err_in` (Euclidean errors) or `pixel_errors` ((n, 2), returned as
    err_xy) set on the object replace the projection."""

    def __init__(self, err_in=None, pixel_errors=None):
        self.pixel_errors = None if pixel_errors is None else np.ascontiguousarray(pixel_errors, dtype=np.float64).reshape(-1, 2)
        self.err_in = err_in if self.pixel_errors is None else np.sqrt(np.einsum("ij,ij->i", self.pixel_errors, self.pixel_errors))
        self.calls = 0

    def reprojection_filter(self, cam_model, cam_const, cam_pose, points, obs_cam, obs_pt, obs_uv, *, obs_group=None, n_groups=0, err_in=None,
                            mode="stats", scope="per_camera", value=0.0, min_per_camera=10, want_errors=True):
        args = check_reprojection_arguments(cam_model, cam_const, cam_pose, points, obs_cam, obs_pt, obs_uv, obs_group, n_groups,
                                            self.err_in if self.err_in is not None else err_in, mode, scope, value, min_per_camera)
        self.calls += 1
        lib = harness()
        result = run_reprojection_call(lib.rh_reprojection_filter, args, want_errors, "cba_reprojection_filter", lambda: lib.rh_last_error().decode())
        if self.pixel_errors is not None and want_errors:
            object.__setattr__(result, "err_xy", self.pixel_errors.copy())
        return result


# ---- the brute force and the tables ---------------------------------------------------------------------------------------------------

def brute_force_filter(err, obs_cam, n_cams, mode, value, scope="per_camera", min_per_camera=10):
    """(threshold[n_cams], keep[n] bool, kept[n_cams], cameras topped up) by sorting: np.percentile per segment, err <= threshold,
    and for a camera that keeps fewer than r = min(min_per_camera, rows) the r-th smallest error as its threshold."""
    err, obs_cam = np.asarray(err, dtype=np.float64), np.asarray(obs_cam)
    thr = np.full(n_cams, np.inf)
    if mode == "absolute":
        thr[:] = value
    elif scope == "overall":
        if len(err):
            thr[:] = np.percentile(err, 100 - value)
    else:
        for c in range(n_cams):
            e = err[obs_cam == c]
            if len(e):
                thr[c] = np.percentile(e, 100 - value)
    n_floor = 0
    for c in range(n_cams):
        e = np.sort(err[obs_cam == c])
        r = min(min_per_camera, len(e))
        if int((e <= thr[c]).sum()) < r:
            thr[c] = e[r - 1]
            n_floor += 1
    keep = err <= thr[obs_cam] if len(err) else np.zeros(0, dtype=bool)
    return thr, keep, np.bincount(obs_cam[keep], minlength=n_cams).astype(np.int64), n_floor


def random_errors(n_obs: int, n_cams: int, seed: int, outliers: float = 0.05):
    """(err[n_obs], obs_cam[n_obs]): gamma-distributed pixel errors with a share of large ones, cameras at random (every camera
    occupied where there are enough rows), some exact ties."""
    rng = np.random.default_rng(seed)
    err = rng.gamma(2.0, 0.3, n_obs)
    bad = rng.random(n_obs) < outliers
    err[bad] += rng.uniform(5.0, 50.0, int(bad.sum()))
    if n_obs > 8:
        err[rng.integers(0, n_obs, n_obs // 8)] = err[rng.integers(0, n_obs, n_obs // 8)]
    cam = rng.integers(0, n_cams, n_obs)
    if n_obs >= n_cams:
        cam[rng.permutation(n_obs)[:n_cams]] = np.arange(n_cams)
    return err, cam.astype(np.int32)


def placeholder_cameras(n_cams: int):
    """cam_model, cam_const, cam_pose and points of a call whose errors are given (not read by the library then)."""
    const = np.zeros((n_cams, 12))
    const[:, :2] = 1.0
    return np.zeros(n_cams, dtype=np.int32), const, np.zeros((n_cams, 6)), np.zeros((1, 3))


def filter_with_given_errors(solver, err, obs_cam, n_cams, mode, value, scope="per_camera", min_per_camera=10, obs_group=None, n_groups=0):
    model, const, pose, points = placeholder_cameras(n_cams)
    return solver.reprojection_filter(model, const, pose, points, obs_cam, None, None, err_in=err, obs_group=obs_group, n_groups=n_groups, mode=mode,
                                      scope=scope, value=value, min_per_camera=min_per_camera)


# ---- the reference's filter fixtures (tests/golden/reference_host/filter_*.npz) through filter_outliers ------------------------------------
FILTER_FIXTURES = sorted((Path(__file__).parent / "golden" / "reference_host").glob("filter_*.npz"))
REPORT_FIXTURES = sorted((Path(__file__).parent / "golden" / "reference_host").glob("report_*.npz"))
WORLD_COLS = ["sync_index", "object_id", "keypoint_id", "x_coord", "y_coord", "z_coord", "frame_time"]
IMG_COLS = ["sync_index", "cam_id", "object_id", "keypoint_id", "img_loc_x", "img_loc_y"]


def sorted_rows(a):
    a = np.asarray(a, dtype=np.float64)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def fixture_tables(ref):
    import pandas as pd

    wdf = pd.DataFrame(ref["world"], columns=WORLD_COLS).astype({"sync_index": "int64", "object_id": "int64", "keypoint_id": "int64"})
    idf = pd.DataFrame(ref["image"], columns=IMG_COLS).astype({c: "int64" for c in IMG_COLS[:4]})
    return wdf, idf


def run_filter_fixture(path, make_solver) -> tuple[int, int]:
    """Every run of one filter fixture through ``filter_outliers(_solver=make_solver(stored errors))``, compared as
    tests/test_reference_host_fixtures.py compares the host filters: rows, world-row set and world key per observation equal to the
    reference's output; runs with two or more cameras below the floor (where the reference tops up only the first) take the
    subset-and-floor comparison.  Returns (runs, runs that took the weaker comparison)."""
    import warnings

    from caliscope_amd.cameras import CameraArray, CameraData
    from caliscope_amd.capture_volume import CaptureVolume
    from caliscope_amd.constraints import ConstraintSet
    from caliscope_amd.point_data import ImagePoints, WorldPoints

    ref = np.load(path)
    wdf, idf = fixture_tables(ref)
    K = np.array([[400.0, 0.0, 200.0], [0.0, 400.0, 200.0], [0.0, 0.0, 1.0]])
    cams = CameraArray({c: CameraData(cam_id=c, size=(400, 400), matrix=K.copy(), distortions=np.zeros(5), rotation=np.eye(3),
                                      translation=np.array([0.1 * c, 0.0, 0.0])) for c in (0, 1)})
    static = frozenset(int(o) for o in ref["static_ids"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vol = CaptureVolume(cams, ImagePoints(idf), WorldPoints(wdf), ConstraintSet((), static) if static else None)
    raw = ref["raw_errors"]  # sync_index, cam_id, object_id, keypoint_id, error_x, error_y, euclidean_error
    matched = vol.img_to_obj_map >= 0
    assert len(raw) == int(matched.sum()) and np.array_equal(raw[:, 1].astype(np.int64), idf["cam_id"].to_numpy()[matched])
    solver = make_solver(raw[:, 6].copy())

    def world_key_of_rows(volume):
        w = volume.world_points.df[WORLD_COLS[:3]].to_numpy()
        m = volume.img_to_obj_map
        return np.where(m[:, None] >= 0, w[np.maximum(m, 0)], -7)

    weaker = 0
    for n in range(int(ref["n_runs"])):
        kind, value, scope, floor = ref[f"run{n}_args"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if kind == 0.0:
                out = vol.filter_outliers(float(value), scope="per_camera" if scope == 0.0 else "overall", min_per_camera=int(floor), _solver=solver)
            else:
                out = vol.filter_outliers(max_pixels=float(value), min_per_camera=int(floor), _solver=solver)
        assert out.optimization_status is None
        mine = out.image_points.df[IMG_COLS].to_numpy(dtype=np.float64)
        if int(ref[f"run{n}_floor_cameras"]) >= 2:
            weaker += 1
            theirs = {tuple(r) for r in ref[f"run{n}_image"][:, :4].astype(np.int64).tolist()}
            ours = {tuple(r) for r in mine[:, :4].astype(np.int64).tolist()}
            assert theirs <= ours, n
            cam_rows, cam_kept = np.bincount(raw[:, 1].astype(np.int64), minlength=2), np.bincount(mine[:, 1].astype(np.int64), minlength=2)
            assert np.all(cam_kept >= np.minimum(int(floor), cam_rows)), (n, cam_kept, cam_rows, floor)
            continue
        assert np.array_equal(mine, ref[f"run{n}_image"]), n
        assert np.array_equal(sorted_rows(out.world_points.df[WORLD_COLS].to_numpy(dtype=np.float64)), sorted_rows(ref[f"run{n}_world"]), equal_nan=True), n
        theirs_w, theirs_m = ref[f"run{n}_world"][:, :3].astype(np.int64), ref[f"run{n}_map"]
        assert np.array_equal(world_key_of_rows(out), np.where(theirs_m[:, None] >= 0, theirs_w[np.maximum(theirs_m, 0)], -7)), n
    return int(ref["n_runs"]), weaker
