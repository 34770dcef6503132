"""Redundancy numbers and the w-test on the CPU: csrc/reliability_math.h and the whole call through the g++ harness
(tests/reliability_native.py), the report, the CaptureVolume seam with data snooping, and the header of the C ABI.

Reference and tolerance.  The reference (a) is the dense projector: R = I - J Q+ L+^-1 Q+^T J^T from the float64 eigh of the oracle's
J^T J with the seven smallest eigenvalues zeroed; the yardstick is its disagreement with (b), the block formula of
include/caliscope/reliability.h in numpy with C from the bordered system (two CPU formulations, neither is the code under test).  The
code under test may differ from (a) by ten times that disagreement, floor 1e-12, absolute on every entry of every R_oo; a scene whose
disagreement exceeds 1e-8 fails.  w is compared row by row, relative, within that tolerance divided by the reference r_j; sigma0^2, cost
and dof as covariance_native.check_against_pinv compares them (reliability_native.check_against_dense has the details, and why the
residual has a bound of its own).  Measured on the harness (disagreement of (a) and (b), error of R_oo, error of w times r_j, smallest
reference r, share of rows with r < 0.01):

    LEAST   2 cameras x 8 points, 2 views (dof 3)      1.3e-14  1.2e-14  6.0e-15  0.0031  12.5 %
    SMALL   4 x 30, 3 views                            4.2e-15  3.9e-15  2.2e-15  0.0032   1.1 %
    ragged  (2 views, all views, a repeated pair)      8.4e-15  8.4e-15  4.2e-15  0.0012   0.5 %
    ROBUST  soft_l1, 5 % outliers, 6 x 300             8.7e-14  1.0e-13  5.2e-14  0.0010   3.0 %
    FREE27  3 free pinhole cameras x 300               8.8e-13  8.8e-13  4.4e-13  0.020    0
    MIXED33 1 free pinhole + 4 fisheye x 300           6.3e-14  6.9e-14  3.4e-14  0.13     0
    WIDE9   9 locked cameras x 300, 9 views            1.2e-15  1.2e-15  1.0e-15  0.30     0
    WIDE10  1 free pinhole + 9 fisheye x 300           2.7e-13  2.7e-13  1.3e-13  0.30     0

No reference row is at or below REL_R_TINY = 1e-10, so n_uncontrolled == 0 and no w is NaN on every scene; the NaN rule is tested on
rel_w of reliability_math.h directly.
"""
import copy
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from caliscope_amd import _lib, build, reliability
from caliscope_amd.exceptions import BackendError, CalibrationError
from tests import covariance_native as cn
from tests import reliability_native as rn
from tests.dense_solve_cases import widths
from tests.native_build import CSRC, NATIVE, compile_native
from tests.test_uncertainty import FREE27, LEAST, MIXED33, ROBUST, SIX, SMALL, _args, error_cases

ROOT = Path(__file__).resolve().parent.parent
F_1PX = 1.0 / 1394.6  # one pixel (not read for the linear loss)
WIDE9 = ("wide", (6,) * 9, False)
WIDE10 = ("wide", (9,) + (6,) * 9, True)
SCENES = [(LEAST, "linear"), (SMALL, "linear"), (("ragged",), "linear"), (ROBUST, "soft_l1"), (FREE27, "linear"), (MIXED33, "linear"), (WIDE9, "linear"),
          (WIDE10, "linear")]
SCENE_IDS = ["least", "small", "ragged", "robust", "free27", "mixed33", "wide9", "wide10"]
BUMPED_ROWS = (10, 777, 1500)
BUMP_PX = 8.0
OUT_FIELDS = [f for f, _ in reliability.RelOut._fields_]


def harness_call(key, loss="linear", f_scale=1.0):
    return rn.HarnessReliability().observation_reliability(*rn.scene_arguments(key), loss=loss, f_scale=f_scale)


# ---- the whole call against the dense projector -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,loss", SCENES, ids=SCENE_IDS)
def test_harness_call_matches_the_dense_projector(key, loss):
    figures = rn.check_against_dense(harness_call(key, loss, F_1PX), key, loss, F_1PX)
    assert figures["lam8"] > 1e-6


def test_scenes_are_what_the_table_says():
    """Views per point: 2 (LEAST), 3 (SMALL), 9 and 10 on the wide scenes (81 and 100 pairs per point: more than one wave has lanes, and
    more than four observations: the kernel's loop over groups of four wraps), 2 / 5 / 6 on the ragged scene; weakly controlled rows exist."""
    for key, k in ((LEAST, 2), (SMALL, 3), (WIDE9, 9), (WIDE10, 10)):
        assert set(np.bincount(cn.key_scene(key)["obj"])) == {k}
    assert sorted(set(np.bincount(cn.key_scene(("ragged",))["obj"]))) == [2, 5, 6]
    assert cn.key_scene(MIXED33)["par"].n_camera_params == 33 and tuple(b.n_params for b in cn.key_scene(WIDE10)["par"].blocks) == WIDE10[1]
    assert rn.reference(LEAST)["r"].min() < 0.01 and rn.reference(SMALL)["r"].min() < 0.01 and rn.reference(("ragged",))["r"].min() < 0.01


def permuted_call(call, key, seed=7):
    """(result on the rows as they are, result on randomly permuted rows, the permutation)."""
    args = rn.scene_arguments(key)
    perm = np.random.default_rng(seed).permutation(len(args[5]))
    return call(*args), call(*args[:5], args[5][perm], args[6][perm], args[7][perm]), perm


def check_permuted(plain, moved, perm, key, bitwise):
    ref = rn.reference(key)
    tol = max(10.0 * ref["dis"], 1e-12)
    err_R = float(np.max(np.abs(moved.redundancy - plain.redundancy[perm])))
    err_w = float(np.max(np.abs(moved.w - plain.w[perm]) * ref["r"][perm] / np.abs(plain.w[perm])))
    print(dict(key=key, bitwise=bitwise, err_R=err_R, err_w_times_r=err_w, tol=tol))
    assert err_R <= tol and err_w <= tol and np.array_equal(moved.residual, plain.residual[perm])
    assert moved.dof == plain.dof and moved.n_uncontrolled == plain.n_uncontrolled
    if bitwise:
        assert np.array_equal(moved.redundancy, plain.redundancy[perm]) and np.array_equal(moved.w, plain.w[perm])
        assert moved.sigma0_sq == plain.sigma0_sq and moved.cost == plain.cost


@pytest.mark.parametrize("key", [("ragged",), WIDE10], ids=["ragged", "wide10"])
def test_permuted_rows_return_permuted_outputs(key):
    """The harness adds in one fixed order, and the observations of a point are put in an order of their own first: bit-equal."""
    plain, moved, perm = permuted_call(rn.HarnessReliability().observation_reliability, key)
    check_permuted(plain, moved, perm, key, bitwise=True)


def nulled(call, fields):
    def wrapped(desc, out):
        for f in fields:
            setattr(out._obj, f, None)
        return call(desc, out)
    return wrapped


def check_null_outputs(make_call, exact):
    """Every subset of the seven output pointers NULL: the others are returned as in the full call, the NULL ones stay as the wrapper
    initialised them (zeros).  ``make_call(fields) -> ReliabilityResult``."""
    full = make_call(())
    for n in range(1, len(OUT_FIELDS) + 1):
        for fields in itertools.combinations(OUT_FIELDS, n):
            some = make_call(fields)
            for name, attr in (("redundancy", "redundancy"), ("w", "w"), ("residual", "residual")):
                got, want = getattr(some, attr), getattr(full, attr)
                if name in fields:
                    assert not got.any(), (fields, name)
                else:
                    assert np.array_equal(got, want) if exact else np.allclose(got, want, rtol=1e-9, atol=1e-12), (fields, name)
            for name in ("sigma0_sq", "dof", "cost", "n_uncontrolled"):
                got, want = getattr(some, name), getattr(full, name)
                assert got == 0 if name in fields else got == pytest.approx(want, rel=1e-12), (fields, name)
    return full


def test_null_outputs_in_every_combination():
    lib = rn.harness()
    args = reliability.check_covariance_arguments(*rn.scene_arguments(SMALL), "linear", 1.0)
    full = check_null_outputs(lambda fields: reliability.run_reliability_call(nulled(lib.rh_observation_reliability, fields), args, "harness",
                                                                              lambda: lib.rh_last_error().decode()), exact=True)
    assert full.redundancy.any() and full.dof == rn.reference(SMALL)["dof"]


# ---- the NaN rule -----------------------------------------------------------------------------------------------------------------------
def test_uncontrolled_rows_have_nan_w_and_r_is_clamped_for_the_root_only():
    lib = rn.harness()
    tiny = np.zeros(1)
    lib.rh_constants(tiny.ctypes.data_as(rn.F64))
    assert tiny[0] == 1e-10 == reliability.REL_R_TINY
    for r in (1e-10, 0.0, -1e-3, float("nan"), np.nextafter(1e-10, 0.0)):
        assert np.isnan(lib.rh_w(0.5, r, 2.0)), r
    above = float(np.nextafter(1e-10, 1.0))
    assert lib.rh_w(0.5, above, 2.0) == 0.5 / (2.0 * np.sqrt(above))
    assert lib.rh_w(0.5, 0.25, 2.0) == 0.5 and lib.rh_w(-3.0, 1.0, 1.5) == -2.0
    assert lib.rh_w(0.5, 1.0 + 1e-9, 2.0) == 0.25 and lib.rh_w(0.5, 7.0, 2.0) == 0.25  # clamped to 1 for the root


# ---- error paths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", error_cases(), ids=lambda c: c[0])
def test_host_checks_give_the_codes_of_the_covariance_call(case):
    _, args, code, words = case
    with pytest.raises(BackendError, match=re.escape(f"(code {code})")) as info:
        rn.HarnessReliability().observation_reliability(*args)
    assert words in str(info.value) and "cba_observation_reliability" in str(info.value)


def test_degenerate_scenes_return_the_numeric_error():
    with pytest.raises(BackendError, match=r"code -6.*not positive definite beyond the gauge"):
        rn.HarnessReliability().observation_reliability(*cn.planar_degenerate_scene())
    a = _args()
    rows = np.flatnonzero(a[6] == 3)
    a[5][rows] = a[5][rows[0]]  # every view of point 3 from one camera: one ray
    with pytest.raises(BackendError, match=r"code -6.*point 3"):
        rn.HarnessReliability().observation_reliability(*a)
    with pytest.raises(ValueError, match="loss must be one of"):
        rn.HarnessReliability().observation_reliability(*_args(), loss="tukey")


# ---- the report -------------------------------------------------------------------------------------------------------------------------
def test_critical_value_is_the_two_sided_normal_quantile():
    assert reliability.critical_value(0.001) == pytest.approx(3.2905267314919255, abs=1e-9)
    assert reliability.critical_value(0.05) == pytest.approx(1.959963984540054, abs=1e-9)
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            reliability.critical_value(bad)


def test_report_fields():
    args = rn.scene_arguments(FREE27)
    res = harness_call(FREE27)
    n = len(args[5])
    rows = np.arange(n) * 2 + 1  # every observation on an odd row of twice as many image rows
    fx = args[2][args[5], 0]
    rep = reliability.build_report(res, rows, 2 * n, fx, [10, 11, 12], args[5], args[6] + 4, 304, delta0=3.0)
    assert rep.dof == res.dof and rep.sigma0 == pytest.approx(np.sqrt(res.sigma0_sq)) and rep.delta0 == 3.0 and rep.n_uncontrolled == 0
    assert rep.redundancy.shape == (2 * n, 2) and rep.redundancy_uv.shape == (2 * n,) and rep.w.shape == rep.residual_px.shape == rep.mdb_px.shape == (2 * n, 2)
    for a in (rep.redundancy, rep.w, rep.residual_px, rep.mdb_px):
        assert np.isnan(a[0::2]).all() and np.isfinite(a[1::2]).all()
    assert np.isnan(rep.redundancy_uv[0::2]).all()
    assert np.array_equal(rep.redundancy[rows], np.stack([res.redundancy[:, 0, 0], res.redundancy[:, 1, 1]], axis=1))
    assert np.array_equal(rep.redundancy_uv[rows], res.redundancy[:, 0, 1]) and np.array_equal(rep.w[rows], res.w)
    assert np.allclose(rep.residual_px[rows], res.residual * 500.0) and np.allclose(rep.mdb_px[rows], 3.0 * rep.sigma0 * 500.0 / np.sqrt(rep.redundancy[rows]))
    assert np.nansum(rep.redundancy) == pytest.approx(rep.dof, rel=1e-9)
    assert sorted(rep.camera_redundancy) == [10, 11, 12]
    for i, cid in enumerate((10, 11, 12)):
        assert rep.camera_redundancy[cid] == pytest.approx(rep.redundancy[rows][args[5] == i].mean())
    assert rep.point_redundancy.shape == (304,) and np.isnan(rep.point_redundancy[:4]).all()
    assert rep.point_redundancy[4 + 17] == pytest.approx(rep.redundancy[rows][args[6] == 17].mean())
    flagged = rep.flagged(0.001)
    assert np.array_equal(flagged, rows[np.abs(res.w).max(axis=1) > reliability.critical_value(0.001)])
    assert len(rep.flagged(0.5)) > len(flagged)
    worst = rep.worst_observations(3)
    top = rows[np.argsort(-np.abs(res.w).max(axis=1))[:3]]
    assert [w[0] for w in worst] == top.tolist() and worst[0][1] >= worst[1][1] >= worst[2][1] and 0 < worst[0][2] <= 1
    assert rep.worst_observations(0) == []


def test_snooping_mask_takes_one_observation_per_point_and_leaves_two_views():
    #                 point 0: two over the line      point 1: two views    point 2: nothing     point 3: NaN beside a hit
    w = np.array([5.0, 9.0, 1.0, 4.0,                 8.0, 0.5,             3.0, 2.0, 1.0,       np.nan, 6.0, 0.1])
    obj = np.array([0, 0, 0, 0,                       1, 1,                 2, 2, 2,             3, 3, 3])
    perm = np.random.default_rng(0).permutation(len(w))
    keep = reliability.snooping_mask(w[perm], obj[perm], np.bincount(obj), 3.29)
    back = np.empty(len(w), dtype=bool)
    back[perm] = keep
    assert np.flatnonzero(~back).tolist() == [1, 10]


# ---- detection end to end ---------------------------------------------------------------------------------------------------------------
def solved_volume(bumped_row):
    """SIX with BUMP_PX added to u of one observation row (None: none), solved by scipy's least_squares on the oracle's functions:
    (volume at the solution, uv)."""
    from scipy.optimize import least_squares

    from caliscope_amd.capture_volume import CaptureVolume
    from oracle.residuals import joint_jacobian, joint_residuals
    from tests.helpers import small_problem

    sc, par, x0 = small_problem(n_cams=6, n_points=300, k=6)
    uv = np.array(sc.image_coords, dtype=np.float64)
    if bumped_row is not None:
        uv[bumped_row, 0] += BUMP_PX
    sol = least_squares(joint_residuals, x0, jac=joint_jacobian, args=(par, sc.camera_indices, uv, sc.obj_indices), method="trf", x_scale="jac",
                        ftol=1e-12, xtol=1e-12, gtol=1e-12)
    assert sol.status > 0
    cams = copy.deepcopy(sc.cameras_init)
    pts = par.unpack_into(cams, sol.x).copy()
    return CaptureVolume.from_arrays(cams, sc.camera_indices, uv, sc.obj_indices, pts), uv


def check_detection(vol, bumped_row, **how):
    """The bumped row carries the largest |w| of the volume, the runner-up lies on its point, and one pass of data snooping at 0.1 %
    removes it and no other row of its point."""
    rep = vol.observation_reliability(**how)
    m = rep.max_abs_w
    obj = vol.img_to_obj_map
    order = np.argsort(-m)
    print(dict(row=bumped_row, w=float(m[bumped_row]), runner_up=float(m[order[1]]), runner_up_row=int(order[1]), flagged=len(rep.flagged(0.001))))
    assert order[0] == bumped_row and obj[order[1]] == obj[bumped_row]
    assert rep.worst_observations(1)[0][0] == bumped_row and bumped_row in rep.flagged(0.001)
    before, after = vol.image_points._df, vol.filter_by_w_test(0.001, **how).image_points._df
    pair = lambda df: set(zip(df["cam_id"].tolist(), df["object_id"].tolist()))  # noqa: E731  (one row per (camera, point) on this scene)
    gone = pair(before) - pair(after)
    cam, point = int(before["cam_id"].iloc[bumped_row]), int(before["object_id"].iloc[bumped_row])
    assert (cam, point) in gone and [g for g in gone if g[1] == point] == [(cam, point)]
    assert len(gone) == len(before) - len(after) and max(np.bincount([g[1] for g in gone])) == 1
    return rep


def check_clean(vol, **how):
    """Nothing is wrong: the volume loses no more than one observation per point and keeps every point."""
    after = vol.filter_by_w_test(0.001, **how)
    lost = np.bincount(vol.image_points._df["object_id"], minlength=300) - np.bincount(after.image_points._df["object_id"], minlength=300)
    print(dict(lost=int(lost.sum())))
    assert lost.min() >= 0 and lost.max() <= 1 and len(after.world_points) == len(vol.world_points) == 300
    assert lost.sum() <= len(vol.observation_reliability(**how).flagged(0.001))


@pytest.mark.parametrize("row", BUMPED_ROWS)
def test_blunder_is_found_and_removed(row):
    vol, _ = solved_volume(row)
    check_detection(vol, row, _solver=rn.HarnessReliability())


def test_clean_volume_keeps_its_points():
    vol, _ = solved_volume(None)
    check_clean(vol, _solver=rn.HarnessReliability())


# ---- the seam ---------------------------------------------------------------------------------------------------------------------------
def seam_volume():
    """SMALL as a volume with, in the middle of its tables, a world point seen once (row 7 of the world points) and an image row that
    matches no world point: (volume, image rows that take part)."""
    from caliscope_amd.capture_volume import CaptureVolume
    from tests.helpers import small_problem

    sc, _, _ = small_problem(n_cams=4, n_points=30, k=3)
    cam_ids, uv, obj = np.array(sc.camera_indices), np.array(sc.image_coords), np.array(sc.obj_indices)
    pts = np.insert(sc.points_init, 7, [0.1, 0.2, 0.3], axis=0)
    obj = np.where(obj >= 7, obj + 1, obj)
    cam_ids, uv, obj = np.insert(cam_ids, 20, 0), np.insert(uv, 20, [600.0, 400.0], axis=0), np.insert(obj, 20, 7)     # one view of point 7
    cam_ids, uv, obj = np.insert(cam_ids, 50, 1), np.insert(uv, 50, [500.0, 300.0], axis=0), np.insert(obj, 50, 4000)  # no such world point
    part = np.ones(len(obj), dtype=bool)
    part[[20, 50]] = False
    return CaptureVolume.from_arrays(sc.cameras_init, cam_ids, uv, obj, pts), part


def test_seam_aligns_the_report_to_the_image_rows():
    import caliscope_amd

    vol, part = seam_volume()
    assert (vol.img_to_obj_map >= 0).sum() == len(part) - 1
    hook = rn.HarnessReliability()
    rep = vol.observation_reliability(_solver=hook)
    assert hook.calls == 1 and isinstance(rep, caliscope_amd.ReliabilityReport)
    direct = harness_call(SMALL)
    for a in (rep.redundancy, rep.w, rep.residual_px, rep.mdb_px, rep.redundancy_uv):
        assert len(a) == len(part) and np.isnan(a[~part]).all() and np.isfinite(a[part]).all()
    assert np.array_equal(rep.w[part], direct.w) and np.array_equal(rep.redundancy[part, 0], direct.redundancy[:, 0, 0]) and rep.dof == direct.dof
    assert np.isnan(rep.point_redundancy[7]) and np.isfinite(np.delete(rep.point_redundancy, 7)).all() and len(rep.point_redundancy) == 31
    assert sorted(rep.camera_redundancy) == [0, 1, 2, 3]
    assert not np.isin(rep.flagged(0.5), np.flatnonzero(~part)).any() and len(rep.flagged(0.5)) > 0
    filtered = vol.filter_by_w_test(0.5, _solver=hook)  # unmatched rows go, as in filter_outliers; SMALL has three views per point
    lost = np.bincount(vol.image_points._df["object_id"], minlength=4001) - np.bincount(filtered.image_points._df["object_id"], minlength=4001)
    assert lost[4000] == 1 and lost[7] == 0 and lost[:31].max() == 1 and lost[:31].sum() > 0 and len(filtered.world_points) == 31


def test_seam_with_free_intrinsics_and_a_robust_loss():
    vol, _ = seam_volume()
    hook = rn.HarnessReliability()
    free = vol.observation_reliability(refine_intrinsics=True, loss="soft_l1", _solver=hook)  # f_scale defaults to pixel_f_scale()
    explicit = vol.observation_reliability(refine_intrinsics=True, loss="soft_l1", f_scale=vol.pixel_f_scale(), _solver=hook)
    locked = vol.observation_reliability(loss="soft_l1", _solver=hook)
    assert np.array_equal(free.w, explicit.w, equal_nan=True) and free.dof == locked.dof - 12
    assert np.nansum(free.redundancy) == pytest.approx(free.dof, rel=1e-9) and np.nansum(locked.redundancy) == pytest.approx(locked.dof, rel=1e-9)
    twice = vol.observation_reliability(delta0=2 * 4.13, _solver=hook)
    assert np.allclose(twice.mdb_px, 2.0 * vol.observation_reliability(_solver=hook).mdb_px, equal_nan=True)


def test_seam_refuses_constraints():
    from caliscope_amd.capture_volume import CaptureVolume
    from caliscope_amd.constraints import ConstraintSet

    vol, _ = seam_volume()
    constrained = CaptureVolume(vol.camera_array, vol.image_points, vol.world_points, ConstraintSet((), frozenset()))
    with pytest.raises(CalibrationError, match="without constraints"):
        constrained.observation_reliability(_solver=rn.HarnessReliability())
    with pytest.raises(CalibrationError, match="without constraints"):
        constrained.filter_by_w_test(_solver=rn.HarnessReliability())


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_is_declared_exported_bound_and_typed():
    build.build(verbose=False)
    lib = _lib.load()
    header = (ROOT / "include" / "caliscope" / "reliability.h").read_text()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", text))
    assert declared == {"cba_observation_reliability"} == set(reliability.RELIABILITY_SIGNATURES)
    assert not declared & set(_lib.SIGNATURES)
    assert hasattr(lib, "cba_observation_reliability")
    typed = _lib.bind(lib, reliability.RELIABILITY_SIGNATURES)
    for name, (res, args) in reliability.RELIABILITY_SIGNATURES.items():
        assert getattr(typed, name).argtypes == args and getattr(typed, name).restype == res
    body = re.search(r"typedef struct \{([^{}]*)\}\s*cba_rel_out", text).group(1)
    assert OUT_FIELDS == re.findall(r"(\w+)\s*;", body)
    assert (CSRC / "reliability_lib.hip") in build.SOURCES
    for dep in (CSRC / "reliability_math.h", CSRC / "covariance_pipeline.h", ROOT / "include" / "caliscope" / "reliability.h"):
        assert dep in build.DEPENDS


def test_device_call_fails_loudly_without_a_device():
    build.build(verbose=False)
    if _lib.load().cba_device_count() > 0:
        return  # (with a device the call runs: tests/test_reliability_gpu.py)
    with pytest.raises(BackendError, match="no HIP device"):
        reliability.DeviceReliability().observation_reliability(*_args())


def test_harness_call_under_sanitizers():
    """tests/native/reliability_check.cpp (the harness call on one scene, null outputs, two refused calls, the NaN rule) as a program of
    its own under AddressSanitizer and UndefinedBehaviorSanitizer: exit status 0 and no report.  No Python in the process under the sanitizers."""
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas")
    exe = compile_native(NATIVE / "reliability_check.cpp", flags=flags, include=(CSRC, NATIVE), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "Sanitizer" not in proc.stderr and "runtime error" not in proc.stderr
    assert "all checks passed" in proc.stdout
