"""The free-network parameter covariance on the CPU: csrc/covariance_math.h and the whole call through the g++ harness
(tests/covariance_native.py), the report's propagation, the CaptureVolume seam and the header of the C ABI.

Reference and tolerance.  The reference is the float64 eigh pseudo-inverse of the oracle's J^T J with the seven smallest eigenvalues
zeroed; the yardstick is its disagreement with the bordered formula evaluated in numpy on the same scene (two CPU formulations,
neither is the code under test), both computed in the test per scene.  The code under test may differ from the pinv by ten times
that disagreement (summation order), floor 1e-12, relative to the block-wise max-norm; every scene must show a CPU disagreement of at
most 1e-8 (asserted) so that a weak scene cannot widen the tolerance.  Measured disagreements (camera block, point blocks) and the
eighth eigenvalue relative to the largest:

    4 cameras x 30 points, 3 views, locked            5.1e-14  3.8e-14   1.0e-03
    2 cameras x 8 points, locked (ncp = 12)           1.0e-12  3.5e-13   5.0e-04
    6 cameras x 300 points, 6 views, locked           2.1e-14  4.3e-15   2.3e-03
    ragged (2 views, all views, a repeated pair)      2.5e-14  1.2e-14   5.9e-03
    soft_l1, 5 % outliers, 6 x 300                    9.4e-13  2.1e-13   3.3e-05
    wide, 3 free pinhole cameras x 300 (ncp = 27)     4.4e-12  1.3e-12   1.5e-05
    wide, 1 free pinhole + 4 fisheye x 300 (ncp = 33) 1.1e-12  5.5e-13   5.0e-05
    wide, 11 free pinhole x 300 (ncp = 99)            9.5e-12  1.0e-12   1.7e-05

With free intrinsics the narrow scenes of tests.helpers.small_problem are too weak for this rule (4 cameras x 300 points, every point in
every camera: 2.0e-08 and 1.9e-07; the mixed rig of tests/dense_solve_cases.py with ncp = 33: 7.3e-09 and 6.0e-08), so the free-intrinsic
scenes are covariance_native.wide_scene: every point in every camera, 300 points, points over the whole field of view.
"""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from caliscope_amd import _lib, build, uncertainty
from caliscope_amd.exceptions import BackendError, CalibrationError
from tests import covariance_native as cn
from tests.dense_solve_cases import widths
from tests.native_build import CSRC, NATIVE, compile_native

ROOT = Path(__file__).resolve().parent.parent

SMALL = ("small", 4, 30, 3, False, "linear", 0.0)
LEAST = ("small", 2, 8, 2, False, "linear", 0.0)
SIX = ("small", 6, 300, 6, False, "linear", 0.0)
ROBUST = ("small", 6, 300, 6, False, "soft_l1", 0.05)
FREE27 = ("wide", (9, 9, 9), False)
MIXED33 = ("wide", widths(33), True)


def _harness_call(key, loss="linear", f_scale=1.0):
    sc = cn.key_scene(key)
    return cn.HarnessUncertainty().parameter_covariance(*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]), loss=loss, f_scale=f_scale)


# ---- gauge columns ------------------------------------------------------------------------------------------------------------------------
def test_gauge_columns_span_the_null_space_of_the_jacobian():
    """|J N| <= 1e-12 |J| with J the oracle's Jacobian and N from covariance_math.h, on a rig that holds a free pinhole camera, fisheye
    cameras, a camera with |rvec| < 1e-4 (the series branch of cam_prepare) and one a milliradian from pi."""
    from oracle.residuals import joint_jacobian

    sc = cn.key_scene(("wide", (9, 6, 6, 9), True))
    par, x = sc["par"], sc["x"].copy()
    off = par.camera_param_offsets
    x[off[1]: off[1] + 6] = [3e-5, -2e-5, 4e-5, 0.1, -0.2, 3.0]              # fisheye, series branch: X_c = X + t to first order
    x[off[3]: off[3] + 6] = [np.pi - 1e-3, 0.0, 0.0, 0.2, 0.1, 4.0]          # free pinhole, half a turn about x: z_c = 4 - z > 0
    assert np.linalg.norm(x[off[1]: off[1] + 3]) < 1e-4
    tabs = par.device_tables()
    assert tabs["cam_model"].tolist() == [0, 1, 1, 0] and tabs["cam_n_params"].tolist() == [9, 6, 6, 9]
    J = joint_jacobian(x, par, sc["cam"], sc["uv"], sc["obj"]).toarray()
    N = np.zeros((len(x), 7))
    for i, (blk, o) in enumerate(zip(par.blocks, off)):
        x9 = np.zeros(9)
        x9[: blk.n_params] = x[o: o + blk.n_params]
        rows = cn.gauge_cam(x9, tabs["cam_const"][i], tabs["cam_model"][i], blk.n_params)
        assert not rows[6:].any()  # intrinsics do not move under a similarity
        N[o: o + blk.n_params] = rows[: blk.n_params]
    ncp = par.n_camera_params
    for p, X in enumerate(x[ncp:].reshape(-1, 3)):
        N[ncp + 3 * p: ncp + 3 * p + 3] = cn.gauge_point(X)
    assert np.linalg.matrix_rank(N) == 7
    ratio = np.linalg.norm(J @ N) / np.linalg.norm(J)
    print("|J N| / |J| =", ratio)
    assert ratio <= 1e-12
    assert np.allclose(N, cn.gauge_matrix(par, x), rtol=0, atol=1e-12 * np.abs(N).max())  # the numpy formulation uses the same columns


# ---- the whole call against the pseudo-inverse ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,loss", [(SMALL, "linear"), (LEAST, "linear"), (SIX, "linear"), (("ragged",), "linear"), (ROBUST, "soft_l1"),
                                      (FREE27, "linear"), (MIXED33, "linear")], ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v[:3])))
def test_harness_call_matches_the_pseudo_inverse(key, loss):
    f_scale = 1.0 / 1394.6  # one pixel (not read for the linear loss)
    figures = cn.check_against_pinv(_harness_call(key, loss, f_scale), key, loss, f_scale)
    assert figures["lam8"] > 1e-6


def test_ragged_scene_is_what_it_says():
    sc = cn.key_scene(("ragged",))
    views = np.bincount(sc["obj"], minlength=40)
    assert views[0] == 2 and views[1] == 5 and views[2] == 6
    pairs = np.stack([sc["cam"], sc["obj"]], axis=1)
    assert len(np.unique(pairs, axis=0)) == len(pairs) - 1


def test_robust_loss_changes_the_covariance():
    a, b = _harness_call(ROBUST, "linear"), _harness_call(ROBUST, "soft_l1", 1.0 / 1394.6)
    assert b.cost < 0.5 * a.cost and not np.allclose(a.cam_cov_full / a.sigma0_sq, b.cam_cov_full / b.sigma0_sq, rtol=1e-3)


# ---- error paths -----------------------------------------------------------------------------------------------------------------------------
def _args(key=SMALL):
    sc = cn.key_scene(key)
    return [np.array(a) for a in cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"])]


def error_cases():
    """(name, arguments, expected code, words of the message): inputs the host checks of the call refuse, shared with the GPU tests."""
    cases = []
    a = _args(); a[5][7] = 4
    cases.append(("camera index", a, -1, "observation 7: camera index 4"))
    a = _args(); a[6][11] = -1
    cases.append(("point index", a, -1, "observation 11: point index -1"))
    a = _args(); rows = np.flatnonzero(a[6] == 5)[1:]; keep = np.setdiff1d(np.arange(len(a[6])), rows)
    a[5], a[6], a[7] = a[5][keep], a[6][keep], a[7][keep]
    cases.append(("one view", a, -1, "point 5 has 1 observation"))
    a = _args(); keep = a[5] != 2
    a[5], a[6], a[7] = a[5][keep], a[6][keep], a[7][keep]
    views = np.bincount(a[6], minlength=30)
    a[4] = a[4][views >= 2]; renumber = np.cumsum(views >= 2) - 1; ok = views[a[6]] >= 2
    a[5], a[6], a[7] = a[5][ok], renumber[a[6][ok]].astype(np.int32), a[7][ok]
    cases.append(("unobserved camera", a, -1, "camera 2 has no observation"))
    a = _args(LEAST); keep = a[6] < 5
    a[4], a[5], a[6], a[7] = a[4][:5], a[5][keep], a[6][keep], a[7][keep]
    cases.append(("dof", a, -1, "dof = 2 n_obs - n_params + 7 = 0 is not positive"))
    a = _args(); a[0][1] = 1; a[1][1] = 9
    cases.append(("fisheye with nine", a, -4, "camera 1: a fisheye camera has no free intrinsics"))
    a = _args(); a[1][0] = 7
    cases.append(("seven parameters", a, -1, "camera 0: cam_nparams must be 6 or 9, got 7"))
    a = _args(); a[5], a[6], a[7] = a[5][:0], a[6][:0], a[7][:0]
    cases.append(("no observations", a, -1, "n_obs must be positive"))
    return cases


@pytest.mark.parametrize("case", error_cases(), ids=lambda c: c[0])
def test_host_checks_name_the_offender(case):
    _, args, code, words = case
    with pytest.raises(BackendError, match=re.escape(f"(code {code})")) as info:
        cn.HarnessUncertainty().parameter_covariance(*args)
    assert words in str(info.value)


def test_degenerate_scenes_return_the_numeric_error():
    """Free focal lengths in front of a fronto-parallel plane (the reduced system is singular beyond the gauge) and a point whose two rays
    coincide: CBA_ERR_NUMERIC, never NaNs."""
    with pytest.raises(BackendError, match=r"code -6.*not positive definite beyond the gauge"):
        cn.HarnessUncertainty().parameter_covariance(*cn.planar_degenerate_scene())
    a = _args()
    rows = np.flatnonzero(a[6] == 3)
    a[5][rows] = a[5][rows[0]]  # every view of point 3 from one camera: one ray
    with pytest.raises(BackendError, match=r"code -6.*point 3"):
        cn.HarnessUncertainty().parameter_covariance(*a)
    with pytest.raises(ValueError, match="loss must be one of"):
        cn.HarnessUncertainty().parameter_covariance(*_args(), loss="tukey")
    with pytest.raises(BackendError, match="f_scale must be positive"):
        cn.HarnessUncertainty().parameter_covariance(*_args(), loss="huber", f_scale=0.0)


# ---- the report ----------------------------------------------------------------------------------------------------------------------------
def _rotation(r):
    return uncertainty.rotation_and_left_jacobian(r)[0]


@pytest.mark.parametrize("rvec", [(0.3, -0.2, 0.5), (2e-5, 1e-5, -3e-5), (3.0, 0.4, -0.3)])
def test_propagation_matches_finite_differences(rvec):
    """The centre Jacobian against central differences of c = -R(r)^T t, and the left Jacobian against the rotation between R(r) and R(r + dr)."""
    r, t, h = np.array(rvec), np.array([0.4, -1.1, 2.7]), 1e-6
    centre = lambda v: -_rotation(v[:3]).T @ v[3:]  # noqa: E731
    v = np.concatenate([r, t])
    fd = np.stack([(centre(v + h * e) - centre(v - h * e)) / (2 * h) for e in np.eye(6)], axis=1)
    assert np.allclose(uncertainty.centre_jacobian(r, t), fd, rtol=0, atol=1e-8)
    R, Jl = uncertainty.rotation_and_left_jacobian(r)
    for e in np.eye(3):
        rel = _rotation(r + h * e) @ R.T  # ~ I + [Jl e h]x
        w = 0.5 * np.array([rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1]]) / h
        assert np.allclose(Jl @ e, w, rtol=0, atol=1e-5)


def test_report_fields():
    sc = cn.key_scene(FREE27)
    args = cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"])
    res = cn.HarnessUncertainty().parameter_covariance(*args)
    rep = uncertainty.build_report(res, [10, 11, 12], args[1], args[3])
    assert rep.gauge == "inner" and rep.dof == res.dof and rep.sigma0 == pytest.approx(np.sqrt(res.sigma0_sq))
    assert sorted(rep.cameras) == [10, 11, 12] and rep.point_cov.shape == (300, 3, 3) and rep.point_std.shape == (300, 3)
    assert np.allclose(rep.point_std ** 2, np.einsum("ijj->ij", res.point_cov))
    cam = rep.cameras[11]
    Jc = uncertainty.centre_jacobian(args[3][1, :3], args[3][1, 3:6])
    assert cam.param_cov.shape == (9, 9) and np.allclose(cam.centre_cov, Jc @ res.cam_cov[1, :6, :6] @ Jc.T)
    assert np.allclose(cam.centre_std ** 2, np.diag(cam.centre_cov)) and cam.position_std == pytest.approx(np.sqrt(np.trace(cam.centre_cov)))
    _, Jl = uncertainty.rotation_and_left_jacobian(args[3][1, :3])
    assert cam.rotation_std_deg == pytest.approx(np.degrees(np.sqrt(np.trace(Jl @ res.cam_cov[1, :3, :3] @ Jl.T))))
    assert cam.scale_std == pytest.approx(np.sqrt(res.cam_cov[1, 6, 6])) and cam.k1_std > 0 and cam.k2_std > cam.k1_std
    worst = rep.worst_cameras(2)
    assert len(worst) == 2 and worst[0][1] >= worst[1][1] >= min(c.position_std for c in rep.cameras.values())
    locked = uncertainty.build_report(_harness_call(SMALL), range(4), [6] * 4, _args()[3])
    assert locked.cameras[0].scale_std is None and locked.cameras[0].param_cov.shape == (6, 6)


# ---- the seam ------------------------------------------------------------------------------------------------------------------------------
def _volume(extra_point=False):
    from caliscope_amd.capture_volume import CaptureVolume
    from tests.helpers import small_problem

    sc, par, x0 = small_problem(n_cams=4, n_points=30, k=3)
    cam_ids, uv, obj, pts = sc.camera_indices, sc.image_coords, sc.obj_indices, sc.points_init
    if extra_point:  # a world point with one observation, in the middle of the table
        pts = np.insert(pts, 7, [0.1, 0.2, 0.3], axis=0)
        obj = np.where(obj >= 7, obj + 1, obj)
        cam_ids, uv, obj = np.append(cam_ids, 0), np.vstack([uv, [[600.0, 400.0]]]), np.append(obj, 7)
    return CaptureVolume.from_arrays(sc.cameras_init, cam_ids, uv, obj, pts), sc


def test_seam_runs_the_solver_hook_on_the_matched_arrays():
    import caliscope_amd

    vol, sc = _volume()
    hook = cn.HarnessUncertainty()
    rep = vol.parameter_uncertainty(_solver=hook)
    assert hook.calls == 1 and isinstance(rep, caliscope_amd.UncertaintyReport) and rep.gauge == "inner"
    direct = _harness_call(SMALL)
    assert rep.dof == direct.dof and np.array_equal(rep.cam_cov_full, direct.cam_cov_full) and np.array_equal(rep.point_cov, direct.point_cov)
    assert sorted(rep.cameras) == sorted(sc.cameras_init.posed_cameras)
    free = vol.parameter_uncertainty(refine_intrinsics=True, loss="soft_l1", _solver=hook)  # f_scale defaults to pixel_f_scale()
    assert free.cameras[0].param_cov.shape == (9, 9) and free.cameras[0].k1_std > 0
    explicit = vol.parameter_uncertainty(refine_intrinsics=True, loss="soft_l1", f_scale=vol.pixel_f_scale(), _solver=hook)
    assert np.array_equal(free.cam_cov_full, explicit.cam_cov_full)


def test_seam_leaves_out_points_with_one_view_and_refuses_constraints():
    from caliscope_amd.capture_volume import CaptureVolume
    from caliscope_amd.constraints import ConstraintSet

    vol, _ = _volume(extra_point=True)
    rep = vol.parameter_uncertainty(_solver=cn.HarnessUncertainty())
    direct = _harness_call(SMALL)
    assert np.isnan(rep.point_cov[7]).all() and np.isnan(rep.point_std[7]).all()
    assert np.array_equal(np.delete(rep.point_cov, 7, axis=0), direct.point_cov) and rep.dof == direct.dof
    constrained = CaptureVolume(vol.camera_array, vol.image_points, vol.world_points, ConstraintSet((), frozenset()))
    with pytest.raises(CalibrationError, match="without constraints"):
        constrained.parameter_uncertainty(_solver=cn.HarnessUncertainty())


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_is_declared_exported_bound_and_typed():
    """include/caliscope/uncertainty.h against the built library and UNCERTAINTY_SIGNATURES, as tests/test_library_abi.py checks the headers
    of include/ itself: declared == exported == bound by exactly this table, and typed by it; the structures have the header's fields."""
    build.build(verbose=False)
    lib = _lib.load()
    header = (ROOT / "include" / "caliscope" / "uncertainty.h").read_text()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", text))
    assert declared == {"cba_parameter_covariance"} == set(uncertainty.UNCERTAINTY_SIGNATURES)
    assert not declared & set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared but not exported"
    typed = _lib.bind(lib, uncertainty.UNCERTAINTY_SIGNATURES)
    for name, (res, args) in uncertainty.UNCERTAINTY_SIGNATURES.items():
        assert getattr(typed, name).argtypes == args and getattr(typed, name).restype == res
    for struct, cname in ((uncertainty.CovDesc, "cba_cov_desc"), (uncertainty.CovOut, "cba_cov_out")):
        body = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname, text).group(1)
        assert [f for f, _ in struct._fields_] == re.findall(r"(\w+)\s*;", body)
    assert (CSRC / "covariance_lib.hip") in build.SOURCES and (CSRC / "covariance_math.h") in build.DEPENDS
    assert (ROOT / "include" / "caliscope" / "uncertainty.h") in build.DEPENDS


def test_device_call_fails_loudly_without_a_device():
    build.build(verbose=False)
    if _lib.load().cba_device_count() > 0:
        return  # (with a device the call runs: tests/test_uncertainty_gpu.py)
    with pytest.raises(BackendError, match="no HIP device"):
        uncertainty.DeviceUncertainty().parameter_covariance(*_args())


def test_harness_call_under_sanitizers():
    """tests/native/covariance_check.cpp (the harness call on one scene, null outputs, two refused calls) as a program of its own under
    AddressSanitizer and UndefinedBehaviorSanitizer: exit status 0 and no report.  No Python in the process under the sanitizers."""
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas")
    exe = compile_native(NATIVE / "covariance_check.cpp", flags=flags, include=(CSRC, NATIVE), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "Sanitizer" not in proc.stderr and "runtime error" not in proc.stderr
    assert "all checks passed" in proc.stdout
