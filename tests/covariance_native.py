"""g++ build of caliscope_amd/csrc/covariance_math.h (tests/native/covariance_harness.cpp), a `_solver` hook for
CaptureVolume.parameter_uncertainty that runs on it, and what the uncertainty tests share: the scenes, the float64 eigenvalue
pseudo-inverse of the oracle's J^T J (the reference), the bordered formula in numpy (the second CPU formulation: the disagreement of
the two is the yardstick of the tolerance) and the comparison itself."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.uncertainty import CovDesc, CovOut, check_covariance_arguments, run_covariance_call
from tests.native_build import CSRC, NATIVE, load_native

I32 = C.POINTER(C.c_int32)
F64 = C.POINTER(C.c_double)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "covariance_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.ch_last_error.restype = C.c_char_p
    lib.ch_constants.restype = None
    lib.ch_constants.argtypes = [I32]
    lib.ch_gauge_cam.restype = None
    lib.ch_gauge_cam.argtypes = [F64, F64, C.c_int32, C.c_int32, F64]
    lib.ch_gauge_point.restype = None
    lib.ch_gauge_point.argtypes = [F64, F64]
    lib.ch_parameter_covariance.restype = C.c_int
    lib.ch_parameter_covariance.argtypes = [C.POINTER(CovDesc), C.POINTER(CovOut)]
    return lib


def gauge_cam(x9, cconst, model, nparams):
    x9, cconst, N = np.ascontiguousarray(x9, dtype=np.float64), np.ascontiguousarray(cconst, dtype=np.float64), np.zeros((9, 7))
    harness().ch_gauge_cam(x9.ctypes.data_as(F64), cconst.ctypes.data_as(F64), int(model), int(nparams), N.ctypes.data_as(F64))
    return N


def gauge_point(X):
    X, N = np.ascontiguousarray(X, dtype=np.float64), np.zeros((3, 7))
    harness().ch_gauge_point(X.ctypes.data_as(F64), N.ctypes.data_as(F64))
    return N


class HarnessUncertainty:
    """The `_solver` hook on the g++ build: same arguments, checks, result and error type as caliscope_amd.uncertainty.DeviceUncertainty."""

    def __init__(self):
        self.calls = 0

    def parameter_covariance(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, *, loss="linear", f_scale=1.0):
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        self.calls += 1
        lib = harness()
        return run_covariance_call(lib.ch_parameter_covariance, args, "cba_parameter_covariance", lambda: lib.ch_last_error().decode())


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def call_arguments(par, x, cam, obj, uv):
    """The positional arguments of ``parameter_covariance`` for a parameterisation and a parameter vector."""
    tabs = par.device_tables()
    cam_x = np.zeros((len(par.blocks), 9))
    for i, (blk, off) in enumerate(zip(par.blocks, par.camera_param_offsets)):
        cam_x[i, : blk.n_params] = x[off : off + blk.n_params]
    return (tabs["cam_model"], tabs["cam_n_params"], tabs["cam_const"], cam_x, x[par.n_camera_params:].reshape(-1, 3).copy(), np.asarray(cam, dtype=np.int32),
            np.asarray(obj, dtype=np.int32), np.asarray(uv, dtype=np.float64))


def scene(n_cams, n_points, k, refine=False, loss="linear", outliers=0.0, seed=42):
    """dict(par, x, cam, obj, uv) of tests.helpers.small_problem at its initial parameters."""
    from tests.helpers import small_problem

    sc, par, x0 = small_problem(n_cams=n_cams, n_points=n_points, k=k, refine=refine, loss=loss, outliers=outliers, seed=seed)
    return dict(par=par, x=x0, cam=np.ascontiguousarray(sc.camera_indices), obj=np.ascontiguousarray(sc.obj_indices), uv=np.ascontiguousarray(sc.image_coords))


def wide_scene(cam_widths, fisheye_six=False, n_points=300, seed=5):
    """Cameras of the given parameter widths (9: pinhole with free intrinsics, 6: locked; ``fisheye_six`` makes the six-wide ones fisheye
    cameras) on a ring around a box of ``n_points`` points, every point observed by every camera with half a pixel of noise; evaluated a
    few millimetres and milliradians off the truth.  The points fill the whole field of view, which is what determines k1 and k2: on
    these scenes the two CPU formulations agree to 1e-11 with free intrinsics (tests/test_uncertainty.py lists the figures), where the
    narrow scenes of tests.helpers.small_problem give 1e-7."""
    from caliscope_amd.bundle_parameterization import BundleParameterization
    from caliscope_amd.cameras import CameraArray, CameraData, matrix_to_rvec, rvec_to_matrix
    from caliscope_amd.synthetic import _look_at
    from oracle.camera_model import project_fisheye, project_pinhole, rotation_to_rvec

    rng = np.random.default_rng(seed)
    n = len(cam_widths)
    pts = rng.uniform(-0.9, 0.9, (n_points, 3)) * [1.0, 1.0, 0.6] + [0.0, 0.0, 0.6]
    cams, uv = {}, []
    for c, w in enumerate(cam_widths):
        ang = 2 * np.pi * c / n + 0.1
        pos = np.array([2.0 * np.cos(ang), 2.0 * np.sin(ang), 0.4 + 0.5 * (c % 3)])
        R = _look_at(pos, np.array([0.0, 0.0, 0.6]))
        t = -R @ pos
        K = np.array([[500.0, 0.0, 640.0], [0.0, 500.0, 360.0], [0.0, 0.0, 1.0]])
        fish = fisheye_six and w == 6
        dist = np.zeros(4) if fish else np.array([-0.1, 0.02, 0.0, 0.0, 0.0])
        exact, _ = (project_fisheye if fish else project_pinhole)(pts, rotation_to_rvec(R), t, K, dist)
        uv.append(exact + rng.normal(0, 0.5, exact.shape))
        rvec = matrix_to_rvec(R) + rng.normal(0, 0.005, 3)
        cams[c] = CameraData(cam_id=c, size=(1280, 720), matrix=K, distortions=dist, fisheye=fish, rotation=rvec_to_matrix(rvec),
                             translation=t + rng.normal(0, 0.01, 3))
    ca = CameraArray(cams)
    par = BundleParameterization.from_camera_array(ca, n_points=n_points, refine_intrinsics=9 in cam_widths)
    assert tuple(b.n_params for b in par.blocks) == tuple(cam_widths)
    x = par.pack(ca, pts + rng.normal(0, 0.005, pts.shape))
    return dict(par=par, x=x, cam=np.repeat(np.arange(n), n_points).astype(np.int32), obj=np.tile(np.arange(n_points), n).astype(np.int32),
                uv=np.concatenate(uv))


def ragged_scene():
    """Five six-wide cameras, 40 points seen by all of them, then: point 0 keeps exactly two views, point 1 all five, and one
    (camera, point) observation of point 2 is there twice."""
    sc = scene(5, 40, 5)
    cam, obj, uv = sc["cam"], sc["obj"], sc["uv"]
    assert np.all(np.bincount(obj, minlength=40) == 5)
    rows0 = np.flatnonzero(obj == 0)
    keep = np.ones(len(obj), dtype=bool)
    keep[rows0[2:]] = False
    again = int(np.flatnonzero(obj == 2)[1])
    order = np.concatenate([np.flatnonzero(keep), [again]])
    return dict(par=sc["par"], x=sc["x"], cam=np.ascontiguousarray(cam[order]), obj=np.ascontiguousarray(obj[order]), uv=np.ascontiguousarray(uv[order]))


def planar_degenerate_scene():
    """Three pinhole cameras with free intrinsics, all looking straight down the world z axis at points of the plane z = 0 from different
    heights: for every camera the focal scale and the height are the same column of J up to a factor, so the reduced system is singular
    beyond the gauge.  Returns the positional arguments of the call."""
    rng = np.random.default_rng(3)
    n_pts = 40
    pts = np.zeros((n_pts, 3))
    pts[:, :2] = rng.uniform(-1.0, 1.0, (n_pts, 2))
    n_cams = 3
    cam_x = np.zeros((n_cams, 9))
    cam_x[:, 3:6] = [[0.2, 0.1, 3.0], [-0.3, 0.2, 4.0], [0.1, -0.2, 5.0]]  # identity rotation: X_c = X + t
    cam_x[:, 6] = 1.0
    const = np.zeros((n_cams, 12))
    const[:, :4] = [800.0, 800.0, 640.0, 360.0]
    cam = np.repeat(np.arange(n_cams), n_pts).astype(np.int32)
    obj = np.tile(np.arange(n_pts), n_cams).astype(np.int32)
    Xc = pts[obj] + cam_x[cam, 3:6]
    uv = 800.0 * Xc[:, :2] / Xc[:, 2:3] + [640.0, 360.0] + rng.normal(0, 0.3, (len(cam), 2))
    return (np.zeros(n_cams, dtype=np.int32), np.full(n_cams, 9, dtype=np.int32), const, cam_x, pts, cam, obj, uv)


# ---- the two CPU formulations -----------------------------------------------------------------------------------------------------------
def robust_row_scale(f, loss="linear", f_scale=1.0):
    """(js, cost) of residuals f: the factor scipy's least_squares scales every row of J by for the loss (ones for the linear loss), and
    the cost 0.5 sum rho."""
    if loss == "linear":
        return np.ones(len(f)), 0.5 * float(f @ f)
    assert loss == "soft_l1"
    z = (f / f_scale) ** 2
    t = 1.0 + z
    rho0, rho1, rho2 = 2.0 * (np.sqrt(t) - 1.0), t ** -0.5, -0.5 * t ** -1.5
    return np.sqrt(np.maximum(rho1 + 2.0 * rho2 * z, np.finfo(float).eps)), 0.5 * f_scale ** 2 * float(rho0.sum())


def robust_jacobian(sc, loss="linear", f_scale=1.0):
    """(J dense, cost) with the oracle's residuals and Jacobian, rows scaled as scipy's least_squares scales them."""
    from oracle.residuals import joint_jacobian, joint_residuals

    par, x = sc["par"], sc["x"]
    J = joint_jacobian(x, par, sc["cam"], sc["uv"], sc["obj"]).toarray()
    js, cost = robust_row_scale(joint_residuals(x, par, sc["cam"], sc["uv"], sc["obj"]), loss, f_scale)
    return J * js[:, None], cost


def pinv_blocks(J, ncp, gauge=7):
    """(pinv(J^T J)_cc, the 3 x 3 diagonal blocks of pinv(J^T J)_pp, eigenvalues ascending) by eigh with the ``gauge`` smallest eigenvalues zeroed."""
    lam, Q = np.linalg.eigh(J.T @ J)
    inv = np.zeros_like(lam)
    inv[gauge:] = 1.0 / lam[gauge:]
    P = (Q * inv) @ Q.T
    n_pts = (J.shape[1] - ncp) // 3
    pp = np.stack([P[ncp + 3 * i: ncp + 3 * i + 3, ncp + 3 * i: ncp + 3 * i + 3] for i in range(n_pts)])
    return P[:ncp, :ncp], pp, lam


def _rodrigues_pair(r):
    from caliscope_amd.uncertainty import rotation_and_left_jacobian

    return rotation_and_left_jacobian(r)


def gauge_matrix(par, x):
    """N (n_params x 7) in numpy, from the table of the header."""
    ncp = par.n_camera_params
    N = np.zeros((len(x), 7))
    for blk, off in zip(par.blocks, par.camera_param_offsets):
        R, Jl = _rodrigues_pair(x[off: off + 3])
        N[off: off + 3, 3:6] = -np.linalg.solve(Jl, R)
        N[off + 3: off + 6, 0:3] = -R
        N[off + 3: off + 6, 6] = x[off + 3: off + 6]
    pts = x[ncp:].reshape(-1, 3)
    for i, X in enumerate(pts):
        rows = slice(ncp + 3 * i, ncp + 3 * i + 3)
        N[rows, 0:3] = np.eye(3)
        N[rows, 3:6] = -np.array([[0.0, -X[2], X[1]], [X[2], 0.0, -X[0]], [-X[1], X[0], 0.0]])
        N[rows, 6] = X
    return N


def bordered_blocks(J, N, ncp):
    """The bordered formula of the header in numpy: (pinv_cc, 3 x 3 diagonal blocks of pinv_pp)."""
    H = J.T @ J
    U, W = H[:ncp, :ncp], H[:ncp, ncp:]
    n_pts = (J.shape[1] - ncp) // 3
    Vinv = np.zeros((3 * n_pts, 3 * n_pts))
    for i in range(n_pts):
        s = slice(ncp + 3 * i, ncp + 3 * i + 3)
        Vinv[3 * i: 3 * i + 3, 3 * i: 3 * i + 3] = np.linalg.inv(H[s, s])
    Nc, Np = N[:ncp], N[ncp:]
    Y = W @ Vinv
    Z = Vinv @ Np
    D = Np.T @ Z
    B = Nc - W @ Z
    Dinv = np.linalg.inv(D)
    St = U - Y @ W.T + B @ Dinv @ B.T
    C = np.linalg.inv(0.5 * (St + St.T))
    pp = np.zeros((n_pts, 3, 3))
    for i in range(n_pts):
        s = slice(3 * i, 3 * i + 3)
        T = Y[:, s].T + Z[s] @ Dinv @ B.T
        pp[i] = Vinv[s, s] - Z[s] @ Dinv @ Z[s].T + T @ C @ T.T
    return C, pp


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _rel_blocks(a, b):
    return float(np.max(np.max(np.abs(a - b), axis=(1, 2)) / np.max(np.abs(b), axis=(1, 2))))


@functools.lru_cache(maxsize=None)
def _reference(key, loss, f_scale):
    sc = key_scene(key)
    J, cost = robust_jacobian(sc, loss, f_scale)
    ncp = sc["par"].n_camera_params
    cc, pp, lam = pinv_blocks(J, ncp)
    bc, bp = bordered_blocks(J, gauge_matrix(sc["par"], sc["x"]), ncp)
    dof = J.shape[0] - J.shape[1] + 7
    return dict(cc=cc, pp=pp, lam=lam, dis_c=_rel(bc, cc), dis_p=_rel_blocks(bp, pp), sigma0_sq=2.0 * cost / dof, dof=dof, cost=cost)


_SCENES = {}
SCENE_BUILDERS = {"small": scene, "wide": wide_scene, "ragged": ragged_scene}  # (tests/covariance_edge_scenes.py adds its own)


def key_scene(key):
    """Scenes by hashable key, built once and never written to: ("small", n_cams, n_points, k, refine, loss, outliers),
    ("wide", widths, fisheye_six[, n_points]), ("ragged",), and the keys of the builders other modules put into SCENE_BUILDERS."""
    if key not in _SCENES:
        _SCENES[key] = SCENE_BUILDERS[key[0]](*key[1:])
    return _SCENES[key]


def reference(key, loss="linear", f_scale=1.0):
    """The pinv reference of a scene and the disagreement of the two CPU formulations, computed once and shared."""
    return _reference(key, loss, float(f_scale))


def check_result_against_pinv(result, ref, par, gauge, report=print, **labels):
    """The tolerance rule, for a reference of ``gauge`` null directions (7, or 6 with constraint rows: tests/covariance_constrained_native.py):
    exactly ``gauge`` eigenvalues below 1e-12 lambda_max; the two CPU formulations agree to 1e-8 (the scene is strong enough to test with: a
    weak one cannot widen the tolerance); the code under test differs from the pinv by at most ten times their disagreement, with a floor of
    1e-12, relative to the block-wise max-norm; dof equal, cost and sigma0^2 to 1e-12 relative; the per-camera blocks are those of the full
    matrix, zero-padded.  Returns the measured figures (``labels`` in front; the first eigenvalue behind the gauge as lam<gauge + 1>)."""
    lam = ref["lam"]
    assert int(np.sum(lam < 1e-12 * lam[-1])) == gauge, lam[:9] / lam[-1]
    assert ref["dis_c"] <= 1e-8 and ref["dis_p"] <= 1e-8, (ref["dis_c"], ref["dis_p"])
    s2 = ref["sigma0_sq"]
    err_c = _rel(result.cam_cov_full, s2 * ref["cc"])
    err_p = _rel_blocks(result.point_cov, s2 * ref["pp"])
    figures = dict(**labels, dis_c=ref["dis_c"], dis_p=ref["dis_p"], err_c=err_c, err_p=err_p, **{f"lam{gauge + 1}": float(lam[gauge] / lam[-1])})
    report(figures)
    assert result.dof == ref["dof"]
    assert abs(result.cost - ref["cost"]) <= 1e-12 * ref["cost"] and abs(result.sigma0_sq - s2) <= 1e-12 * s2
    assert err_c <= max(10.0 * ref["dis_c"], 1e-12), figures
    assert err_p <= max(10.0 * ref["dis_p"], 1e-12), figures
    for i, (blk, off) in enumerate(zip(par.blocks, par.camera_param_offsets)):  # the per-camera blocks are those of the full matrix
        n = blk.n_params
        assert np.array_equal(result.cam_cov[i, :n, :n], result.cam_cov_full[off: off + n, off: off + n])
        assert not result.cam_cov[i, n:].any() and not result.cam_cov[i, :, n:].any()
    return figures


def check_against_pinv(result, key, loss="linear", f_scale=1.0, report=print):
    """check_result_against_pinv for a scene of this module (seven null directions).  Returns the measured figures."""
    return check_result_against_pinv(result, reference(key, loss, f_scale), key_scene(key)["par"], 7, report, key=key, loss=loss)
