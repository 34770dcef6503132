"""g++ build of caliscope_amd/csrc/reliability_math.h (tests/native/reliability_harness.cpp), a `_solver` hook for
CaptureVolume.observation_reliability that runs on it, and what the reliability tests share: the two CPU formulations of the 2 x 2
redundancy blocks — (a) the dense projector from the float64 eigh pseudo-inverse of the oracle's J^T J (the reference), (b) the block
formula of include/caliscope/reliability.h in numpy with C from covariance_native.bordered_blocks (the disagreement of the two is the
yardstick of the tolerance) — and the comparison itself.  Scenes are those of tests/covariance_native.py, by key."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.reliability import RelOut, run_reliability_call
from caliscope_amd.uncertainty import CovDesc, check_covariance_arguments
from tests import covariance_native as cn
from tests.native_build import CSRC, NATIVE, load_native

F64 = C.POINTER(C.c_double)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "reliability_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.rh_last_error.restype = C.c_char_p
    lib.rh_constants.restype = None
    lib.rh_constants.argtypes = [F64]
    lib.rh_w.restype = C.c_double
    lib.rh_w.argtypes = [C.c_double, C.c_double, C.c_double]
    lib.rh_observation_reliability.restype = C.c_int
    lib.rh_observation_reliability.argtypes = [C.POINTER(CovDesc), C.POINTER(RelOut)]
    return lib


class HarnessReliability:
    """The `_solver` hook on the g++ build: same arguments, checks, result and error type as caliscope_amd.reliability.DeviceReliability."""

    def __init__(self):
        self.calls = 0

    def observation_reliability(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, *, loss="linear", f_scale=1.0):
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        self.calls += 1
        lib = harness()
        return run_reliability_call(lib.rh_observation_reliability, args, "cba_observation_reliability", lambda: lib.rh_last_error().decode())


def scene_arguments(key):
    sc = cn.key_scene(key)
    return cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"])


# ---- the two CPU formulations -----------------------------------------------------------------------------------------------------------
def scaled_residuals(sc, loss="linear", f_scale=1.0):
    """The oracle's residuals, (n_obs, 2), scaled for the loss as scipy's least_squares scales them (f rho' / sqrt(rho' + 2 rho'' f^2)),
    and the derivative of the scaled residual with respect to the residual (1 for the linear loss; soft_l1: f~ = f t^(1/4) with
    t = 1 + (f / f_scale)^2, so t^(1/4) (1 + z / (2 t)))."""
    from oracle.residuals import joint_residuals

    f = joint_residuals(sc["x"], sc["par"], sc["cam"], sc["uv"], sc["obj"])
    amp = np.ones_like(f)
    if loss != "linear":
        assert loss == "soft_l1"
        z = (f / f_scale) ** 2
        t = 1.0 + z
        rho1, rho2 = t ** -0.5, -0.5 * t ** -1.5
        f = f * rho1 / np.sqrt(np.maximum(rho1 + 2.0 * rho2 * z, np.finfo(float).eps))
        amp = t ** 0.25 * (1.0 + 0.5 * z / t)
    return f.reshape(-1, 2), amp.reshape(-1, 2)


def dense_blocks(J):
    """(a): the 2 x 2 diagonal blocks of R = I - J Q+ L+^-1 Q+^T J^T, eigh of J^T J with the seven smallest eigenvalues zeroed; and the
    eigenvalues, ascending."""
    lam, Q = np.linalg.eigh(J.T @ J)
    M = (J @ Q[:, 7:]) / np.sqrt(lam[7:])
    M = M.reshape(-1, 2, M.shape[1])
    return np.eye(2) - np.einsum("oik,ojk->oij", M, M), lam


def formula_blocks(J, N, ncp, cam_of_obs, pt_of_obs, offsets):
    """(b): R_oo = I - P_oo by the block formula of the header, C from the bordered system (covariance_native.bordered_blocks)."""
    Cm, _ = cn.bordered_blocks(J, N, ncp)
    H = J.T @ J
    W = H[:ncp, ncp:]
    n_pts = (J.shape[1] - ncp) // 3
    Vinv = [np.linalg.inv(H[ncp + 3 * i: ncp + 3 * i + 3, ncp + 3 * i: ncp + 3 * i + 3]) for i in range(n_pts)]
    out = np.empty((len(cam_of_obs), 2, 2))
    CY = {}
    for o, (a, i) in enumerate(zip(cam_of_obs, pt_of_obs)):
        if i not in CY:
            Yi = W[:, 3 * i: 3 * i + 3] @ Vinv[i]       # every Y_b of the point, stacked at its camera's rows
            G = Cm @ Yi                                 # G_o = its rows at camera a
            CY[i] = (G, Vinv[i] + Yi.T @ G)
        G, K = CY[i]
        rows = slice(offsets[a], offsets[a + 1])
        A, B = J[2 * o: 2 * o + 2, rows], J[2 * o: 2 * o + 2, ncp + 3 * i: ncp + 3 * i + 3]
        AGB = A @ G[rows] @ B.T
        out[o] = np.eye(2) - (B @ K @ B.T + A @ Cm[rows, rows] @ A.T - AGB - AGB.T)
    return out


@functools.lru_cache(maxsize=None)
def _reference(key, loss, f_scale):
    sc = cn.key_scene(key)
    J, cost = cn.robust_jacobian(sc, loss, f_scale)
    par = sc["par"]
    ncp = par.n_camera_params
    Ra, lam = dense_blocks(J)
    offsets = list(par.camera_param_offsets) + [ncp]
    Rb = formula_blocks(J, cn.gauge_matrix(par, sc["x"]), ncp, sc["cam"], sc["obj"], offsets)
    dof = J.shape[0] - J.shape[1] + 7
    s2 = 2.0 * cost / dof
    f, amp = scaled_residuals(sc, loss, f_scale)
    r = np.stack([Ra[:, 0, 0], Ra[:, 1, 1]], axis=1)
    for a in (Ra, r, f, amp):
        a.setflags(write=False)
    return dict(R=Ra, r=r, f=f, amp=amp, lam=lam, dis=float(np.max(np.abs(Ra - Rb))), sigma0_sq=s2, dof=dof, cost=cost)


def reference(key, loss="linear", f_scale=1.0):
    """The dense reference of a scene and the disagreement of the two CPU formulations, computed once, shared and read-only."""
    return _reference(key, loss, float(f_scale))


# What separates the residual of the code under test from the oracle's is rounding alone: both evaluate (projection - observation) / fx0
# with projections and observations of up to 2000 pixels in float64 (eps 2.2e-16) over a few dozen operations, so 64 eps of the largest
# coordinate, in residual units, bounds the difference of the residuals with room for the order of the operations.  A robust loss passes
# that difference through the scaling (times its derivative `amp`) and adds the rounding of a square root, a division and two products
# to the scaled value (16 eps of it).
def residual_tolerance(args, ref):
    base = 64.0 * np.finfo(float).eps * max(2000.0, float(np.abs(args[7]).max())) / float(np.min(args[2][:, 0]))
    return base * ref["amp"] + 16.0 * np.finfo(float).eps * np.abs(ref["f"])


def check_against_dense(result, key, loss="linear", f_scale=1.0, report=print):
    """The tolerance rule: exactly seven eigenvalues below 1e-12 lambda_max; the two CPU formulations agree to 1e-8, absolute on R_oo (the
    scene is strong enough to test with); the code under test differs from (a) by at most tol = max(ten times their disagreement, 1e-12),
    absolute, on every entry of every R_oo — no row is left out.  sum r = dof to 1e-9 dof; R_oo symmetric positive semi-definite and
    r_j <= 1 within tol.  The residuals match the oracle's to rounding (residual_tolerance).  w, row by row and relative, within tol / r_j
    of f~_j / (sigma0 sqrt(r_j)) with r_j and sigma0 of the REFERENCE (first-order propagation through 1 / sqrt(r)) and the residual the
    call returned, which the line before tied to the oracle's: a residual of 1e-7 pixels carries a relative rounding error far above
    1e-12 whoever computes it, and that is not what the rule on w is about.  The difference to the w formed from the oracle's own residual
    is printed (w_oracle_abs, in units of w).  Returns the measured figures."""
    ref = reference(key, loss, f_scale)
    lam = ref["lam"]
    assert int(np.sum(lam < 1e-12 * lam[-1])) == 7, lam[:9] / lam[-1]
    assert ref["dis"] <= 1e-8, ref["dis"]
    tol = max(10.0 * ref["dis"], 1e-12)
    R, r_ref, s2 = result.redundancy, ref["r"], ref["sigma0_sq"]
    assert R.shape == ref["R"].shape and result.w.shape == r_ref.shape and result.residual.shape == r_ref.shape
    err_R = float(np.max(np.abs(R - ref["R"])))
    r = np.stack([R[:, 0, 0], R[:, 1, 1]], axis=1)
    err_f = float(np.max(np.abs(result.residual - ref["f"]) / residual_tolerance(scene_arguments(key), ref)))  # in units of its tolerance
    w_ref = result.residual / np.sqrt(s2 * r_ref)
    err_w = float(np.max(np.abs(result.w - w_ref) * r_ref / np.abs(w_ref)))  # in units of tol: |dw| / |w| <= tol / r_j
    w_oracle = float(np.nanmax(np.abs(result.w - ref["f"] / np.sqrt(s2 * r_ref))))
    sum_r = float(r.sum())
    min_eig = float(np.min(np.linalg.eigvalsh(R)))
    figures = dict(key=key, loss=loss, dis=ref["dis"], tol=tol, err_R=err_R, err_w_times_r=err_w, err_f_over_tol=err_f, w_oracle_abs=w_oracle,
                   sum_r_minus_dof=sum_r - ref["dof"], min_r=float(r_ref.min()), share_below_001=float(np.mean(r_ref < 0.01)), min_eig=min_eig,
                   max_r=float(r.max()), max_abs_w=float(np.nanmax(np.abs(result.w))), lam8=float(lam[7] / lam[-1]))
    report(figures)
    assert r_ref.min() > 1e-10  # (REL_R_TINY: no reference row is uncontrolled on the scenes of these tests)
    assert result.n_uncontrolled == 0 and not np.isnan(result.w).any()
    assert result.dof == ref["dof"]
    assert abs(result.cost - ref["cost"]) <= 1e-12 * ref["cost"] and abs(result.sigma0_sq - s2) <= 1e-12 * s2
    assert err_R <= tol, figures
    assert abs(sum_r - ref["dof"]) <= 1e-9 * ref["dof"], figures
    assert np.array_equal(R[:, 0, 1], R[:, 1, 0]) and min_eig >= -tol and r.max() <= 1.0 + tol, figures
    assert err_f <= 1.0, figures
    assert err_w <= tol, figures
    return figures
