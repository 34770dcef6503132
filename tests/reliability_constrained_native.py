"""g++ build of caliscope_amd/csrc/reliability_constraint_math.h (tests/native/reliability_constrained_harness.cpp), a `_solver` hook on it,
and what the tests of the constrained reliability share: the scenes of tests/covariance_constrained_native.py (and one more), the two CPU
formulations of the projector's diagonal with the constraint rows in J — (a) the dense projector from the float64 eigh pseudo-inverse of the
oracle's J^T J with SIX eigenvalues zeroed (the reference), (b) the block formula of include/caliscope/reliability_constrained.h in numpy
with a dense V~^-1 — and the comparison by the rule of tests.reliability_native.check_against_dense with six for seven and the constraint
rows included."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.reliability import RelConOut, RelOut, run_reliability_constrained_call
from caliscope_amd.uncertainty import CovConstraints, CovDesc, check_constraint_arguments, check_covariance_arguments, constraint_struct
from tests import covariance_constrained_native as ccn
from tests import covariance_native as cn
from tests import reliability_native as rn
from tests.native_build import CSRC, NATIVE, load_native

WHAT = "cba_observation_reliability_constrained"
EPS = float(np.finfo(float).eps)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "reliability_constrained_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.rch_last_error.restype = C.c_char_p
    lib.rch_observation_reliability_constrained.restype = C.c_int
    lib.rch_observation_reliability_constrained.argtypes = [C.POINTER(CovDesc), C.POINTER(CovConstraints), C.POINTER(RelOut), C.POINTER(RelConOut),
                                                            C.POINTER(C.c_int32)]
    return lib


def last_error():
    return harness().rch_last_error().decode()


class HarnessConstrainedReliability:
    """The `_solver` hook on the g++ build: same arguments, checks, result and error type as caliscope_amd.reliability.DeviceReliability."""

    def __init__(self):
        self.calls = 0
        self.constrained_calls = 0

    def observation_reliability(self, *eight, loss="linear", f_scale=1.0):
        return self.observation_reliability_constrained(*eight, None, None, None, None, loss=loss, f_scale=f_scale)

    def observation_reliability_constrained(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, groups_a, groups_b, distances,
                                            weights, *, loss="linear", f_scale=1.0, null_struct=False):
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        con = check_constraint_arguments(groups_a, groups_b, distances, weights)
        struct = None if null_struct else constraint_struct(con)
        self.calls += 1
        self.constrained_calls += con is not None
        lib = harness()
        gauge = C.c_int32(0)
        res = run_reliability_constrained_call(
            lambda d, o, c: lib.rch_observation_reliability_constrained(d, C.byref(struct) if struct is not None else None, o, c, C.byref(gauge)), args,
            None if null_struct else con, WHAT, last_error)
        assert gauge.value == res.gauge_dim  # what the binding reports is what the plan did
        return res


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
REPEAT = ("repeat", 70)  # DEFAULT with one (camera, point) pair of a component there 70 times: more observations of a point than lanes
REPEAT_PAIR = (1, 17)    # camera 1's observation of frame 1, corner 5

_SCENES = {}


def key_scene(key):
    """covariance_constrained_native.key_scene, REPEAT, and whatever a test has put into _SCENES under a key of its own.  Built once and never
    written to."""
    if key in _SCENES:
        return _SCENES[key]
    if key[0] != "repeat":
        return ccn.key_scene(key)
    if key not in _SCENES:
        sc = dict(ccn.key_scene(ccn.DEFAULT))
        at = int(np.flatnonzero((sc["cam"] == REPEAT_PAIR[0]) & (sc["obj"] == REPEAT_PAIR[1]))[0])
        order = np.concatenate([np.arange(len(sc["cam"])), np.full(key[1] - 1, at)])
        sc.update(cam=np.ascontiguousarray(sc["cam"][order]), obj=np.ascontiguousarray(sc["obj"][order]), uv=np.ascontiguousarray(sc["uv"][order]))
        _SCENES[key] = sc
    return _SCENES[key]


def call_arguments(key):
    """The twelve positional arguments of ``observation_reliability_constrained``."""
    sc = key_scene(key)
    ga, gb, dist, w = sc["con"]
    return (*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]), ga, gb, dist, w)


# ---- the two CPU formulations -----------------------------------------------------------------------------------------------------------
def scale_for_loss(f, loss, f_scale):
    """(f~, d f~ / d f) as tests.reliability_native.scaled_residuals forms them, for any residual vector."""
    f = np.asarray(f, dtype=np.float64)
    if loss == "linear":
        return f.copy(), np.ones_like(f)
    assert loss == "soft_l1"
    z = (f / f_scale) ** 2
    t = 1.0 + z
    rho1, rho2 = t ** -0.5, -0.5 * t ** -1.5
    return f * rho1 / np.sqrt(np.maximum(rho1 + 2.0 * rho2 * z, EPS)), t ** 0.25 * (1.0 + 0.5 * z / t)


def dense_diagonal(J, n_obs):
    """(a): the 2 x 2 diagonal blocks of R = I - J pinv(J^T J) J^T on the observation rows and its diagonal on the constraint rows, eigh of
    J^T J with the six smallest eigenvalues zeroed; and the eigenvalues, ascending."""
    lam, Q = np.linalg.eigh(J.T @ J)
    M = (J @ Q[:, 6:]) / np.sqrt(lam[6:])
    Mo = M[: 2 * n_obs].reshape(n_obs, 2, -1)
    return np.eye(2) - np.einsum("oik,ojk->oij", Mo, Mo), 1.0 - np.einsum("jk,jk->j", M[2 * n_obs:], M[2 * n_obs:]), lam


def formula_diagonal(J, N6, ncp, n_obs):
    """(b): the same from G^- = [[C, -C Y], [-Y^T C, V~^-1 + Y^T C Y]] with V~ inverted densely and C from the bordered system with six columns."""
    Cm, _ = ccn.bordered_blocks(J, N6, ncp)
    H = J.T @ J
    W, Vinv = H[:ncp, ncp:], np.linalg.inv(H[ncp:, ncp:])
    Y = W @ Vinv
    CY = Cm @ Y
    Gm = np.block([[Cm, -CY], [-CY.T, Vinv + Y.T @ CY]])
    JG = J @ Gm
    Jo, JGo = J[: 2 * n_obs].reshape(n_obs, 2, -1), JG[: 2 * n_obs].reshape(n_obs, 2, -1)
    P = np.einsum("oik,ojk->oij", JGo, Jo)
    return np.eye(2) - 0.5 * (P + P.transpose(0, 2, 1)), 1.0 - np.einsum("jk,jk->j", JG[2 * n_obs:], J[2 * n_obs:])


@functools.lru_cache(maxsize=None)
def _reference(key, loss, f_scale):
    sc = key_scene(key)
    J, cost, js, f = ccn.robust_jacobian(sc, loss, f_scale)
    par = sc["par"]
    ncp, n_obs = par.n_camera_params, len(sc["cam"])
    Ra, rca, lam = dense_diagonal(J, n_obs)
    Rb, rcb = formula_diagonal(J, cn.gauge_matrix(par, sc["x"])[:, :6], ncp, n_obs)
    dof = J.shape[0] - J.shape[1] + 6
    fo, amp = scale_for_loss(f[: 2 * n_obs], loss, f_scale)
    fc, ampc = scale_for_loss(f[2 * n_obs:], loss, f_scale)
    out = dict(R=Ra, r=np.stack([Ra[:, 0, 0], Ra[:, 1, 1]], axis=1), rc=rca, f=fo.reshape(-1, 2), amp=amp.reshape(-1, 2), fc=fc, ampc=ampc, lam=lam,
               dis=float(max(np.max(np.abs(Ra - Rb)), np.max(np.abs(rca - rcb)))), sigma0_sq=2.0 * cost / dof, dof=dof, cost=cost)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def reference(key, loss="linear", f_scale=1.0):
    """The dense reference of a scene and the disagreement of the two CPU formulations, computed once, shared and read-only."""
    return _reference(key, loss, float(f_scale))


# A constraint residual is weight * (length - distance) with the length formed from eight points' coordinates in a few dozen float64
# operations: 64 eps of the largest coordinate or distance, times the weight, bounds the difference to the oracle's with room for the
# order of the operations; a robust loss passes it through the scaling (times `ampc`) and adds the rounding of the scaling itself
# (16 eps of the value), as tests.reliability_native.residual_tolerance argues for the reprojection rows.
def constraint_residual_tolerance(sc, ref):
    _, _, dist, w = sc["con"]
    return 64.0 * EPS * max(float(np.abs(sc["x"][sc["par"].n_camera_params:]).max()), float(np.max(dist))) * w * ref["ampc"] + 16.0 * EPS * np.abs(ref["fc"])


def check_against_dense(result, key, loss="linear", f_scale=1.0, report=print):
    """The rule of tests.reliability_native.check_against_dense with six null eigenvalues and the constraint rows included: exactly six
    eigenvalues below 1e-12 lambda_max; the two CPU formulations agree to 1e-8, absolute, on every R_oo and every constraint r_j; the code
    under test differs from (a) by at most tol = max(ten times their disagreement, 1e-12), absolute, on every entry of every R_oo and on
    every constraint r_j — no row is left out.  sum r over ALL rows = dof to 1e-9 dof.  The residuals match the oracle's to rounding; w,
    row by row and relative, within tol / r_j of f~_j / (sigma0 sqrt(r_j)) with r_j and sigma0 of the reference and the residual the call
    returned.  Every constraint row of these scenes has positive weight.  Returns the measured figures."""
    sc, ref = key_scene(key), reference(key, loss, f_scale)
    lam = ref["lam"]
    assert int(np.sum(lam < 1e-12 * lam[-1])) == 6, lam[:8] / lam[-1]
    assert ref["dis"] <= 1e-8, ref["dis"]
    tol = max(10.0 * ref["dis"], 1e-12)
    assert result.gauge_dim == 6
    R, r_ref, rc_ref, s2 = result.redundancy, ref["r"], ref["rc"], ref["sigma0_sq"]
    rc = result.constraint_redundancy
    assert R.shape == ref["R"].shape and result.w.shape == r_ref.shape and result.residual.shape == r_ref.shape
    assert rc.shape == rc_ref.shape == result.constraint_w.shape == result.constraint_residual.shape
    err_R, err_rc = float(np.max(np.abs(R - ref["R"]))), float(np.max(np.abs(rc - rc_ref)))
    r = np.stack([R[:, 0, 0], R[:, 1, 1]], axis=1)
    eight = call_arguments(key)[:8]
    err_f = float(np.max(np.abs(result.residual - ref["f"]) / rn.residual_tolerance(eight, ref)))  # in units of its tolerance
    err_fc = float(np.max(np.abs(result.constraint_residual - ref["fc"]) / constraint_residual_tolerance(sc, ref)))
    w_ref = result.residual / np.sqrt(s2 * r_ref)
    wc_ref = result.constraint_residual / np.sqrt(s2 * rc_ref)
    with np.errstate(invalid="ignore", divide="ignore"):  # (a residual of exactly zero: w and its reference are both zero)
        err_w = float(np.nanmax(np.where(w_ref == 0.0, np.abs(result.w), np.abs(result.w - w_ref) * r_ref / np.abs(w_ref))))
        err_wc = float(np.nanmax(np.where(wc_ref == 0.0, np.abs(result.constraint_w), np.abs(result.constraint_w - wc_ref) * rc_ref / np.abs(wc_ref))))
    sum_r = float(r.sum() + rc.sum())
    min_eig = float(np.min(np.linalg.eigvalsh(R)))
    figures = dict(key=key, loss=loss, dis=ref["dis"], tol=tol, err_R=err_R, err_rc=err_rc, err_w_times_r=err_w, err_wc_times_r=err_wc, err_f_over_tol=err_f,
                   err_fc_over_tol=err_fc, sum_r_minus_dof=sum_r - ref["dof"], min_r=float(r_ref.min()), min_rc=float(rc_ref.min()), min_eig=min_eig,
                   max_r=float(max(r.max(), rc.max())), max_abs_w=float(np.nanmax(np.abs(result.w))), max_abs_wc=float(np.nanmax(np.abs(result.constraint_w))),
                   lam7=float(lam[6] / lam[-1]))
    report(figures)
    assert min(r_ref.min(), rc_ref.min()) > 1e-10  # (REL_R_TINY: no reference row is uncontrolled on the scenes of these tests)
    assert result.n_uncontrolled == 0 and result.n_constraints_uncontrolled == 0
    assert not np.isnan(result.w).any() and not np.isnan(result.constraint_w).any()
    assert result.dof == ref["dof"]
    assert abs(result.cost - ref["cost"]) <= 1e-12 * ref["cost"] and abs(result.sigma0_sq - s2) <= 1e-12 * s2
    assert err_R <= tol and err_rc <= tol, figures
    assert abs(sum_r - ref["dof"]) <= 1e-9 * ref["dof"], figures
    assert np.array_equal(R[:, 0, 1], R[:, 1, 0]) and min_eig >= -tol and max(r.max(), rc.max()) <= 1.0 + tol, figures
    assert err_f <= 1.0 and err_fc <= 1.0, figures
    assert err_w <= tol and err_wc <= tol, figures
    return figures
