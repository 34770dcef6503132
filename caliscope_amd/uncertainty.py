"""How well the observations determine every camera and every point: the free-network covariance in one device call.

Reprojection RMS says how well a calibration fits, not how well the data pin it down: a rig can fit to 0.3 px and still have a
camera whose depth is barely constrained.  ``cba_parameter_covariance`` (``include/caliscope/uncertainty.h``,
``csrc/covariance_math.h``, ``csrc/covariance_lib.hip``) returns the covariance of the bundle-adjustment parameters in the
inner-constraint (minimum-trace, free-network) gauge, ``sigma0^2 pinv(J^T J)``, with ``J`` the Jacobian the solver uses: the
camera blocks from a dense factorisation of the reduced camera system bordered by the seven gauge directions, the point blocks
from a 3 x 3 formula per point.  :meth:`CaptureVolume.parameter_uncertainty` is built on it and returns an
:class:`UncertaintyReport`: per camera the covariance of its parameters, of its centre (world units) and the standard deviation of
its orientation (degrees), per world point its covariance.  The reference computes no covariance.

Scope: reprojection rows, and with ``parameter_covariance_constrained`` (``include/caliscope/uncertainty_constrained.h``) the
rigid-distance rows of a ``ConstraintSet`` too: the rows couple the points of a board (one connected component per board in a frame,
at most 54 points each) and fix the scale, so the gauge then has six columns (``gauge_dim == 6``) and the rows count in ``dof``.
``CaptureVolume.parameter_uncertainty(include_constraints=True)`` takes that path, and so does ``observation_reliability(include_constraints=True)`` (``caliscope_amd/reliability.py``).

There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.  ``_solver`` of the method replaces the
device call (an object with ``parameter_covariance``, as :class:`DeviceUncertainty`) — the CPU test-suite passes a g++ build of the
same arithmetic.

The sums behind every output are added with floating-point atomics in the order of arrival: results vary in their last bits from
run to run.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError

LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}


class CovDesc(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_points", C.c_int64), ("n_obs", C.c_int64), ("cam_model", _lib.c_int32_p), ("cam_nparams", _lib.c_int32_p),
                ("cam_const", _lib.c_double_p), ("cam_x", _lib.c_double_p), ("points", _lib.c_double_p), ("obs_cam", _lib.c_int32_p),
                ("obs_pt", _lib.c_int32_p), ("obs_uv", _lib.c_double_p), ("loss", C.c_int32), ("f_scale", C.c_double)]


class CovOut(C.Structure):
    _fields_ = [("cam_cov", _lib.c_double_p), ("cam_cov_full", _lib.c_double_p), ("point_cov", _lib.c_double_p), ("sigma0_sq", _lib.c_double_p),
                ("dof", _lib.c_int64_p), ("cost", _lib.c_double_p)]


class CovConstraints(C.Structure):
    _fields_ = [("n_con", C.c_int32), ("groups_a", _lib.c_int32_p), ("groups_b", _lib.c_int32_p), ("distances", _lib.c_double_p),
                ("weights", _lib.c_double_p)]


UNCERTAINTY_SIGNATURES = {
    "cba_parameter_covariance": (C.c_int, [C.POINTER(CovDesc), C.c_int32, C.POINTER(CovOut)]),
}
# include/caliscope/uncertainty_constrained.h
CONSTRAINED_UNCERTAINTY_SIGNATURES = {
    "cba_parameter_covariance_constrained": (C.c_int, [C.POINTER(CovDesc), C.POINTER(CovConstraints), C.c_int32, C.POINTER(CovOut)]),
}


@dataclass(frozen=True)
class CovarianceResult:
    """What one ``parameter_covariance`` call returns: ``cam_cov`` (n_cams, 9, 9) with the upper-left nparams x nparams used,
    ``cam_cov_full`` (ncp, ncp), ``point_cov`` (n_points, 3, 3), ``cam_offsets`` (n_cams + 1) into the rows of ``cam_cov_full``.
    ``gauge_dim`` is 7 (translation, rotation, scale) or, with ``n_constraint_rows`` > 0 distance rows of positive weight, 6."""

    cam_cov: np.ndarray
    cam_cov_full: np.ndarray
    point_cov: np.ndarray
    cam_offsets: np.ndarray
    sigma0_sq: float
    dof: int
    cost: float
    gauge_dim: int = 7
    n_constraint_rows: int = 0


def check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale):
    """The arguments of a ``parameter_covariance`` call in the layout of ``cba_cov_desc``, as a dict (``ValueError`` for an unknown
    loss, arrays of the wrong shape or mismatched lengths; the range of every index, the observation counts and the degrees of
    freedom are the library's check)."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {sorted(LOSSES)}, got {loss!r}")
    cam_model = np.ascontiguousarray(cam_model, dtype=np.int32).reshape(-1)
    n_cams = len(cam_model)
    cam_nparams = np.ascontiguousarray(cam_nparams, dtype=np.int32).reshape(-1)
    cam_const = np.ascontiguousarray(cam_const, dtype=np.float64).reshape(-1, 12)
    cam_x = np.ascontiguousarray(cam_x, dtype=np.float64).reshape(-1, 9)
    if len(cam_nparams) != n_cams or len(cam_const) != n_cams or len(cam_x) != n_cams:
        raise ValueError("parameter_covariance: cam_model, cam_nparams, cam_const and cam_x differ in length")
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    obs_pt = np.ascontiguousarray(obs_pt, dtype=np.int32).reshape(-1)
    obs_uv = np.ascontiguousarray(obs_uv, dtype=np.float64).reshape(-1, 2)
    if len(obs_pt) != len(obs_cam) or len(obs_uv) != len(obs_cam):
        raise ValueError("parameter_covariance: obs_cam, obs_pt and obs_uv differ in length")
    return dict(cam_model=cam_model, cam_nparams=cam_nparams, cam_const=cam_const, cam_x=cam_x, points=points, obs_cam=obs_cam, obs_pt=obs_pt,
                obs_uv=obs_uv, loss=LOSSES[loss], f_scale=float(f_scale))


def check_constraint_arguments(groups_a, groups_b, distances, weights):
    """The constraint rows of a ``parameter_covariance_constrained`` call in the layout of ``cba_cov_constraints``, as a dict
    (``ValueError`` for arrays of the wrong shape or mismatched lengths; the range of every index and the sign and finiteness of every
    weight and distance are the library's check).  All ``None``: no rows."""
    if groups_a is None and groups_b is None and distances is None and weights is None:
        return None
    if groups_a is None or groups_b is None or distances is None or weights is None:
        raise ValueError("parameter_covariance_constrained: groups_a, groups_b, distances and weights go together")
    groups_a = np.ascontiguousarray(groups_a, dtype=np.int32)
    groups_b = np.ascontiguousarray(groups_b, dtype=np.int32)
    distances = np.ascontiguousarray(distances, dtype=np.float64).reshape(-1)
    weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    n_con = len(distances)
    if groups_a.shape != (n_con, 4) or groups_b.shape != (n_con, 4) or len(weights) != n_con:
        raise ValueError(f"parameter_covariance_constrained: groups_a and groups_b must be ({n_con}, 4) and weights ({n_con},), got "
                         f"{groups_a.shape}, {groups_b.shape}, {weights.shape}")
    return dict(groups_a=groups_a, groups_b=groups_b, distances=distances, weights=weights)


def constraint_struct(con: dict | None):
    """``cba_cov_constraints`` over the arrays of ``check_constraint_arguments`` (the dict keeps them alive), or None."""
    if con is None:
        return None
    return CovConstraints(n_con=len(con["distances"]), groups_a=_lib.ptr(con["groups_a"]), groups_b=_lib.ptr(con["groups_b"]),
                          distances=_lib.ptr(con["distances"]), weights=_lib.ptr(con["weights"]))


def run_covariance_call(call, args: dict, what: str, last_error, n_constraint_rows: int = 0) -> CovarianceResult:
    """Fill ``cba_cov_desc`` / ``cba_cov_out`` from checked arguments, run ``call(desc_ref, out_ref) -> code`` and collect the result
    (shared by the device binding and the test harness: same structures, same error type and message).  ``n_constraint_rows``: the
    distance rows of positive weight the call was given; any makes the gauge six-dimensional."""
    n_cams, n_points = len(args["cam_model"]), len(args["points"])
    widths = np.where((args["cam_nparams"] == 6) | (args["cam_nparams"] == 9), args["cam_nparams"], 0).astype(np.int64)  # (others: refused by the call)
    offsets = np.concatenate([[0], np.cumsum(widths)])
    ncp = int(offsets[-1])
    cam_cov, cam_cov_full, point_cov = np.zeros((n_cams, 9, 9)), np.zeros((ncp, ncp)), np.zeros((n_points, 6))
    sigma0_sq, dof, cost = np.zeros(1), np.zeros(1, dtype=np.int64), np.zeros(1)
    desc = CovDesc(n_cams=n_cams, n_points=n_points, n_obs=len(args["obs_cam"]), cam_model=_lib.ptr(args["cam_model"]),
                   cam_nparams=_lib.ptr(args["cam_nparams"]), cam_const=_lib.ptr(args["cam_const"]), cam_x=_lib.ptr(args["cam_x"]),
                   points=_lib.ptr(args["points"]), obs_cam=_lib.ptr(args["obs_cam"]), obs_pt=_lib.ptr(args["obs_pt"]), obs_uv=_lib.ptr(args["obs_uv"]),
                   loss=args["loss"], f_scale=args["f_scale"])
    out = CovOut(cam_cov=_lib.ptr(cam_cov), cam_cov_full=_lib.ptr(cam_cov_full), point_cov=_lib.ptr(point_cov), sigma0_sq=_lib.ptr(sigma0_sq),
                 dof=_lib.ptr(dof), cost=_lib.ptr(cost))
    rc = call(C.byref(desc), C.byref(out))
    if rc != 0:
        raise BackendError(f"{what} failed (code {rc}): {last_error()}")
    full = np.empty((n_points, 3, 3))
    for (a, b), e in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        full[:, a, b] = full[:, b, a] = point_cov[:, e]
    return CovarianceResult(cam_cov=cam_cov, cam_cov_full=cam_cov_full, point_cov=full, cam_offsets=offsets, sigma0_sq=float(sigma0_sq[0]),
                            dof=int(dof[0]), cost=float(cost[0]), gauge_dim=6 if n_constraint_rows else 7, n_constraint_rows=int(n_constraint_rows))


class DeviceUncertainty:
    """The device call ``cba_parameter_covariance`` on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def parameter_covariance(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, *, loss="linear",
                             f_scale=1.0) -> CovarianceResult:
        """Covariance of every camera's parameters and of every point at the given parameters; see ``include/caliscope/uncertainty.h``."""
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        lib = _lib.bind(_lib.load(), UNCERTAINTY_SIGNATURES)
        return run_covariance_call(lambda d, o: lib.cba_parameter_covariance(d, self.device_id, o), args, "cba_parameter_covariance",
                                   lambda: _lib.last_error(lib))

    def parameter_covariance_constrained(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, groups_a, groups_b,
                                         distances, weights, *, loss="linear", f_scale=1.0) -> CovarianceResult:
        """The same with the rigid-distance rows ``weights * (|mean points[groups_a] - mean points[groups_b]| - distances)`` in the
        Jacobian (six gauge columns); see ``include/caliscope/uncertainty_constrained.h``.  Without a row of positive weight it is
        ``parameter_covariance``."""
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        con = check_constraint_arguments(groups_a, groups_b, distances, weights)
        struct = constraint_struct(con)
        lib = _lib.bind(_lib.load(), CONSTRAINED_UNCERTAINTY_SIGNATURES)
        n_rows = 0 if con is None else int(np.count_nonzero(con["weights"] > 0))
        return run_covariance_call(lambda d, o: lib.cba_parameter_covariance_constrained(d, C.byref(struct) if struct is not None else None, self.device_id, o),
                                   args, "cba_parameter_covariance_constrained", lambda: _lib.last_error(lib), n_constraint_rows=n_rows)


# ---- first-order propagation on the host ------------------------------------------------------------------------------------------------
def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rotation_and_left_jacobian(rvec):
    """``R = exp([r]x)`` and the left Jacobian ``Jl`` of SO(3) at ``r`` (``exp([r + dr]x) ~ exp([Jl dr]x) exp([r]x)``), with the series
    of ``cam_prepare`` below 1e-4."""
    r = np.asarray(rvec, dtype=np.float64)
    th2 = float(r @ r)
    th = np.sqrt(th2)
    if th < 1e-4:
        sinc, a, b = 1.0 - th2 / 6.0 + th2 * th2 / 120.0, 0.5 - th2 / 24.0 + th2 * th2 / 720.0, 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0
    else:
        sinc, a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    K = _skew(r)
    K2 = K @ K
    return np.eye(3) + sinc * K + a * K2, np.eye(3) + a * K + b * K2


def centre_jacobian(rvec, tvec):
    """d c / d (rvec, tvec) (3 x 6) of the camera centre ``c = -R(r)^T t``: a rotation increment ``w = Jl dr`` turns ``R^T`` into
    ``R^T (I - [w]x)``, so ``dc = R^T [w]x t - R^T dt = -R^T [t]x Jl dr - R^T dt``."""
    R, Jl = rotation_and_left_jacobian(rvec)
    return np.hstack([-R.T @ _skew(np.asarray(tvec, dtype=np.float64)) @ Jl, -R.T])


@dataclass(frozen=True)
class CameraUncertainty:
    """One camera of an :class:`UncertaintyReport`.  ``param_cov`` is nparams x nparams in the order rvec, tvec (, s, k1, k2);
    ``centre_cov`` / ``centre_std`` are in world units; ``rotation_std_deg`` is the root of the summed variances of the three rotation
    angles (``sqrt(trace(Jl S_rr Jl^T))``); ``scale_std``, ``k1_std``, ``k2_std`` are None unless the intrinsics were free (``scale_std``
    is relative: the focal length's is ``scale_std * f``)."""

    cam_id: int
    param_cov: np.ndarray
    centre_cov: np.ndarray
    centre_std: np.ndarray
    rotation_std_deg: float
    scale_std: float | None = None
    k1_std: float | None = None
    k2_std: float | None = None

    @property
    def position_std(self) -> float:
        """``sqrt(trace(centre_cov))``."""
        return float(np.sqrt(np.trace(self.centre_cov)))


@dataclass(frozen=True)
class UncertaintyReport:
    """Parameter uncertainty of a calibration in the inner-constraint gauge (the covariance of smallest trace among all gauges:
    no camera or point is held fixed).  ``sigma0`` is the a-posteriori standard deviation of unit weight in residual units
    (pixels / fx) under the loss of the call, ``dof`` the degrees of freedom 2 n_obs - n_params + 7.  ``point_cov[i]`` /
    ``point_std[i]`` belong to row ``i`` of the volume's world points.  With the distance rows of a ``ConstraintSet`` in the adjustment
    (``n_constraint_rows`` > 0) the scale is no gauge direction: ``gauge_dim`` is 6 and ``dof`` = 2 n_obs + n_constraint_rows -
    n_params + 6."""

    sigma0: float
    dof: int
    cameras: dict
    point_cov: np.ndarray
    point_std: np.ndarray
    cam_cov_full: np.ndarray
    gauge: str = "inner"
    gauge_dim: int = 7
    n_constraint_rows: int = 0

    def worst_cameras(self, n: int = 3) -> list:
        """The ``n`` cameras with the largest centre uncertainty, worst first: ``(cam_id, position_std, rotation_std_deg)``."""
        ranked = sorted(self.cameras.values(), key=lambda c: c.position_std, reverse=True)
        return [(c.cam_id, c.position_std, c.rotation_std_deg) for c in ranked[: max(int(n), 0)]]


def build_report(result: CovarianceResult, cam_ids, cam_nparams, cam_x) -> UncertaintyReport:
    """The report of one call: the covariance blocks as returned, the centre and the rotation propagated to first order."""
    cameras = {}
    cam_x = np.asarray(cam_x, dtype=np.float64).reshape(-1, 9)
    for i, cam_id in enumerate(cam_ids):
        np_i = int(cam_nparams[i])
        cov = result.cam_cov[i, :np_i, :np_i].copy()
        Jc = centre_jacobian(cam_x[i, :3], cam_x[i, 3:6])
        centre_cov = Jc @ cov[:6, :6] @ Jc.T
        centre_cov = 0.5 * (centre_cov + centre_cov.T)
        _, Jl = rotation_and_left_jacobian(cam_x[i, :3])
        rot_var = float(np.trace(Jl @ cov[:3, :3] @ Jl.T))
        free = {} if np_i == 6 else dict(zip(("scale_std", "k1_std", "k2_std"), (float(v) for v in np.sqrt(np.maximum(np.diag(cov)[6:9], 0.0)))))
        cameras[int(cam_id)] = CameraUncertainty(cam_id=int(cam_id), param_cov=cov, centre_cov=centre_cov,
                                                 centre_std=np.sqrt(np.maximum(np.diag(centre_cov), 0.0)),
                                                 rotation_std_deg=float(np.degrees(np.sqrt(max(rot_var, 0.0)))), **free)
    point_std = np.sqrt(np.maximum(np.einsum("ijj->ij", result.point_cov), 0.0))
    return UncertaintyReport(sigma0=float(np.sqrt(max(result.sigma0_sq, 0.0))), dof=result.dof, cameras=cameras, point_cov=result.point_cov,
                             point_std=point_std, cam_cov_full=result.cam_cov_full, gauge_dim=result.gauge_dim, n_constraint_rows=result.n_constraint_rows)


__all__ = ["DeviceUncertainty", "CovarianceResult", "CameraUncertainty", "UncertaintyReport", "check_covariance_arguments", "check_constraint_arguments",
           "constraint_struct", "run_covariance_call", "build_report", "centre_jacobian", "rotation_and_left_jacobian", "UNCERTAINTY_SIGNATURES",
           "CONSTRAINED_UNCERTAINTY_SIGNATURES", "LOSSES"]
