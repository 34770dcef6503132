"""How strongly the other observations control each observation, and which observations contradict the adjustment: redundancy numbers and
the w-test in one device call.

:meth:`CaptureVolume.parameter_uncertainty` says how well the data determine every camera and point; this module says the same about the
observations.  ``cba_observation_reliability`` (``include/caliscope/reliability.h``, ``csrc/reliability_math.h``,
``csrc/reliability_lib.hip``) returns per residual row ``j`` the redundancy number ``r_j`` — the diagonal of
``R = I - J pinv(J^T J) J^T``, between 0 (the adjustment absorbs any error in the row: nothing checks it) and 1 (fully checked) — and the
standardised residual ``w_j = f_j / (sigma0 sqrt(r_j))`` of Baarda's / Pope's data snooping, behind the launches of
``cba_parameter_covariance`` and without the dense projector.  :meth:`CaptureVolume.observation_reliability` returns a
:class:`ReliabilityReport` aligned to the rows of the image points, :meth:`CaptureVolume.filter_by_w_test` does one pass of data snooping.
The reference's only outlier tool cuts a fixed share of the raw reprojection errors, and the raw residual of a weakly controlled
observation is small however wrong the observation is.

Scope: reprojection rows, and with ``observation_reliability_constrained`` (``include/caliscope/reliability_constrained.h``,
``csrc/reliability_constraint_math.h``; ``include_constraints=True`` of the two methods) the rigid-distance rows of a ``ConstraintSet`` too:
they are rows of ``J`` like any other, the gauge then has six columns, and every constraint row gets its own redundancy number, ``w``
and smallest detectable error — a wrong board dimension is a blunder in a constraint row.  Components of at most 54 points, as
``parameter_covariance_constrained``.  Under a robust loss ``J`` and the residuals are the scaled ones
scipy forms and ``w`` is an approximation.  One removal per world point per pass: a blunder smears onto the other observations of its
point.

There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.  ``_solver`` of the methods replaces the device
call (an object with ``observation_reliability``, as :class:`DeviceReliability`).
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace
from statistics import NormalDist

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError
from caliscope_amd.uncertainty import CovConstraints, CovDesc, check_constraint_arguments, check_covariance_arguments, constraint_struct

REL_R_TINY = 1e-10  # csrc/reliability_math.h
DELTA0 = 4.13       # Baarda's non-centrality for alpha0 = 0.1 % and beta0 = 80 %: a convention, not a measurement


class RelOut(C.Structure):
    _fields_ = [("redundancy", _lib.c_double_p), ("w", _lib.c_double_p), ("residual", _lib.c_double_p), ("sigma0_sq", _lib.c_double_p),
                ("dof", _lib.c_int64_p), ("cost", _lib.c_double_p), ("n_uncontrolled", _lib.c_int64_p)]


RELIABILITY_SIGNATURES = {
    "cba_observation_reliability": (C.c_int, [C.POINTER(CovDesc), C.c_int32, C.POINTER(RelOut)]),
}


class RelConOut(C.Structure):
    _fields_ = [("redundancy", _lib.c_double_p), ("w", _lib.c_double_p), ("residual", _lib.c_double_p), ("n_uncontrolled", _lib.c_int64_p)]


# include/caliscope/reliability_constrained.h
RELIABILITY_CONSTRAINED_SIGNATURES = {
    "cba_observation_reliability_constrained": (C.c_int, [C.POINTER(CovDesc), C.POINTER(CovConstraints), C.c_int32, C.POINTER(RelOut), C.POINTER(RelConOut)]),
}


@dataclass(frozen=True)
class ReliabilityResult:
    """What one ``observation_reliability`` call returns, rows in the order of the call's observations: ``redundancy`` (n_obs, 2, 2) the
    blocks ``R_oo`` (not clamped), ``w`` (n_obs, 2) with NaN where ``r_j <= REL_R_TINY``, ``residual`` (n_obs, 2) in residual units
    (pixels / fx0), scaled for the loss.  ``observation_reliability_constrained`` adds, in the order of the call's constraint rows (NaN for
    a row of weight 0): ``constraint_redundancy``, ``constraint_w`` and ``constraint_residual`` (n_con,), the last being
    ``weight * (length - distance)`` scaled for the loss; ``gauge_dim`` is 6 when a row of positive weight took part, else 7."""

    redundancy: np.ndarray
    w: np.ndarray
    residual: np.ndarray
    sigma0_sq: float
    dof: int
    cost: float
    n_uncontrolled: int
    gauge_dim: int = 7
    constraint_redundancy: np.ndarray | None = None
    constraint_w: np.ndarray | None = None
    constraint_residual: np.ndarray | None = None
    n_constraints_uncontrolled: int = 0


def run_reliability_constrained_call(call, args: dict, con: dict | None, what: str, last_error) -> ReliabilityResult:
    """``run_reliability_call`` for ``call(desc_ref, out_ref, con_out_ref) -> code`` with the constraint rows of
    ``check_constraint_arguments`` (shared by the device binding and the test harness)."""
    n_con = 0 if con is None else len(con["distances"])
    cr, cw, cf, cbad = np.full(n_con, np.nan), np.full(n_con, np.nan), np.full(n_con, np.nan), np.zeros(1, dtype=np.int64)
    con_out = RelConOut(redundancy=_lib.ptr(cr), w=_lib.ptr(cw), residual=_lib.ptr(cf), n_uncontrolled=_lib.ptr(cbad))
    res = run_reliability_call(lambda d, o: call(d, o, C.byref(con_out)), args, what, last_error)
    n_rows = 0 if con is None else int(np.count_nonzero(con["weights"] > 0))
    return replace(res, gauge_dim=6 if n_rows else 7, constraint_redundancy=cr, constraint_w=cw, constraint_residual=cf,
                   n_constraints_uncontrolled=int(cbad[0]))


def run_reliability_call(call, args: dict, what: str, last_error) -> ReliabilityResult:
    """Fill ``cba_cov_desc`` / ``cba_rel_out`` from checked arguments (``check_covariance_arguments``), run
    ``call(desc_ref, out_ref) -> code`` and collect the result (shared by the device binding and the test harness)."""
    n_obs = len(args["obs_cam"])
    red, w, res = np.zeros((n_obs, 3)), np.zeros((n_obs, 2)), np.zeros((n_obs, 2))
    sigma0_sq, dof, cost, bad = np.zeros(1), np.zeros(1, dtype=np.int64), np.zeros(1), np.zeros(1, dtype=np.int64)
    desc = CovDesc(n_cams=len(args["cam_model"]), n_points=len(args["points"]), n_obs=n_obs, cam_model=_lib.ptr(args["cam_model"]),
                   cam_nparams=_lib.ptr(args["cam_nparams"]), cam_const=_lib.ptr(args["cam_const"]), cam_x=_lib.ptr(args["cam_x"]),
                   points=_lib.ptr(args["points"]), obs_cam=_lib.ptr(args["obs_cam"]), obs_pt=_lib.ptr(args["obs_pt"]), obs_uv=_lib.ptr(args["obs_uv"]),
                   loss=args["loss"], f_scale=args["f_scale"])
    out = RelOut(redundancy=_lib.ptr(red), w=_lib.ptr(w), residual=_lib.ptr(res), sigma0_sq=_lib.ptr(sigma0_sq), dof=_lib.ptr(dof), cost=_lib.ptr(cost),
                 n_uncontrolled=_lib.ptr(bad))
    rc = call(C.byref(desc), C.byref(out))
    if rc != 0:
        raise BackendError(f"{what} failed (code {rc}): {last_error()}")
    full = np.empty((n_obs, 2, 2))
    full[:, 0, 0], full[:, 0, 1], full[:, 1, 0], full[:, 1, 1] = red[:, 0], red[:, 1], red[:, 1], red[:, 2]
    return ReliabilityResult(redundancy=full, w=w, residual=res, sigma0_sq=float(sigma0_sq[0]), dof=int(dof[0]), cost=float(cost[0]),
                             n_uncontrolled=int(bad[0]))


class DeviceReliability:
    """The device call ``cba_observation_reliability`` on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def observation_reliability(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, *, loss="linear",
                                f_scale=1.0) -> ReliabilityResult:
        """Redundancy blocks, standardised and scaled residuals of every observation at the given parameters; see
        ``include/caliscope/reliability.h``."""
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        lib = _lib.bind(_lib.load(), RELIABILITY_SIGNATURES)
        return run_reliability_call(lambda d, o: lib.cba_observation_reliability(d, self.device_id, o), args, "cba_observation_reliability",
                                    lambda: _lib.last_error(lib))

    def observation_reliability_constrained(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, groups_a, groups_b,
                                            distances, weights, *, loss="linear", f_scale=1.0) -> ReliabilityResult:
        """The same with the rigid-distance rows ``weights * (|mean points[groups_a] - mean points[groups_b]| - distances)`` in the
        adjustment, and the redundancy, ``w`` and scaled residual of every such row; see ``include/caliscope/reliability_constrained.h``.
        Without a row of positive weight it is ``observation_reliability`` (``gauge_dim == 7``, the constraint arrays NaN)."""
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        con = check_constraint_arguments(groups_a, groups_b, distances, weights)
        struct = constraint_struct(con)
        lib = _lib.bind(_lib.load(), RELIABILITY_CONSTRAINED_SIGNATURES)
        return run_reliability_constrained_call(
            lambda d, o, c: lib.cba_observation_reliability_constrained(d, C.byref(struct) if struct is not None else None, self.device_id, o, c), args, con,
            "cba_observation_reliability_constrained", lambda: _lib.last_error(lib))


def critical_value(alpha: float) -> float:
    """The two-sided critical value of the standard normal distribution at significance ``alpha`` (3.29 for 0.1 %)."""
    if not (0.0 < alpha < 1.0):
        raise ValueError(f"alpha must be in (0, 1), got {alpha}")
    return NormalDist().inv_cdf(1.0 - alpha / 2.0)


@dataclass(frozen=True)
class ReliabilityReport:
    """Reliability of the observations of a calibration; every per-observation array is aligned to the rows of the volume's image points,
    with NaN in rows that took no part (unmatched, or on a world point with fewer than two matched views).

    ``sigma0`` is the a-posteriori standard deviation of unit weight in residual units (pixels / fx) under the loss of the call, ``dof``
    the degrees of freedom.  ``redundancy`` (n, 2) holds ``r_u, r_v`` (they sum to ``dof`` over the volume), ``redundancy_uv`` (n,) the
    off-diagonal entry of the 2 x 2 block, ``w`` (n, 2) the standardised residuals (NaN where ``r_j <= 1e-10``: ``n_uncontrolled`` such
    rows), ``residual_px`` (n, 2) the residuals (scaled for the loss) in pixels, ``mdb_px`` (n, 2) the smallest blunder detectable with
    Baarda's ``delta0``: ``delta0 sigma0 fx / sqrt(r)``, infinite for an uncontrolled row.  ``camera_redundancy`` maps a cam_id to the
    mean ``r`` over its rows, ``point_redundancy`` (n_world_points,) is the mean ``r`` per world point (NaN for a point that took no
    part).  Under a robust loss ``w`` is an approximation.

    With ``include_constraints=True`` the distance rows of the volume's ``ConstraintSet`` took part (``gauge_dim == 6``) and are judged
    too, one entry per instance in the order of ``constraint_instances`` (``(constraint, sync_index)``): ``constraint_redundancy``,
    ``constraint_w``, ``constraint_residual_m`` (measured minus nominal distance, scaled for the loss, in world units) and
    ``constraint_mdb_m`` (``delta0 sigma0 / (weight sqrt(r))``: the smallest error of the nominal distance the adjustment would
    detect).  Without it these arrays are empty."""

    sigma0: float
    dof: int
    redundancy: np.ndarray
    redundancy_uv: np.ndarray
    w: np.ndarray
    residual_px: np.ndarray
    mdb_px: np.ndarray
    camera_redundancy: dict
    point_redundancy: np.ndarray
    n_uncontrolled: int
    delta0: float = DELTA0
    gauge_dim: int = 7
    constraint_redundancy: np.ndarray = field(default_factory=lambda: np.zeros(0))
    constraint_w: np.ndarray = field(default_factory=lambda: np.zeros(0))
    constraint_residual_m: np.ndarray = field(default_factory=lambda: np.zeros(0))
    constraint_mdb_m: np.ndarray = field(default_factory=lambda: np.zeros(0))
    constraint_instances: tuple = ()

    @property
    def max_abs_w(self) -> np.ndarray:
        """``max_j |w_j|`` per observation (an uncontrolled row of the two is passed over); NaN where the observation took no part or both of
        its rows are uncontrolled."""
        a = np.abs(self.w)
        return np.fmax(a[:, 0], a[:, 1])

    def flagged(self, alpha: float = 0.001) -> np.ndarray:
        """The rows of the image points whose ``max_j |w_j|`` exceeds the two-sided critical value at ``alpha``, ascending."""
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(self.max_abs_w > critical_value(alpha))

    def worst_observations(self, n: int = 10) -> list:
        """The ``n`` observations with the largest ``max_j |w_j|``, worst first: ``(row, max |w|, min r of the row)``."""
        m = self.max_abs_w
        rows = np.flatnonzero(np.isfinite(m))
        rows = rows[np.argsort(-m[rows], kind="stable")][: max(int(n), 0)]
        return [(int(i), float(m[i]), float(self.redundancy[i].min())) for i in rows]

    def flagged_constraints(self, alpha: float = 0.001) -> np.ndarray:
        """The constraint instances (positions in ``constraint_instances``) whose ``|w|`` exceeds the two-sided critical value at ``alpha``,
        ascending."""
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(np.abs(self.constraint_w) > critical_value(alpha))

    def worst_constraints(self, n: int = 10) -> list:
        """The ``n`` constraint instances with the largest ``|w|``, worst first: ``(position, |w|, r, residual_m)``."""
        m = np.abs(self.constraint_w)
        rows = np.flatnonzero(np.isfinite(m))
        rows = rows[np.argsort(-m[rows], kind="stable")][: max(int(n), 0)]
        return [(int(i), float(m[i]), float(self.constraint_redundancy[i]), float(self.constraint_residual_m[i])) for i in rows]


def build_report(result: ReliabilityResult, rows, n_rows, fx, cam_ids, obs_cam, obs_world, n_world, delta0=DELTA0, constraint_weights=None,
                 constraint_instances=()) -> ReliabilityReport:
    """The report of one call.  ``constraint_weights`` (with a result of ``observation_reliability_constrained``): the weight of every
    constraint row of the call, which turns its scaled residual and its smallest detectable error into world units; ``constraint_instances``
    names the rows.  ``rows``: the image-point row of every observation of the call, ``n_rows`` the number of image-point
    rows; ``fx`` (n_obs,) the focal length that turns residual units into pixels (``fx0`` of the observation's camera);
    ``cam_ids[obs_cam]`` and ``obs_world`` name the camera and the world-point row of every observation."""
    rows = np.asarray(rows, dtype=np.int64)
    fx = np.asarray(fx, dtype=np.float64).reshape(-1, 1)
    sigma0 = float(np.sqrt(max(result.sigma0_sq, 0.0)))

    def spread(values, width):
        out = np.full((n_rows,) + ((width,) if width else ()), np.nan)
        out[rows] = values
        return out

    r = np.stack([result.redundancy[:, 0, 0], result.redundancy[:, 1, 1]], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mdb = np.where(r > REL_R_TINY, delta0 * sigma0 * fx / np.sqrt(np.clip(r, REL_R_TINY, 1.0)), np.inf)
    obs_cam = np.asarray(obs_cam, dtype=np.int64)
    mean_r = r.mean(axis=1)
    cam_sum, cam_n = np.bincount(obs_cam, weights=mean_r, minlength=len(cam_ids)), np.bincount(obs_cam, minlength=len(cam_ids))
    camera_redundancy = {int(c): (float(cam_sum[i] / cam_n[i]) if cam_n[i] else float("nan")) for i, c in enumerate(cam_ids)}
    pt_sum, pt_n = np.bincount(obs_world, weights=mean_r, minlength=n_world), np.bincount(obs_world, minlength=n_world)
    with np.errstate(divide="ignore", invalid="ignore"):
        point_redundancy = np.where(pt_n > 0, pt_sum / pt_n, np.nan)
    return ReliabilityReport(sigma0=sigma0, dof=result.dof, redundancy=spread(r, 2), redundancy_uv=spread(result.redundancy[:, 0, 1], 0),
                             w=spread(result.w, 2), residual_px=spread(result.residual * fx, 2), mdb_px=spread(mdb, 2),
                             camera_redundancy=camera_redundancy, point_redundancy=point_redundancy, n_uncontrolled=result.n_uncontrolled,
                             delta0=float(delta0), gauge_dim=result.gauge_dim, **_constraint_columns(result, constraint_weights, sigma0, delta0),
                             constraint_instances=tuple(constraint_instances))


def _constraint_columns(result: ReliabilityResult, weights, sigma0, delta0) -> dict:
    if weights is None or result.constraint_redundancy is None:
        return {}
    weights = np.asarray(weights, dtype=np.float64)
    r = result.constraint_redundancy
    with np.errstate(divide="ignore", invalid="ignore"):
        mdb = np.where(r > REL_R_TINY, delta0 * sigma0 / (weights * np.sqrt(np.clip(r, REL_R_TINY, 1.0))), np.inf)
        mdb = np.where(np.isnan(r), np.nan, mdb)
        residual_m = result.constraint_residual / weights
    return dict(constraint_redundancy=r, constraint_w=result.constraint_w, constraint_residual_m=residual_m, constraint_mdb_m=mdb)


def snooping_mask(max_abs_w, obs_world, views, critical) -> np.ndarray:
    """One pass of data snooping over the observations of a call: per world point the observation with the largest ``|w|`` goes if
    that ``|w|`` exceeds ``critical`` and the point keeps at least two views without it.  ``max_abs_w`` (n_obs,) with NaN for rows
    that cannot be judged, ``obs_world`` the world point of every observation, ``views`` the matched views per world point.  Returns
    the keep mask (n_obs,)."""
    keep = np.ones(len(max_abs_w), dtype=bool)
    m = np.where(np.isfinite(max_abs_w), max_abs_w, -np.inf)
    order = np.lexsort((-m, obs_world))  # by point, the largest |w| first
    first = np.ones(len(order), dtype=bool)
    first[1:] = obs_world[order][1:] != obs_world[order][:-1]
    worst = order[first]
    drop = worst[(m[worst] > critical) & (views[obs_world[worst]] >= 3)]
    keep[drop] = False
    return keep


__all__ = ["DeviceReliability", "ReliabilityResult", "ReliabilityReport", "RelOut", "RelConOut", "RELIABILITY_SIGNATURES",
           "RELIABILITY_CONSTRAINED_SIGNATURES", "run_reliability_call", "run_reliability_constrained_call", "critical_value",
           "build_report", "snooping_mask", "REL_R_TINY", "DELTA0"]
