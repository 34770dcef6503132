"""Robust-loss scenes near a minimum, and two references of the damped step there (tests/test_robust_scenes.py shows on the CPU that each
scene is fit to test with; tests/test_robust_step_gpu.py holds the device to the linear-loss bars on them).

At the perturbed start x0 of the suite's other scenes residuals are many pixels: most rows of huber, cauchy and arctan then sit at scipy's
sqrt(EPS) floor (rho' + 2 rho'' z <= 0, scipy optimize/_lsq/common.py scale_for_robust_loss_function), whole columns live at 1e-8 and a
comparison of steps is noise on both sides.  Here every scene is evaluated at

    x = x* + FRACTION (x0 - x*),      x* = MAX_NFEV evaluations of the oracle's linear-loss trf_solve from x0,

where residuals are of the size of the loss scale: a few per cent of the rows are at the floor, a third and more are curved, no column
is starved, and the step can be compared on ALL parameters.

References, independent of each other and of every Schur kernel, computed once per (scene, loss) and shared (``reference``):

1. ``oracle.engine.OracleEngine(loss=, f_scale=, constraints=)``: numpy Schur solve (with constraint rows a sparse LU of the point block);
2. the oracle's sparse J, f scaled by scipy's own ``construct_loss_function`` / ``scale_for_robust_loss_function`` here, the damped normal
   equations (J^T J + lam D^2) s = -g solved as ONE system by ``splu``, and S_ref = Hcc - Hcp Hpp^-1 Hpc from its blocks.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from tests.helpers import small_problem

EPS = np.finfo(np.float64).eps
FRACTION = 0.01
MAX_NFEV = 12
LAMS = (1e-3, 1e-7)
TRIAL = (-1e-3, 0.5)
GRAM = (0.3, -1.2, 1.1, 0.4)
SHAPES = {
    "L6": dict(n_cams=6, n_points=300, k=6),
    "R6": dict(n_cams=6, n_points=300, k=6, refine=True),
    "L24": dict(n_cams=24, n_points=600, k=10),
    "R20": dict(n_cams=20, n_points=400, k=8, refine=True),
}
LOSSES = ("huber", "soft_l1", "cauchy", "arctan")
F_SCALE_PX = {"huber": 0.75, "soft_l1": 0.5, "cauchy": 1.0, "arctan": 1.0, "linear": 1.0}
# the remaining routes: (scene, loss) pairs
COMPONENT_SHAPES = {"component_small": (55, 12), "component_large": (56, 12)}  # rows, points; four six-parameter cameras (ncp = 24)
ROUTE_SCENES = (("board", "huber"), ("board", "soft_l1"), ("component_small", "soft_l1"), ("component_large", "soft_l1"),
                ("sparse_ids", "soft_l1"), ("sparse_ids_refine", "soft_l1"), ("fisheye_pinhole", "soft_l1"))
ALL_SCENES = tuple((shape, loss) for shape in SHAPES for loss in LOSSES) + ROUTE_SCENES
BOARD_MOVED_ROWS = (3, 40, 29)  # rows of the board's constraints whose recorded distance is moved under huber; 29: frame 0's centroid row
BOARD_MOVE_M = 0.008


def pixel(par) -> float:
    """One pixel in the normalised residual units (``CaptureVolume.pixel_f_scale(1.0)``)."""
    return 1.0 / float(np.median([b.fx_initial for b in par.blocks]))


def _oracle(sc, loss="linear", f_scale=1.0):
    from oracle.engine import OracleEngine

    return OracleEngine(sc["par"], sc["cam"], sc["uv"], sc["obj"], loss=loss, f_scale=f_scale, constraints=sc.get("constraints"))


def _near(sc):
    """x* + FRACTION (x0 - x*) of a scene dict (par, x0, cam, uv, obj[, constraints])."""
    from oracle.trf_driver import trf_solve

    x_star = trf_solve(_oracle(sc), sc["x0"], max_nfev=MAX_NFEV).x
    return x_star + FRACTION * (sc["x0"] - x_star)


@lru_cache(maxsize=None)
def base_scene(name: str, moved: bool = False) -> dict:
    """The arrays of a scene and its near-minimum point ``x`` (one oracle solve per scene, cached).  ``moved``: the board with three recorded
    distances changed by BOARD_MOVE_M, so that those rows sit at huber's floor."""
    if name in SHAPES:
        s, par, x0 = small_problem(**SHAPES[name])
        sc = dict(par=par, x0=x0, cam=s.camera_indices, uv=s.image_coords, obj=s.obj_indices, source=s)
    elif name == "board":
        from tests.constrained_scene import board_scene

        sc = board_scene()
        if moved:
            ga, gb, dist, w = sc["constraints"]
            dist = dist.copy()
            dist[list(BOARD_MOVED_ROWS)] += BOARD_MOVE_M
            sc["constraints"] = (ga, gb, dist, w)
    elif name in COMPONENT_SHAPES:
        from tests.edge_scenes import component_scene

        sc = component_scene([COMPONENT_SHAPES[name]] * 2, n_cams=4)
    elif name in ("sparse_ids", "sparse_ids_refine"):
        from tests.edge_scenes import sparse_id_scene

        sc = sparse_id_scene(stride=8, heavy_obs=256, refine=name.endswith("refine"))
    elif name == "fisheye_pinhole":
        from caliscope_amd.bundle_parameterization import BundleParameterization
        from tests.test_oracle_pins import _mixed_arrays

        ca, points, uv, cam_idx, obj_idx = _mixed_arrays()
        par = BundleParameterization.from_camera_array(ca, n_points=len(points), refine_intrinsics=True)
        sc = dict(par=par, x0=par.pack(ca, points), cam=cam_idx.astype(np.int32), uv=uv, obj=obj_idx)
    else:
        raise KeyError(name)
    sc.setdefault("constraints", None)
    sc["x"] = _near(sc)
    sc["name"] = name
    return sc


def scene(name: str, loss: str) -> dict:
    """The scene dict of a (scene, loss) pair with ``loss`` and ``f_scale`` filled in (the arrays are shared: do not write to them)."""
    sc = dict(base_scene(name, moved=(name == "board" and loss == "huber")))
    sc["loss"], sc["f_scale"] = loss, F_SCALE_PX[loss] * pixel(sc["par"])
    return sc


def near_minimum(shape: str, loss: str):
    """(sc, par, x, f_scale) of one of SHAPES under ``loss``: the make_scene scene (no outliers), its parameterization, the evaluation point
    and the loss scale in residual units."""
    sc = scene(shape, loss)
    return sc["source"], sc["par"], sc["x"], sc["f_scale"]


def problem(sc, loss=None, f_scale=None):
    """The BAProblem of a scene dict (what a HIP handle is created from)."""
    from caliscope_amd.engine import BAProblem

    kw = {}
    if sc["constraints"] is not None:
        ga, gb, dist, w = sc["constraints"]
        kw = dict(constraint_groups_a=ga, constraint_groups_b=gb, constraint_distances=dist, constraint_weights=w)
    return BAProblem(sc["par"], sc["cam"], sc["uv"], sc["obj"], loss=sc["loss"] if loss is None else loss,
                     f_scale=sc["f_scale"] if f_scale is None else f_scale, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------------
def raw_system(sc):
    """The oracle's sparse J and f at the scene's point, before any loss."""
    from oracle.residuals import joint_jacobian, joint_residuals

    con = () if sc["constraints"] is None else sc["constraints"]
    args = (sc["par"], sc["cam"], sc["uv"], sc["obj"], *con)
    return joint_jacobian(sc["x"], *args).tocsr(), joint_residuals(sc["x"], *args)


def row_scale_longdouble(f, loss, f_scale):
    """scipy's row scale (rho' + 2 rho'' z clamped at EPS; its square root multiplies the row of J) in np.longdouble, its z, and the rows at
    the floor."""
    f = np.asarray(f, dtype=np.longdouble)
    z = (f / np.longdouble(f_scale)) ** 2
    one, two, half = np.longdouble(1), np.longdouble(2), np.longdouble(0.5)
    if loss == "linear":
        r1, r2 = np.ones_like(z), np.zeros_like(z)
    elif loss == "huber":
        out = z > 1
        zs = np.where(out, z, one)
        r1 = np.where(out, zs ** -half, one)
        r2 = np.where(out, -half * zs ** np.longdouble(-1.5), 0 * one)
    elif loss == "soft_l1":
        t = one + z
        r1, r2 = t ** -half, -half * t ** np.longdouble(-1.5)
    elif loss == "cauchy":
        r1, r2 = one / (one + z), -one / (one + z) ** 2
    elif loss == "arctan":
        t = one + z * z
        r1, r2 = one / t, -two * z / t ** 2
    else:
        raise KeyError(loss)
    js = r1 + two * r2 * z
    floor = js < EPS
    return np.where(floor, np.longdouble(EPS), js), z, floor


@dataclass
class StepRef:
    s_oracle: np.ndarray
    s_lu: np.ndarray
    S_oracle: np.ndarray
    S_ref: np.ndarray
    p_sq: float
    gh_dot_p: float
    w_sq: float
    gram: tuple
    trial_cost: float
    trial_step_norm: float


@dataclass
class Reference:
    cost: float
    lin: object                     # the oracle's first linearisation (g_norm_inf, gh_sq, jg_sq, x_scaled_norm, x_norm)
    g: np.ndarray
    scale_inv: np.ndarray
    scale_inv_longdouble: np.ndarray
    scale_inv_disagreement: float   # oracle vs. np.longdouble column norms, the largest relative difference of a column
    has_rows: np.ndarray            # parameters that some row of J touches
    z: np.ndarray                   # (f / f_scale)^2 per scalar row, constraint rows last
    floor: np.ndarray               # scalar rows at the sqrt(EPS) floor
    n_obs_rows: int
    steps: dict = field(default_factory=dict)   # lam -> StepRef
    s_linear: dict = field(default_factory=dict)  # lam -> the oracle's linear-loss step at the same point
    lin2: object = None             # second linearisation, after accept() of the trial point of the last lam
    scale_inv2: np.ndarray = None


def rel(a, b) -> float:
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@lru_cache(maxsize=None)
def reference(name: str, loss: str) -> Reference:
    """Both references of a (scene, loss) pair.  The returned arrays are shared among the tests: read only."""
    import scipy.sparse as sp
    from scipy.optimize._lsq.common import scale_for_robust_loss_function
    from scipy.optimize._lsq.least_squares import construct_loss_function
    from scipy.sparse.linalg import splu

    sc = scene(name, loss)
    par, x, fs = sc["par"], sc["x"], sc["f_scale"]
    ncp = par.n_camera_params
    ora = _oracle(sc, loss, fs)
    cost = ora.begin(x)
    lin = ora.linearize()
    # reference 2: the same raw J, f scaled by scipy's helpers here
    J_raw, f_raw = raw_system(sc)
    if loss == "linear":
        J, f = J_raw.copy(), f_raw.copy()
    else:
        fn = construct_loss_function(len(f_raw), loss, fs)
        J, f = scale_for_robust_loss_function(J_raw.copy(), f_raw.copy(), fn(f_raw))
    J = sp.csr_matrix(J)
    g = np.asarray(J.T @ f).ravel()
    col_sq = np.asarray(J.multiply(J).sum(axis=0)).ravel()
    d = np.sqrt(col_sq)
    d[d == 0] = 1.0
    # column norms in np.longdouble from the raw J and a longdouble row scale
    js, z, floor = row_scale_longdouble(f_raw, loss, fs)
    coo = J_raw.tocoo()
    col_ld = np.zeros(J.shape[1], dtype=np.longdouble)
    np.add.at(col_ld, coo.col, coo.data.astype(np.longdouble) ** 2 * js[coo.row])
    d_ld = np.sqrt(col_ld)
    d_ld[d_ld == 0] = 1.0
    has_rows = np.asarray((J_raw != 0).sum(axis=0)).ravel() > 0
    ref = Reference(cost=cost, lin=lin, g=ora.g.copy(), scale_inv=ora.scale_inv.copy(), scale_inv_longdouble=d_ld,
                    scale_inv_disagreement=float(np.max(np.abs(ora.scale_inv - d_ld)[has_rows] / d_ld[has_rows])), has_rows=has_rows,
                    z=np.asarray(z, dtype=np.float64), floor=np.asarray(floor), n_obs_rows=2 * len(sc["cam"]))
    assert rel(g, ora.g) < 1e-13 and rel(d, ora.scale_inv) < 1e-13  # (two scalings of one J: the references share their inputs, not their solves)
    lin_ora = _oracle(sc) if loss != "linear" else None
    if lin_ora is not None:
        lin_ora.begin(x)
        lin_ora.linearize()
    for lam in LAMS:
        so = ora.newton_step(lam)
        assert so.ok
        H = (J.T @ J + lam * sp.diags(d ** 2)).tocsc()
        s_lu = splu(H).solve(-g)
        s_lu[~has_rows] = 0.0   # (columns without rows: the damping alone, right-hand side 0)
        Hcc, Hcp, Hpp = H[:ncp, :ncp].toarray(), H[:ncp, ncp:], H[ncp:, ncp:].tocsc()
        S_ref = Hcc - Hcp @ splu(Hpp).solve(Hcp.T.toarray())
        gram = ora.subspace_gram(*GRAM)
        tr = ora.trial(*TRIAL)
        ref.steps[lam] = StepRef(ora.s.copy(), s_lu, ora.S.copy(), S_ref, so.p_sq, so.gh_dot_p, so.w_sq, gram, tr.cost, tr.step_norm)
        if lin_ora is not None:
            assert lin_ora.newton_step(lam).ok
            ref.s_linear[lam] = lin_ora.s.copy()
    ora.accept()
    ref.lin2 = ora.linearize()
    ref.scale_inv2 = ora.scale_inv.copy()
    return ref
