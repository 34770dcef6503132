"""Scenes for the rank-by-rank checks of a point-sharded step (tests/test_sharded_scenes.py on the CPU, tests/test_sharded_step_gpu.py on the
device).  Each is the smallest that shows its edge; tests/test_sharded_scenes.py asserts the edge from the product's ``shard_problem``.

A scene is a dict: ``par``, ``problem`` (the whole BAProblem), ``x0``, ``loss``, ``f_scale``, ``constraints`` (the oracle's tuple or None),
``name`` and ``worlds``.
"""
from __future__ import annotations

import functools

import numpy as np

from caliscope_amd.bundle_parameterization import BundleParameterization
from caliscope_amd.engine import BAProblem
from tests.helpers import small_problem

HEAVY_OBS = 40   # csrc/cba_kernels.h: a point with more views takes k_heavy_schur
GROUP_MAX = 16   # csrc/cba_lib.hip: ranks of one device group
NB = 32          # csrc/chol_schedule.h: one Cholesky block

# name -> (builder, its arguments, worlds)
# The seeds are part of a scene's shape.  At lam = 1e-7 the seven gauge directions of the damped system are held by the damping alone, so the
# oracle's Schur step and the sparse LU of the same system differ by cond(H) eps: 1e-9 .. 2e-8 from one draw of points and noise to the next
# (median 2e-9 .. 1e-8 over sixty draws of each shape).  The draws below are ones whose references agree to a tenth of the step bar
# (tests/test_sharded_scenes.py::test_the_references_agree_within_a_tenth_of_the_step_bar), most of them to half of that.
_SPECS = {
    "EVEN": ("synthetic", dict(n_cams=8, n_points=240, k=6, seed=48), (2, 3)),
    "TINY_RIG": ("synthetic", dict(n_cams=2, n_points=60, k=2, seed=56), (2,)),
    "GLOBAL": ("synthetic", dict(n_cams=24, n_points=600, k=10, seed=37), (3,)),
    "GLOBAL_REFINE": ("synthetic", dict(n_cams=20, n_points=400, k=8, refine=True), (2,)),
    "SUBSET": ("subset", dict(n_cams=8, n_points=200, k=5, blind_camera=7, blind_share=0.6, seed=52), (2,)),
    "ONE_POINT": ("one_point", dict(n_cams=44, n_points=44, k_rest=7, seed=37, pixel_sigma=0.005), (8,)),
    "CONSTRAINED": ("constrained", dict(n_frames=6, constrained_frames=3, seed=34), (2,)),
    "ROBUST": ("synthetic", dict(n_cams=8, n_points=400, k=8, loss="huber", outliers=0.05), (2,)),
    "MIXED": ("mixed", dict(), (2,)),
    "WORLD16": ("synthetic", dict(n_cams=4, n_points=96, k=4, seed=51), (GROUP_MAX,)),
}
SCENES = tuple(_SPECS)
CASES = tuple((name, world) for name, (_, _, worlds) in _SPECS.items() for world in worlds)
FUSED_CASES = (("EVEN", 2), ("EVEN", 3), ("GLOBAL", 3), ("GLOBAL_REFINE", 2), ("ROBUST", 2))  # cba_step_supported == 1 on every rank
SOLVE_CASES = (("SUBSET", 2), ("ONE_POINT", 8))
CPU_BUILD_CASES = (("EVEN", 2), ("EVEN", 3), ("SUBSET", 2), ("ROBUST", 2), ("GLOBAL_REFINE", 2))
LAMBDAS = (1e-3, 1e-7)


def _pack(par, x0, cam, uv, obj, loss="linear", f_scale=1.0, constraints=None):
    kw = {}
    if constraints is not None:
        ga, gb, d, w = constraints
        kw = dict(constraint_groups_a=ga, constraint_groups_b=gb, constraint_distances=d, constraint_weights=w)
    prob = BAProblem(par, np.ascontiguousarray(cam, dtype=np.int32), np.ascontiguousarray(uv, dtype=np.float64),
                     np.ascontiguousarray(obj, dtype=np.int32), loss=loss, f_scale=f_scale, **kw)
    return dict(par=par, problem=prob, x0=x0, loss=loss, f_scale=f_scale, constraints=constraints)


def _synthetic(**kw):
    loss = kw.get("loss", "linear")
    sc, par, x0 = small_problem(**kw)
    fs = sc.f_scale_1px() * 2.0 if loss != "linear" else 1.0
    return _pack(par, x0, sc.camera_indices, sc.image_coords, sc.obj_indices, loss, fs)


def _subset(n_cams, n_points, k, blind_camera, blind_share, seed=42):
    """The first ``blind_share`` of the points lose their views from ``blind_camera``: rank 0 of two (half of the observations, the first points)
    never sees that camera; the later points still do."""
    sc, par, x0 = small_problem(n_cams=n_cams, n_points=n_points, k=k, seed=seed)
    keep = ~((sc.camera_indices == blind_camera) & (sc.obj_indices < int(blind_share * n_points)))
    return _pack(par, x0, sc.camera_indices[keep], sc.image_coords[keep], sc.obj_indices[keep])


def _one_point(n_cams, n_points, k_rest, seed=42, pixel_sigma=0.5):
    """Every camera sees every point in the synthetic scene; point 0 keeps all its views (more than HEAVY_OBS), the others keep ``k_rest`` views
    dealt round the rig so that every camera keeps its share.

    The scene's definition caps its observations at 8 x (views of point 0) <= 8 x (cameras): about eight per camera, so the minimum is flat,
    and a solve that stops by ftol leaves x known to sqrt(ftol F / curvature) only.  At half a pixel of noise that is 3e-7 between ANY two
    drivers (the CPU test build on 1 and 8 ranks shows the same figure), above the 1e-7 bar of the whole-solve comparison; at a twentieth
    of a pixel the end point is defined to 3e-8 but max |g| arrives at gtol = 1e-12 together with the ftol test and one rank count ends
    with status 1, the other with 2.  ``pixel_sigma`` = 0.005 px makes the end decisive: the last step takes max |g| from about 1e-8 to
    1e-16, every driver stops by gtol, and x is defined to 1e-9."""
    from caliscope_amd.synthetic import make_scene

    sc = make_scene(n_cams=n_cams, n_points=n_points, n_obs=n_points * n_cams, seed=seed, pixel_sigma=pixel_sigma)
    par = BundleParameterization.from_camera_array(sc.cameras_init, n_points=n_points, refine_intrinsics=False)
    x0 = par.pack(sc.cameras_init, sc.points_init)
    cam, obj = sc.camera_indices, sc.obj_indices
    slot = (cam - 7 * obj) % n_cams  # the views a point keeps start at camera 7 p and are spread evenly over the rig
    keep = (obj == 0) | (slot % (n_cams // k_rest) == 0) & (slot // (n_cams // k_rest) < k_rest)
    return _pack(par, x0, cam[keep], sc.image_coords[keep], obj[keep])


def _constrained(n_frames, constrained_frames, seed=3):
    """board_scene with the rigid-distance rows of the first ``constrained_frames`` boards only: the later boards are free points."""
    from tests.constrained_scene import board_scene

    sc = board_scene(n_frames=n_frames, seed=seed)
    ga, gb, d, w = sc["constraints"]
    rows = ga[:, 0] < constrained_frames * sc["n_per"]
    con = (ga[rows], gb[rows], d[rows], w[rows])
    return _pack(sc["par"], sc["x0"], sc["cam"], sc["uv"], sc["obj"], constraints=con)


def _mixed():
    from tests.test_oracle_pins import _mixed_arrays

    ca, points, uv, cam, obj = _mixed_arrays()
    par = BundleParameterization.from_camera_array(ca, n_points=len(points), refine_intrinsics=True)
    order = np.argsort(obj, kind="stable")
    return _pack(par, par.pack(ca, points), cam[order], uv[order], obj[order])


_BUILDERS = dict(synthetic=_synthetic, subset=_subset, one_point=_one_point, constrained=_constrained, mixed=_mixed)


NEAR_FRACTION, NEAR_MAX_NFEV = 0.01, 12  # tests/robust_scenes.py


@functools.lru_cache(maxsize=None)
def fused_start(name: str) -> np.ndarray:
    """Where the fused step of a scene is taken.  The linear-loss scenes: x0.  ROBUST: at x0 residuals are many pixels and six rows of seven lie
    beyond huber's quadratic region, at scipy's sqrt(EPS) floor; the damped step is then nearly collinear with the gradient and ``cba_step``
    hands the iteration back to the primitives (need_host = 1: no trial point, nothing to compare).  The recipe of tests/robust_scenes.py gives
    a point where the outlier rows alone are beyond the loss scale: x* + 0.01 (x0 - x*), x* = 12 evaluations of the oracle's linear-loss solve."""
    sc = scene(name)
    if sc["loss"] == "linear":
        return sc["x0"]
    from oracle.engine import OracleEngine
    from oracle.trf_driver import trf_solve

    prob = sc["problem"]
    x_star = trf_solve(OracleEngine(sc["par"], prob.camera_indices, prob.image_coords, prob.obj_indices), sc["x0"], max_nfev=NEAR_MAX_NFEV).x
    return x_star + NEAR_FRACTION * (sc["x0"] - x_star)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> dict:
    """The scene ``name`` (built once per process; treat it as read-only)."""
    kind, kw, worlds = _SPECS[name]
    out = _BUILDERS[kind](**kw)
    out["name"], out["worlds"] = name, worlds
    return out
