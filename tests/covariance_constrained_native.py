"""g++ build of caliscope_amd/csrc/covariance_constraint_plan.h and covariance_constraint_math.h
(tests/native/covariance_constrained_harness.cpp), a `_solver` hook on it, and what the tests of the constrained covariance share: the
scenes, the float64 eigenvalue pseudo-inverse of the oracle's J^T J with the constraint rows in J and SIX eigenvalues zeroed (the
reference), the bordered formula with a dense V~^-1 in numpy (the second CPU formulation) and the comparison by the rule of
tests.covariance_native.check_result_against_pinv with six for seven; the row scaling, the pseudo-inverse and that rule are its helpers."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.uncertainty import (CovConstraints, CovDesc, CovOut, check_constraint_arguments, check_covariance_arguments, constraint_struct,
                                       run_covariance_call)
from tests import covariance_native as cn
from tests.native_build import CSRC, NATIVE, load_native

I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)
F64 = C.POINTER(C.c_double)
PLAN_ARRAYS = ("comp_pt", "pts", "comp_row", "row_src", "row_loc", "free_pts", "comp_cam", "cams", "cc_obs", "obs_pos", "obs_loc", "entry_start", "entry_cam")


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "covariance_constrained_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.cch_last_error.restype = C.c_char_p
    lib.cch_constants.restype = None
    lib.cch_constants.argtypes = [I64]
    lib.cch_parameter_covariance_constrained.restype = C.c_int
    lib.cch_parameter_covariance_constrained.argtypes = [C.POINTER(CovDesc), C.POINTER(CovConstraints), C.POINTER(CovOut), I32, I64]
    lib.cch_plan.restype = C.c_int
    lib.cch_plan.argtypes = [C.c_int64, C.POINTER(CovDesc), C.POINTER(CovConstraints), C.c_int32, I64]
    lib.cch_plan_copy.restype = None
    lib.cch_plan_copy.argtypes = [C.c_int32, I64]
    lib.cch_row.restype = C.c_double
    lib.cch_row.argtypes = [F64, I32, C.c_double, C.c_double, C.c_int32, C.c_double, F64, F64]
    lib.cch_device_bytes.restype = C.c_double
    lib.cch_device_bytes.argtypes = [C.POINTER(CovDesc)]
    lib.cch_memory_check.restype = C.c_int
    lib.cch_memory_check.argtypes = [C.c_double, C.c_double]
    return lib


def constants():
    out = np.zeros(4, dtype=np.int64)
    harness().cch_constants(out.ctypes.data_as(I64))
    return dict(cap=int(out[0]), gauge_rigid=int(out[1]), gauge=int(out[2]), lds_doubles_at_cap=int(out[3]))


def last_error():
    return harness().cch_last_error().decode()


class HarnessConstrainedUncertainty:
    """The `_solver` hook on the g++ build: same arguments, checks, result and error type as caliscope_amd.uncertainty.DeviceUncertainty."""

    def __init__(self):
        self.calls = 0
        self.constrained_calls = 0

    def parameter_covariance(self, *eight, loss="linear", f_scale=1.0):
        return self.parameter_covariance_constrained(*eight, None, None, None, None, loss=loss, f_scale=f_scale)

    def parameter_covariance_constrained(self, cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, groups_a, groups_b, distances,
                                         weights, *, loss="linear", f_scale=1.0, null_struct=False):
        args = check_covariance_arguments(cam_model, cam_nparams, cam_const, cam_x, points, obs_cam, obs_pt, obs_uv, loss, f_scale)
        con = check_constraint_arguments(groups_a, groups_b, distances, weights)
        struct = None if null_struct else constraint_struct(con)
        self.calls += 1
        self.constrained_calls += con is not None
        lib = harness()
        gauge, rows = C.c_int32(0), C.c_int64(0)
        n_rows = 0 if con is None or null_struct else int(np.count_nonzero(con["weights"] > 0))
        res = run_covariance_call(lambda d, o: lib.cch_parameter_covariance_constrained(d, C.byref(struct) if struct is not None else None, o, C.byref(gauge),
                                                                                        C.byref(rows)),
                                  args, "cba_parameter_covariance_constrained", last_error, n_constraint_rows=n_rows)
        assert (gauge.value, rows.value) == (res.gauge_dim, res.n_constraint_rows)  # what the binding reports is what the plan did
        return res


def _desc(args):
    from caliscope_amd._lib import ptr

    return CovDesc(n_cams=len(args["cam_model"]), n_points=len(args["points"]), n_obs=len(args["obs_cam"]), cam_model=ptr(args["cam_model"]),
                   cam_nparams=ptr(args["cam_nparams"]), cam_const=ptr(args["cam_const"]), cam_x=ptr(args["cam_x"]), points=ptr(args["points"]),
                   obs_cam=ptr(args["obs_cam"]), obs_pt=ptr(args["obs_pt"]), obs_uv=ptr(args["obs_uv"]), loss=args["loss"], f_scale=args["f_scale"])


def plan(n_points, groups_a, groups_b, distances, weights, eight=None, cap=None):
    """The host plan as a dict of int64 arrays (PLAN_ARRAYS) and sizes; ``eight``: the positional arguments of the call, for the camera tables.
    Raises RuntimeError(code, message) when the plan refuses."""
    lib = harness()
    con = check_constraint_arguments(groups_a, groups_b, distances, weights)
    struct = constraint_struct(con)
    args = check_covariance_arguments(*eight, "linear", 1.0) if eight is not None else None
    desc = _desc(args) if args is not None else None
    sizes = np.zeros(8, dtype=np.int64)
    rc = lib.cch_plan(int(n_points), C.byref(desc) if desc is not None else None, C.byref(struct), constants()["cap"] if cap is None else int(cap), sizes.ctypes.data_as(I64))
    if rc:
        raise RuntimeError(rc, last_error())
    n_rows, n_comp, max_m, n_pts, n_free, n_cc, n_cobs, n_entries = (int(v) for v in sizes)
    with_tables = desc is not None and n_rows > 0
    lengths = dict(comp_pt=n_comp + 1, pts=n_pts, comp_row=n_comp + 1, row_src=n_rows, row_loc=8 * n_rows, free_pts=n_free, comp_cam=n_comp + 1 if with_tables else 0,
                   cams=n_cc, cc_obs=n_cc + 1 if with_tables else 0, obs_pos=n_cobs, obs_loc=n_cobs, entry_start=int(n_points) + 1 if with_tables else 0, entry_cam=n_entries)
    out = dict(n_rows=n_rows, n_comp=n_comp, max_m=max_m)
    for which, name in enumerate(PLAN_ARRAYS):
        arr = np.zeros(max(lengths[name], 1), dtype=np.int64)
        if n_rows and lengths[name]:
            lib.cch_plan_copy(which, arr.ctypes.data_as(I64))
        out[name] = arr[: lengths[name] if n_rows else 0]
    if with_tables:
        out["device_bytes"] = float(lib.cch_device_bytes(C.byref(desc)))
    return out


def constraint_row(points, pt8, dist, weight, loss="linear", f_scale=1.0):
    """(rho, u[3], coef[8]) of one row by the shared per-row arithmetic."""
    from caliscope_amd.uncertainty import LOSSES

    points, pt8 = np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(pt8, dtype=np.int32)
    u, coef = np.zeros(3), np.zeros(8)
    rho = harness().cch_row(points.ctypes.data_as(F64), pt8.ctypes.data_as(I32), float(dist), float(weight), LOSSES[loss], float(f_scale), u.ctypes.data_as(F64),
                            coef.ctypes.data_as(F64))
    return float(rho), u, coef


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def board(n_cams=5, n_frames=6, rows=3, cols=4, sigma_m=0.002):
    """tests.constrained_scene.board_scene at its start vector as dict(par, x, cam, obj, uv, con=(ga, gb, dist, w), base)."""
    from tests.constrained_scene import board_scene

    sc = board_scene(n_cams=n_cams, n_frames=n_frames, rows=rows, cols=cols, sigma_m=sigma_m)
    par, x = sc["par"], sc["x0"]
    return dict(par=par, x=x, cam=np.ascontiguousarray(sc["cam"]), obj=np.ascontiguousarray(sc["obj"]), uv=np.ascontiguousarray(sc["uv"]), con=sc["constraints"], base=sc)


MIXED_EXTRA = 5        # unconstrained points appended to the mixed scene
MIXED_SINGLE = 12      # frame 1, corner 0: left with one observation
MIXED_BLIND = (2, 3)   # camera 2 sees nothing of frame 3's board
MIXED_TWICE = (0, 29)  # camera 0's observation of frame 2, corner 5 is there twice


def mixed():
    """board() with: MIXED_EXTRA points in no row seen by every camera appended, one corner left with a single observation, one camera that sees
    nothing of one component, one (camera, point) observation inside a component given twice."""
    from caliscope_amd.bundle_parameterization import BundleParameterization
    from caliscope_amd.synthetic import project_pinhole_bc5

    sc = board()
    base, n_per = sc["base"], sc["base"]["n_per"]
    ncp = sc["par"].n_camera_params
    n_pts = (len(sc["x"]) - ncp) // 3
    rng = np.random.default_rng(11)
    extra = rng.uniform(-0.25, 0.25, (MIXED_EXTRA, 3)) + [0.0, 0.0, 0.6]
    cam, obj, uv = [sc["cam"]], [sc["obj"]], [sc["uv"]]
    for c, camera in sorted(base["cameras_true"].cameras.items()):
        K = camera.matrix
        p, z = project_pinhole_bc5(extra, camera.rotation, camera.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], camera.distortions)
        assert (z > 0).all()
        cam.append(np.full(MIXED_EXTRA, c)); obj.append(n_pts + np.arange(MIXED_EXTRA)); uv.append(p + rng.normal(0, 0.4, p.shape))
    cam, obj, uv = np.concatenate(cam).astype(np.int32), np.concatenate(obj).astype(np.int32), np.vstack(uv)
    keep = np.ones(len(cam), dtype=bool)
    keep[np.flatnonzero(obj == MIXED_SINGLE)[1:]] = False
    keep[(cam == MIXED_BLIND[0]) & (obj // n_per == MIXED_BLIND[1]) & (obj < n_pts)] = False
    again = int(np.flatnonzero((cam == MIXED_TWICE[0]) & (obj == MIXED_TWICE[1]))[0])
    order = np.concatenate([np.flatnonzero(keep), [again]])
    par = BundleParameterization.from_camera_array(base["cameras_init"], n_points=n_pts + MIXED_EXTRA, refine_intrinsics=False)
    x = np.concatenate([sc["x"], (extra + rng.normal(0, 0.01, extra.shape)).reshape(-1)])
    return dict(par=par, x=x, cam=np.ascontiguousarray(cam[order]), obj=np.ascontiguousarray(obj[order]), uv=np.ascontiguousarray(uv[order]), con=sc["con"], base=base)


def free_intrinsics():
    """board() with nine-wide cameras.  The boards alone fill a small part of every image and leave k1 and k2 almost undetermined (the two CPU
    formulations then disagree by 1e-5: too weak to test with), so 300 points in no row fill the field of view, as tests.covariance_native.wide_scene
    does for the unconstrained call: every one in front of and inside the image of the cameras that observe it."""
    from caliscope_amd.bundle_parameterization import BundleParameterization
    from caliscope_amd.synthetic import project_pinhole_bc5

    sc = board()
    base = sc["base"]
    pts0 = sc["x"][sc["par"].n_camera_params:].reshape(-1, 3)
    n_pts, n_extra = len(pts0), 300
    rng = np.random.default_rng(7)
    extra = rng.uniform(-0.9, 0.9, (n_extra, 3)) * [1.0, 1.0, 0.6] + [0.0, 0.0, 0.6]
    cam, obj, uv = [sc["cam"]], [sc["obj"]], [sc["uv"]]
    for c, camera in sorted(base["cameras_true"].cameras.items()):
        K = camera.matrix
        p, z = project_pinhole_bc5(extra, camera.rotation, camera.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], camera.distortions)
        ok = (z > 0) & (p[:, 0] > 0) & (p[:, 0] < camera.size[0]) & (p[:, 1] > 0) & (p[:, 1] < camera.size[1])
        cam.append(np.full(ok.sum(), c)); obj.append(n_pts + np.flatnonzero(ok)); uv.append(p[ok] + rng.normal(0, 0.4, (ok.sum(), 2)))
    cam, obj, uv = np.concatenate(cam).astype(np.int32), np.concatenate(obj).astype(np.int32), np.vstack(uv)
    assert np.bincount(obj, minlength=n_pts + n_extra).min() >= 2
    par = BundleParameterization.from_camera_array(base["cameras_init"], n_points=n_pts + n_extra, refine_intrinsics=True)
    x = par.pack(base["cameras_init"], np.vstack([pts0, extra + rng.normal(0, 0.005, extra.shape)]))
    return dict(par=par, x=x, cam=np.ascontiguousarray(cam), obj=np.ascontiguousarray(obj), uv=np.ascontiguousarray(uv), con=sc["con"], base=base)


_SCENES = {}
SCENE_BUILDERS = {"board": board, "mixed": mixed, "free intrinsics": free_intrinsics}  # (tests/covariance_constrained_edge_scenes.py adds its own)


def key_scene(key):
    """Scenes by hashable key, built once and never written to: ("board", n_cams, n_frames, rows, cols, sigma_m), ("mixed",), ("free intrinsics",),
    and the keys of the builders other modules put into SCENE_BUILDERS."""
    if key not in _SCENES:
        _SCENES[key] = SCENE_BUILDERS[key[0]](*key[1:])
    return _SCENES[key]


TWO_BY_TWO = ("board", 3, 2, 2, 2, 0.002)   # scene 1: four-point components, a centroid row with coincident endpoints
DEFAULT = ("board", 5, 6, 3, 4, 0.002)      # scene 2: 12 points and 30 rows a component, a true centroid row
MANY_ROWS = ("board", 4, 3, 5, 5, 0.002)    # scene 3: 25 points, 73 rows
MIXED = ("mixed",)                                  # scene 4
FREE_INTRINSICS = ("free intrinsics",)              # scene 5: scene 2 nine wide, with free points that fill the field of view
CAP = ("board", 4, 1, 6, 9, 0.002)          # scene 6: one component of exactly 54 points
TIGHT = ("board", 5, 6, 3, 4, 0.0005)       # scene 9: the rows ten times stronger (in the cofactor: a hundred)
LOOSE = ("board", 5, 6, 3, 4, 0.005)


def call_arguments(sc):
    """The twelve positional arguments of ``parameter_covariance_constrained``."""
    ga, gb, dist, w = sc["con"]
    return (*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]), ga, gb, dist, w)


# ---- the two CPU formulations -----------------------------------------------------------------------------------------------------------
def robust_jacobian(sc, loss="linear", f_scale=1.0):
    """(J dense with the constraint rows, cost, row scales js) by the oracle, every row scaled as scipy's least_squares scales it."""
    from oracle.residuals import joint_jacobian, joint_residuals

    ga, gb, dist, w = sc["con"]
    J = joint_jacobian(sc["x"], sc["par"], sc["cam"], sc["uv"], sc["obj"], ga, gb, dist, w).toarray()
    f = joint_residuals(sc["x"], sc["par"], sc["cam"], sc["uv"], sc["obj"], ga, gb, dist, w)
    js, cost = cn.robust_row_scale(f, loss, f_scale)
    return J * js[:, None], cost, js, f


def bordered_blocks(J, N6, ncp):
    """The bordered formula with V~ = V + C^T C inverted densely and six gauge columns, in numpy: (pinv_cc, 3 x 3 diagonal blocks of pinv_pp)."""
    H = J.T @ J
    U, W, Vt = H[:ncp, :ncp], H[:ncp, ncp:], H[ncp:, ncp:]
    Vinv = np.linalg.inv(Vt)
    Nc, Np = N6[:ncp], N6[ncp:]
    Y, Z = W @ Vinv, Vinv @ Np
    D = Np.T @ Z
    B = Nc - W @ Z
    Dinv = np.linalg.inv(D)
    St = U - Y @ W.T + B @ Dinv @ B.T
    Cm = np.linalg.inv(0.5 * (St + St.T))
    n_pts = (J.shape[1] - ncp) // 3
    pp = np.zeros((n_pts, 3, 3))
    for i in range(n_pts):
        s = slice(3 * i, 3 * i + 3)
        T = Y[:, s].T + Z[s] @ Dinv @ B.T
        pp[i] = Vinv[s, s] - Z[s] @ Dinv @ Z[s].T + T @ Cm @ T.T
    return Cm, pp


@functools.lru_cache(maxsize=None)
def _reference(key, loss, f_scale):
    sc = key_scene(key)
    J, cost, js, f = robust_jacobian(sc, loss, f_scale)
    ncp = sc["par"].n_camera_params
    cc, pp, lam = cn.pinv_blocks(J, ncp, gauge=6)
    N6 = cn.gauge_matrix(sc["par"], sc["x"])[:, :6]
    bc, bp = bordered_blocks(J, N6, ncp)
    dof = J.shape[0] - J.shape[1] + 6
    n_con = len(sc["con"][2])
    return dict(cc=cc, pp=pp, lam=lam, dis_c=cn._rel(bc, cc), dis_p=cn._rel_blocks(bp, pp), sigma0_sq=2.0 * cost / dof, dof=dof, cost=cost,
                jn=float(np.abs(J @ N6).max()), js_con=js[len(js) - n_con:], f_con=f[len(f) - n_con:])


def reference(key, loss="linear", f_scale=1.0):
    """The pinv reference of a scene and the disagreement of the two CPU formulations, computed once and shared."""
    return _reference(key, loss, float(f_scale))


def check_against_pinv(result, key, loss="linear", f_scale=1.0, report=print):
    """tests.covariance_native.check_result_against_pinv with six null directions for a scene of this module, and: the call reports six gauge
    columns and the rows of positive weight.  Returns the measured figures."""
    sc = key_scene(key)
    assert result.gauge_dim == 6 and result.n_constraint_rows == int(np.count_nonzero(sc["con"][3] > 0))
    return cn.check_result_against_pinv(result, reference(key, loss, f_scale), sc["par"], 6, report, key=key, loss=loss)
