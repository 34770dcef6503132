"""Scenes that put cba_parameter_covariance and cba_observation_reliability at the edges of their loops (tests/test_covariance_edges.py on
the CPU, tests/test_covariance_edges_gpu.py on the device), by key for covariance_native.key_scene; the bordered formula restated
block-sparsely, which is the second CPU formulation where a dense J^T J is out of reach; and the recorded reference of MANY_POINTS
(tests/golden/covariance_many_points.npz, written by tests/golden/make_covariance_many_points_fixture.py) with its comparison.

    MANY_VIEWS         65 six-wide fisheye cameras x 60 points, every point in every camera: ncp = 390, 13 blocks, the last of six rows
    MANY_VIEWS_RAGGED  the same with point 0 at exactly 64 views, point 1 at 65, point 2 at two and one row of point 3 twice (66 rows)
    REL_VIEWS(_RAGGED) both with 30 points, for the reliability call (its dense projector is (2 n_obs)^2)
    MANY_VIEWS_MIXED   66 cameras, a free pinhole at every seventh index among fisheye ones: ncp = 426, 14 blocks, the last of ten rows
    LIMIT_SIX / _NINE  192 six-wide / 128 nine-wide cameras x 40 points: ncp = 1152 = COV_MAX_NCP, 36 whole blocks
    BELOW_LIMIT        190 six-wide fisheye cameras and one free pinhole: ncp = 1149, 36 blocks, the last of 29 rows
    OVER_LIMIT         193 six-wide cameras: ncp = 1158, refused
    OBS_256 / OBS_257  four cameras x 64 points, and the same with one (camera, point) row twice
    POINTS_256 / _257  three cameras x 256 and 257 points
    MANY_POINTS        three cameras x 65 793 points (197 379 observations): a second trip of k_unc_d's grid-stride loop
"""
from __future__ import annotations

import functools
import hashlib
from pathlib import Path

import numpy as np

from tests import covariance_native as cn

GOLDEN = Path(__file__).resolve().parent / "golden"
MANY_POINTS_FIXTURE = GOLDEN / "covariance_many_points.npz"

MANY_VIEWS = ("wide", (6,) * 65, True, 60)
MANY_VIEWS_RAGGED = ("many_views_ragged", 60)
REL_VIEWS = ("wide", (6,) * 65, True, 30)
REL_VIEWS_RAGGED = ("many_views_ragged", 30)
MANY_VIEWS_MIXED = ("wide", tuple(9 if c % 7 == 0 else 6 for c in range(66)), True, 60)
LIMIT_SIX = ("wide", (6,) * 192, False, 40)
LIMIT_NINE = ("wide", (9,) * 128, False, 40)
BELOW_LIMIT = ("wide", (6,) * 190 + (9,), True, 40)
OVER_LIMIT = ("wide", (6,) * 193, False, 40)
OBS_256 = ("wide", (6, 6, 6, 6), False, 64)
OBS_257 = ("repeated", OBS_256, 100)
POINTS_256 = ("wide", (6, 6, 6), False, 256)
POINTS_257 = ("wide", (6, 6, 6), False, 257)
MANY_POINTS = ("wide", (6, 6, 6), False, 65536 + 257)
MANY_POINTS_SAMPLE = (0, 255, 256, 65535, 65536, 65792, 1000, 30000)  # the ends of k_unc_d's blocks and of its first grid trip, and two inside


def _rows(sc, order):
    return dict(par=sc["par"], x=sc["x"], cam=np.ascontiguousarray(sc["cam"][order]), obj=np.ascontiguousarray(sc["obj"][order]),
                uv=np.ascontiguousarray(sc["uv"][order]))


def repeated_scene(base, row):
    """The scene of key ``base`` with observation ``row`` once more behind its last row."""
    sc = cn.key_scene(base)
    return _rows(sc, np.concatenate([np.arange(len(sc["obj"])), [row]]))


def many_views_ragged_scene(n_points):
    """65 six-wide fisheye cameras, ``n_points`` points seen by all of them, then, as covariance_native.ragged_scene does it: point 0 loses
    its last view (64 left: the last whole trip of a wave over the views), point 1 keeps all 65, point 2 keeps its first two, and the
    second observation of point 3 is there twice (66 rows)."""
    sc = cn.key_scene(("wide", (6,) * 65, True, n_points))
    obj = sc["obj"]
    assert np.all(np.bincount(obj, minlength=n_points) == 65)
    keep = np.ones(len(obj), dtype=bool)
    keep[np.flatnonzero(obj == 0)[64:]] = False
    keep[np.flatnonzero(obj == 2)[2:]] = False
    again = int(np.flatnonzero(obj == 3)[1])
    return _rows(sc, np.concatenate([np.flatnonzero(keep), [again]]))


cn.SCENE_BUILDERS["repeated"] = repeated_scene
cn.SCENE_BUILDERS["many_views_ragged"] = many_views_ragged_scene


def describe(key):
    """What a scene is, for the assertions of the tests: dict(ncp, blocks, last_rows, n_obs, n_points, views (per point), cam_obs (per camera),
    repeated (rows beyond the distinct (camera, point) pairs))."""
    sc = cn.key_scene(key)
    ncp, n_points = sc["par"].n_camera_params, sc["par"].n_points
    pairs = np.stack([sc["cam"], sc["obj"]], axis=1)
    return dict(ncp=ncp, blocks=-(-ncp // 32), last_rows=ncp - 32 * ((ncp - 1) // 32), n_obs=len(sc["obj"]), n_points=n_points,
                views=np.bincount(sc["obj"], minlength=n_points), cam_obs=np.bincount(sc["cam"], minlength=len(sc["par"].blocks)),
                repeated=len(pairs) - len(np.unique(pairs, axis=0)))


# ---- the bordered formula, block-sparse --------------------------------------------------------------------------------------------------
def observation_blocks(sc):
    """(A (n_obs, 2, 9) zero-padded, B (n_obs, 2, 3), cost) from the oracle's sparse Jacobian and residuals (linear loss)."""
    from oracle.residuals import joint_jacobian, joint_residuals

    par, x, cam, obj = sc["par"], sc["x"], sc["cam"], sc["obj"]
    ncp, n_obs = par.n_camera_params, len(cam)
    J = joint_jacobian(x, par, cam, sc["uv"], obj).tocoo()
    assert J.shape == (2 * n_obs, len(x))
    off = np.asarray(par.camera_param_offsets)
    o, i = J.row // 2, J.row % 2
    A, B = np.zeros((n_obs, 2, 9)), np.zeros((n_obs, 2, 3))
    c = J.col < ncp
    loc = J.col[c] - off[cam[o[c]]]
    assert loc.min() >= 0 and loc.max() < 9
    np.add.at(A, (o[c], i[c], loc), J.data[c])
    loc = J.col[~c] - ncp - 3 * obj[o[~c]]
    assert loc.min() >= 0 and loc.max() < 3
    np.add.at(B, (o[~c], i[~c], loc), J.data[~c])
    f = joint_residuals(x, par, cam, sc["uv"], obj)
    return A, B, 0.5 * float(f @ f)


def sparse_bordered_blocks(sc):
    """covariance_native.bordered_blocks without a dense J^T J: per-observation W blocks, per-point 3 x 3 V, sums by einsum.  The same
    arithmetic in another order; only the camera block (ncp x ncp) is dense.  Returns dict(cc, pp, cost, dof)."""
    par, x, cam, obj = sc["par"], sc["x"], sc["cam"], sc["obj"]
    ncp, n_points = par.n_camera_params, par.n_points
    off = np.asarray(par.camera_param_offsets)
    width = np.array([b.n_params for b in par.blocks])
    A, B, cost = observation_blocks(sc)
    N = cn.gauge_matrix(par, x)
    Nc, Np = N[:ncp], N[ncp:].reshape(n_points, 3, 7)
    U = np.zeros((ncp, ncp))
    W = np.zeros((n_points, ncp, 3))  # W[p, rows of camera a] = sum of A_o^T B_o over the observations of p in a
    AtA, AtB = np.einsum("oir,oiq->orq", A, A), np.einsum("oir,oiq->orq", A, B)
    r9 = np.arange(9)
    for c_, (o_, w_) in enumerate(zip(off, width)):
        sel = np.flatnonzero(cam == c_)
        U[o_: o_ + w_, o_: o_ + w_] = AtA[sel][:, :w_, :w_].sum(axis=0)
        np.add.at(W, (obj[sel][:, None], (o_ + r9[:w_])[None, :]), AtB[sel][:, :w_])
    V = np.zeros((n_points, 3, 3))
    np.add.at(V, obj, np.einsum("oip,oiq->opq", B, B))
    Vinv = np.linalg.inv(V)
    Y = np.einsum("pci,pij->pcj", W, Vinv)
    Z = np.einsum("pij,pjg->pig", Vinv, Np)
    D = np.einsum("pig,pih->gh", Np, Z)
    Bm = Nc - np.einsum("pci,pig->cg", W, Z)
    Dinv = np.linalg.inv(D)
    St = U - np.einsum("pci,pdi->cd", Y, W) + Bm @ Dinv @ Bm.T
    C = np.linalg.inv(0.5 * (St + St.T))
    T = np.swapaxes(Y, 1, 2) + np.einsum("pig,gh,ch->pic", Z, Dinv, Bm)
    pp = Vinv - np.einsum("pig,gh,pjh->pij", Z, Dinv, Z) + np.einsum("pic,cd,pjd->pij", T, C, T)
    return dict(cc=C, pp=pp, cost=cost, dof=2 * len(obj) - len(x) + 7)


# ---- MANY_POINTS against its recorded reference -------------------------------------------------------------------------------------------
def scene_hash(sc):
    """SHA-256 over the bytes of the scene's parameter vector and observation arrays."""
    h = hashlib.sha256()
    for name, dtype in (("x", np.float64), ("cam", np.int32), ("obj", np.int32), ("uv", np.float64)):
        h.update(np.ascontiguousarray(sc[name], dtype=dtype).tobytes())
    return h.hexdigest()


@functools.cache
def many_points_reference():
    """The recorded blocks of pinv(J^T J) of MANY_POINTS (refused unless the scene rebuilt from its seed has the recorded hash), the
    block-sparse restatement on the same scene, and their disagreement: dict(cc, idx, pp, bc, bp, dis_c, dis_p, dof, cost, sigma0_sq)."""
    sc = cn.key_scene(MANY_POINTS)
    with np.load(MANY_POINTS_FIXTURE) as z:
        fix = {k: z[k] for k in z.files}
    assert scene_hash(sc) == str(fix["sha256"]), "tests/golden/covariance_many_points.npz was recorded on another scene"
    idx = fix["point_index"]
    assert tuple(idx) == MANY_POINTS_SAMPLE
    sp = sparse_bordered_blocks(sc)
    dof, cost = int(fix["dof"]), float(fix["cost"])
    assert sp["dof"] == dof == 2 * 197379 - (18 + 3 * 65793) + 7 and abs(sp["cost"] - cost) <= 1e-13 * cost
    assert float(fix["sigma0_sq"]) == 2.0 * cost / dof
    ref = dict(cc=fix["cam_block"], idx=idx, pp=fix["point_blocks"], bc=sp["cc"], bp=sp["pp"], dof=dof, cost=cost, sigma0_sq=2.0 * cost / dof,
               dis_c=cn._rel(sp["cc"], fix["cam_block"]), dis_p=cn._rel_blocks(sp["pp"][idx], fix["point_blocks"]))
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def check_many_points(result, report=print, **labels):
    """The tolerance rule of covariance_native.check_result_against_pinv with the recorded blocks as the reference and the block-sparse
    restatement as the second formulation: their disagreement at most 1e-8; the code under test within ten times it, floor 1e-12, of the
    recorded camera block and of the recorded point blocks; every other point within the same bar of the restatement; dof equal, cost and
    sigma0^2 to 1e-12 relative.  Returns the measured figures."""
    ref = many_points_reference()
    assert ref["dis_c"] <= 1e-8 and ref["dis_p"] <= 1e-8, (ref["dis_c"], ref["dis_p"])
    s2, idx = ref["sigma0_sq"], ref["idx"]
    err_c = cn._rel(result.cam_cov_full, s2 * ref["cc"])
    err_p = cn._rel_blocks(result.point_cov[idx], s2 * ref["pp"])
    err_rest = cn._rel_blocks(result.point_cov, s2 * ref["bp"])
    figures = dict(**labels, dis_c=ref["dis_c"], dis_p=ref["dis_p"], err_c=err_c, err_p=err_p, err_rest=err_rest,
                   err_cost=abs(result.cost - ref["cost"]) / ref["cost"])
    report(figures)
    assert result.point_cov.shape == (65536 + 257, 3, 3)
    assert result.dof == ref["dof"]
    assert abs(result.cost - ref["cost"]) <= 1e-12 * ref["cost"] and abs(result.sigma0_sq - s2) <= 1e-12 * s2, figures
    assert err_c <= max(10.0 * ref["dis_c"], 1e-12), figures
    assert err_p <= max(10.0 * ref["dis_p"], 1e-12) and err_rest <= max(10.0 * ref["dis_p"], 1e-12), figures
    assert np.array_equal(result.cam_cov[:, :6, :6], np.stack([result.cam_cov_full[6 * c: 6 * c + 6, 6 * c: 6 * c + 6] for c in range(3)]))
    assert not result.cam_cov[:, 6:].any() and not result.cam_cov[:, :, 6:].any()
    return figures
