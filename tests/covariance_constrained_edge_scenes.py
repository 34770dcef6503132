"""Scenes that put cba_parameter_covariance_constrained and cba_observation_reliability_constrained at the edges of the loops of their five
kernels (tests/test_covariance_constrained_edges.py on the CPU, tests/test_covariance_constrained_edges_gpu.py on the device), by key for
covariance_constrained_native.key_scene (and so for reliability_constrained_native.key_scene).  Every scene is
covariance_native.wide_scene (cameras on a ring, points filling the field of view, every camera seeing every point, nine-wide pinhole
beside six-wide fisheye cameras allowed) with rigid bodies declared among its points: boards alone leave k1 and k2 of a nine-wide camera
undetermined (covariance_constrained_native.free_intrinsics says by how much).

    NINE_MIXED             nine cameras of widths 9 6 6 9 6 6 9 6 6 (offsets 0 9 15 21 30 36 42 51 57, ncp = 63), 120 points, components of
                           4, 12, 2 and 8 points; camera 4 sees one point of the first, camera 7 nothing of the second: 57 rows
    NINE_MIXED_RELABELLED  the same with the 120 point labels permuted: the components lie among each other and among the free points
    SIXTY_FIVE             65 six-wide fisheye cameras (ncp = 390), 30 points, components of 2, 4 and 3 points; camera 64 is blind to the second
    STICKS_257             three six-wide pinhole cameras, 514 points in 257 components of two points and one row each: no free point
    STICKS_256             the same with the weight of the caller's last row zero: 256 rows, two free points
    STICKS_256_KEPT        the adjustment STICKS_256 asks for, stated without the row of weight zero: what its references are formed on
    SIZES                  four six-wide fisheye cameras, 100 points, components of 54 (COV_COMPONENT_CAP), 4, 2 and 2 points: 165 rows
    SIZES_OVER_CAP         SIZES with point 54 tied to point 53: a component of 55 points, refused
"""
from __future__ import annotations

import numpy as np

from tests import covariance_constrained_native as ccn
from tests import covariance_native as cn

FOCAL = 500.0  # of every camera of covariance_native.wide_scene: a row's weight is (1 px / FOCAL) / sigma_m, as tests.constrained_scene weighs its rows

NINE_WIDTHS = (9, 6, 6, 9, 6, 6, 9, 6, 6)
NINE_GROUPS = (tuple(range(0, 4)), tuple(range(10, 22)), (30, 31), tuple(range(40, 48)))
NINE_ONE_POINT = (4, 0)   # camera 4 keeps its view of point 0 alone among the points of the first component
NINE_BLIND = (7, 1)       # camera 7 sees nothing of the second component
SIXTY_FIVE_GROUPS = ((0, 1), (5, 6, 7, 8), (12, 13, 14))
SIXTY_FIVE_BLIND = (64, 1)
N_STICKS = 257
SIZES_GROUPS = (tuple(range(0, 54)), (60, 61, 62, 63), (70, 71), (80, 81))

NINE_MIXED = ("rigid edges", "nine_mixed")
NINE_MIXED_RELABELLED = ("rigid edges", "nine_mixed_relabelled")
SIXTY_FIVE = ("rigid edges", "sixty_five")
STICKS_257 = ("rigid edges", "sticks_257")
STICKS_256 = ("rigid edges", "sticks_256")
STICKS_256_KEPT = ("rigid edges", "sticks_256_kept")
SIZES = ("rigid edges", "sizes")
SIZES_OVER_CAP = ("rigid edges", "sizes_over_cap")


def rigid(sc, groups, sigma_m=0.002, seed=1):
    """``sc`` with constraint rows that make a rigid body of every group of points: in the group's listed order the corner rows
    (g[i], g[i + d]) for d = 1, 2, 3 (each endpoint one point four times, as tests.constrained_scene.board_scene encodes a corner) and, for
    a group of eight points or more, one centroid row of its first four points against its last four.  The distance of a row is the one the
    points of ``sc['x']`` have plus N(0, sigma_m); its weight (1 / FOCAL) / sigma_m."""
    rng = np.random.default_rng(seed)
    pts = sc["x"][sc["par"].n_camera_params:].reshape(-1, 3)
    ga, gb, dist = [], [], []
    for g in groups:
        ends = [([g[i]] * 4, [g[i + d]] * 4) for d in (1, 2, 3) for i in range(len(g) - d)]
        if len(g) >= 8:
            ends.append((list(g[:4]), list(g[-4:])))
        for a, b in ends:
            ga.append(a); gb.append(b)
            dist.append(float(np.linalg.norm(pts[a].mean(axis=0) - pts[b].mean(axis=0))) + rng.normal(0.0, sigma_m))
    con = (np.array(ga, dtype=np.int32), np.array(gb, dtype=np.int32), np.array(dist), np.full(len(dist), (1.0 / FOCAL) / sigma_m))
    return dict(sc, con=con)


def drop(sc, mask):
    """``sc`` without the observation rows of ``mask``."""
    keep = ~np.asarray(mask, dtype=bool)
    return dict(sc, cam=np.ascontiguousarray(sc["cam"][keep]), obj=np.ascontiguousarray(sc["obj"][keep]), uv=np.ascontiguousarray(sc["uv"][keep]))


def relabel(sc, perm):
    """``sc`` with point p renamed perm[p], in the parameter vector, the observations and both group arrays; no row changes its place."""
    perm = np.asarray(perm)
    ncp = sc["par"].n_camera_params
    pts = sc["x"][ncp:].reshape(-1, 3)
    moved = np.empty_like(pts)
    moved[perm] = pts
    ga, gb, dist, w = sc["con"]
    return dict(sc, x=np.concatenate([sc["x"][:ncp], moved.reshape(-1)]), obj=np.ascontiguousarray(perm[sc["obj"]].astype(np.int32)),
                con=(perm[ga].astype(np.int32), perm[gb].astype(np.int32), dist, w), perm=perm)


def views(sc, camera, points):
    """The mask of the observations of ``points`` by ``camera``."""
    return (sc["cam"] == camera) & np.isin(sc["obj"], points)


def _nine_mixed():
    sc = rigid(cn.key_scene(("wide", NINE_WIDTHS, True, 120)), NINE_GROUPS)
    sc = drop(sc, views(sc, NINE_ONE_POINT[0], NINE_GROUPS[0][1:]))
    return drop(sc, views(sc, NINE_BLIND[0], NINE_GROUPS[NINE_BLIND[1]]))


def _nine_mixed_relabelled():
    return relabel(ccn.key_scene(NINE_MIXED), np.random.default_rng(9).permutation(120))


def _sixty_five():
    sc = rigid(cn.key_scene(("wide", (6,) * 65, True, 30)), SIXTY_FIVE_GROUPS)
    return drop(sc, views(sc, SIXTY_FIVE_BLIND[0], SIXTY_FIVE_GROUPS[SIXTY_FIVE_BLIND[1]]))


def _sticks_257():
    return rigid(cn.key_scene(("wide", (6, 6, 6), False, 2 * N_STICKS)), [(2 * i, 2 * i + 1) for i in range(N_STICKS)])


def _sticks_256():
    sc = ccn.key_scene(STICKS_257)
    ga, gb, dist, w = sc["con"]
    w = w.copy()
    w[-1] = 0.0
    return dict(sc, con=(ga, gb, dist, w))


def _sticks_256_kept():
    ga, gb, dist, w = ccn.key_scene(STICKS_256)["con"]
    return dict(ccn.key_scene(STICKS_256), con=(ga[:-1], gb[:-1], dist[:-1], w[:-1]))


def _sizes():
    return rigid(cn.key_scene(("wide", (6, 6, 6, 6), True, 100)), SIZES_GROUPS)


def _sizes_over_cap():
    sc = ccn.key_scene(SIZES)
    ga, gb, dist, w = sc["con"]
    return dict(sc, con=(np.vstack([ga, [[53] * 4]]).astype(np.int32), np.vstack([gb, [[54] * 4]]).astype(np.int32), np.append(dist, 0.3), np.append(w, 1.0)))


_BUILDERS = dict(nine_mixed=_nine_mixed, nine_mixed_relabelled=_nine_mixed_relabelled, sixty_five=_sixty_five, sticks_257=_sticks_257, sticks_256=_sticks_256,
                 sticks_256_kept=_sticks_256_kept, sizes=_sizes, sizes_over_cap=_sizes_over_cap)
ccn.SCENE_BUILDERS["rigid edges"] = lambda name: _BUILDERS[name]()


def describe(key):
    """What a scene is, from the host plan of its call and its arrays: dict(n_rows, n_comp, max_m, n_free, n_obs, ncp, widths, offsets,
    members (per component its points, ascending), cams (per component its cameras, ascending), cc_obs (per component, per camera of it, the
    local indices of the points its observations are of), entries (per point), plan)."""
    sc = ccn.key_scene(key)
    twelve = ccn.call_arguments(sc)
    p = ccn.plan(len(twelve[4]), *twelve[8:], eight=twelve[:8])
    n_comp = p["n_comp"]
    members = [p["pts"][p["comp_pt"][k]: p["comp_pt"][k + 1]].tolist() for k in range(n_comp)]
    cams = [p["cams"][p["comp_cam"][k]: p["comp_cam"][k + 1]].tolist() for k in range(n_comp)]
    cc_obs = [[p["obs_loc"][p["cc_obs"][q]: p["cc_obs"][q + 1]].tolist() for q in range(p["comp_cam"][k], p["comp_cam"][k + 1])] for k in range(n_comp)]
    return dict(n_rows=p["n_rows"], n_comp=n_comp, max_m=p["max_m"], n_free=len(p["free_pts"]), n_obs=len(sc["obj"]), ncp=sc["par"].n_camera_params,
                widths=tuple(b.n_params for b in sc["par"].blocks), offsets=tuple(int(o) for o in sc["par"].camera_param_offsets), members=members, cams=cams,
                cc_obs=cc_obs, entries=np.diff(p["entry_start"]), plan=p)
