"""Scenes that reach the special branches of the Schur and constraint kernels (tests/test_kernel_edges_gpu.py; their planning properties are
checked without a GPU in tests/test_kernel_edge_scenes.py).

* ``sparse_id_scene``: observed points only at every ``stride``-th id, long runs of unobserved ids before the first and after the last, and one
  static-marker point seen ``heavy_obs`` times by the same few cameras.  A chunk of 256 observations then spans more than 256 (stride 5) or
  more than 512 (stride 8) point ids, so the loops of k_build / k_backsub / k_backsub_rec over "points beyond the first 256" run, and
  k_build_cs is refused a chunk range above 512 ids.
* ``component_scene``: constraint components of a chosen number of rows over a chosen number of points, built directly as (ga, gb, dist, w).
"""
from __future__ import annotations

from itertools import combinations

import numpy as np

from caliscope_amd.bundle_parameterization import BundleParameterization
from caliscope_amd.synthetic import make_scene, project_pinhole_bc5

CHUNK = 256        # observations per chunk (csrc/cba_kernels.h CHUNK)
CS_MAX_PTS = 512   # point ids per super-chunk of k_build_cs (csrc/cba_kernels.h CS_MAX_PTS)
NB = 32            # pivot block of the small-component Cholesky (csrc/chol_schedule.h NB)
CON_SMALL_M = 2 * NB
CON_SMALL_LDS = 120 * 1024


def _project(cam, X):
    K = cam.matrix
    uv, _ = project_pinhole_bc5(np.atleast_2d(X), cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
    return uv


def sparse_id_scene(stride: int, heavy_obs: int | None = 256, refine: bool = False, n_observed: int = 600, lead: int = 300, tail: int = 300,
                    seed: int = 11) -> dict:
    """Six cameras.  Observed point j has id ``lead + stride * j`` and 3 views (2 for every fourth point: 11 observations per 4 points);
    the point in the middle is instead seen ``heavy_obs`` times, its three cameras in turn (a static marker seen again in every frame;
    None: no marker)."""
    sc = make_scene(n_cams=6, n_points=n_observed, n_obs=3 * n_observed, refine=refine, seed=seed)
    rng = np.random.default_rng(seed + 100)
    cams_true = [sc.cameras_true.cameras[c] for c in sorted(sc.cameras_true.cameras)]
    heavy_j = n_observed // 2
    cam, uv, obj = [], [], []
    for j in range(n_observed):
        rows = slice(3 * j, 3 * j + 3)
        cj, uvj = sc.camera_indices[rows], sc.image_coords[rows]
        pid = lead + stride * j
        if heavy_obs and j == heavy_j:
            cj = cj[np.arange(heavy_obs) % 3]
            uvj = np.vstack([_project(cams_true[c], sc.points_true[j]) for c in cj]) + rng.normal(0, 0.5, (heavy_obs, 2))
        elif j % 4 == 3:
            cj, uvj = cj[:2], uvj[:2]
        cam.append(cj); uv.append(uvj); obj.append(np.full(len(cj), pid))
    cam = np.concatenate(cam).astype(np.int32)
    uv = np.vstack(uv)
    obj = np.concatenate(obj).astype(np.int32)
    P = lead + stride * (n_observed - 1) + 1 + tail
    pts0 = rng.uniform(-0.5, 0.5, (P, 3)) + [0.0, 0.0, 0.6]  # (unobserved ids: anywhere; nothing may move them)
    pts0[lead + stride * np.arange(n_observed)] = sc.points_init
    par = BundleParameterization.from_camera_array(sc.cameras_init, n_points=P, refine_intrinsics=refine)
    observed = np.zeros(P, dtype=bool)
    observed[obj] = True
    return dict(par=par, x0=par.pack(sc.cameras_init, pts0), cam=cam, uv=uv, obj=obj, observed=observed,
                heavy_id=lead + stride * heavy_j if heavy_obs else None, heavy_obs=heavy_obs, lead=lead, tail=tail)


def con_small_lds_bytes(m: int, n_points: int, ncp: int) -> int:
    """Dynamic LDS of k_con_schur_small for a component of m rows over n_points points (csrc/cba_kernels.h ConSmallLayout)."""
    ZL, GW, ML = (3 * n_points) | 1, (ncp + 1) | 1, m | 1
    oL = 2 * NB * (NB + 1)
    oY = oL + 6 * n_points
    oZ = oY + 3 * n_points
    oW = oZ + m * ZL
    oG = oW + 3 * n_points * GW
    oM = oG + m * GW
    oX = oM + m * ML
    oT = oX + m * ML
    oR = oT + NB * NB
    return 8 * (oR + m * GW)


def component_rows(m: int, pts: np.ndarray, truth: np.ndarray):
    """m rows over the points ``pts`` (one component): with 8 or more points first a centroid row between four distinct points on either side,
    then distance rows (the point repeated four times, as the reference encodes them) over all pairs in turn, pairs repeated where m asks for
    more rows than there are pairs.  Target distances from the true geometry."""
    ga, gb, dist = [], [], []
    if len(pts) >= 8 and m > 1:
        a, b = pts[:4], pts[4:8]
        ga.append(list(a)); gb.append(list(b)); dist.append(float(np.linalg.norm(truth[a].mean(0) - truth[b].mean(0))))
    pairs = list(combinations(range(len(pts)), 2))
    k = 0
    while len(dist) < m:
        i, j = pairs[k % len(pairs)]
        ga.append([pts[i]] * 4); gb.append([pts[j]] * 4); dist.append(float(np.linalg.norm(truth[pts[i]] - truth[pts[j]])))
        k += 1
    return ga, gb, dist


def component_scene(shapes, n_cams: int, refine: bool = False, n_points: int = 160, orphans=(), seed: int = 21) -> dict:
    """Cameras on a ring, n_points points each seen by min(n_cams, 3) of them, and one constraint component per (m, n_points_of_component) in
    ``shapes`` on fresh points (ids 0, 1, ... in component order).  ``orphans``: (component, local point) whose observations are all removed —
    points that only constraint rows see.  Weights as in tests/constrained_scene.py: (1 px / median focal length) / 2 mm."""
    sc = make_scene(n_cams=n_cams, n_points=n_points, n_obs=n_points * min(n_cams, 3), refine=refine, seed=seed)
    truth = sc.points_true
    ga, gb, dist, comps = [], [], [], []
    nxt = 0
    for m, npts in shapes:
        pts = np.arange(nxt, nxt + npts)
        nxt += npts
        a, b, d = component_rows(m, pts, truth)
        assert len(d) == m and len(np.unique(np.concatenate([np.ravel(a), np.ravel(b)]))) == npts, (m, npts)
        ga += a; gb += b; dist += d
        comps.append(pts)
    assert nxt <= n_points
    keep = np.ones(sc.n_obs, dtype=bool)
    orphan_ids = [int(comps[k][i]) for k, i in orphans]
    for p in orphan_ids:
        keep[sc.obj_indices == p] = False
    f_median = float(np.median([c.matrix[0, 0] for c in sc.cameras_init.cameras.values()]))
    w = np.full(len(dist), (1.0 / f_median) / 0.002)
    par = BundleParameterization.from_camera_array(sc.cameras_init, n_points=n_points, refine_intrinsics=refine)
    return dict(par=par, x0=par.pack(sc.cameras_init, sc.points_init), cam=sc.camera_indices[keep], uv=sc.image_coords[keep],
                obj=sc.obj_indices[keep], constraints=(np.array(ga, dtype=np.int32), np.array(gb, dtype=np.int32), np.array(dist), w),
                orphans=orphan_ids, components=comps)
