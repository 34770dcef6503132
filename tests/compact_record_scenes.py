"""Scenes for tests/test_compact_records_gpu.py: the smallest shapes at which the kernels that write and read the compact six-parameter Schur record
(k_tprep, k_schur_reg3, k_backsub_rec; csrc/cba_kernels.h) can go wrong, and a long double direct sum of the reduced camera system.

A scene is given by its visibility (the cameras of every point, a camera may repeat), optionally with one fisheye camera and one camera 100 m from the
world origin (|t| = 100: the translation a reader of the record rebuilds the normalised point with).  Cameras stand on the ring of
caliscope_amd.synthetic; observations are projections of the true points plus half a pixel of noise, from wherever the point falls (no image
bounds: only the arithmetic matters here)."""
from __future__ import annotations

import numpy as np

from caliscope_amd.bundle_parameterization import BundleParameterization
from caliscope_amd.cameras import CameraArray, CameraData, matrix_to_rvec, rvec_to_matrix
from caliscope_amd.synthetic import _look_at, project_pinhole_bc5, ring_camera_array

SCHUNK = 320  # slots of one chunk buffer of k_schur_reg3 (Reg3Cfg<6>::SCHUNK)
FISHEYE_D = np.array([0.031, -0.012, 0.0042, -0.0009])
TARGET = np.array([0.0, 0.0, 0.6])


def _project_fisheye(X, R, t, fx, fy, cx, cy, d):
    Xc = X @ R.T + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3]))))
    s = np.where(r > 1e-8, thd / np.maximum(r, 1e-300), 1.0)
    return np.stack([cx + fx * x * s, cy + fy * y * s], axis=1)


def build_scene(n_cams: int, visibility, *, fisheye_cam: int | None = None, far_cam: int | None = None, seed: int = 7) -> dict:
    rng = np.random.default_rng(seed)
    true = dict(ring_camera_array(n_cams).cameras)
    if fisheye_cam is not None:
        c = true[fisheye_cam]
        true[fisheye_cam] = CameraData(cam_id=c.cam_id, size=c.size, matrix=c.matrix.copy(), distortions=FISHEYE_D.copy(), rotation=c.rotation,
                                       translation=c.translation, fisheye=True)
    if far_cam is not None:  # the same direction, 100 m from the origin, a lens 30 times as long
        c = true[far_cam]
        pos = -c.rotation.T @ c.translation
        pos = pos * (100.0 / np.linalg.norm(pos))
        R = _look_at(pos, TARGET)
        K = c.matrix.copy()
        K[0, 0] *= 30.0
        K[1, 1] *= 30.0
        true[far_cam] = CameraData(cam_id=c.cam_id, size=c.size, matrix=K, distortions=c.distortions.copy(), rotation=R, translation=-R @ pos)
    P = len(visibility)
    rad, ang = 0.6 * np.sqrt(rng.uniform(0, 1, P)), rng.uniform(0, 2 * np.pi, P)
    pts = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(0, 1.2, P)], axis=1)
    cam = np.concatenate([np.sort(np.asarray(v, dtype=np.int32)) for v in visibility]).astype(np.int32)
    obj = np.repeat(np.arange(P, dtype=np.int32), [len(v) for v in visibility])
    uv = np.empty((len(cam), 2))
    for i, (c, p) in enumerate(zip(cam, obj)):
        cd = true[int(c)]
        K = cd.matrix
        args = (pts[p:p + 1], cd.rotation, cd.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cd.distortions)
        uv[i] = _project_fisheye(*args)[0] if cd.fisheye else project_pinhole_bc5(*args)[0][0]
    uv += rng.normal(0, 0.5, uv.shape)
    init = {}
    for cid, c in true.items():
        sig = 1e-4 if cid == far_cam else 0.01  # (a hundredth of a radian is a metre at 100 m)
        init[cid] = CameraData(cam_id=cid, size=c.size, matrix=c.matrix.copy(), distortions=c.distortions.copy(),
                               rotation=rvec_to_matrix(matrix_to_rvec(c.rotation) + rng.normal(0, sig, 3)),
                               translation=c.translation + rng.normal(0, 0.02, 3), fisheye=c.fisheye)
    cams_init = CameraArray(init)
    par = BundleParameterization.from_camera_array(cams_init, n_points=P, refine_intrinsics=False)
    x0 = par.pack(cams_init, pts + rng.normal(0, 0.01, pts.shape))
    return dict(par=par, x0=x0, cam=cam, uv=uv, obj=obj, n_cams=n_cams)


def _views(rng, n_cams, counts):
    return [rng.choice(n_cams, size=int(k), replace=False) for k in counts]


def scene(name: str) -> dict:
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "pair":        # 2 cameras, 1 point, 2 observations: one block per kind, one record per camera
        return build_scene(2, [[0, 1]])
    if name == "rig17":       # two camera groups (9 + 8): a diagonal and an off-diagonal tile; 2..12 views per point; a repeated camera; fisheye; |t| = 100
        vis = _views(rng, 17, [2 + i % 11 for i in range(88)])
        vis[0] = np.concatenate([vis[0], vis[0][:1]])  # point 0 is seen twice by one camera
        for v in (5, 40, 77):                          # (the special cameras see points of few and of many views)
            vis[v] = np.unique(np.concatenate([vis[v], [3, 11]]))
        sc = build_scene(17, vis, fisheye_cam=3, far_cam=11)
        t = sc["x0"][sc["par"].camera_param_offsets[11] + 3: sc["par"].camera_param_offsets[11] + 6]
        assert 99.0 < np.linalg.norm(t) < 101.0
        return sc
    if name == "chunk321":    # one tile of SCHUNK + 1 slots: 4 cameras (blocks replicated over 16 threads), 107 points of 3 views
        sc = build_scene(4, _views(rng, 4, [3] * 107))
        assert len(sc["cam"]) == SCHUNK + 1
        return sc
    if name == "chunk641":    # one tile of 2 SCHUNK + 1 slots: 16 cameras (one thread per block), 127 points of 5 views and one of 6
        sc = build_scene(16, _views(rng, 16, [5] * 127 + [6]))
        assert len(sc["cam"]) == 2 * SCHUNK + 1
        return sc
    raise KeyError(name)


def reduced_system_long_double(J, f, cam, obj, cam_off, ncp, scale_inv, lam):
    """S = U + lam D_c^2 - sum_p W_p V'_p^-1 W_p^T and rhs = -g_c + sum_p W_p V'_p^-1 g_p summed over the observations in long double, from the
    rows of the (double) Jacobian ``J`` (CSR: two rows per observation, six camera columns from cam_off[cam], three point columns) and the residual
    ``f``; D = ``scale_inv``, V' = V + lam D_p^2."""
    LD = np.longdouble
    N, P = len(cam), int(obj.max()) + 1
    Jd = J.toarray() if J.shape[0] * J.shape[1] < 4e7 else None
    assert Jd is not None
    rows = np.arange(N)
    A = np.stack([np.stack([Jd[2 * rows + r, cam_off[cam] + k] for k in range(6)], axis=1) for r in range(2)], axis=1).astype(LD)  # (N, 2, 6)
    B = np.stack([np.stack([Jd[2 * rows + r, ncp + 3 * obj + k] for k in range(3)], axis=1) for r in range(2)], axis=1).astype(LD)  # (N, 2, 3)
    e = np.asarray(f, dtype=LD).reshape(N, 2)
    D2 = np.asarray(scale_inv, dtype=LD) ** 2
    S = np.zeros((ncp, ncp), dtype=LD)
    rhs = np.zeros(ncp, dtype=LD)
    V = np.zeros((P, 3, 3), dtype=LD)
    gp = np.zeros((P, 3), dtype=LD)
    for i in range(N):
        o = cam_off[cam[i]]
        S[o:o + 6, o:o + 6] += A[i].T @ A[i]
        rhs[o:o + 6] -= A[i].T @ e[i]
        V[obj[i]] += B[i].T @ B[i]
        gp[obj[i]] += B[i].T @ e[i]
    S[np.arange(ncp), np.arange(ncp)] += LD(lam) * D2[:ncp]
    for p in range(P):
        idx = np.flatnonzero(obj == p)
        if not len(idx):
            continue
        Vd = V[p] + np.diag(LD(lam) * D2[ncp + 3 * p: ncp + 3 * p + 3])
        a, b, c, d, e2, f2 = Vd[0, 0], Vd[0, 1], Vd[0, 2], Vd[1, 1], Vd[1, 2], Vd[2, 2]
        adj = np.array([[d * f2 - e2 * e2, c * e2 - b * f2, b * e2 - c * d], [c * e2 - b * f2, a * f2 - c * c, b * c - a * e2],
                        [b * e2 - c * d, b * c - a * e2, a * d - b * b]], dtype=LD)
        Vi = adj / (a * adj[0, 0] + b * adj[0, 1] + c * adj[0, 2])
        Wi = [A[i].T @ B[i] for i in idx]  # (6, 3) each
        for ii, i in enumerate(idx):
            oi = cam_off[cam[i]]
            rhs[oi:oi + 6] += Wi[ii] @ (Vi @ gp[p])
            for jj, j in enumerate(idx):
                oj = cam_off[cam[j]]
                S[oi:oi + 6, oj:oj + 6] -= Wi[ii] @ Vi @ Wi[jj].T
    return S, rhs
