"""2-D-only sessions for the epipolar bootstrap tests: a box-like 3-D target and an articulated 33-keypoint "body" that move
through a ring of cameras (``obj_loc`` all NaN unless asked for), with keypoint dropout and gross outliers."""
from __future__ import annotations

import numpy as np
import pandas as pd

from caliscope_amd.cameras import CameraArray, CameraData, rvec_to_matrix
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.synthetic import WEBCAM_SIZE, project_pinhole_bc5, ring_camera_array

FISHEYE_DIST = np.array([0.05, -0.01, 0.002, -0.0005])


def box_points(size=(0.5, 0.4, 0.3)):
    """Corners, edge midpoints and face centres of a box (26 points), centred on the origin."""
    g = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=float)
    return 0.5 * g * np.asarray(size)


def body_points(n=33, seed=0):
    """A standing-person-like constellation: n keypoints in a 0.5 x 0.3 x 1.7 m volume, feet at z = 0."""
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-0.25, 0.25, n), rng.uniform(-0.15, 0.15, n), rng.uniform(0.0, 1.7, n)])


def _project(cam, X):
    K = cam.matrix
    if not cam.fisheye:
        return project_pinhole_bc5(X, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
    Xc = X @ cam.rotation.T + cam.translation
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r = np.hypot(x, y)
    th = np.arctan(r)
    k1, k2, k3, k4 = cam.distortions[:4]
    thd = th * (1 + k1 * th**2 + k2 * th**4 + k3 * th**6 + k4 * th**8)
    s = np.where(r > 1e-12, thd / np.maximum(r, 1e-12), 1.0)
    return np.column_stack([K[0, 0] * x * s + K[0, 2], K[1, 1] * y * s + K[1, 2]]), Xc[:, 2]


def constellation_session(n_cams=4, n_frames=30, kind="box", noise_px=0.5, dropout=0.0, outliers=0.0, radius=2.5, cam_ids=None,
                          fisheye=(), with_obj_loc=False, seed=42):
    """Returns ``(image_points, cameras (posed truth), truth)``; ``truth`` as ``tests.scenario_scenes.keyed_errors`` takes it.
    The constellation tumbles and drifts through the ring (so that the pooled points span a volume); ``cam_ids`` renames the
    ring's cameras, ``fisheye`` lists (renamed) cameras given the fisheye model."""
    rng = np.random.default_rng(seed)
    ring = ring_camera_array(n_cams, radius=radius, target=(0.0, 0.0, 0.8 if kind == "body" else 0.6))
    ids = list(cam_ids) if cam_ids is not None else list(range(n_cams))
    cams = {}
    for i, (c, cam) in enumerate(sorted(ring.cameras.items())):
        fe = ids[i] in fisheye
        cams[ids[i]] = CameraData(cam_id=ids[i], size=cam.size, matrix=cam.matrix.copy(), fisheye=fe,
                                  distortions=FISHEYE_DIST.copy() if fe else cam.distortions.copy(), rotation=cam.rotation, translation=cam.translation)
    cameras = CameraArray(cams)
    P = box_points() if kind == "box" else body_points(seed=seed)
    w, h = WEBCAM_SIZE
    out, truth = [], {}
    for f in range(n_frames):
        s = f / max(n_frames - 1, 1)
        if kind == "box":
            R = rvec_to_matrix(np.array([1.3 * np.sin(3 * s), 0.9 * np.cos(2 * s), 2 * np.pi * s]))
            X = P @ R.T + np.array([0.5 * np.cos(2 * np.pi * s), 0.5 * np.sin(2 * np.pi * s), 0.6 + 0.2 * np.sin(5 * s)])
        else:
            # walk a circle, turn with it, swing the upper half (articulation)
            Q = P.copy()
            upper = Q[:, 2] > 0.9
            Q[upper] = Q[upper] @ rvec_to_matrix(np.array([0.0, 0.0, 0.4 * np.sin(6 * np.pi * s)])).T
            legs = Q[:, 2] < 0.8
            Q[legs, 0] += 0.15 * np.sin(8 * np.pi * s) * np.sign(Q[legs, 1])
            R = rvec_to_matrix(np.array([0.0, 0.0, 2 * np.pi * s]))
            X = Q @ R.T + np.array([0.6 * np.cos(2 * np.pi * s), 0.6 * np.sin(2 * np.pi * s), 0.0])
        for c, cam in sorted(cameras.cameras.items()):
            p, z = _project(cam, X)
            ok = (z > 0.1) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)
            ok &= rng.random(len(X)) >= dropout
            p = p + rng.normal(0, noise_px, p.shape)
            bad = rng.random(len(X)) < outliers
            p[bad] = np.column_stack([rng.uniform(0, w, int(bad.sum())), rng.uniform(0, h, int(bad.sum()))])
            for k in np.flatnonzero(ok):
                o = P[k] if with_obj_loc else (np.nan, np.nan, np.nan)
                out.append(dict(sync_index=f, cam_id=c, object_id=0, keypoint_id=int(k), img_loc_x=p[k, 0], img_loc_y=p[k, 1],
                                obj_loc_x=o[0], obj_loc_y=o[1], obj_loc_z=o[2]))
            for k in range(len(X)):
                truth[(f, 0, k)] = X[k]
    return ImagePoints(pd.DataFrame(out)), cameras, dict(cameras=cameras, points=truth)


def unposed(cameras):
    return CameraArray({c: CameraData(cam_id=c, size=cam.size, matrix=cam.matrix.copy(), distortions=cam.distortions.copy(), fisheye=cam.fisheye)
                        for c, cam in cameras.cameras.items()})
