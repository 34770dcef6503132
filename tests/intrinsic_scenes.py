"""Scenes and the yardstick of the intrinsic-calibration tests.  TEST INFRASTRUCTURE.

Scenes: one camera looking at random views of a planar board (the recipe the issue's probe validated: 1920 x 1080, 6 x 9 corners at
0.04 m, webcam distortion / a mild equidistant fisheye), rigs of several such cameras in the CSR form of the batch call, and a ring
board session for the end-to-end test.

Yardstick: the least-squares minimum of the pixel reprojection error, which is the reference's own definition of the result,
computed by ``scipy.optimize.least_squares(method="trf", x_scale="jac", ftol=xtol=gtol=1e-15)`` over
``oracle.camera_model.project_pinhole / project_fisheye`` with the analytic Jacobian from their ``jacobian=True`` columns.  The
problem has no gauge freedom (the board fixes the frame), so intrinsics are compared raw.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import pandas as pd
from scipy.optimize import least_squares

from oracle.camera_model import project_fisheye, project_pinhole, rodrigues, rotation_to_rvec

SIZE = (1920, 1080)
PINHOLE_TRUTH = (np.array([1394.6, 1390.0, 950.0, 545.0]), np.array([0.115, -0.219, 0.0012, 0.0086, 0.113]))
FISHEYE_D = np.array([0.05, -0.01, 0.004, -0.001])


def fisheye_truth(f=620.0):
    return np.array([f, f - 5.0, 950.0, 545.0]), FISHEYE_D.copy()


def board(rows=6, cols=9, spacing=0.04):
    return np.array([[c * spacing, r * spacing, 0.0] for r in range(rows) for c in range(cols)])


@dataclass
class CameraScene:
    fisheye: bool
    size: tuple
    intr: np.ndarray  # fx fy cx cy
    dist: np.ndarray
    views: list = field(default_factory=list)  # (obj[n, 3], xy[n, 2], rvec, tvec)

    @property
    def truth9(self):
        out = np.zeros(9)
        out[:4] = self.intr
        out[4:4 + len(self.dist)] = self.dist
        return out


def _project(fisheye, X, rv, t, intr, dist, jacobian=False):
    K = np.array([[intr[0], 0.0, intr[2]], [0.0, intr[1], intr[3]], [0.0, 0.0, 1.0]])
    return (project_fisheye if fisheye else project_pinhole)(X, rv, t, K, dist, jacobian=jacobian)


def camera_scene(seed, n_views=30, *, fisheye=False, intr=None, dist=None, noise=0.3, rows=6, cols=9, spacing=0.04, size=SIZE, min_corners=12):
    """The probe's recipe: random board poses in front of the camera, corners outside the image dropped, Gaussian pixel noise."""
    rng = np.random.default_rng(seed)
    if intr is None:
        intr, dist = fisheye_truth() if fisheye else (PINHOLE_TRUTH[0].copy(), PINHOLE_TRUTH[1].copy())
    w, h = size
    grid = board(rows, cols, spacing)
    scene = CameraScene(fisheye, size, np.asarray(intr, float), np.asarray(dist, float))
    while len(scene.views) < n_views:
        rv = rng.normal(0, 0.35, 3)
        R = rodrigues(rv)
        depth = rng.uniform(0.5, 1.2) * (0.45 if fisheye else 1.0)
        wide = 2 if fisheye else 1
        ctr = np.array([rng.uniform(-0.35, 0.35) * depth * wide, rng.uniform(-0.2, 0.2) * depth * wide, depth])
        t = ctr - R @ grid.mean(0)
        uv, _ = _project(fisheye, grid, rv, t, scene.intr, scene.dist)
        Xc = grid @ R.T + t
        ok = (Xc[:, 2] > 0.1) & (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
        if ok.sum() < min_corners:
            continue
        scene.views.append((grid[ok], uv[ok] + rng.normal(0, noise, (int(ok.sum()), 2)), rv, t))
    return scene


def pack(scenes):
    """CSR arguments of the batch call for a list of CameraScene: (cam_model, cam_size, view_start, view_cam, obs_xy, obs_obj)."""
    sizes, cam, xy, obj = [], [], [], []
    for c, s in enumerate(scenes):
        for X, uv, _, _ in s.views:
            sizes.append(len(X)); cam.append(c); xy.append(uv); obj.append(X)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return (np.array([1 if s.fisheye else 0 for s in scenes], np.int32), np.array([s.size for s in scenes], float), start,
            np.array(cam, np.int32), np.concatenate(xy) if xy else np.zeros((0, 2)), np.concatenate(obj) if obj else np.zeros((0, 3)))


def rig_scenes(seed=5):
    """Six cameras with different true intrinsics, models and view counts from 3 to a few hundred."""
    specs = [
        dict(n_views=3, intr=[1200.0, 1210.0, 940.0, 530.0], dist=[0.05, -0.08, 0.001, -0.002, 0.01]),
        dict(n_views=12, intr=[1394.6, 1390.0, 950.0, 545.0], dist=PINHOLE_TRUTH[1]),
        dict(n_views=30, fisheye=True, intr=[620.0, 615.0, 950.0, 545.0], dist=FISHEYE_D),
        dict(n_views=60, intr=[1800.0, 1795.0, 975.0, 520.0], dist=[-0.1, 0.05, -0.001, 0.001, 0.0]),
        dict(n_views=45, fisheye=True, intr=[430.0, 432.0, 965.0, 535.0], dist=FISHEYE_D * 0.5),
        dict(n_views=240, intr=[1000.0, 1004.0, 955.0, 541.0], dist=[0.2, -0.3, 0.002, 0.001, 0.15], rows=4, cols=5, spacing=0.06, min_corners=8),
    ]
    return [camera_scene(seed + 17 * i, **sp) for i, sp in enumerate(specs)]


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------

def _unpack(x, nd, i):
    return x[:4], x[4:4 + nd], x[4 + nd + 6 * i: 4 + nd + 6 * i + 3], x[4 + nd + 6 * i + 3: 4 + nd + 6 * i + 6]


def yardstick_residuals(x, views, fisheye):
    nd = 4 if fisheye else 5
    out = []
    for i, (X, uv) in enumerate(views):
        intr, d, rv, t = _unpack(x, nd, i)
        out.append((_project(fisheye, X, rv, t, intr, d)[0] - uv).ravel())
    return np.concatenate(out)


def yardstick_jacobian(x, views, fisheye):
    nd = 4 if fisheye else 5
    m = 2 * sum(len(X) for X, _ in views)
    J = np.zeros((m, len(x)))
    row = 0
    for i, (X, uv) in enumerate(views):
        intr, d, rv, t = _unpack(x, nd, i)
        _, Jc = _project(fisheye, X, rv, t, intr, d, jacobian=True)
        k = len(Jc)
        if fisheye:
            J[row:row + k, :4 + nd] = Jc[:, 0:8]
            J[row:row + k, 4 + nd + 6 * i: 4 + nd + 6 * i + 6] = Jc[:, 8:14]
        else:
            J[row:row + k, :4 + nd] = Jc[:, 6:15]
            J[row:row + k, 4 + nd + 6 * i: 4 + nd + 6 * i + 6] = Jc[:, 0:6]
        row += k
    return J


def yardstick(views, fisheye, intr9, poses, max_nfev=400):
    """scipy's minimum from (intr9, poses[k, 12] as R row-major then t).  ``views``: list of (obj, xy).  Returns (intr9, sum of
    squared pixel errors, rmse as cv2 defines it, scipy result)."""
    nd = 4 if fisheye else 5
    x0 = np.concatenate([np.asarray(intr9, float)[:4 + nd]] + [np.concatenate([rotation_to_rvec(np.asarray(p[:9]).reshape(3, 3)), p[9:12]]) for p in poses])
    res = least_squares(yardstick_residuals, x0, jac=yardstick_jacobian, args=(views, fisheye), method="trf", x_scale="jac", ftol=1e-15,
                        xtol=1e-15, gtol=1e-15, max_nfev=max_nfev)
    out = np.zeros(9)
    out[:4 + nd] = res.x[:4 + nd]
    n = sum(len(X) for X, _ in views)
    ssq = 2.0 * res.cost
    return out, ssq, float(np.sqrt(ssq / n)), res


def truth_poses(scene, keep=None):
    idx = range(len(scene.views)) if keep is None else keep
    return np.array([np.concatenate([rodrigues(scene.views[i][2]).ravel(), scene.views[i][3]]) for i in idx])


def cold_start_poses(scenes, float32_io=True):
    """The product's own start of every view: pixels undistorted with the start intrinsics, then the existing PnP (g++ build)."""
    from tests.intrinsic_native import start_intrinsics
    from tests.pnp_native import HarnessPnP

    model, size, vstart, vcam, xy, obj = pack(scenes)
    start = np.array([start_intrinsics(m, s[0], s[1]) for m, s in zip(model, size)])
    pose, _, status, _ = HarnessPnP().pnp_batch(vstart, vcam, model, start, xy, obj, 4, float32_io)
    return start, pose, status


# ---- a board session for the end-to-end test ------------------------------------------------------------------------------------------

def ring_board_session(n_cams=6, n_frames=40, rows=6, cols=9, spacing=0.04, noise_px=0.5, seed=11, fisheye_cam=None):
    """Ring cameras around a planar board (object 0 at z = 0) that tilts and drifts through the volume (the generator of
    tests/test_pose_bootstrap_gpu.py).  ``fisheye_cam``: that camera is an equidistant fisheye (f = 700, FISHEYE_D) instead of
    the webcam.  Returns (ImagePoints, the true CameraArray)."""
    from caliscope_amd.cameras import rvec_to_matrix
    from caliscope_amd.point_data import ImagePoints
    from caliscope_amd.synthetic import WEBCAM_SIZE, project_pinhole_bc5, ring_camera_array

    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams, radius=1.5, target=(0.0, 0.0, 0.5))
    grid = board(rows, cols, spacing)
    off = grid.mean(axis=0)
    w, h = WEBCAM_SIZE
    if fisheye_cam is not None:
        cam = cams.cameras[fisheye_cam]
        cam.fisheye, cam.distortions = True, FISHEYE_D.copy()
        cam.matrix = np.array([[700.0, 0.0, w / 2.0], [0.0, 700.0, h / 2.0], [0.0, 0.0, 1.0]])
    out = []
    for f in range(n_frames):
        s = f / max(n_frames - 1, 1)
        R = rvec_to_matrix(np.array([0.0, 0.0, 2 * np.pi * s])) @ rvec_to_matrix(np.array([np.pi / 2 + 0.3 * np.sin(4 * s), 0.0, 0.0]))
        X = (grid - off) @ R.T + np.array([0.2 * np.cos(3 * s), 0.2 * np.sin(2 * s), 0.5 + 0.1 * np.sin(5 * s)])
        for c, cam in sorted(cams.cameras.items()):
            K = cam.matrix
            if cam.fisheye:
                p, _ = project_fisheye(X, rotation_to_rvec(cam.rotation), cam.translation, K, cam.distortions)
                z = (X @ cam.rotation.T + cam.translation)[:, 2]
            else:
                p, z = project_pinhole_bc5(X, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
            ok = (z > 0.1) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)
            if ok.sum() < 8 or abs(float(R[:, 2] @ (-cam.rotation.T @ cam.translation - X.mean(0)))) < 0.3:
                continue
            p = p + rng.normal(0, noise_px, p.shape)
            for k in np.flatnonzero(ok):
                out.append(dict(sync_index=f, cam_id=c, object_id=0, keypoint_id=int(k), img_loc_x=p[k, 0], img_loc_y=p[k, 1],
                                obj_loc_x=grid[k, 0], obj_loc_y=grid[k, 1], obj_loc_z=0.0))
    return ImagePoints(pd.DataFrame(out)), cams


def scene_image_points(scenes, cam_ids=None):
    """ImagePoints of a list of CameraScene (view k of a camera at sync_index k, keypoint ids by position in the view)."""
    from caliscope_amd.point_data import ImagePoints

    rows = []
    for c, s in enumerate(scenes):
        cid = c if cam_ids is None else cam_ids[c]
        for f, (X, uv, _, _) in enumerate(s.views):
            for k in range(len(X)):
                rows.append(dict(sync_index=f, cam_id=cid, object_id=0, keypoint_id=k, img_loc_x=uv[k, 0], img_loc_y=uv[k, 1],
                                 obj_loc_x=X[k, 0], obj_loc_y=X[k, 1], obj_loc_z=X[k, 2]))
    return ImagePoints(pd.DataFrame(rows))
