"""The recording the refinement tests share (tests/test_trajectory_refine.py on the g++ harness, tests/test_trajectory_refine_gpu.py
on the device): the seven cameras of `ring_camera_array(7)` — cam_ids 0..5 posed, cam_id 2 the fisheye of
tests/trajectory_native.rig, cam_id 6 without a pose — and 3 trajectories x 100 frames from sync index 5, i.e. 300 slots: two
workgroups of k_traj_refine, the second partly filled.  0.3 px of noise everywhere; an outlier is 60 px in a direction that depends
on the frame alone.

* trajectory 0, all six posed cameras: frames f % 4 == 0 have outliers in cameras f % 6 and (f + 3) % 6 (opposite in the ring), in
  unequal directions, both within 0.7 rad of +u: cameras that face each other see a 3-D displacement with opposite signs of u, so
  these two outliers contradict each other as well as the other four views (two that agree with each other outvote four good
  views under a bounded-influence loss: scipy then drops good views too); frames f % 4 == 1 have one in camera f % 6;
* trajectory 1, cameras 0, 1, 2, 3: frames f % 3 == 0 have one outlier, in camera (0, 1, 2, 3)[(f // 3) % 4], close to vertical in
  the image (across the epipolar lines of a ring of cameras at one height);
* trajectory 2, cameras 0 and 4, no outliers; camera 4 has no row in frames 10-12 (one view: no point), neither has in 20-21;
* trajectory 1 loses camera 3 in frames 40-41 (three views) and cameras 1, 2, 3 in frame 50 (one view);
* the unposed camera sees everything.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import pandas as pd

from caliscope_amd.cameras import CameraArray, CameraData, matrix_to_rvec
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.synthetic import ring_camera_array
from oracle import camera_model as cm

SYNC0, N_FRAMES, N_TRAJ = 5, 100, 3
POSED, FISHEYE, UNPOSED = (0, 1, 2, 3, 4, 5), 2, 6
TRAJ = ((0, 0), (0, 1), (1, 4))  # (object_id, keypoint_id) of trajectory 0..2
SEES = {0: (0, 1, 2, 3, 4, 5), 1: (0, 1, 2, 3), 2: (0, 4)}
OUTLIER_PX, NOISE_PX = 60.0, 0.3
FISHEYE_DIST = np.array([0.05, -0.02, 0.004, 0.001])


@dataclass(frozen=True)
class Scene:
    image_points: ImagePoints
    cameras: CameraArray
    truth: np.ndarray    # [N_FRAMES, N_TRAJ, 3]
    outlier: np.ndarray  # [7, N_FRAMES, N_TRAJ] bool: the cell of that cam_id is an outlier
    seen: np.ndarray     # [7, N_FRAMES, N_TRAJ] bool: the cam_id has a row there


def rig():
    """(cam_id, CameraData, rvec, project) of the seven cameras."""
    out = []
    for src in ring_camera_array(7).cameras.values():
        cid = src.cam_id
        fisheye, posed = cid == FISHEYE, cid != UNPOSED
        dist = FISHEYE_DIST if fisheye else src.distortions
        camera = CameraData(cam_id=cid, size=src.size, matrix=src.matrix.copy(), distortions=dist.copy(), fisheye=fisheye,
                            rotation=src.rotation if posed else None, translation=src.translation if posed else None)
        model = cm.project_fisheye if fisheye else cm.project_pinhole
        out.append((cid, camera, functools.partial(model, rvec=matrix_to_rvec(src.rotation), tvec=src.translation, K=src.matrix, dist=dist)))
    return out


@functools.cache
def scene(seed: int = 11) -> Scene:
    rng = np.random.default_rng(seed)
    frames = np.arange(N_FRAMES)
    base = np.array([[0.2, 0.1, 0.5], [-0.3, 0.2, 0.8], [0.1, -0.3, 0.3]])
    phase = 0.09 * frames[:, None, None] + np.arange(N_TRAJ)[None, :, None] + np.array([0.0, 1.3, 2.1])[None, None, :]
    truth = base[None] + 0.15 * np.sin(phase)
    outlier = np.zeros((7, N_FRAMES, N_TRAJ), dtype=bool)
    angle = np.zeros((7, N_FRAMES, N_TRAJ))
    for f in frames:
        if f % 4 == 0:
            outlier[f % 6, f, 0] = outlier[(f + 3) % 6, f, 0] = True
            angle[f % 6, f, 0], angle[(f + 3) % 6, f, 0] = 0.3 * np.sin(0.7 * f), 0.4 + 0.3 * np.cos(1.1 * f)
        if f % 4 == 1:
            outlier[f % 6, f, 0] = True
            angle[f % 6, f, 0] = 1.9 + 0.41 * f
        if f % 3 == 0:
            c = SEES[1][(f // 3) % 4]
            outlier[c, f, 1] = True
            angle[c, f, 1] = np.pi / 2 + 0.3 * np.sin(1.0 * f) + np.pi * ((f // 3) % 2)
    seen = np.zeros((7, N_FRAMES, N_TRAJ), dtype=bool)
    for j, cams in SEES.items():
        seen[list(cams), :, j] = True
    seen[UNPOSED] = True
    seen[4, 10:13, 2] = False
    seen[[0, 4], 20:22, 2] = False
    seen[3, 40:42, 1] = False
    seen[[1, 2, 3], 50, 1] = False
    outlier &= seen
    cams, rows = {}, []
    for k, (cid, camera, project) in enumerate(rig()):
        uv = project(truth.reshape(-1, 3))[0].reshape(N_FRAMES, N_TRAJ, 2)
        uv = uv + rng.normal(0.0, NOISE_PX, uv.shape)
        uv = uv + OUTLIER_PX * outlier[cid][..., None] * np.stack([np.cos(angle[cid]), np.sin(angle[cid])], axis=-1)
        f, j = np.nonzero(seen[cid])
        rows.append(pd.DataFrame({"sync_index": f + SYNC0, "cam_id": cid, "object_id": np.array(TRAJ)[j, 0], "keypoint_id": np.array(TRAJ)[j, 1],
                                  "img_loc_x": uv[f, j, 0], "img_loc_y": uv[f, j, 1], "frame_time": (f + SYNC0) / 30.0 + 1e-3 * k}))
        cams[cid] = camera
    df = pd.concat(rows, ignore_index=True)
    df = df.iloc[rng.permutation(len(df))].reset_index(drop=True)  # the table arrives in no particular order
    return Scene(ImagePoints(df), CameraArray(cams), truth, outlier, seen)


def restricted(sc: Scene, trajectory: int, cam_ids) -> ImagePoints:
    """The rows of one trajectory in the given cameras alone."""
    df = sc.image_points.df
    obj, kp = TRAJ[trajectory]
    return ImagePoints(df[(df["object_id"] == obj) & (df["keypoint_id"] == kp) & df["cam_id"].isin(list(cam_ids))].reset_index(drop=True))


def relabelled(sc: Scene, n_slots: int) -> ImagePoints:
    """The first `n_slots` slots of the scene (slot = 3 frame + trajectory) as one trajectory of `n_slots` frames: slot k of the new
    grid holds the cells of slot k of the scene, so a launch of exactly that many threads can be held against the scene's own."""
    df = sc.image_points.df
    j = np.array([TRAJ.index((int(o), int(k))) for o, k in zip(df["object_id"], df["keypoint_id"])])
    slot = (df["sync_index"].to_numpy() - SYNC0) * N_TRAJ + j
    out = df[slot < n_slots].copy()
    out["sync_index"], out["object_id"], out["keypoint_id"] = slot[slot < n_slots] + SYNC0, 0, 0
    return ImagePoints(out.reset_index(drop=True))


def behind_camera_case():
    """(ImagePoints, CameraArray): one frame, one landmark, cameras 0, 1 and 3 of the rig, and pixels that are the exact images of a
    point 0.3 m BEHIND camera 3 (its image through the centre of projection) and in front of the other two.  The DLT knows no sign
    of depth and returns that point; the refinement must leave it alone."""
    cams = {cid: camera for cid, camera, _ in rig() if cid in (0, 1, 3)}
    c3 = cams[3]
    point = c3.rotation.T @ (np.array([0.05, 0.02, -0.3]) - c3.translation)
    rows = []
    for cid, camera, project in rig():
        if cid in cams:
            u, v = project(point.reshape(1, 3))[0][0]
            rows.append({"sync_index": 0, "cam_id": cid, "object_id": 0, "keypoint_id": 0, "img_loc_x": u, "img_loc_y": v, "frame_time": 0.0})
    return ImagePoints(pd.DataFrame(rows)), CameraArray(cams), point
