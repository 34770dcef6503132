"""Recordings that put cba_reconstruct_trajectories at the edges of its launches, its holes and its filter: the generator of
tests/trajectory_native.py's `recording` for any number of trajectories and frames, and the two scenes the edge tests run
(tests/test_reconstruction.py on the g++ harness, tests/test_reconstruction_edges_gpu.py on the device).

WIDE, 86 trajectories x 40 frames: 258 threads of k_traj_filtfilt, two of them in a second workgroup; trajectory 85 has its x
coordinate in the first workgroup and y and z in the second.  Trajectory 0 reaches the filter with 3 samples (left alone at every
order), trajectory 84 with 28 = 3 (8 + 1) + 1 (the fewest order 8 filters), the others with all 40.
LONG, 2 trajectories x 257 frames: one thread of k_traj_frame_time in a second workgroup, signals longer than a workgroup, and two
consecutive sync indices without a row from any camera.

Every property above is asserted by `check` from the tables a scene is made of, not from its seed.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import pandas as pd

from caliscope_amd.cameras import CameraArray
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.reconstruction import trajectory_grid
from tests import trajectory_native as N

BLOCK = 256                # TRAJ_BLOCK of csrc/trajectory_math.h
MAX_ORDER, GAP = 8, 3      # CBA_TRAJ_MAX_ORDER, and the xy_gap = xyz_gap the sample counts below are counted after
SMALLEST = 3 * (MAX_ORDER + 1) + 1


@dataclass(frozen=True)
class Scene:
    name: str
    image_points: ImagePoints
    cameras: CameraArray
    gone: np.ndarray  # [n_frames, n_traj] bool: no camera has a row there


def _holes(rng, length: int) -> np.ndarray:
    """[length] bool, the frames of a trajectory that no camera sees: holes of 1 to 5 frames with 2 to 11 seen frames between them;
    the first and the last frame are seen.  A trajectory too short for a random start has its hole at frame 1."""
    gone = np.zeros(length, dtype=bool)
    f = 1 if length < 12 else int(rng.integers(1, 5))
    while True:
        size = min(int(rng.integers(1, 6)), length - 1 - f)
        if size < 1:
            return gone
        gone[f:f + size] = True
        f += size + int(rng.integers(2, 12))


def generate(name: str, n_traj: int, n_frames: int, seed: int, lengths=None, no_rows=(), camera2_loss: float = 0.12) -> Scene:
    """The cameras, the noise (0.3 px), the times (sync / 30 + 1e-3 k) and the shuffled rows of `recording`, from sync index
    N.SYNC0.  Trajectory j is (object_id, keypoint_id) = (j // 7, j % 7) and lasts `lengths.get(j, n_frames)` frames; within them it
    has the holes of `_holes`, common to all cameras, and camera 2 loses `camera2_loss` of the cells it has left.  The frames
    `no_rows` lose every row."""
    rng = np.random.default_rng(seed)
    frames, traj = np.arange(n_frames), np.arange(n_traj)
    base = rng.uniform([-0.3, -0.3, 0.3], [0.2, 0.4, 0.9], (n_traj, 3))
    truth = base[None] + 0.15 * np.sin(0.09 * frames[:, None, None] + traj[None, :, None] + np.array([0.0, 1.3, 2.1])[None, None, :])
    gone = np.ones((n_frames, n_traj), dtype=bool)
    for j in traj:
        length = (lengths or {}).get(int(j), n_frames)
        gone[:length, j] = _holes(rng, length)
    gone[list(no_rows)] = True
    cams, rows = {}, []
    for k, (cid, camera, project) in enumerate(N.rig()):
        uv = project(truth.reshape(-1, 3)).reshape(n_frames, n_traj, 2)
        uv = uv + rng.normal(0.0, 0.3, uv.shape)
        seen = ~gone
        if cid == 2:
            seen = seen & (rng.random(seen.shape) >= camera2_loss)
        f, j = np.nonzero(seen)
        rows.append(pd.DataFrame({"sync_index": f + N.SYNC0, "cam_id": cid, "object_id": j // 7, "keypoint_id": j % 7, "img_loc_x": uv[f, j, 0],
                                  "img_loc_y": uv[f, j, 1], "frame_time": (f + N.SYNC0) / 30.0 + 1e-3 * k}))
        cams[cid] = camera
    df = pd.concat(rows, ignore_index=True)
    df = df.iloc[rng.permutation(len(df))].reset_index(drop=True)
    return Scene(name, ImagePoints(df), CameraArray(cams), gone)


def samples(scene: Scene, xy_gap: int = GAP, xyz_gap: int = GAP) -> np.ndarray:
    """[n_traj] cells of every trajectory that reach the filter, counted from the table: a slot holds a point when two posed cameras
    have a row there or get one from the 2-D fill (the first min(hole, xy_gap) frames of a hole of their own track), and the 3-D
    fill adds the first min(hole, xyz_gap) frames of what is still missing between two points."""
    df = scene.image_points.df
    grid = trajectory_grid(scene.image_points, scene.cameras)
    posed = [int(c) for c, p in zip(grid.cam_ids, grid.cam_posed) if p]
    j = (df["object_id"] * 7 + df["keypoint_id"]).to_numpy()
    f = df["sync_index"].to_numpy() - grid.sync_min
    views = np.zeros((grid.n_frames, grid.n_traj), dtype=np.int64)
    for cid in posed:
        at = df["cam_id"].to_numpy() == cid
        has = np.zeros((grid.n_frames, grid.n_traj), dtype=bool)
        has[f[at], j[at]] = True
        views += _closed(has, xy_gap)
    return _closed(views >= 2, xyz_gap).sum(axis=0)


def _closed(has: np.ndarray, gap: int) -> np.ndarray:
    """`has` [n_frames, n_traj] with the first min(hole, gap) frames of every hole between two set cells of a column set."""
    out = has.copy()
    for j in range(has.shape[1]):
        at = np.flatnonzero(has[:, j])
        for lo, hi in zip(at[:-1], at[1:]):
            out[lo + 1:lo + 1 + min(hi - lo - 1, gap), j] = True
    return out


def check(scene: Scene) -> Scene:
    """What makes a scene the edge it is named for, from its own tables."""
    df = scene.image_points.df
    grid = trajectory_grid(scene.image_points, scene.cameras)
    assert grid.cam_ids.tolist() == [0, 2, 3, 5] and grid.cam_posed.tolist() == [1, 1, 0, 1] and grid.cam_model.tolist() == [0, 1, 0, 0]
    assert grid.sync_min == N.SYNC0 > 0 and len(df) > BLOCK
    assert np.array_equal(grid.traj_object, np.arange(grid.n_traj) // 7) and np.array_equal(grid.traj_keypoint, np.arange(grid.n_traj) % 7)
    assert not np.all(np.diff(df["sync_index"].to_numpy()) >= 0)  # shuffled
    # holes common to all cameras, of every size from 1 to 5, in every trajectory; camera 2 has holes of its own
    seen = np.zeros((grid.n_cams, grid.n_frames, grid.n_traj), dtype=bool)
    seen[np.searchsorted(grid.cam_ids, df["cam_id"].to_numpy()), df["sync_index"].to_numpy() - grid.sync_min,
         (df["object_id"] * 7 + df["keypoint_id"]).to_numpy()] = True
    common = ~seen.any(axis=0)
    assert np.array_equal(common, scene.gone)
    sizes = set()
    for j in range(grid.n_traj):
        at = np.flatnonzero(~common[:, j])
        holes = np.diff(at) - 1
        assert (holes > 0).any() and (holes.max() <= 5 or scene.name == "LONG"), (j, holes.max())  # (LONG: a hole may touch the two frames taken out)
        sizes |= set(holes[holes > 0].tolist())
    assert sizes >= {1, 2, 3, 4, 5}
    assert np.array_equal(seen[0], seen[2]) and np.array_equal(seen[0], seen[3]) and not (seen[1] & ~seen[0]).any()
    assert 0.08 < 1.0 - seen[1].sum() / seen[0].sum() < 0.16
    n = samples(scene)
    if scene.name == "WIDE":
        assert (grid.n_traj, grid.n_frames) == (86, 40)
        assert 3 * grid.n_traj == BLOCK + 2                          # k_traj_filtfilt: two live threads in the second workgroup
        assert (3 * 85) // BLOCK == 0 and (3 * 85 + 1) // BLOCK == 1  # trajectory 85: x in workgroup 0, y and z in workgroup 1
        assert n[0] == 3 and n[84] == SMALLEST == 28 and n[85] == grid.n_frames and (n[1:84] == grid.n_frames).all()
    if scene.name == "LONG":
        assert (grid.n_traj, grid.n_frames) == (2, 257)
        assert grid.n_frames == BLOCK + 1                             # k_traj_frame_time: one live thread in the second workgroup
        assert (n > BLOCK).all()                                      # signals longer than a workgroup's worth of frames
        empty = np.flatnonzero(common.all(axis=1))
        assert len(empty) >= 2 and (np.diff(empty) == 1).any()       # frames without a row from any camera, two of them in a row
    # no trajectory is one the call refuses to filter, at any order
    assert not any(((n > 3 * order) & (n <= 3 * (order + 1))).any() for order in range(1, MAX_ORDER + 1))
    return scene


@functools.cache
def wide() -> Scene:
    return check(generate("WIDE", 86, 40, seed=86, lengths={0: 3, 84: SMALLEST}))


@functools.cache
def long() -> Scene:
    return check(generate("LONG", 2, 257, seed=257, no_rows=(128, 129)))


SCENES = {"WIDE": wide, "LONG": long}
