"""Timing of the scale report (CaptureVolume.compute_volumetric_scale_accuracy -> cba_scale_errors) on three seeded sessions.

    python tools/scale_accuracy_timing.py [--sessions a,b,c] [--repeats 10] [--fraction 1.0]

    (a) 30 000 frames x one 7 x 5 board x 8 cameras        ~1M world points, 30 000 groups of 595 pairs
    (b) 250 000 frames x one 4-corner marker + two static markers seen in every frame, 2 cameras     750 000 groups of 6 pairs
    (c) 200 frames x one 600-corner board x 4 cameras       200 groups of 179 700 pairs

Per session it prints: the host marshalling time (``_scale_groups``: sorts and prefix sums over the tables); the ``cba_scale_errors``
call (upload, launches, copy-back: the call returns after its copy-back, which synchronises) after a warm-up call, median / min / max
of ``--repeats`` calls; the same statistics by vectorised numpy on one host thread; and the cost of the reference's way — a Python loop
over ``groupby(["sync_index", "object_id"])`` with a filter of the whole world table, a merge and two ``pdist`` per group, restated
here without any of the reference's code — measured on at most 200 groups and scaled by the number of groups: an EXTRAPOLATION,
labelled as one.  ``--fraction`` shrinks the frame counts (a quick look on a small machine).

Kernel times: run this program once under ``rocprofv3 --kernel-trace --stats -- python tools/scale_accuracy_timing.py --repeats 3``."""
import argparse
import sys
import time
import warnings
from pathlib import Path

import numpy as np
import pandas as pd

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd.capture_volume import CaptureVolume  # noqa: E402
from caliscope_amd.constraints import ConstraintSet  # noqa: E402
from caliscope_amd.point_data import STATIC_SYNC_INDEX, ImagePoints, WorldPoints  # noqa: E402
from caliscope_amd.scale_accuracy import DeviceScaleErrors  # noqa: E402
from caliscope_amd.synthetic import ring_camera_array  # noqa: E402


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def grid(rows, cols, spacing):
    return np.array([[c * spacing, r * spacing, 0.0] for r in range(rows) for c in range(cols)])


def session(seed, n_frames, objects, n_cams):
    """``objects``: (object_id, points[nk, 3], static).  World points: a rigid motion of 1.001 x the object's points per frame (one
    for a static object, at STATIC_SYNC_INDEX) plus 0.5 mm of noise; every camera sees every corner in every frame."""
    rng = np.random.default_rng(seed)
    world, image = [], []
    for oid, pts, static in objects:
        nk = len(pts)
        n_pose = 1 if static else n_frames
        placed = 1.001 * np.einsum("fij,kj->fki", rotations(rng, n_pose), pts) + rng.normal(size=(n_pose, 1, 3)) + rng.normal(size=(n_pose, nk, 3)) * 5e-4
        sync = np.full(1, STATIC_SYNC_INDEX) if static else np.arange(n_frames)
        world.append(np.column_stack([np.repeat(sync, nk), np.full(n_pose * nk, oid), np.tile(np.arange(nk), n_pose), placed.reshape(-1, 3)]))
        f, c, k = np.meshgrid(np.arange(n_frames), np.arange(n_cams), np.arange(nk), indexing="ij")
        n = f.size
        image.append(np.column_stack([f.ravel(), c.ravel(), np.full(n, oid), k.ravel(), rng.uniform(0, 1000, n), rng.uniform(0, 1000, n), pts[k.ravel()]]))
    wdf = pd.DataFrame(np.concatenate(world), columns=["sync_index", "object_id", "keypoint_id", "x_coord", "y_coord", "z_coord"])
    idf = pd.DataFrame(np.concatenate(image), columns=["sync_index", "cam_id", "object_id", "keypoint_id", "img_loc_x", "img_loc_y", "obj_loc_x", "obj_loc_y", "obj_loc_z"])
    wdf = wdf.astype({c: "int64" for c in ("sync_index", "object_id", "keypoint_id")})
    idf = idf.astype({c: "int64" for c in ("sync_index", "cam_id", "object_id", "keypoint_id")})
    static_ids = frozenset(oid for oid, _, static in objects if static)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CaptureVolume(ring_camera_array(n_cams, radius=3.0, target=(0.0, 0.0, 0.5)), ImagePoints(idf), WorldPoints(wdf),
                             ConstraintSet((), static_ids) if static_ids else None)


def numpy_statistics(xyz, group_start, ent_world, ent_obj, max_pairs=4_000_000):
    """The eight numbers per group by vectorised numpy (groups of one size together, in chunks of at most ``max_pairs`` pairs)."""
    size = np.diff(group_start)
    out = np.zeros((len(size), 8))
    for s in np.unique(size).tolist():
        if s < 2:
            continue
        i, j = np.triu_indices(s, 1)
        groups = np.flatnonzero(size == s)
        step = max(1, max_pairs // len(i))
        for a in range(0, len(groups), step):
            g = groups[a:a + step]
            idx = group_start[g][:, None] + np.arange(s)[None, :]
            w, o = xyz[ent_world[idx]], ent_obj[idx]
            dt = np.sqrt(((o[:, i] - o[:, j]) ** 2).sum(axis=2))
            err = np.sqrt(((w[:, i] - w[:, j]) ** 2).sum(axis=2)) - dt
            out[g] = np.column_stack([err.sum(axis=1), (err * err).sum(axis=1), np.abs(err).max(axis=1), dt.max(axis=1), w.mean(axis=1), np.full(len(g), len(i))])
    return out


def per_group_loop_seconds(vol, limit=200):
    """Seconds per group of a per-group Python loop in the reference's style (see the module docstring), on the first ``limit`` groups."""
    from scipy.spatial.distance import pdist

    idf, wdf = vol.image_points.df, vol.world_points.df
    idf = idf[~idf[["obj_loc_x", "obj_loc_y"]].isna().any(axis=1)]
    static = vol.constraints.static_object_ids if vol.constraints else frozenset()
    done, t0 = 0, time.perf_counter()
    for (si, oid), rows in idf.groupby(["sync_index", "object_id"]):
        at = STATIC_SYNC_INDEX if oid in static else si
        sub = wdf[(wdf["sync_index"] == at) & (wdf["object_id"] == oid)]
        loc = rows[["object_id", "keypoint_id", "obj_loc_x", "obj_loc_y", "obj_loc_z"]].drop_duplicates(subset=["object_id", "keypoint_id"])
        both = sub.merge(loc, on=["object_id", "keypoint_id"], how="inner")
        if len(both) >= 3:
            err = pdist(both[["x_coord", "y_coord", "z_coord"]].to_numpy()) - pdist(both[["obj_loc_x", "obj_loc_y", "obj_loc_z"]].to_numpy())
            float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max()), rows["cam_id"].nunique()
        done += 1
        if done >= limit:
            break
    return (time.perf_counter() - t0) / max(done, 1), done


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sessions", default="a,b,c")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--fraction", type=float, default=1.0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    marker = np.array([[-0.05, 0.05, 0.0], [0.05, 0.05, 0.0], [0.05, -0.05, 0.0], [-0.05, -0.05, 0.0]])
    frames = lambda n: max(4, int(round(n * args.fraction)))  # noqa: E731
    specs = {
        "a": ("30 000 frames x 7 x 5 board x 8 cameras", lambda: session(1, frames(30_000), [(0, grid(5, 7, 0.04), False)], 8)),
        "b": ("250 000 frames x 4-corner marker + 2 static markers x 2 cameras",
              lambda: session(2, frames(250_000), [(0, marker, False), (1, marker * 2.0, True), (2, marker * 3.0, True)], 2)),
        "c": ("200 frames x 600-corner board x 4 cameras", lambda: session(3, frames(200), [(0, grid(20, 30, 0.03), False)], 4)),
    }
    dev = DeviceScaleErrors(args.device)
    for key in args.sessions.split(","):
        title, make = specs[key]
        t0 = time.perf_counter()
        vol = make()
        t_make = time.perf_counter() - t0
        t0 = time.perf_counter()
        g_sync, g_obj, n_cams, n_corners, group_start, ent_world, ent_obj = vol._scale_groups()
        t_marshal = time.perf_counter() - t0
        xyz = vol.world_points.points
        pairs = int((n_corners * (n_corners - 1) // 2).sum())
        print(f"session ({key}) {title}: {len(vol.image_points)} image rows, {len(xyz)} world points, {len(g_sync)} groups, {pairs} pairs "
              f"(built in {t_make:.1f} s)", flush=True)
        print(f"  host marshalling (_scale_groups): {t_marshal * 1e3:.1f} ms")
        stats = dev.scale_errors(xyz, group_start, ent_world, ent_obj)  # warm-up: module load, first allocation
        times = []
        for _ in range(max(args.repeats, 1)):
            t0 = time.perf_counter()
            again = dev.scale_errors(xyz, group_start, ent_world, ent_obj)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(again, stats)
        print(f"  cba_scale_errors (upload + launches + copy-back), {len(times)} calls: median {np.median(times) * 1e3:.2f} ms, "
              f"min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}")
        t0 = time.perf_counter()
        ref = numpy_statistics(xyz, group_start, ent_world, ent_obj)
        t_numpy = time.perf_counter() - t0
        print(f"  vectorised numpy, one host thread: {t_numpy * 1e3:.1f} ms; largest difference of sum err^2 from the device: "
              f"{np.abs(ref[:, 1] - stats[:, 1]).max():.3e} (largest sum {stats[:, 1].max():.3e})")
        per_group, measured = per_group_loop_seconds(vol)
        print(f"  per-group Python loop in the reference's style: {per_group * 1e3:.2f} ms per group on {measured} groups; EXTRAPOLATED to "
              f"{len(g_sync)} groups: {per_group * len(g_sync):.1f} s", flush=True)
        t0 = time.perf_counter()
        rep = vol.compute_volumetric_scale_accuracy()
        print(f"  compute_volumetric_scale_accuracy() in all (marshalling, device call, {len(rep.frame_errors)} report entries): "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms; pooled RMSE {rep.pooled_rmse_mm:.3f} mm")


if __name__ == "__main__":
    main()
