"""Timing of the reconstruction of a recording: the host chain against reconstruct_trajectories (cba_reconstruct_trajectories).

    python tools/reconstruction_timing.py [--frames 20000] [--cameras 8] [--keypoints 33] [--repeats 5] [--skip-host]

A seeded synthetic recording: ``--cameras`` ring cameras x ``--keypoints`` landmarks of one object x ``--frames`` frames, every camera
sees every landmark, 0.5 px of noise, and 5 % of the rows taken out in runs of 1 to 6 frames per (camera, landmark) track.

Host chain, each step timed once: ``ImagePoints.fill_gaps(3)`` (pandas sorts), ``.triangulate`` (lexsort, a Python loop over the rows,
then ``cba_triangulate`` on the device), ``WorldPoints.fill_gaps(3)``, ``WorldPoints.smooth(30, 6, 2)`` (a scipy call per trajectory).

New path: ``trajectory_grid`` (host: np.unique and one argsort), the ``cba_reconstruct_trajectories`` call (checks on the host, upload,
five launches, copy-back; after a warm-up call, median / min / max of ``--repeats`` calls), ``world_points_of`` (compaction into a
table).  The call does not time its parts; for the kernels alone run this program once under
``rocprofv3 --kernel-trace --stats -- python tools/reconstruction_timing.py --skip-host --repeats 2``: what is left of the call's time
is the host check, the upload and the copy-back."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd.point_data import ImagePoints  # noqa: E402
from caliscope_amd.reconstruction import DeviceTrajectorySolver, filter_coefficients, trajectory_grid, world_points_of  # noqa: E402
from caliscope_amd.synthetic import project_pinhole_bc5, ring_camera_array  # noqa: E402


def recording(n_cams, n_kp, n_frames, seed=11, dropped=0.05):
    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams)
    frames = np.arange(n_frames)
    base = np.column_stack([rng.uniform(-0.4, 0.4, n_kp), rng.uniform(-0.4, 0.4, n_kp), rng.uniform(0.2, 1.0, n_kp)])
    phase = 0.02 * frames[:, None, None] + rng.uniform(0, 6.28, (1, n_kp, 3))
    truth = (base[None] + 0.15 * np.sin(phase)).reshape(-1, 3)
    f, k = np.divmod(np.arange(n_frames * n_kp), n_kp)
    parts = []
    for cid in sorted(cams.cameras):
        cam = cams.cameras[cid]
        K = cam.matrix
        uv, _ = project_pinhole_bc5(truth, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
        uv = uv + rng.normal(0, 0.5, uv.shape)
        # runs of 1..6 missing frames per track: starts at a rate that takes out `dropped` of the rows (mean run 3.5)
        start = rng.random((n_frames, n_kp)) < dropped / 3.5
        length = rng.integers(1, 7, (n_frames, n_kp))
        edge = np.zeros((n_frames + 7, n_kp), dtype=np.int64)
        sf, sk = np.nonzero(start)
        np.add.at(edge, (sf, sk), 1)
        np.add.at(edge, (sf + length[sf, sk], sk), -1)
        seen = (np.cumsum(edge, axis=0)[:n_frames] == 0).reshape(-1)
        parts.append(pd.DataFrame({"sync_index": f[seen], "cam_id": cid, "object_id": 0, "keypoint_id": k[seen], "img_loc_x": uv[seen, 0],
                                   "img_loc_y": uv[seen, 1], "frame_time": f[seen] / 30.0 + 1e-4 * cid}))
    return ImagePoints(pd.concat(parts, ignore_index=True)), cams


def timed(label, fn):
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    print(f"  {label}: {dt * 1e3:.1f} ms", flush=True)
    return out, dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=20_000)
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--keypoints", type=int, default=33)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    smooth = (30.0, 6.0, 2)
    t0 = time.perf_counter()
    ip, cams = recording(args.cameras, args.keypoints, args.frames)
    full = args.cameras * args.keypoints * args.frames
    print(f"recording: {args.cameras} cameras x {args.keypoints} keypoints x {args.frames} frames, {len(ip)} rows ({100 - 100 * len(ip) / full:.2f} % taken "
          f"out; built in {time.perf_counter() - t0:.1f} s)", flush=True)

    host = None
    if not args.skip_host:
        print("host chain (fill_gaps(3) -> triangulate -> fill_gaps(3) -> smooth(30, 6, 2)):")
        filled, t1 = timed("ImagePoints.fill_gaps(3)", lambda: ip.fill_gaps(3))
        world, t2 = timed("ImagePoints.triangulate (host grouping + cba_triangulate)", lambda: filled.triangulate(cams))
        world, t3 = timed("WorldPoints.fill_gaps(3)", lambda: world.fill_gaps(3))
        host, t4 = timed("WorldPoints.smooth(30, 6, 2)", lambda: world.smooth(*smooth))
        print(f"  total: {(t1 + t2 + t3 + t4) * 1e3:.1f} ms, {len(host)} world rows", flush=True)

    print("reconstruct_trajectories (xy_gap_fill=3, xyz_gap_fill=3, smooth=(30, 6, 2)):")
    grid, t_grid = timed("trajectory_grid (host marshalling)", lambda: trajectory_grid(ip, cams))
    solver, filt = DeviceTrajectorySolver(args.device), filter_coefficients(smooth)
    call = lambda: solver.reconstruct(grid, xy_gap=3, xyz_gap=3, filt=filt)  # noqa: E731
    result, t_first = timed("first call (module load, first allocations)", call)
    times = []
    for _ in range(max(args.repeats, 1)):
        t0 = time.perf_counter()
        again = call()
        times.append(time.perf_counter() - t0)
    assert again.xyz.tobytes() == result.xyz.tobytes() and again.valid.tobytes() == result.valid.tobytes()
    print(f"  cba_reconstruct_trajectories (host checks + upload + launches + copy-back), {len(times)} calls: median {np.median(times) * 1e3:.1f} ms, "
          f"min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}")
    up = (grid.row_cam.nbytes + grid.row_slot.nbytes + grid.row_xy.nbytes + grid.row_time.nbytes) / 1e6
    down = (result.xyz.nbytes + result.valid.nbytes + result.slot_time.nbytes + result.frame_time.nbytes) / 1e6
    print(f"  uploaded {up:.1f} MB, copied back {down:.1f} MB; grid {grid.n_cams} x {grid.n_frames} x {grid.n_traj} = {grid.n_cams * grid.n_slots} cells")
    mine, t_table = timed("world_points_of (compaction into a table)", lambda: world_points_of(grid, result))
    print(f"  total with a median call: {(t_grid + np.median(times) + t_table) * 1e3:.1f} ms, {len(mine)} world rows", flush=True)
    if host is not None:
        a = mine.df.to_numpy(dtype=np.float64)
        b = host.df.sort_values(["sync_index", "object_id", "keypoint_id"]).to_numpy(dtype=np.float64)
        same_keys = a.shape == b.shape and np.array_equal(a[:, :3], b[:, :3])
        print(f"agreement with the host chain: keys {'identical' if same_keys else 'DIFFERENT'}"
              + (f", max |xyz difference| {np.max(np.abs(a[:, 3:6] - b[:, 3:6])):.3e}, rows with identical xyz bits "
                 f"{int((a[:, 3:6] == b[:, 3:6]).all(axis=1).sum())} of {len(a)}" if same_keys else ""))
        print(f"host chain / new path: {(t1 + t2 + t3 + t4) / (t_grid + np.median(times) + t_table):.2f} x")


if __name__ == "__main__":
    main()
