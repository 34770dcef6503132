"""Timing of cba_estimate_time_offsets on one MI355X.

    python tools/time_offsets_timing.py [--cameras 8] [--frames 20000] [--trajectories 33] [--repeats 5] [--skip-oracle]

A seeded synthetic recording on the dense grid of the call, the shape of profiles/reconstruction_timing.txt: ``--cameras`` ring cameras,
every one of which sees every landmark in every frame, landmarks on sinusoids of up to 0.5 m/s, 0.3 px of noise, camera offsets of
-6 .. 6 ms and a stamp jitter of up to 5 ms.  The grid is built directly (the pandas marshalling of ``trajectory_grid`` is not what is
measured).  Timed: the first call (module load, first allocations), then ``--repeats`` calls, host checks, upload, launches, the
host's reads between them and the copy-back included; the median, the smallest and the largest are printed with the rounds taken and
the recovered offsets.  Unless ``--skip-oracle``, the numpy restatement of tests/time_offset_oracle.py is timed on the CURVED scene of
tests/time_offset_scenes.py (360 slots), which it can still finish.  For the per-kernel split run the tool under a kernel trace
(``rocprofv3 --kernel-trace --stats -- python tools/time_offsets_timing.py --repeats 2 --skip-oracle``)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd.reconstruction import TrajectoryGrid  # noqa: E402
from caliscope_amd.synthetic import project_pinhole_bc5, ring_camera_array  # noqa: E402
from caliscope_amd.time_offsets import DeviceTimeOffsetSolver, TimeOffsetOptions, options_struct  # noqa: E402
from caliscope_amd.triangulation import camera_tables  # noqa: E402


def grid_of(n_cams, n_frames, n_traj, seed=11):
    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams)
    ids = sorted(cams.cameras)
    offsets = np.array([0.0] + [1e-3 * ((5 * c) % 13 - 6) for c in range(1, n_cams)])
    base = np.column_stack([rng.uniform(-0.4, 0.4, n_traj), rng.uniform(-0.4, 0.4, n_traj), rng.uniform(0.2, 1.0, n_traj)])
    phase = rng.uniform(0, 6.28, (n_traj, 3))
    rate = rng.uniform(1.0, 3.0, (n_traj, 3))
    order = np.arange(n_frames * n_traj).reshape(n_frames, n_traj).T.ravel()  # rows of a camera: trajectory, then frame
    xy = np.empty((n_cams, n_frames * n_traj, 2))
    stamps = np.empty((n_cams, n_frames * n_traj))
    for c, cid in enumerate(ids):
        stamp = np.arange(n_frames) / 30.0 + rng.uniform(-5e-3, 5e-3, n_frames)
        t = (stamp + offsets[c])[:, None, None]
        truth = (base[None] + 0.15 * np.sin(rate[None] * t + phase[None])).reshape(-1, 3)  # slot order: frame, then trajectory
        cam = cams.cameras[cid]
        K = cam.matrix
        uv, _ = project_pinhole_bc5(truth, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
        xy[c] = (uv + rng.normal(0, 0.3, uv.shape))[order]
        stamps[c] = np.repeat(stamp, n_traj)[order]
    model, intr, P = camera_tables(cams, ids)
    grid = TrajectoryGrid(sync_min=0, n_frames=n_frames, cam_ids=np.array(ids), traj_object=np.zeros(n_traj, dtype=np.int64),
                          traj_keypoint=np.arange(n_traj), cam_posed=np.ones(n_cams, dtype=np.uint8), cam_model=model, cam_intr=intr, cam_P=P,
                          row_cam=np.repeat(np.arange(n_cams, dtype=np.int32), len(order)), row_slot=np.tile(order.astype(np.int64), n_cams),
                          row_xy=np.ascontiguousarray(xy.reshape(-1, 2)), row_time=np.ascontiguousarray(stamps.reshape(-1)))
    return grid, offsets


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--trajectories", type=int, default=33)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--skip-oracle", action="store_true")
    args = ap.parse_args()

    t0 = time.perf_counter()
    grid, offsets = grid_of(args.cameras, args.frames, args.trajectories)
    print(f"recording: {args.cameras} cameras x {args.trajectories} landmarks x {args.frames} frames, {len(grid.row_cam)} rows, {grid.n_slots} slots "
          f"(built in {time.perf_counter() - t0:.1f} s)")
    solver = DeviceTimeOffsetSolver(args.device)
    options = options_struct(TimeOffsetOptions(), grid)
    t0 = time.perf_counter()
    res = solver.estimate(grid, options)
    print(f"first call (module load, first allocations): {(time.perf_counter() - t0) * 1e3:.1f} ms")
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        res = solver.estimate(grid, options)
        times.append((time.perf_counter() - t0) * 1e3)
    print(f"cba_estimate_time_offsets (host checks + upload + launches + reads + copy-back), {args.repeats} calls: median {np.median(times):.1f} ms, "
          f"min {min(times):.1f}, max {max(times):.1f}")
    print(f"rounds {res.rounds}, converged {res.converged}, sigma0 {res.sigma0_px:.4f} px; largest |offset - truth| {np.nanmax(np.abs(res.offsets - offsets)):.3e} s, "
          f"largest sigma {np.nanmax(res.sigma):.3e} s; rms before {np.nanmax(res.rms_before):.3f} px, after {np.nanmax(res.rms_after):.3f} px")
    if not args.skip_oracle:
        from tests import time_offset_oracle as TO
        from tests import time_offset_scenes as TS

        small = TS.curved().grid
        t0 = time.perf_counter()
        o = TO.estimate(small)
        print(f"host oracle (numpy, dense Jacobian, lstsq) on CURVED, {small.n_cams} cameras x {small.n_traj} landmarks x {small.n_frames} frames = {small.n_slots} "
              f"slots: {time.perf_counter() - t0:.1f} s, {o.rounds} rounds")
        t0 = time.perf_counter()
        r = solver.estimate(small, options_struct(TimeOffsetOptions(), small))
        print(f"the device call on the same scene: {(time.perf_counter() - t0) * 1e3:.1f} ms, {r.rounds} rounds")


if __name__ == "__main__":
    main()
