"""Timing of the trajectory reconstruction with and without the robust reprojection refinement, on one MI355X.

    python tools/trajectory_refine_timing.py [--cameras 8] [--frames 2000] [--trajectories 500] [--runs 10] [--warmup 2]
                                             [--parent-lib PATH] [--out profiles/trajectory_refine.json]

A seeded synthetic recording on the dense grid of the call: ``--cameras`` ring cameras, every one of which sees every landmark in every
frame (8 x 2 000 x 500: 1 M slots, 8 M rows), 0.3 px of noise, and 2 % of the cells moved by 60 px.  The grid is built directly (the
pandas marshalling of ``trajectory_grid`` is not what is measured).

Timed, each as the median of ``--runs`` calls after ``--warmup`` calls, host checks, upload, launches and copy-back included:
``cba_reconstruct_trajectories`` and ``cba_reconstruct_trajectories_refined`` with the defaults of ``RefineOptions`` plus
``reject_px = 5`` (both with ``xy_gap = xyz_gap = 0`` and no filter: the refinement is the only difference).  With ``--parent-lib`` the
unrefined call is timed once more, in a child process of its own, on the library at that path — the build of the commit before the
refinement, which is the figure to set the refined call against.  The evaluations summed over the slots come from the call's own
``iterations`` output.  ``--out`` writes the figures as JSON."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd.reconstruction import DeviceTrajectorySolver, TrajectoryGrid  # noqa: E402
from caliscope_amd.synthetic import project_pinhole_bc5, ring_camera_array  # noqa: E402
from caliscope_amd.triangulation import camera_tables  # noqa: E402


def grid_of(n_cams, n_frames, n_traj, seed=11, outliers=0.02) -> TrajectoryGrid:
    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams)
    ids = sorted(cams.cameras)
    frames = np.arange(n_frames)
    base = np.column_stack([rng.uniform(-0.4, 0.4, n_traj), rng.uniform(-0.4, 0.4, n_traj), rng.uniform(0.2, 1.0, n_traj)])
    phase = 0.02 * frames[:, None, None] + rng.uniform(0, 6.28, (1, n_traj, 3))
    truth = (base[None] + 0.15 * np.sin(phase)).reshape(-1, 3)              # slot order: frame, then trajectory
    order = np.arange(n_frames * n_traj).reshape(n_frames, n_traj).T.ravel()  # rows of a camera: trajectory, then frame
    xy = np.empty((n_cams, n_frames * n_traj, 2))
    for c, cid in enumerate(ids):
        cam = cams.cameras[cid]
        K = cam.matrix
        uv, _ = project_pinhole_bc5(truth, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
        uv = uv + rng.normal(0, 0.3, uv.shape)
        bad = rng.random(len(uv)) < outliers
        angle = rng.uniform(0, 2 * np.pi, len(uv))
        uv[bad] += 60.0 * np.column_stack([np.cos(angle[bad]), np.sin(angle[bad])])
        xy[c] = uv[order]
    model, intr, P = camera_tables(cams, ids)
    return TrajectoryGrid(sync_min=0, n_frames=n_frames, cam_ids=np.array(ids), traj_object=np.zeros(n_traj, dtype=np.int64),
                          traj_keypoint=np.arange(n_traj), cam_posed=np.ones(n_cams, dtype=np.uint8), cam_model=model, cam_intr=intr, cam_P=P,
                          row_cam=np.repeat(np.arange(n_cams, dtype=np.int32), len(order)), row_slot=np.tile(order.astype(np.int64), n_cams),
                          row_xy=np.ascontiguousarray(xy.reshape(-1, 2)), row_time=np.tile(order // n_traj / 30.0, n_cams))


def median_ms(call, runs, warmup):
    for _ in range(warmup):
        out = call()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = call()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times], out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--trajectories", type=int, default=500)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-lib", type=Path, default=None, help="libcaliscope_ba.so built from the commit before the refinement")
    ap.add_argument("--plain-only", action="store_true", help="time the unrefined call alone and print its JSON (what the child process runs)")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    grid = grid_of(args.cameras, args.frames, args.trajectories)
    plain = DeviceTrajectorySolver(args.device)
    plain_ms, plain_all, base = median_ms(lambda: plain.reconstruct(grid), args.runs, args.warmup)
    if args.plain_only:
        print(json.dumps({"plain_ms_median": plain_ms, "plain_ms": plain_all, "valid": int(base.valid.sum())}))
        return

    from caliscope_amd.build import source_digest
    from caliscope_amd.trajectory_refinement import DeviceRefinedTrajectorySolver, RefineOptions

    options = RefineOptions(reject_px=5.0)
    refined = DeviceRefinedTrajectorySolver(args.device)
    refined_ms, refined_all, (res, q) = median_ms(lambda: refined.reconstruct_refined(grid, options), args.runs, args.warmup)
    uploaded = grid.row_cam.nbytes + grid.row_slot.nbytes + grid.row_xy.nbytes + grid.row_time.nbytes
    figures = {
        "what": "median wall time of one call (host checks, upload, launches, copy-back) on one MI355X",
        "cameras": args.cameras, "frames": args.frames, "trajectories": args.trajectories, "slots": grid.n_slots, "rows": len(grid.row_cam),
        "uploaded_mb": round(uploaded / 1e6, 1), "runs": args.runs, "warmup": args.warmup,
        "options": {"loss": options.loss, "f_scale": options.f_scale, "max_iter": options.max_iter, "reject_px": options.reject_px,
                    "max_reject": options.max_reject, "min_views": options.min_views},
        "unrefined_ms_median": plain_ms, "unrefined_ms": plain_all, "refined_ms_median": refined_ms, "refined_ms": refined_all,
        "iterations_sum": int(q.iterations.sum()), "iterations_max": int(q.iterations.max()), "status_counts": np.bincount(q.status, minlength=4).tolist(),
        "views_rejected": int((q.view_state == 2).sum()), "library_source_sha256": source_digest(),
    }
    if args.parent_lib is not None:
        env = dict(os.environ, CALISCOPE_BA_LIB=str(args.parent_lib.resolve()))
        child = subprocess.run([sys.executable, __file__, "--plain-only", "--cameras", str(args.cameras), "--frames", str(args.frames), "--trajectories",
                                str(args.trajectories), "--runs", str(args.runs), "--warmup", str(args.warmup), "--device", str(args.device)],
                               env=env, check=True, capture_output=True, text=True, timeout=600)
        parent = json.loads(child.stdout.strip().splitlines()[-1])
        assert parent["valid"] == int(base.valid.sum())
        figures["parent_unrefined_ms_median"], figures["parent_unrefined_ms"] = parent["plain_ms_median"], parent["plain_ms"]
    print(json.dumps(figures, indent=1))
    if args.out is not None:
        args.out.write_text(json.dumps(figures, indent=1) + "\n")


if __name__ == "__main__":
    main()
