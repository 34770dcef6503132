"""Timing of the trajectory reconstruction with and without the per-sample 3-D covariance, on one MI355X.

    python tools/trajectory_uncertainty_timing.py [--cameras 8] [--frames 2000] [--trajectories 500] [--runs 10] [--warmup 2]
                                                  [--out profiles/trajectory_uncertainty.json]

The seeded synthetic recording of tools/trajectory_refine_timing.py on the dense grid of the call: ``--cameras`` ring cameras, every
one of which sees every landmark in every frame (8 x 2 000 x 500: 1 M slots, 8 M rows; 36 camera pairs per slot), 0.3 px of noise,
2 % of the cells moved by 60 px.  The calibration is a dense random PSD ``cam_cov`` over nine-wide cameras, so every block of the
pair pass is a full 9 x 9.

Timed, each as the median of ``--runs`` calls after ``--warmup`` calls, host checks, upload, launches and copy-back included, in
rounds that alternate the five calls: ``cba_reconstruct_trajectories``, ``cba_reconstruct_trajectories_refined`` (the defaults of
``RefineOptions`` plus ``reject_px = 5``), and ``cba_reconstruct_trajectories_uncertain`` on the refined call with the noise term
alone, on the refined call with the calibration term, and on the plain call with the calibration term (``xy_gap = xyz_gap = 0``, no
filter: the covariance is the only difference).  The covariance adds 97 bytes per slot to the copy-back (49 noise-only), which is
part of what it costs.  ``--out`` writes the figures as JSON."""
import argparse
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from trajectory_refine_timing import grid_of  # noqa: E402

from caliscope_amd.build import source_digest  # noqa: E402
from caliscope_amd.reconstruction import DeviceTrajectorySolver  # noqa: E402
from caliscope_amd.synthetic import ring_camera_array  # noqa: E402
from caliscope_amd.trajectory_refinement import DeviceRefinedTrajectorySolver, RefineOptions  # noqa: E402
from caliscope_amd.trajectory_uncertainty import CovarianceOptions, DeviceUncertainTrajectorySolver, uncertainty_tables  # noqa: E402


def report_of(cam_ids, width=9, seed=3, scale=1e-8):
    """What ``uncertainty_tables`` reads of an UncertaintyReport: ``width``-wide cameras and a dense PSD ``cam_cov_full``."""
    ncp = width * len(cam_ids)
    G = np.random.default_rng(seed).normal(size=(ncp, ncp))
    full = G @ G.T * scale
    full = 0.5 * (full + full.T)
    cameras = {int(c): SimpleNamespace(param_cov=full[width * i:width * (i + 1), width * i:width * (i + 1)]) for i, c in enumerate(cam_ids)}
    return SimpleNamespace(cameras=cameras, cam_cov_full=full)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--trajectories", type=int, default=500)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sigma-px", type=float, default=0.3)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    grid = grid_of(args.cameras, args.frames, args.trajectories)
    cams = ring_camera_array(args.cameras)
    options = RefineOptions(reject_px=5.0)
    full = uncertainty_tables(grid, cams, CovarianceOptions(args.sigma_px, report_of(sorted(cams.cameras))))
    noise = uncertainty_tables(grid, cams, CovarianceOptions(args.sigma_px))
    plain, refined, uncertain = DeviceTrajectorySolver(args.device), DeviceRefinedTrajectorySolver(args.device), DeviceUncertainTrajectorySolver(args.device)
    calls = {
        "unrefined": lambda: plain.reconstruct(grid),
        "refined": lambda: refined.reconstruct_refined(grid, options),
        "refined_cov_noise_only": lambda: uncertain.reconstruct_uncertain(grid, noise, options),
        "refined_cov_full": lambda: uncertain.reconstruct_uncertain(grid, full, options),
        "unrefined_cov_full": lambda: uncertain.reconstruct_uncertain(grid, full, None),
    }
    times, last = {name: [] for name in calls}, {}
    for round_ in range(args.warmup + args.runs):
        for name, call in calls.items():
            t0 = time.perf_counter()
            last[name] = call()
            if round_ >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    cov = last["refined_cov_full"][2]
    ok = cov.cov_status == 1
    std = np.sqrt(cov.cov[ok][:, [0, 3, 5]].sum(axis=1))
    figures = {
        "what": "median wall time of one call (host checks, upload, launches, copy-back) on one MI355X, the five calls alternating",
        "cameras": args.cameras, "frames": args.frames, "trajectories": args.trajectories, "slots": grid.n_slots, "rows": len(grid.row_cam),
        "pairs_per_slot": args.cameras * (args.cameras + 1) // 2, "ncp": int(full.cam_cov.shape[0]), "sigma_px": args.sigma_px, "runs": args.runs,
        "warmup": args.warmup,
        **{f"{name}_ms_median": float(np.median(t)) for name, t in times.items()}, **{f"{name}_ms": [round(v, 3) for v in t] for name, t in times.items()},
        "cov_status_counts": np.bincount(cov.cov_status, minlength=3).tolist(), "sqrt_trace_cov_median_mm": float(np.median(std) * 1e3),
        "calib_share_median": float(np.median(cov.cov_calib[ok][:, [0, 3, 5]].sum(axis=1) / cov.cov[ok][:, [0, 3, 5]].sum(axis=1))),
        "same_points_as_the_refined_call": bool(last["refined_cov_full"][0].xyz.tobytes() == last["refined"][0].xyz.tobytes()),
        "library_source_sha256": source_digest(),
    }
    print(json.dumps(figures, indent=1))
    if args.out is not None:
        args.out.write_text(json.dumps(figures, indent=1) + "\n")


if __name__ == "__main__":
    main()
