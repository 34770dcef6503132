"""Timing of the covariance-weighted smoother beside the Butterworth filter it competes with, on one MI355X.

    python tools/trajectory_smoother_timing.py [--cameras 8] [--keypoints 33] [--frames 20000] [--runs 10] [--warmup 2]
                                               [--accel-density 0.02] [--kernel-stats STATS.csv] [--out profiles/trajectory_smoother.json]

The seeded synthetic recording of tools/reconstruction_timing.py: ``--cameras`` ring cameras x
``--keypoints`` landmarks of one object x ``--frames`` frames, 0.5 px of noise, 5 % of the rows taken out in runs of 1 to 6 frames
(8 x 33 x 20 000: 660 000 slots, 5.0 M rows).  33 trajectories are 33 threads of ``k_traj_smooth`` and 99 of ``k_traj_filtfilt`` (one
per coordinate): both are serial recurrences over the frames, bound by latency, and would take as long for thousands of
trajectories.

Timed, each as the median of ``--runs`` calls after ``--warmup`` calls, host checks, upload, launches and copy-back included, in
rounds that alternate the three calls (``xy_gap = 3``, no refinement, the noise term alone, ``sigma_px = 0.5``):
``cba_reconstruct_trajectories_uncertain``; the same with ``smooth = (30, 6, 2)``, the order-2 Butterworth filter at 6 Hz; and
``cba_reconstruct_trajectories_smoothed`` (``velocity_prior_std = 10``, ``max_gap = 3`` and ``accel_density = 0.02``, at which the
mean ``nis`` of this slow recording is 3: the model and ``sigma_px`` are consistent with the data).  The smoothed call
copies 201 bytes per slot more back than the uncertain call, which is part of what it costs.

The calls do not time their kernels.  For those, run this program once under
``rocprofv3 --kernel-trace --stats -o NAME -- python tools/trajectory_smoother_timing.py --runs 3 --warmup 1`` and hand its
``NAME_kernel_stats.csv`` to a second, unprofiled run as ``--kernel-stats``: the mean time per launch of every ``k_traj_*`` kernel goes
into the figures.  ``--out`` writes them as JSON.  There is no pass / fail time."""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from reconstruction_timing import recording  # noqa: E402

from caliscope_amd.build import source_digest  # noqa: E402
from caliscope_amd.reconstruction import filter_coefficients, trajectory_grid  # noqa: E402
from caliscope_amd.trajectory_smoother import DeviceTrajectorySmoother, SmootherOptions  # noqa: E402
from caliscope_amd.trajectory_uncertainty import CovarianceOptions, DeviceUncertainTrajectorySolver, uncertainty_tables  # noqa: E402


def kernel_stats(path: Path) -> dict:
    """``{kernel: {"launches": n, "mean_ms": t}}`` of the ``k_traj_*`` kernels in a ``rocprofv3 --stats`` kernel table."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if "k_traj_" not in name:
                continue
            short = name[name.index("k_traj_"):].split("(")[0].split("<")[0]
            entry = out.setdefault(short, {"launches": 0, "total_ms": 0.0})
            entry["launches"] += int(row["Calls"])
            entry["total_ms"] += float(row["TotalDurationNs"]) * 1e-6
    return {k: {"launches": v["launches"], "mean_ms": v["total_ms"] / v["launches"]} for k, v in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--keypoints", type=int, default=33)
    ap.add_argument("--frames", type=int, default=20_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sigma-px", type=float, default=0.5)
    ap.add_argument("--accel-density", type=float, default=0.02)
    ap.add_argument("--kernel-stats", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    image_points, cams = recording(args.cameras, args.keypoints, args.frames)
    grid = trajectory_grid(image_points, cams)
    tables = uncertainty_tables(grid, cams, CovarianceOptions(args.sigma_px))
    smooth, options = (30.0, 6.0, 2), SmootherOptions(fps=30.0, accel_density=args.accel_density)
    filt = filter_coefficients(smooth)
    uncertain, smoother = DeviceUncertainTrajectorySolver(args.device), DeviceTrajectorySmoother(args.device)
    calls = {
        "uncertain": lambda: uncertain.reconstruct_uncertain(grid, tables, None, xy_gap=3),
        "uncertain_butterworth": lambda: uncertain.reconstruct_uncertain(grid, tables, None, xy_gap=3, filt=filt),
        "smoothed": lambda: smoother.reconstruct_smoothed(grid, tables, options, None, xy_gap=3),
    }
    times, last = {name: [] for name in calls}, {}
    for round_ in range(args.warmup + args.runs):
        for name, call in calls.items():
            t0 = time.perf_counter()
            last[name] = call()
            if round_ >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    sm, cov = last["smoothed"][3], last["smoothed"][2]
    ok = sm.status == 1
    figures = {
        "what": "median wall time of one call (host checks, upload, launches, copy-back) on one MI355X, the three calls alternating",
        "cameras": args.cameras, "keypoints": args.keypoints, "frames": args.frames, "trajectories": grid.n_traj, "slots": grid.n_slots,
        "rows": len(grid.row_cam), "sigma_px": args.sigma_px, "butterworth": list(smooth), "fps": options.fps, "accel_density": options.accel_density,
        "velocity_prior_std": options.velocity_prior_std, "max_gap": options.max_gap, "runs": args.runs, "warmup": args.warmup,
        **{f"{name}_ms_median": float(np.median(t)) for name, t in times.items()}, **{f"{name}_ms": [round(v, 3) for v in t] for name, t in times.items()},
        "smooth_status_counts": np.bincount(sm.status, minlength=3).tolist(), "cov_status_counts": np.bincount(cov.cov_status, minlength=3).tolist(),
        "sqrt_trace_sample_cov_median_mm": float(np.median(np.sqrt(sm.meas_cov[ok][:, [0, 3, 5]].sum(axis=1))) * 1e3),
        "sqrt_trace_smoothed_cov_median_mm": float(np.median(np.sqrt(sm.pos_cov[ok][:, [0, 3, 5]].sum(axis=1))) * 1e3),
        "nis_mean": float(np.nanmean(sm.nis)),
        "same_points_as_the_uncertain_call": bool(last["smoothed"][0].xyz.tobytes() == last["uncertain"][0].xyz.tobytes()),
        "library_source_sha256": source_digest(),
    }
    if args.kernel_stats is not None:
        figures["kernels"] = kernel_stats(args.kernel_stats)
    print(json.dumps(figures, indent=1))
    if args.out is not None:
        args.out.write_text(json.dumps(figures, indent=1) + "\n")


if __name__ == "__main__":
    main()
