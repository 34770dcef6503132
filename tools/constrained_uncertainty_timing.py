"""Timing of the parameter covariance with and without the rigid-distance rows of the boards, on one MI355X.

    python tools/constrained_uncertainty_timing.py [--cameras 8] [--frames 2000] [--rows 6] [--cols 9] [--runs 10] [--warmup 2]
                                                   [--out profiles/uncertainty_constrained.json]

A seeded synthetic session: ``--cameras`` ring cameras, ``--frames`` poses of a ``--rows`` x ``--cols`` board (8 x 2 000 x 54: 108 000
points, 864 000 observations with 0.4 px of noise), every camera seeing every corner; per pose the neighbour, diagonal and one
centroid row of the board (174 rows on 54 points: one constraint component per pose, at the cap of the component kernel), weighted
``(1 px / f) / 2 mm`` as ``CaptureVolume.optimize`` weights them.  Evaluated a millimetre off the truth.

Timed, each as the median of ``--runs`` calls after ``--warmup`` calls, everything included (argument checks, the host plan with its
union-find, upload, launches, copy-back), in rounds that alternate the two calls on the same arrays:
``cba_parameter_covariance_constrained`` with the rows and ``cba_parameter_covariance`` without them.  ``--out`` writes the figures as
JSON."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd.build import source_digest  # noqa: E402
from caliscope_amd.bundle_parameterization import BundleParameterization  # noqa: E402
from caliscope_amd.cameras import rvec_to_matrix  # noqa: E402
from caliscope_amd.synthetic import project_pinhole_bc5, ring_camera_array  # noqa: E402
from caliscope_amd.uncertainty import DeviceUncertainty  # noqa: E402


def board_rows(rows, cols, spacing):
    """(grid [rows * cols, 3], endpoints a [n, 4], endpoints b [n, 4], distances [n]) of one board: horizontal and vertical neighbours, both
    diagonals of every cell, and the centroid of the first cell against the centroid of the last."""
    grid = np.array([[c * spacing, r * spacing, 0.0] for r in range(rows) for c in range(cols)])
    grid -= grid.mean(axis=0)
    idx = lambda r, c: r * cols + c
    a, b = [], []
    for r in range(rows):
        for c in range(cols):
            if c + 1 < cols:
                a.append([idx(r, c)] * 4); b.append([idx(r, c + 1)] * 4)
            if r + 1 < rows:
                a.append([idx(r, c)] * 4); b.append([idx(r + 1, c)] * 4)
            if c + 1 < cols and r + 1 < rows:
                a.append([idx(r, c)] * 4); b.append([idx(r + 1, c + 1)] * 4)
                a.append([idx(r, c + 1)] * 4); b.append([idx(r + 1, c)] * 4)
    a.append([idx(0, 0), idx(0, 1), idx(1, 0), idx(1, 1)])
    b.append([idx(rows - 2, cols - 2), idx(rows - 2, cols - 1), idx(rows - 1, cols - 2), idx(rows - 1, cols - 1)])
    a, b = np.array(a, dtype=np.int32), np.array(b, dtype=np.int32)
    return grid, a, b, np.linalg.norm(grid[a].mean(axis=1) - grid[b].mean(axis=1), axis=1)


def session(n_cams, n_frames, rows, cols, spacing=0.03, seed=1, noise_px=0.4, sigma_m=0.002):
    """The twelve positional arguments of ``parameter_covariance_constrained``."""
    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams)
    grid, a, b, dist = board_rows(rows, cols, spacing)
    n_per = len(grid)
    pts = np.empty((n_frames, n_per, 3))
    for f in range(n_frames):
        R = rvec_to_matrix(rng.normal(0, 0.5, 3))
        pts[f] = grid @ R.T + [rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(0.35, 0.85)]
    pts = pts.reshape(-1, 3)
    cam_idx, uv = [], []
    for c, cam in sorted(cams.cameras.items()):
        K = cam.matrix
        p, z = project_pinhole_bc5(pts, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
        assert (z > 0).all()
        cam_idx.append(np.full(len(pts), c, dtype=np.int32)); uv.append(p + rng.normal(0, noise_px, p.shape))
    par = BundleParameterization.from_camera_array(cams, n_points=len(pts), refine_intrinsics=False)
    x = par.pack(cams, pts + rng.normal(0, 0.001, pts.shape))
    tabs = par.device_tables()
    cam_x = np.zeros((n_cams, 9))
    for i, (blk, off) in enumerate(zip(par.blocks, par.camera_param_offsets)):
        cam_x[i, : blk.n_params] = x[off: off + blk.n_params]
    base = (np.arange(n_frames, dtype=np.int32) * n_per)[:, None, None]
    f_median = float(np.median([cam.matrix[0, 0] for cam in cams.cameras.values()]))
    return (tabs["cam_model"], tabs["cam_n_params"], tabs["cam_const"], cam_x, x[par.n_camera_params:].reshape(-1, 3).copy(), np.concatenate(cam_idx),
            np.tile(np.arange(len(pts), dtype=np.int32), n_cams), np.vstack(uv), (a[None] + base).reshape(-1, 4), (b[None] + base).reshape(-1, 4),
            np.tile(dist, n_frames), np.full(n_frames * len(dist), (1.0 / f_median) / sigma_m))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rows", type=int, default=6)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()

    twelve = session(args.cameras, args.frames, args.rows, args.cols)
    dev = DeviceUncertainty(args.device)
    calls = {"constrained": lambda: dev.parameter_covariance_constrained(*twelve), "unconstrained": lambda: dev.parameter_covariance(*twelve[:8])}
    times, last = {name: [] for name in calls}, {}
    for round_ in range(args.warmup + args.runs):
        for name, call in calls.items():
            t0 = time.perf_counter()
            last[name] = call()
            if round_ >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    con, unc = last["constrained"], last["unconstrained"]
    std = lambda r: float(np.median(np.sqrt(np.trace(r.point_cov, axis1=1, axis2=2))) * 1e3)
    figures = {
        "what": "median wall time of one call (argument checks, host plan, upload, launches, copy-back) on one MI355X, the two calls alternating",
        "cameras": args.cameras, "frames": args.frames, "board": [args.rows, args.cols], "points": int(len(twelve[4])), "observations": int(len(twelve[5])),
        "constraint_rows": int(len(twelve[10])), "components": args.frames, "points_per_component": args.rows * args.cols, "runs": args.runs,
        "warmup": args.warmup,
        **{f"{name}_ms_median": float(np.median(t)) for name, t in times.items()}, **{f"{name}_ms": [round(v, 3) for v in t] for name, t in times.items()},
        "constrained_over_unconstrained": float(np.median(times["constrained"]) / np.median(times["unconstrained"])),
        "gauge_dim": [con.gauge_dim, unc.gauge_dim], "dof": [con.dof, unc.dof], "sigma0_px": [float(np.sqrt(r.sigma0_sq) * np.median(twelve[2][:, 0])) for r in (con, unc)],
        "point_std_median_mm": [std(con), std(unc)],
        "library_source_sha256": source_digest(),
    }
    print(json.dumps(figures, indent=1))
    if args.out is not None:
        args.out.write_text(json.dumps(figures, indent=1) + "\n")


if __name__ == "__main__":
    main()
