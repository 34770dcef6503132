"""Timing of the intrinsic calibration of a whole rig (cba_pose_intrinsics_batch) on a seeded synthetic session at user scale:
every camera sees a 6 x 9 board in thousands of random views, ALL frames enter the solve.

    timeout -k 10 300 python tools/intrinsics_timing.py --part device [--cams 16] [--frames 3000] [--seed 7] [--device 0] [--repeat 5] \
      && timeout -k 10 600 python tools/intrinsics_timing.py --part cpu [--cams 16] [--frames 3000] [--seed 7] [--cpu-views 300]

Two parts, two processes: the device part is the only one that opens the GPU, it runs under a time limit of its own, and the CPU part
starts only if it ended well (`&&`).  Each prints one JSON line.  `device`: views and corners; the device call (host clock around the
synchronous call, uploads and downloads included: one warm-up, then `--repeat` runs, median / min / max).  `cpu`: the g++ build of
the same arithmetic on ONE CPU thread for the first `--cpu-views` views of every camera, scaled by views to the full session (an
extrapolation, labelled so: the work per iteration is linear in the views; the iteration counts are printed by both parts).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd.calibrate_intrinsics import DeviceIntrinsics  # noqa: E402  (binds nothing until the device part calls it)
from caliscope_amd.cameras import rvec_to_matrix  # noqa: E402
from caliscope_amd.synthetic import WEBCAM_DIST, WEBCAM_FOCAL, WEBCAM_SIZE, project_pinhole_bc5  # noqa: E402


def session(n_cams, n_frames, seed, rows=6, cols=9, spacing=0.04, noise_px=0.3):
    """CSR views of `n_cams` webcams (focal lengths spread by +-10 %), `n_frames` random board poses each."""
    rng = np.random.default_rng(seed)
    grid = np.array([[c * spacing, r * spacing, 0.0] for r in range(rows) for c in range(cols)])
    w, h = WEBCAM_SIZE
    sizes, cam, xy, obj, truth = [], [], [], [], []
    for c in range(n_cams):
        f = WEBCAM_FOCAL * (0.9 + 0.2 * c / max(n_cams - 1, 1))
        truth.append(f)
        done = 0
        while done < n_frames:
            R = rvec_to_matrix(rng.normal(0, 0.35, 3))
            depth = rng.uniform(0.5, 1.2)
            t = np.array([rng.uniform(-0.35, 0.35) * depth, rng.uniform(-0.2, 0.2) * depth, depth]) - R @ grid.mean(0)
            p, z = project_pinhole_bc5(grid, R, t, f, f, w / 2.0, h / 2.0, np.array(WEBCAM_DIST))
            ok = (z > 0.1) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)
            if ok.sum() < 12:
                continue
            sizes.append(int(ok.sum())); cam.append(c); obj.append(grid[ok])
            xy.append(p[ok] + rng.normal(0, noise_px, (int(ok.sum()), 2)))
            done += 1
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return (np.zeros(n_cams, np.int32), np.tile(np.array(WEBCAM_SIZE, float), (n_cams, 1)), start, np.array(cam, np.int32), np.concatenate(xy),
            np.concatenate(obj), np.array(truth))


def subset(args, per_cam):
    """The first `per_cam` views of every camera."""
    model, size, start, cam, xy, obj = args
    keep = np.concatenate([np.flatnonzero(cam == c)[:per_cam] for c in range(len(model))])
    rows = np.concatenate([np.arange(start[v], start[v + 1]) for v in keep])
    n = np.diff(start)[keep]
    return model, size, np.concatenate([[0], np.cumsum(n)]).astype(np.int64), cam[keep], xy[rows], obj[rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cpu-views", type=int, default=300)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--part", choices=("device", "cpu"), required=True)
    a = ap.parse_args()
    t0 = time.perf_counter()
    *args, truth = session(a.cams, a.frames, a.seed)
    t_gen = time.perf_counter() - t0
    model, size, start, cam, xy, obj = args
    out = {"part": a.part, "cams": a.cams, "frames": a.frames, "n_views": int(len(cam)), "n_corners": int(start[-1]), "generate_s": round(t_gen, 3)}
    if a.part == "device":
        dev = DeviceIntrinsics(a.device)
        call = lambda: dev.intrinsics_batch(model, size, None, start, cam, xy, obj, True, 0)  # noqa: E731
        intr, rmse, status, iters, _, _, vstat = call()  # warm-up (library load, first launch)
        ts = []
        for _ in range(a.repeat):
            t = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t)
        out.update({
            "n_views_used": int((vstat == 0).sum()), "device_call_s_median": float(np.median(ts)), "device_call_s_min": float(min(ts)),
            "device_call_s_max": float(max(ts)), "device_repeats": a.repeat, "status": status.tolist(), "iterations": iters.tolist(),
            "rmse_px_max": float(rmse.max()), "f_rel_error_max": float(np.abs(intr[:, 0] / truth - 1).max()),
        })
    else:
        from tests.intrinsic_native import HarnessIntrinsics

        sub = subset(args, a.cpu_views)
        h = HarnessIntrinsics()
        h.intrinsics_batch(sub[0], sub[1], None, *sub[2:], True, 0)  # (builds the harness)
        t = time.perf_counter()
        res = h.intrinsics_batch(sub[0], sub[1], None, *sub[2:], True, 0)
        t_cpu = time.perf_counter() - t
        out.update({"cpu_one_thread_s_subset": t_cpu, "cpu_subset_views": int(len(sub[3])), "cpu_iterations": res[3].tolist(),
                    "cpu_one_thread_s_extrapolated": t_cpu * len(cam) / len(sub[3]),
                    "cpu_note": "g++ -O2 build of csrc/intrinsic_math.h on one thread, timed on the subset and scaled by views"})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
