"""Timing of the epipolar pose bootstrap (CaptureVolume.bootstrap(estimate_poses="auto") on a 2-D-only session) at user scale: a
seeded 33-keypoint moving 3-D constellation (tests/epipolar_scenes.py, "body") seen by a ring of cameras for thousands of frames.

    python tools/epipolar_bootstrap_timing.py [--cams 16] [--frames 3000] [--seed 3] [--device 0] [--cpu-pairs 4]

Prints one JSON line: pairs, correspondences; the essential device call alone (host clock around the synchronous call, uploads and
downloads included, best of 3 after a warm-up); one warm run of the builder with the wall time of each of its stages (the real
resection call over every (scaffold candidate, camera) job among them); the whole bootstrap; and a CPU
baseline — the g++ harness of the same arithmetic (tests/native/epipolar_harness.cpp), single-threaded, on the first
--cpu-pairs pairs, scaled to all pairs by correspondence count (an extrapolation, labelled so).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd import epipolar_pose as ep  # noqa: E402
from caliscope_amd.capture_volume import CaptureVolume  # noqa: E402
from caliscope_amd.pose_network import _intrinsic_tables  # noqa: E402
from tests.epipolar_scenes import constellation_session, unposed  # noqa: E402


def best_of(fn, n=3):
    fn()  # warm-up
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cpu-pairs", type=int, default=4)
    a = ap.parse_args()
    ip, cams, _ = constellation_session(n_cams=a.cams, n_frames=a.frames, kind="body", dropout=0.1, outliers=0.01, radius=3.5, seed=a.seed)
    cameras = unposed(cams)
    dev = ep.DeviceEpipolar(a.device)
    df = ip.df

    t0 = time.perf_counter()
    arr = lambda c: df[c].to_numpy(dtype=np.int64)  # noqa: E731
    pairs, start, ra, rb, _ = ep.pair_correspondences(arr("cam_id"), arr("sync_index"), arr("object_id"), arr("keypoint_id"))
    t_corr = time.perf_counter() - t0
    ids = sorted(cams.cameras)
    model, intr = _intrinsic_tables(cameras, ids)
    thr = np.array([ep.RANSAC_THRESHOLD_PX / (0.5 * (intr[ids.index(x), 0] + intr[ids.index(y), 0])) for x, y in pairs])
    xy = df[["img_loc_x", "img_loc_y"]].to_numpy()
    cam_idx = np.searchsorted(ids, arr("cam_id")).astype(np.int32)
    ess_args = (model, intr, xy, cam_idx, start, ra, rb, thr, ep.ESSENTIAL_HYPOTHESES, ep.DEFAULT_SEED)
    t_ess, ess = best_of(lambda: dev.essential_batch(*ess_args))

    # the builder itself, once warm: its report holds the real resection call (every candidate x camera job) and the host stages
    report = {}
    ep.build_epipolar_pose_network(ip, cameras, _epi=dev)
    t0 = time.perf_counter()
    ep.build_epipolar_pose_network(ip, cameras, report=report, _epi=dev)
    t_builder = time.perf_counter() - t0
    t_boot, vol = best_of(lambda: CaptureVolume.bootstrap(ip, cameras, estimate_poses="auto"), n=1)

    # CPU baseline: the g++ harness on the first --cpu-pairs pairs, scaled by correspondences
    from tests.epipolar_native import HarnessEpipolar

    k = min(a.cpu_pairs, len(pairs))
    sub = (model, intr, xy, cam_idx, start[: k + 1], ra[: start[k]], rb[: start[k]], thr[:k], ep.ESSENTIAL_HYPOTHESES, ep.DEFAULT_SEED)
    t1 = time.perf_counter()
    HarnessEpipolar().essential_batch(*sub)
    t_cpu = time.perf_counter() - t1
    n_corr = int(start[-1])
    print(json.dumps({
        "cams": a.cams, "frames": a.frames, "rows": int(len(df)), "pairs": len(pairs), "correspondences": n_corr,
        "mean_correspondences_per_pair": n_corr / max(len(pairs), 1), "essential_hypotheses": ep.ESSENTIAL_HYPOTHESES,
        "essential_batch_s": t_ess, "pooled_correspondences_host_s": t_corr,
        "builder_s": t_builder, "builder_stages": {k: v for k, v in report.items() if k.endswith("_s")},
        "resection_jobs": report["resection_jobs"], "resection_points": report["resection_points"],
        "bootstrap_total_s": t_boot, "posed_cameras": len(vol.camera_array.posed_cameras),
        "cpu_harness_single_thread_pairs": k, "cpu_harness_single_thread_s": t_cpu,
        "cpu_harness_single_thread_extrapolated_all_pairs_s": t_cpu * n_corr / max(int(start[k]), 1),
        "cpu_baseline_note": "g++ -O2 build of the same arithmetic, one thread, measured on the first pairs and scaled by correspondences",
    }))


if __name__ == "__main__":
    main()
