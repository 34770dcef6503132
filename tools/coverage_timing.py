"""Timing of the camera-pair coverage analysis (cba_coverage_counts, caliscope_amd/coverage_analysis.py) on seeded observation tables
in the shapes of BASELINE.json's cfg3 (32 cameras / 50 000 points / 400 000 observations) and cfg5 (128 cameras / 1 000 000 points /
10 000 000 observations).

    timeout -k 10 600 python tools/coverage_timing.py [--shapes cfg3,cfg5] [--seed 7] [--device 0] [--repeat 5] [--out profiles/coverage_timing.json]

One process.  Per shape: the device call (host clock around the synchronous call, validation, uploads and the copy-back included:
one warm-up, then `--repeat` runs, median / min / max) and the end-to-end time of `analyze_multi_camera_coverage` on an ImagePoints
of the same rows (key index, camera index, device call, graph analysis; one run after the warm-up).  There is no pass / fail time.
For context only (the reference cannot run beside the device), the reference's own `compute_coverage_matrix` took 0.22 s on a CPU
for 8 cameras / 5 000 points / 40 000 observations and 2.05 s for the cfg3 shape; it is linear in observations times views per point.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from caliscope_amd import coverage_analysis as CA  # noqa: E402
from caliscope_amd.point_data import ImagePoints  # noqa: E402

SHAPES = {"cfg2": (8, 5_000, 40_000), "cfg3": (32, 50_000, 400_000), "cfg5": (128, 1_000_000, 10_000_000)}
KEYPOINTS_PER_FRAME = 20


def session_table(n_cams: int, n_points: int, n_obs: int, seed: int) -> np.ndarray:
    """[n_obs, 4] sync_index, cam_id, object_id, keypoint_id: every point is seen by n_obs / n_points cameras out of a window of
    neighbouring ones (a ring), rows shuffled."""
    rng = np.random.default_rng(seed)
    views = n_obs // n_points
    point = np.repeat(np.arange(n_points, dtype=np.int64), views)
    first = rng.integers(0, n_cams, n_points)
    window = min(n_cams, 2 * views)
    offset = np.argsort(rng.random((n_points, window)), axis=1)[:, :views]  # `views` different cameras of the window
    cam = ((first[:, None] + offset) % n_cams).reshape(-1)
    table = np.column_stack([point // KEYPOINTS_PER_FRAME, cam, np.zeros(len(point), dtype=np.int64), point % KEYPOINTS_PER_FRAME])
    return table[rng.permutation(len(table))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,cfg5")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "coverage_timing.json"))
    a = ap.parse_args()
    dev = CA.DeviceCoverageCounts(a.device)
    dev.coverage_counts(np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), 1, 1)  # warm-up (library load, first launch)
    results = []
    for name in a.shapes.split(","):
        n_cams, n_points, n_obs = SHAPES[name]
        table = session_table(n_cams, n_points, n_obs, a.seed)
        df = pd.DataFrame(table, columns=["sync_index", "cam_id", "object_id", "keypoint_id"])
        df["img_loc_x"] = 0.0
        df["img_loc_y"] = 0.0
        ip = ImagePoints(df)
        cols = ip.arrays()
        t = time.perf_counter()
        key, n_keys, path = CA.coverage_keys(cols["sync_index"], cols["object_id"], cols["keypoint_id"])
        t_keys = time.perf_counter() - t
        cam = cols["cam_id"].astype(np.int32)
        counts = dev.coverage_counts(key, cam, n_cams, n_keys)
        ts = []
        for _ in range(a.repeat):
            t = time.perf_counter()
            again = dev.coverage_counts(key, cam, n_cams, n_keys)
            ts.append(time.perf_counter() - t)
            assert again.tobytes() == counts.tobytes()
        t = time.perf_counter()
        report = CA.analyze_multi_camera_coverage(ip, device_id=a.device)
        t_all = time.perf_counter() - t
        assert np.array_equal(report.pairwise_observations, counts) and int(np.trace(counts)) == len(table)  # no row twice
        results.append({"shape": name, "cameras": n_cams, "points": n_points, "observations": int(len(table)), "n_keys": int(n_keys), "key_path": path,
                        "key_index_s": t_keys, "device_call_s_median": float(np.median(ts)), "device_call_s_min": float(min(ts)),
                        "device_call_s_max": float(max(ts)), "device_repeats": a.repeat, "end_to_end_s": t_all,
                        "linked_pairs": int((np.triu(counts, 1) > 0).sum()), "components": report.n_connected_components})
        print(json.dumps(results[-1]), flush=True)
    out = {"tool": "tools/coverage_timing.py", "seed": a.seed,
           "timed": "host clock around the synchronous call (validation, uploads, kernels, copy-back); end_to_end_s is analyze_multi_camera_coverage",
           "reference_cpu_context_s": {"8 cameras / 5 000 points / 40 000 observations": 0.22, "32 cameras / 50 000 points / 400 000 observations": 2.05},
           "results": results}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
