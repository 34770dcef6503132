"""Timing of the frame selection of a whole rig (cba_pose_select_frames) on the seeded synthetic session of tools/intrinsics_timing.py:
every camera sees a 6 x 9 board in thousands of random views.

    timeout -k 10 300 python tools/frame_selection_timing.py --part device [--cams 16] [--frames 3000] [--seed 7] [--device 0] [--repeat 5] \
      && timeout -k 10 600 python tools/frame_selection_timing.py --part solve [--cams 16] [--frames 3000] [--seed 7] [--device 0] \
      && timeout -k 10 600 python tools/frame_selection_timing.py --part cpu [--cams 16] [--frames 3000] [--seed 7]

Three parts, three processes, each under a time limit of its own and started only if the one before ended well (`&&`); the CPU part
does not open the GPU.  Each prints one JSON line.  `device`: frames and corners; the selection call (host clock around the
synchronous call, uploads and downloads included: one warm-up, then `--repeat` runs, median / min / max).  `solve`: the intrinsic
solve (cba_pose_intrinsics_batch, after a warm-up on a small subset) from the selected frames, selection included, against the
solve from every frame, one run each.  `cpu`: the g++ build of the same selection arithmetic on ONE CPU thread, the whole session.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from intrinsics_timing import session, subset  # noqa: E402
from caliscope_amd.calibrate_intrinsics import DeviceIntrinsics  # noqa: E402  (binds nothing until a device part calls it)
from caliscope_amd.frame_selector import DeviceFrameSelection  # noqa: E402


def selection_arguments(start, cam, n_cams):
    """The session's views are frames already, camera after camera: cameras in CSR form over them."""
    return np.searchsorted(cam, np.arange(n_cams + 1)).astype(np.int64), start


def selected_views(sel, cam_frame_start):
    return np.concatenate([cam_frame_start[c] + np.sort(sel.selected[c, :sel.n_selected[c]]) for c in range(len(sel.n_selected))]).astype(np.int64)


def take(args, keep):
    model, size, start, cam, xy, obj = args
    rows = np.concatenate([np.arange(start[v], start[v + 1]) for v in keep])
    return model, size, np.concatenate([[0], np.cumsum(np.diff(start)[keep])]).astype(np.int64), cam[keep], xy[rows], obj[rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--part", choices=("device", "solve", "cpu"), required=True)
    a = ap.parse_args()
    t0 = time.perf_counter()
    *args, truth = session(a.cams, a.frames, a.seed)
    t_gen = time.perf_counter() - t0
    model, size, start, cam, xy, obj = args
    cam_frame_start, frame_start = selection_arguments(start, cam, a.cams)
    board = np.ascontiguousarray(obj[:, :2])
    out = {"part": a.part, "cams": a.cams, "frames": a.frames, "n_frames": int(len(cam)), "n_corners": int(start[-1]), "generate_s": round(t_gen, 3)}
    if a.part == "cpu":
        from tests.frame_select_native import HarnessFrameSelection

        h = HarnessFrameSelection()
        h.select_frames([0, 1], size[:1], frame_start[:2], xy[:frame_start[1]], board[:frame_start[1]])  # (builds the harness)
        t = time.perf_counter()
        sel = h.select_frames(cam_frame_start, size, frame_start, xy, board)
        out.update({"cpu_one_thread_s": time.perf_counter() - t, "selected": sel.n_selected.tolist(), "anchors": sel.n_anchors.tolist(),
                    "cpu_note": "g++ -O2 build of csrc/frame_select_math.h on one thread, the whole session"})
        print(json.dumps(out))
        return
    dev = DeviceFrameSelection(a.device)
    call = lambda: dev.select_frames(cam_frame_start, size, frame_start, xy, board)  # noqa: E731
    sel = call()  # warm-up (library load, first launch)
    if a.part == "device":
        ts = []
        for _ in range(a.repeat):
            t = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t)
        out.update({"device_call_s_median": float(np.median(ts)), "device_call_s_min": float(min(ts)), "device_call_s_max": float(max(ts)),
                    "device_repeats": a.repeat, "selected": sel.n_selected.tolist(), "anchors": sel.n_anchors.tolist(),
                    "homography_failed": int((sel.homography_status != 0).sum()), "transfer_rmse_px_median": float(np.median(sel.homography_rmse))})
    else:
        intr = DeviceIntrinsics(a.device)
        small = subset(args, 8)
        intr.intrinsics_batch(small[0], small[1], None, *small[2:], True, 0)  # warm-up
        t = time.perf_counter()
        picked = take(args, selected_views(call(), cam_frame_start))
        res_s = intr.intrinsics_batch(picked[0], picked[1], None, *picked[2:], True, 0)
        t_sel = time.perf_counter() - t
        t = time.perf_counter()
        res_a = intr.intrinsics_batch(model, size, None, start, cam, xy, obj, True, 0)
        t_all = time.perf_counter() - t
        out.update({"select_then_solve_s": t_sel, "solve_all_frames_s": t_all, "views_selected": int(len(picked[3])),
                    "iterations_selected": res_s[3].tolist(), "iterations_all": res_a[3].tolist(),
                    "f_rel_error_max_selected": float(np.abs(res_s[0][:, 0] / truth - 1).max()),
                    "f_rel_error_max_all": float(np.abs(res_a[0][:, 0] / truth - 1).max()),
                    "rmse_px_max_selected": float(res_s[1].max()), "rmse_px_max_all": float(res_a[1].max())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
