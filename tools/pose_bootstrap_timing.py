"""Timing of the pose bootstrap (CaptureVolume.bootstrap(estimate_poses=True)) on a seeded synthetic board session at user
scale: ring cameras around a 6 x 9 board that moves through the volume for thousands of frames.

    python tools/pose_bootstrap_timing.py [--cams 16] [--frames 3000] [--seed 7] [--device 0]

Prints one JSON line: views, pairs, observations; the PnP and pair-RMSE device calls (host clock around the synchronous call,
uploads and downloads included, best of 3 after a warm-up); the host stages of the builder; the whole bootstrap; and a CPU
baseline — scipy least_squares per view on a 1 000-view sample, scaled to all views (an extrapolation, labelled so).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from caliscope_amd.cameras import CameraArray, CameraData, rvec_to_matrix  # noqa: E402
from caliscope_amd.capture_volume import CaptureVolume  # noqa: E402
from caliscope_amd.point_data import ImagePoints  # noqa: E402
from caliscope_amd import pose_network as pn  # noqa: E402
from caliscope_amd.synthetic import WEBCAM_SIZE, project_pinhole_bc5, ring_camera_array  # noqa: E402


def session(n_cams, n_frames, seed, rows=6, cols=9, spacing=0.04, noise_px=0.5):
    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams, radius=2.0, target=(0.0, 0.0, 0.5))
    grid = np.array([[c * spacing, r * spacing, 0.0] for r in range(rows) for c in range(cols)])
    off = grid.mean(axis=0)
    w, h = WEBCAM_SIZE
    cols_out = {k: [] for k in ("sync_index", "cam_id", "keypoint_id", "img_loc_x", "img_loc_y")}
    kp = np.arange(len(grid))
    for f in range(n_frames):
        s = f / max(n_frames - 1, 1)
        R = rvec_to_matrix(np.array([0.0, 0.0, 40 * np.pi * s])) @ rvec_to_matrix(np.array([np.pi / 2 + 0.3 * np.sin(50 * s), 0.0, 0.0]))
        X = (grid - off) @ R.T + np.array([0.3 * np.cos(30 * s), 0.3 * np.sin(20 * s), 0.5 + 0.1 * np.sin(40 * s)])
        for c, cam in cams.cameras.items():
            if float(R[:, 2] @ (-cam.rotation.T @ cam.translation - X.mean(0))) < 0.3:  # the front face only
                continue
            K = cam.matrix
            p, z = project_pinhole_bc5(X, cam.rotation, cam.translation, K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.distortions)
            ok = (z > 0.1) & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)
            if ok.sum() < 4:
                continue
            p = p[ok] + rng.normal(0, noise_px, (int(ok.sum()), 2))
            cols_out["sync_index"].append(np.full(len(p), f))
            cols_out["cam_id"].append(np.full(len(p), c))
            cols_out["keypoint_id"].append(kp[ok])
            cols_out["img_loc_x"].append(p[:, 0])
            cols_out["img_loc_y"].append(p[:, 1])
    df = pd.DataFrame({k: np.concatenate(v) for k, v in cols_out.items()})
    df.insert(2, "object_id", 0)
    df["obj_loc_x"], df["obj_loc_y"], df["obj_loc_z"] = grid[df["keypoint_id"], 0], grid[df["keypoint_id"], 1], 0.0
    unposed = CameraArray({c: CameraData(cam_id=c, size=cam.size, matrix=cam.matrix.copy(), distortions=cam.distortions.copy())
                           for c, cam in cams.cameras.items()})
    return ImagePoints(df), unposed


def best_of(fn, n=3):
    fn()  # warm-up (module load, first launch)
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cpu-sample", type=int, default=1000)
    a = ap.parse_args()
    t0 = time.perf_counter()
    ip, cams = session(a.cams, a.frames, a.seed)
    t_gen = time.perf_counter() - t0
    dev = pn.DevicePnP(a.device)

    # the builder's stages, one after another
    b = pn.PoseNetworkBuilder(cams, ip, _pnp=dev)
    st = {}
    t = time.perf_counter(); b.estimate_camera_to_object_poses(); st["pnp_stage_s"] = time.perf_counter() - t
    t = time.perf_counter(); b.estimate_relative_poses(); st["relative_poses_s"] = time.perf_counter() - t
    t = time.perf_counter(); b.filter_outliers(); st["outlier_rejection_s"] = time.perf_counter() - t
    t = time.perf_counter(); agg = pn.aggregate_poses(b._relative_poses, b._filtered_poses); st["aggregation_s"] = time.perf_counter() - t
    t = time.perf_counter(); common = pn.common_observations(ip, cams, b._undistorted); st["common_observations_s"] = time.perf_counter() - t
    t = time.perf_counter(); net = pn.estimate_pnp_paired_pose_network(agg, common, _pnp=dev); st["pair_rmse_and_graph_s"] = time.perf_counter() - t
    t = time.perf_counter(); net.apply_to(CameraArray(dict(cams.cameras))); st["apply_to_s"] = time.perf_counter() - t

    # the two device calls on their own
    df = ip.df
    cam, sync, obj = df["cam_id"].to_numpy(), df["sync_index"].to_numpy(), df["object_id"].to_numpy()
    order = np.lexsort((obj, sync, cam))
    starts = pn._group_starts(cam[order], sync[order], obj[order])
    ids = sorted(cams.cameras)
    model, intr = pn._intrinsic_tables(cams, ids)
    xy = df[["img_loc_x", "img_loc_y"]].to_numpy()[order]
    xyz = df[["obj_loc_x", "obj_loc_y", "obj_loc_z"]].to_numpy()[order]
    view_cam = np.searchsorted(ids, cam[order][starts[:-1]]).astype(np.int32)
    pnp_args = (starts, view_cam, model, intr, xy, xyz, 4, True)
    t_pnp = best_of(lambda: dev.pnp_batch(*pnp_args))
    pose, _, status, und = dev.pnp_batch(*pnp_args)
    pairs = [p for p in agg if p in common]
    if not pairs:
        raise SystemExit("no camera pair shares a board view: nothing to time")
    pp = np.stack([np.concatenate([agg[p].rotation.ravel(), agg[p].translation]) for p in pairs])
    ps = np.concatenate([[0], np.cumsum([len(common[p][0]) for p in pairs])]).astype(np.int64)
    oa, ob = np.concatenate([common[p][0] for p in pairs]), np.concatenate([common[p][1] for p in pairs])
    t_pair = best_of(lambda: dev.pair_rmse(pp, ps, oa, ob))

    t_boot = best_of(lambda: CaptureVolume.bootstrap(ip, cams, estimate_poses=True), n=1)

    # CPU baseline: scipy per view on a sample, scaled
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(0)
    ok = np.flatnonzero(status == 0)
    sample = rng.choice(ok, size=min(a.cpu_sample, len(ok)), replace=False)
    t = time.perf_counter()
    for v in sample:
        P, u = xyz[starts[v]:starts[v + 1]], und[starts[v]:starts[v + 1]]
        R0 = pose[v, :9].reshape(3, 3) @ rvec_to_matrix(np.full(3, 0.02))
        x0 = np.concatenate([Rotation.from_matrix(R0).as_rotvec(), pose[v, 9:] + 0.01])

        def res(x, P=P, u=u):
            Xc = P @ Rotation.from_rotvec(x[:3]).as_matrix().T + x[3:]
            return (Xc[:, :2] / Xc[:, 2:] - u).ravel()

        least_squares(res, x0, method="lm")
    t_cpu = time.perf_counter() - t
    n_views = len(starts) - 1
    print(json.dumps({
        "cams": a.cams, "frames": a.frames, "n_observations": int(len(df)), "n_views": int(n_views), "n_views_ok": int(len(ok)),
        "n_pairs": len(pairs), "generate_s": round(t_gen, 3),
        "pnp_call_s": t_pnp, "pair_rmse_call_s": t_pair, "stages": st, "bootstrap_total_s": t_boot,
        "cpu_scipy_per_view_extrapolated_s": t_cpu / len(sample) * n_views, "cpu_scipy_sample_views": int(len(sample)),
        "cpu_note": "scipy least_squares (lm) per view from a perturbed start, timed on the sample and scaled to all views",
    }))


if __name__ == "__main__":
    main()
