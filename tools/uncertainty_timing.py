"""Timing of the free-network parameter covariance (cba_parameter_covariance, caliscope_amd/uncertainty.py) on the synthetic scenes of
BASELINE.json's cfg2 (8 cameras / 5 000 points / 40 000 observations), cfg3 (32 / 50 000 / 400 000) and cfg4 (64 / 200 000 / 2 000 000),
locked intrinsics, linear loss, at the scenes' initial parameters.

    timeout -k 10 900 python tools/uncertainty_timing.py [--shapes cfg2,cfg3,cfg4] [--device 0] [--repeat 3] [--out profiles/uncertainty_timing.json]

One process.  Per shape: the device call (host clock around the synchronous call: validation and the point sort on the host, uploads,
kernels, the 7 x 7 inverse and the rank-7 terms on the host, copy-backs; one warm-up, then `--repeat` runs, median / min / max), and
figures of the result (sigma0 in pixels, the median and the largest camera-centre and point standard deviation).  There is no pass /
fail time and nothing to compare with: the reference computes no covariance, and the only CPU route, a dense pseudo-inverse of J^T J,
needs n_params^2 doubles (cfg2: 1.8 GB, cfg4: 2.9 TB)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from caliscope_amd import uncertainty as U  # noqa: E402
from caliscope_amd.bundle_parameterization import BundleParameterization  # noqa: E402
from caliscope_amd.synthetic import make_scene  # noqa: E402

SHAPES = {"cfg2": (8, 5_000, 40_000), "cfg3": (32, 50_000, 400_000), "cfg4": (64, 200_000, 2_000_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg2,cfg3,cfg4")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "uncertainty_timing.json"))
    a = ap.parse_args()
    dev = U.DeviceUncertainty(a.device)
    results = []
    for name in a.shapes.split(","):
        n_cams, n_points, n_obs = SHAPES[name]
        sc = make_scene(name, n_cams=n_cams, n_points=n_points, n_obs=n_obs)
        par = BundleParameterization.from_camera_array(sc.cameras_init, n_points=n_points, refine_intrinsics=False)
        tabs = par.device_tables()
        x = par.pack(sc.cameras_init, sc.points_init)
        cam_x = np.zeros((n_cams, 9))
        cam_x[:, :6] = x[: par.n_camera_params].reshape(-1, 6)
        args = (tabs["cam_model"], tabs["cam_n_params"], tabs["cam_const"], cam_x, sc.points_init, sc.camera_indices, sc.obj_indices, sc.image_coords)
        first = dev.parameter_covariance(*args)  # warm-up (library load, first launches)
        ts = []
        for _ in range(a.repeat):
            t = time.perf_counter()
            res = dev.parameter_covariance(*args)
            ts.append(time.perf_counter() - t)
        assert np.allclose(res.cam_cov_full, first.cam_cov_full, rtol=0, atol=1e-8 * np.abs(first.cam_cov_full).max())
        rep = U.build_report(res, [b.cam_id for b in par.blocks], tabs["cam_n_params"], cam_x)
        centre = np.array([c.position_std for c in rep.cameras.values()])
        point = np.sqrt(np.einsum("ijj->i", rep.point_cov))
        fx = float(np.median(tabs["cam_const"][:, 0]))
        results.append({"shape": name, "cameras": n_cams, "points": n_points, "observations": n_obs, "camera_parameters": int(par.n_camera_params),
                        "device_call_s_median": float(np.median(ts)), "device_call_s_min": float(min(ts)), "device_call_s_max": float(max(ts)),
                        "device_repeats": a.repeat, "dof": rep.dof, "sigma0_px": rep.sigma0 * fx,
                        "centre_std_median": float(np.median(centre)), "centre_std_max": float(centre.max()),
                        "rotation_std_deg_max": float(max(c.rotation_std_deg for c in rep.cameras.values())),
                        "point_std_median": float(np.median(point)), "point_std_max": float(point.max())})
        print(json.dumps(results[-1]), flush=True)
    out = {"tool": "tools/uncertainty_timing.py",
           "timed": "host clock around the synchronous call (validation, point sort, uploads, kernels, host 7 x 7 inverse and rank-7 terms, copy-backs)",
           "scenes": "caliscope_amd.synthetic.make_scene at the BASELINE shapes, initial (perturbed) parameters, locked intrinsics, linear loss",
           "results": results}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
