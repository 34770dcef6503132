"""Timing of the per-observation reliability call (cba_observation_reliability, caliscope_amd/reliability.py) beside
cba_parameter_covariance of the same build, on the synthetic scenes of BASELINE.json's cfg2 (8 cameras / 5 000 points / 40 000
observations), cfg3 (32 / 50 000 / 400 000) and cfg4 (64 / 200 000 / 2 000 000), locked intrinsics, linear loss, at the scenes' initial
parameters.

    timeout -k 10 900 python tools/reliability_timing.py [--shapes cfg2,cfg3,cfg4] [--device 0] [--repeat 7] [--out profiles/reliability_timing.json]

One process.  Per shape: one warm-up of each call, then `--repeat` rounds in which the two calls alternate (so that a drift of the clocks
or of the machine meets both alike); host clock around each synchronous call (validation and the point sort on the host, uploads,
kernels, the 7 x 7 inverse on the host, copy-backs); median / min / max per call and the ratio of the medians.  The two calls share
everything up to C = St^-1; behind it the covariance call runs k_unc_point_cov and returns 6 doubles per point and the camera blocks,
the reliability call runs k_rel_point and returns 7 doubles per observation.  Figures of the result go with the times: the share of
rows with r < 0.01 and < 0.1, the mean r (dof / rows), the largest |w|.  There is no pass / fail time."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from caliscope_amd import reliability as R  # noqa: E402
from caliscope_amd import uncertainty as U  # noqa: E402
from caliscope_amd.bundle_parameterization import BundleParameterization  # noqa: E402
from caliscope_amd.synthetic import make_scene  # noqa: E402

SHAPES = {"cfg2": (8, 5_000, 40_000), "cfg3": (32, 50_000, 400_000), "cfg4": (64, 200_000, 2_000_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg2,cfg3,cfg4")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "reliability_timing.json"))
    a = ap.parse_args()
    cov, rel = U.DeviceUncertainty(a.device), R.DeviceReliability(a.device)
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
        cov.parameter_covariance(*args)  # warm-up (library load, first launches)
        first = rel.observation_reliability(*args)
        t_cov, t_rel = [], []
        for _ in range(a.repeat):
            t = time.perf_counter()
            cov.parameter_covariance(*args)
            t_cov.append(time.perf_counter() - t)
            t = time.perf_counter()
            res = rel.observation_reliability(*args)
            t_rel.append(time.perf_counter() - t)
        r = np.stack([res.redundancy[:, 0, 0], res.redundancy[:, 1, 1]], axis=1)
        assert np.allclose(res.redundancy, first.redundancy, rtol=0, atol=1e-8) and abs(r.sum() - res.dof) <= 1e-9 * res.dof
        views = np.bincount(sc.obj_indices, minlength=n_points)
        results.append({"shape": name, "cameras": n_cams, "points": n_points, "observations": n_obs, "camera_parameters": int(par.n_camera_params),
                        "views_per_point_mean": float(views.mean()), "views_per_point_max": int(views.max()),
                        "reliability_call_s_median": float(np.median(t_rel)), "reliability_call_s_min": float(min(t_rel)), "reliability_call_s_max": float(max(t_rel)),
                        "covariance_call_s_median": float(np.median(t_cov)), "covariance_call_s_min": float(min(t_cov)), "covariance_call_s_max": float(max(t_cov)),
                        "ratio_of_medians": float(np.median(t_rel) / np.median(t_cov)), "repeats": a.repeat, "dof": res.dof,
                        "mean_r": float(r.mean()), "min_r": float(r.min()), "share_r_below_0.01": float(np.mean(r < 0.01)), "share_r_below_0.1": float(np.mean(r < 0.1)),
                        "n_uncontrolled": res.n_uncontrolled, "max_abs_w": float(np.nanmax(np.abs(res.w)))})
        print(json.dumps(results[-1]), flush=True)
    out = {"tool": "tools/reliability_timing.py",
           "timed": "host clock around each synchronous call (validation, point sort, uploads, kernels, host 7 x 7 inverse, copy-backs); the two calls alternate",
           "scenes": "caliscope_amd.synthetic.make_scene at the BASELINE shapes, initial (perturbed) parameters, locked intrinsics, linear loss",
           "results": results}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
