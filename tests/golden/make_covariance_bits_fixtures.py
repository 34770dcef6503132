"""Outputs of ``cba_parameter_covariance`` under ``CBA_DETERMINISTIC=1`` on two scenes of tests/test_uncertainty.py, stored bit for bit
(tests/golden/covariance_bits/*.npz).  Run once on a device with the library of the commit BEFORE the pipeline of the call was shared
with ``cba_observation_reliability``; tests/test_reliability_gpu.py requires the same bits from every later library.

    python tests/golden/make_covariance_bits_fixtures.py [output directory]
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

SMALL = ("small", 4, 30, 3, False, "linear", 0.0)


def main(out_dir):
    os.environ["CBA_DETERMINISTIC"] = "1"
    from caliscope_amd import uncertainty
    from tests import covariance_native as cn
    from tests.dense_solve_cases import widths

    scenes = {"small": SMALL, "mixed33": ("wide", widths(33), True)}
    out_dir.mkdir(parents=True, exist_ok=True)
    for name, key in scenes.items():
        sc = cn.key_scene(key)
        res = uncertainty.DeviceUncertainty().parameter_covariance(*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]))
        again = uncertainty.DeviceUncertainty().parameter_covariance(*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]))
        assert np.array_equal(res.cam_cov_full, again.cam_cov_full) and np.array_equal(res.point_cov, again.point_cov)
        np.savez(out_dir / f"{name}.npz", cam_cov=res.cam_cov, cam_cov_full=res.cam_cov_full, point_cov=res.point_cov,
                 sigma0_sq=np.float64(res.sigma0_sq), dof=np.int64(res.dof), cost=np.float64(res.cost))
        print(name, res.cam_cov_full.shape, res.point_cov.shape, res.sigma0_sq)


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).resolve().parent / "covariance_bits")
