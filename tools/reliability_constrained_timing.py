"""Timing of the observation reliability with the rigid-distance rows of the boards, on one MI355X.

    python tools/reliability_constrained_timing.py [--cameras 8] [--frames 2000] [--rows 6] [--cols 9] [--runs 10] [--warmup 2]
                                                   [--out profiles/reliability_constrained.json]

The session of ``tools/constrained_uncertainty_timing.py`` (8 x 2 000 x 54: 108 000 points, 864 000 observations, 174 rows on 54
points per pose: one constraint component per pose, at the cap of the component kernel).

Timed, each as the median of ``--runs`` calls after ``--warmup`` calls, everything included (argument checks, the host plan, upload,
launches, copy-back), in rounds that alternate the two calls on the same arrays: ``cba_observation_reliability_constrained`` and
``cba_parameter_covariance_constrained``.  Both run the same launches up to ``C = St^-1``; the covariance call then forms a 3 x 3 block
per point, the reliability call a 2 x 2 block per observation and a number per constraint row.  There is no threshold: the ratio of the
two is the result.  ``--out`` writes the figures as JSON, with the covariance call's figure of the previous measurement
(``profiles/uncertainty_constrained.json``) beside them when that file is there."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from caliscope_amd.build import source_digest  # noqa: E402
from caliscope_amd.reliability import DeviceReliability  # noqa: E402
from caliscope_amd.uncertainty import DeviceUncertainty  # noqa: E402
from tools.constrained_uncertainty_timing import session  # noqa: E402


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
    rel, cov = DeviceReliability(args.device), DeviceUncertainty(args.device)
    calls = {"reliability": lambda: rel.observation_reliability_constrained(*twelve), "covariance": lambda: cov.parameter_covariance_constrained(*twelve)}
    times, last = {name: [] for name in calls}, {}
    for round_ in range(args.warmup + args.runs):
        for name, call in calls.items():
            t0 = time.perf_counter()
            last[name] = call()
            if round_ >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    res = last["reliability"]
    r = np.concatenate([res.redundancy[:, 0, 0], res.redundancy[:, 1, 1]])
    figures = {
        "what": "median wall time of one call (argument checks, host plan, upload, launches, copy-back) on one MI355X, the two calls alternating",
        "cameras": args.cameras, "frames": args.frames, "board": [args.rows, args.cols], "points": int(len(twelve[4])), "observations": int(len(twelve[5])),
        "constraint_rows": int(len(twelve[10])), "components": args.frames, "points_per_component": args.rows * args.cols, "runs": args.runs,
        "warmup": args.warmup,
        **{f"{name}_ms_median": float(np.median(t)) for name, t in times.items()}, **{f"{name}_ms": [round(v, 3) for v in t] for name, t in times.items()},
        "reliability_over_covariance": float(np.median(times["reliability"]) / np.median(times["covariance"])),
        "gauge_dim": res.gauge_dim, "dof": [res.dof, last["covariance"].dof], "sum_r_minus_dof": float(r.sum() + res.constraint_redundancy.sum() - res.dof),
        "redundancy_min_median": [float(r.min()), float(np.median(r))],
        "constraint_redundancy_min_median": [float(res.constraint_redundancy.min()), float(np.median(res.constraint_redundancy))],
        "n_uncontrolled": [res.n_uncontrolled, res.n_constraints_uncontrolled],
        "library_source_sha256": source_digest(),
    }
    before = ROOT / "profiles" / "uncertainty_constrained.json"
    if before.exists():
        old = json.loads(before.read_text())
        same = all(old.get(k) == figures[k] for k in ("cameras", "frames", "board"))
        if same and "constrained_ms_median" in old:
            figures["covariance_ms_median_previous_measurement"] = old["constrained_ms_median"]
            figures["previous_measurement_library_source_sha256"] = old.get("library_source_sha256")
            figures["reliability_over_previous_covariance"] = figures["reliability_ms_median"] / old["constrained_ms_median"]
    print(json.dumps(figures, indent=1))
    if args.out is not None:
        args.out.write_text(json.dumps(figures, indent=1) + "\n")


if __name__ == "__main__":
    main()
