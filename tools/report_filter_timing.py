#!/usr/bin/env python
"""Wall time of the step between the solver passes at a bench configuration, both ways on the same solved volume in one process:
    python tools/report_filter_timing.py [cfg2|cfg3|cfg4] [--repeat 3] [--out profiles/report_filter_timing.txt]
host path: compute_reprojection_report() + filter_by_percentile_error(2.5) (device residuals through an evaluation-only handle, every
group-by, the per-camera percentiles and the keep mask on the host); new path: reprojection_summary() + filter_outliers(2.5)
(cba_reprojection_filter: sums, radix select, mask on the device).  The volume is built as tools/end_to_end.py builds it and solved
once; each path runs once as a warm-up, then `--repeat` times (median and minimum).  The two filtered volumes must hold the same
rows.  There is no pass / fail time."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from caliscope_amd.capture_volume import CaptureVolume  # noqa: E402
from caliscope_amd.synthetic import make_config  # noqa: E402

args = sys.argv[1:]
name = args[0] if args and not args[0].startswith("--") else "cfg4"
repeat = int(args[args.index("--repeat") + 1]) if "--repeat" in args else 3
out_path = args[args.index("--out") + 1] if "--out" in args else None

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    t = time.perf_counter()
    result = fn()
    return time.perf_counter() - t, result


sc = make_config(name)
cam_ids = np.array(sorted(sc.cameras_init.cameras))[sc.camera_indices]
vol = CaptureVolume.from_arrays(sc.cameras_init, cam_ids, sc.image_coords, sc.obj_indices, sc.points_init)
out = vol.optimize(loss=sc.loss, f_scale=vol.pixel_f_scale(1.0) if sc.loss != "linear" else 1.0, refine_intrinsics=sc.refine_intrinsics, strict=False)
say(f"{name}: {len(sc.cameras_init.cameras)} cameras, {len(sc.points_init)} points, {len(sc.camera_indices)} observations; solved "
    f"({out.optimization_status.termination_reason}, {out.optimization_status.iterations} evaluations)")


def host_path():
    out.__dict__.pop("reprojection_report", None)
    t_report, report = timed(out.compute_reprojection_report)
    out.__dict__["reprojection_report"] = report  # the slot filter_by_percentile_error reads
    t_filter, kept = timed(lambda: out.filter_by_percentile_error(2.5))
    return t_report, t_filter, report, kept


def device_path():
    t_summary, summary = timed(out.reprojection_summary)
    t_filter, kept = timed(lambda: out.filter_outliers(2.5))
    return t_summary, t_filter, summary, kept


host_path(), device_path()  # warm-up of both (library load, first launches, the volume's cached arrays)
host, dev = [], []
for _ in range(repeat):  # alternating: whatever else the machine does meets both
    host.append(host_path())
    dev.append(device_path())
report, host_kept = host[-1][2:]
summary, dev_kept = dev[-1][2:]
assert host_kept.image_points.df.equals(dev_kept.image_points.df) and np.array_equal(host_kept.img_to_obj_map, dev_kept.img_to_obj_map)
assert abs(summary.overall_rmse - report.overall_rmse) <= 1e-12 * report.overall_rmse


def ms(values):
    return f"median {1e3 * statistics.median(values):8.2f} ms, min {1e3 * min(values):8.2f} ms"


say(f"host path   compute_reprojection_report(): {ms([h[0] for h in host])}")
say(f"host path   filter_by_percentile_error(2.5): {ms([h[1] for h in host])}")
say(f"host path   both: {ms([h[0] + h[1] for h in host])}")
say(f"new path    reprojection_summary(): {ms([d[0] for d in dev])}")
say(f"new path    filter_outliers(2.5): {ms([d[1] for d in dev])}")
say(f"new path    both: {ms([d[0] + d[1] for d in dev])}")
# the library call alone (argument checks, uploads, kernels, copy-back), without the host work around it
t_call_stats = [timed(lambda: out._reprojection_call(None, groups=True, want_errors=False, mode="stats"))[0] for _ in range(repeat)]
t_call_filter = [timed(lambda: out._reprojection_call(None, groups=False, want_errors=False, mode="percentile", value=2.5, scope="per_camera",
                                                      min_per_camera=10))[0] for _ in range(repeat)]
say(f"new path    of which the device call of the summary (with the group index): {ms(t_call_stats)}")
say(f"new path    of which the device call of the filter: {ms(t_call_filter)}")
say(f"same {len(dev_kept.image_points)} of {len(out.image_points)} observations kept by both; overall RMSE {summary.overall_rmse:.6f} px ({repeat} timed runs each)")
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    with open(out_path, "a") as fh:
        fh.write("\n".join(lines) + "\n\n")
