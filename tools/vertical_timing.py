"""Timing of the batched gravity fit (cba_vertical_fit, caliscope_amd/vertical.py) at the field network's usual 16:9 output size of
320 x 544: 1, 8 and 64 cameras x 12 frames in one device call.

    timeout -k 10 900 python tools/vertical_timing.py [--cameras 1,8,64] [--frames 12] [--seed 7] [--device 0] [--repeat 5] [--out profiles/vertical_timing.json]

One process.  Twelve seeded noisy frames (random orientation, rotated up vectors, latitude noise with 5 % outliers, random
confidences, float32) are made once and repeated over the cameras.  Per workload: the device call (host clock around the synchronous
call: validation, uploads, the sine prologue, num_steps + 1 partial / update pairs, copy-back; one warm-up run of the same shape, then
`--repeat` runs, median / min / max, every run compared bit for bit with the warm-up) and the end-to-end time of `fit_gravity_batch`
(packing the planes included).  There is no pass / fail time.  For context only (the reference cannot run beside the device): the
reference's own `fit_gravity` took REFERENCE_FIT_S per fit of this size on one core of the CPU-only build machine.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from caliscope_amd import vertical as V  # noqa: E402

HEIGHT, WIDTH = 320, 544
REFERENCE_FIT_S = 2.0  # the reference's fit_gravity on one 320 x 544 field set, CPU-only build machine (1.9 - 2.2 s over repeated runs)


def frame(seed: int):
    """One float32 field set of a random near-upright orientation, and its focal lengths."""
    rng = np.random.default_rng(seed)
    roll, pitch = rng.uniform(-0.3, 0.3, 2)
    fx = fy = 280.0
    vec = V.gravity_vec_from_roll_pitch(roll, pitch)
    xs, ys = np.meshgrid(np.arange(WIDTH, dtype=np.float64), np.arange(HEIGHT, dtype=np.float64))
    u, v = (xs - WIDTH / 2) / fx, (ys - HEIGHT / 2) / fy
    up = np.stack([vec[0] - vec[2] * u, vec[1] - vec[2] * v])
    up /= np.linalg.norm(up, axis=0, keepdims=True)
    rays = np.stack([u, v, np.ones_like(u)])
    rays /= np.linalg.norm(rays, axis=0, keepdims=True)
    lat = np.arcsin(np.clip(np.tensordot(vec, rays, axes=1), -1 + 1e-6, 1 - 1e-6))
    ang = rng.normal(0.0, 0.02, lat.shape)
    up = np.stack([np.cos(ang) * up[0] - np.sin(ang) * up[1], np.sin(ang) * up[0] + np.cos(ang) * up[1]])
    lat = lat + rng.normal(0.0, 0.02, lat.shape) + np.where(rng.random(lat.shape) < 0.05, rng.normal(0.0, 0.5, lat.shape), 0.0)
    return tuple(a.astype(np.float32) for a in (up, rng.random(lat.shape), lat[None], rng.random(lat.shape))) + (fx, fy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", default="1,8,64")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vertical_timing.json"))
    a = ap.parse_args()
    dev = V.DeviceVerticalFit(a.device)
    frames = [frame(a.seed + k) for k in range(a.frames)]
    V.fit_gravity_batch(frames[:1], device_id=a.device)  # warm-up (library load, first launch)
    results = []
    for n_cams in (int(c) for c in a.cameras.split(",")):
        sets = frames * n_cams
        n = len(sets)
        planes = [np.tile(np.concatenate([pick(f).reshape(-1) for f in frames]), n_cams)
                  for pick in (lambda f: f[0][0], lambda f: f[0][1], lambda f: f[1], lambda f: f[2], lambda f: f[3])]
        shape = dict(height=[HEIGHT] * n, width=[WIDTH] * n, focal_x=[f[4] for f in sets], focal_y=[f[5] for f in sets],
                     offset=np.arange(n, dtype=np.int64) * (HEIGHT * WIDTH))
        fits, stop, status = dev.vertical_fit(planes, **shape)  # warm-up of this shape
        assert (status == 0).all()
        ts = []
        for _ in range(a.repeat):
            t = time.perf_counter()
            again = dev.vertical_fit(planes, **shape)
            ts.append(time.perf_counter() - t)
            assert again[0].tobytes() == fits.tobytes() and again[1].tobytes() == stop.tobytes()
        del planes
        t = time.perf_counter()
        public = V.fit_gravity_batch(sets, device_id=a.device)
        t_all = time.perf_counter() - t
        assert [f.stop_step for f in public] == stop.tolist() and public[0].roll_rad == fits[0, 0]
        results.append({"cameras": n_cams, "frames_per_camera": a.frames, "fits": n, "height": HEIGHT, "width": WIDTH, "dtype": "float32",
                        "device_call_s_median": float(np.median(ts)), "device_call_s_min": float(min(ts)), "device_call_s_max": float(max(ts)),
                        "device_repeats": a.repeat, "fit_gravity_batch_s": t_all, "stop_step_min": int(stop.min()), "stop_step_max": int(stop.max()),
                        "reference_cpu_context_s": REFERENCE_FIT_S * n})
        print(json.dumps(results[-1]), flush=True)
    out = {"tool": "tools/vertical_timing.py", "seed": a.seed,
           "timed": "host clock around the synchronous call (validation, uploads, kernels, copy-back); fit_gravity_batch_s adds the packing of the planes",
           "reference_fit_gravity_s_per_fit": REFERENCE_FIT_S, "results": results}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
