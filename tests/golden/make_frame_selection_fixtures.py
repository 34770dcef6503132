"""Choices of the REFERENCE's own frame selector on synthetic board sessions, stored as fixtures.

    python tests/golden/make_frame_selection_fixtures.py REFERENCE_SRC [--time]     (build container only: imports the reference's src/)

What is run is the reference's ``select_calibration_frames`` (core/frame_selector.py), unmodified: eligibility, grid cells, pose
features, binning, anchors, the greedy loop and the quality metrics.  The reference imports ``cv2``; it is not installed here, so a
stub module answers the one OpenCV call that is reached, ``cv2.findHomography``, with the least-squares homography of exactly the
float32 arrays the reference hands it: ``scipy.optimize.least_squares`` on the pixel transfer error (h33 = 1, tolerances 1e-15) from a
DLT start on centred and scaled points, finished by Gauss-Newton steps through a QR factorisation.  With no corner beyond cv2's 5 px
RANSAC gate that minimum is what cv2's own refinement converges to.  Nothing of the reference is copied: the fixtures hold the tables this script made and what the reference chose.

Per case ``frame_selection/sel_NN.npz`` stores the input table, the arguments, the nine fields of the report, and for every eligible
frame its covered cells, pose features and orientation features (the reference's ``_compute_*`` functions), plus

* ``orient_tol``: the yardstick's own uncertainty.  Every homography is solved a second time from a different start (the DLT on the
  raw, un-normalised points, iterated in those raw coordinates); per orientation feature the largest difference between the two
  solves over the case, angles on the circle.  The consumer's bound is ten times the largest of these over all cases.
* ``min_margin``: the smallest margin of every discrete decision of the case — top two tilt magnitudes per bin, top two scores per
  greedy round, distance of ``tilt_direction * 8 / 2 pi`` to the nearest integer, ``|tilt_magnitude - 0.1|``, ``|best score - 0.01|``.
  Each must be an exact tie of bit-identical frames or at least MARGIN_FLOOR = 1e-6, so that no choice hangs on a rounding
  difference; a case that violates it is re-seeded, never loosened.

Cases (1280 x 720 images): 00-03 a 70-frame, 24-corner-board camera at target_frame_count 30 (default), 1, 3 and 200; 04 300 frames
of 6-8 corners; 05 / 06 70 frames of which some have 3, 4 and 5 corners, with min_corners_per_frame 3 and the default; 07 every frame
twice under different sync_index; 08 frontal boards only; 09 / 10 grid_size 1 and 8 with corners outside the image; 11 a camera id
without rows; 12 a camera whose frames are all too small.  Consumer: tests/test_frame_selection.py, tests/test_frame_selection_gpu.py.
"""
import sys
import time
import types
from pathlib import Path

import numpy as np
import pandas as pd
from scipy.optimize import least_squares

HERE = Path(__file__).parent
OUT = HERE / "frame_selection"
SIZE = (1280, 720)
MARGIN_FLOOR = 1e-6
CAM = 3  # the camera id of the tables (case 11 asks for another one)

STATE = {"start": "normalised"}


# ---- the stand-in for cv2.findHomography ---------------------------------------------------------------------------------------------

def _dlt(src, dst, normalise):
    Ts, Td = (_similarity(src), _similarity(dst)) if normalise else (np.eye(3), np.eye(3))
    a = np.c_[src, np.ones(len(src))] @ Ts.T
    b = np.c_[dst, np.ones(len(dst))] @ Td.T
    rows = []
    for (x, y, _), (u, v, _) in zip(a, b):
        rows.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
        rows.append([0, 0, 0, x, y, 1, -v * x, -v * y, -v])
    h = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    H = np.linalg.inv(Td) @ h @ Ts
    return H / H[2, 2]


def _similarity(p):
    c = p.mean(0)
    s = np.mean(np.linalg.norm(p - c, axis=1))
    return np.array([[1 / s, 0, -c[0] / s], [0, 1 / s, -c[1] / s], [0, 0, 1]])


def _transfer(h8, src, dst, jac=False):
    H = np.append(h8, 1.0).reshape(3, 3)
    p = np.c_[src, np.ones(len(src))] @ H.T
    w = p[:, 2]
    q = p[:, :2] / w[:, None]
    if not jac:
        return (q - dst).ravel()
    J = np.zeros((len(src), 2, 8))
    x, y = src[:, 0] / w, src[:, 1] / w
    J[:, 0, 0], J[:, 0, 1], J[:, 0, 2], J[:, 0, 6], J[:, 0, 7] = x, y, 1 / w, -q[:, 0] * x, -q[:, 0] * y
    J[:, 1, 3], J[:, 1, 4], J[:, 1, 5], J[:, 1, 6], J[:, 1, 7] = x, y, 1 / w, -q[:, 1] * x, -q[:, 1] * y
    return J.reshape(-1, 8)


def find_homography(src, dst, method=None, threshold=None):
    """The minimum of the transfer error: scipy's Levenberg-Marquardt, then Gauss-Newton steps by QR (lstsq) until they stop
    shrinking.  STATE names the solve.  "normalised": DLT start on centred and scaled points, and the iteration runs in those
    coordinates (an isotropic scale of the pixels does not move the minimum).  "raw": DLT start on the points as they come, and the
    iteration runs on them as they come, pixels in the hundreds against board coordinates in [0, 1]: a second arithmetic, so that
    the difference between the two solves shows what rounding leaves of the minimum.  (Two solves that share the iteration's
    coordinates settle on the same floating-point fixed point whatever their start: they agreed to 6.8e-16 in the tilt magnitude
    while a 40-digit Newton solve of the same frames put that fixed point up to 1.2e-14 from the true minimum.)"""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 2)
    dst = np.asarray(dst, dtype=np.float64).reshape(-1, 2)
    normalised = STATE["start"] == "normalised"
    H0 = _dlt(src, dst, normalised)
    Ts, Td = (_similarity(src), _similarity(dst)) if normalised else (np.eye(3), np.eye(3))
    a = (np.c_[src, np.ones(len(src))] @ Ts.T)[:, :2]
    b = (np.c_[dst, np.ones(len(dst))] @ Td.T)[:, :2]
    G = Td @ H0 @ np.linalg.inv(Ts)
    h = (G / G[2, 2]).ravel()[:8]
    h = least_squares(_transfer, h, jac=lambda *k: _transfer(*k, jac=True), args=(a, b), method="lm", x_scale="jac", ftol=1e-15, xtol=1e-15,
                      gtol=1e-15, max_nfev=2000).x
    prev = np.inf
    for _ in range(20):
        d = np.linalg.lstsq(_transfer(h, a, b, jac=True), -_transfer(h, a, b), rcond=None)[0]
        if not np.abs(d).max() < 0.5 * prev:
            break
        h, prev = h + d, np.abs(d).max()
    H = np.linalg.inv(Td) @ np.append(h, 1.0).reshape(3, 3) @ Ts
    return H / H[2, 2], np.ones((len(src), 1), dtype=np.uint8)


def _stub_modules():
    cv2 = types.ModuleType("cv2")
    cv2.RANSAC = 8
    cv2.findHomography = find_homography
    sys.modules["cv2"] = cv2
    sys.modules.setdefault("rtoml", types.ModuleType("rtoml"))


# ---- tables ---------------------------------------------------------------------------------------------------------------------------

def _rodrigues(rv):
    th = np.linalg.norm(rv)
    if th < 1e-12:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def table(seed, n_frames, *, rows=4, cols=6, tilt=0.45, noise=0.3, keep=None, inside=True, depth=(0.5, 1.1), spread=(0.45, 0.3)):
    """One camera (f = 900 px, mild radial distortion) looking at random poses of a planar board.  ``keep(rng, n)``: how many corners of a
    frame survive detection; ``inside``: drop corners outside the image."""
    rng = np.random.default_rng(seed)
    w, h = SIZE
    grid = np.array([[c * 0.04, r * 0.04, 0.0] for r in range(rows) for c in range(cols)])
    out, f = [], 0
    while f < n_frames:
        rv = rng.normal(0, tilt, 3)
        R = _rodrigues(rv)
        z = rng.uniform(*depth)
        t = np.array([rng.uniform(-spread[0], spread[0]) * z, rng.uniform(-spread[1], spread[1]) * z, z]) - R @ grid.mean(0)
        X = grid @ R.T + t
        xn = X[:, :2] / X[:, 2:]
        r2 = (xn ** 2).sum(1, keepdims=True)
        uv = 900.0 * xn * (1 + 0.05 * r2) + np.array([w / 2 - 3.0, h / 2 + 5.0]) + rng.normal(0, noise, (len(X), 2))
        ok = X[:, 2] > 0.1
        if inside:
            ok &= (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
        idx = np.flatnonzero(ok)
        n_keep = len(idx) if keep is None else min(len(idx), keep(rng, len(idx)))
        if n_keep < 3:
            continue
        idx = np.sort(rng.choice(idx, n_keep, replace=False))
        for k in idx:
            out.append(dict(sync_index=f * 2 + 1, cam_id=CAM, object_id=0, keypoint_id=int(k), img_loc_x=uv[k, 0], img_loc_y=uv[k, 1],
                            obj_loc_x=grid[k, 0], obj_loc_y=grid[k, 1], obj_loc_z=0.0))
        f += 1
    return pd.DataFrame(out)


def twins(df):
    other = df.copy()
    other["sync_index"] = other["sync_index"] + 1000
    return pd.concat([df, other], ignore_index=True)


def cases(bump):
    """(name, table, cam_id, keyword arguments); ``bump[i]`` re-seeds table i."""
    s = lambda i: 100 * i + bump.get(i, 0)  # noqa: E731
    main = table(s(0), 70)
    small = table(s(2), 70, keep=lambda rng, n: int(rng.choice([3, 4, 5, 7, 12, n], p=[0.1, 0.1, 0.1, 0.2, 0.2, 0.3])))
    wide = dict(inside=False, depth=(0.25, 0.6), spread=(0.9, 0.7))
    return [
        ("default", main, CAM, {}, 0),
        ("target 1", main, CAM, dict(target_frame_count=1), 0),
        ("target 3", main, CAM, dict(target_frame_count=3), 0),
        ("target 200", main, CAM, dict(target_frame_count=200), 0),
        ("300 frames of 6-8 corners", table(s(1), 300, keep=lambda rng, n: int(rng.integers(6, 9))), CAM, {}, 1),
        ("3-5 corner frames eligible", small, CAM, dict(min_corners_per_frame=3), 2),
        ("3-5 corner frames ineligible", small, CAM, {}, 2),
        ("every frame twice", twins(table(s(3), 12)), CAM, {}, 3),
        ("frontal only", table(s(4), 40, tilt=0.004, noise=0.05), CAM, {}, 4),
        ("grid 1, corners outside", table(s(5), 30, **wide), CAM, dict(grid_size=1), 5),
        ("grid 8, corners outside", table(s(5), 30, **wide), CAM, dict(grid_size=8), 5),
        ("camera without rows", main, CAM + 1, {}, 0),
        ("no eligible frame", table(s(6), 9, keep=lambda rng, n: int(rng.integers(3, 6))), CAM, {}, 6),
    ]


# ---- one case ------------------------------------------------------------------------------------------------------------------------

def circ(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def run_case(fs, ImagePoints, df, cam_id, kw):
    grid = kw.get("grid_size", 5)
    STATE["start"] = "normalised"
    report = fs.select_calibration_frames(ImagePoints(df), cam_id, SIZE, **kw)
    cam_df = df[df["cam_id"] == cam_id]
    eligible = fs._filter_eligible_frames(cam_df, kw.get("min_corners_per_frame", 6)) if len(cam_df) else []
    data, alt, rows_of = {}, {}, {}
    for sync in eligible:
        frame_df = cam_df[cam_df["sync_index"] == sync]
        rows_of[sync] = frame_df[["img_loc_x", "img_loc_y", "obj_loc_x", "obj_loc_y"]].to_numpy().tobytes()
        STATE["start"] = "normalised"
        data[sync] = fs.FrameCoverageData(fs._compute_frame_coverage(frame_df, SIZE, grid), fs._compute_pose_features(frame_df, SIZE),
                                          fs._compute_orientation_features(frame_df))
        STATE["start"] = "raw"
        alt[sync] = fs._compute_orientation_features(frame_df)
    STATE["start"] = "normalised"
    twin = lambda a, b: rows_of[a] == rows_of[b]  # noqa: E731

    # margins of every discrete decision
    margins = []
    bins = {}
    for sync, d in data.items():
        o = d.orientation
        margins.append(abs(o.tilt_magnitude - fs.MIN_TILT_FOR_DIVERSITY))
        b = fs._get_orientation_bin(o)
        if b is not None:
            q = o.tilt_direction / (2 * np.pi) * 8
            margins.append(abs(q - round(q)))
            bins.setdefault(b, []).append((o.tilt_magnitude, sync))
    anchors = []
    for b in sorted(bins):
        ranked = sorted(bins[b], key=lambda x: (-x[0], x[1]))
        anchors.append(ranked[0][1])
        rivals = [m for m, s_ in ranked[1:] if not twin(s_, ranked[0][1])]
        if rivals:
            margins.append(ranked[0][0] - rivals[0])
    target = kw.get("target_frame_count", 30)
    selected = list(report.selected_frames)
    assert selected[:min(len(anchors), target)] == anchors[:target], "anchors are not the head of the selection"
    if len(anchors) < target:
        for k in range(len(anchors), len(selected) + 1):
            head = selected[:k]
            cov = set().union(*[data[s_].covered_cells for s_ in head]) if head else set()
            poses = [data[s_].pose_features for s_ in head]
            rest = sorted(set(data) - set(head))
            if not rest or k == target:
                break
            scores = sorted(((fs._score_frame(data[s_].covered_cells, cov, data[s_].pose_features, poses, grid), s_) for s_ in rest),
                            key=lambda x: (-x[0], x[1]))
            margins.append(abs(scores[0][0] - 0.01))
            if k < len(selected):
                assert scores[0][1] == selected[k]
                rivals = [v for v, s_ in scores[1:] if not twin(s_, scores[0][1])]
                if rivals:
                    margins.append(scores[0][0] - rivals[0])
    min_margin = float(min(margins)) if margins else np.inf

    syncs = np.array(sorted(data), dtype=np.int64)
    cells = np.zeros((len(syncs), grid, grid), dtype=bool)
    for i, s_ in enumerate(syncs):
        for r, c in data[s_].covered_cells:
            cells[i, r, c] = True
    orient = np.array([tuple(data[s_].orientation) for s_ in syncs], dtype=np.float64).reshape(-1, 3)
    orient2 = np.array([tuple(alt[s_]) for s_ in syncs], dtype=np.float64).reshape(-1, 3)
    tol = np.zeros(3)
    if len(syncs):
        tol = np.array([circ(orient[:, 0], orient2[:, 0]).max(), np.abs(orient[:, 1] - orient2[:, 1]).max(), circ(orient[:, 2], orient2[:, 2]).max()])
    fixture = dict(
        df_int=df[["sync_index", "cam_id", "object_id", "keypoint_id"]].to_numpy(np.int64),
        df_float=df[["img_loc_x", "img_loc_y", "obj_loc_x", "obj_loc_y", "obj_loc_z"]].to_numpy(np.float64),
        cam_id=np.int64(cam_id), image_size=np.array(SIZE, dtype=np.int64),
        target_frame_count=np.int64(target), min_corners_per_frame=np.int64(kw.get("min_corners_per_frame", 6)),
        min_orientations=np.int64(kw.get("min_orientations", 4)), grid_size=np.int64(grid),
        selected_frames=np.array(selected, dtype=np.int64),
        fractions=np.array([report.coverage_fraction, report.edge_coverage_fraction, report.corner_coverage_fraction, report.pose_diversity]),
        orientation_sufficient=np.bool_(report.orientation_sufficient), orientation_count=np.int64(report.orientation_count),
        eligible_frame_count=np.int64(report.eligible_frame_count), total_frame_count=np.int64(report.total_frame_count),
        frame_sync=syncs, frame_cells=cells, frame_pose=np.array([data[s_].pose_features for s_ in syncs], dtype=np.float64).reshape(-1, 5),
        frame_orientation=orient, orient_tol=tol, min_margin=np.float64(min_margin),
    )
    return fixture, report, min_margin


def main(reference_src, timing):
    sys.path.insert(0, reference_src)
    _stub_modules()
    from caliscope.core import frame_selector as fs
    from caliscope.core.point_data import ImagePoints

    OUT.mkdir(exist_ok=True)
    bump = {}
    for attempt in range(20):
        results, bad = [], set()
        for name, df, cam_id, kw, tab in cases(bump):
            fixture, report, margin = run_case(fs, ImagePoints, df, cam_id, kw)
            results.append((name, fixture, report, margin))
            if margin < MARGIN_FLOOR:
                bad.add(tab)
        if not bad:
            break
        for tab in bad:
            bump[tab] = bump.get(tab, 0) + 1
        print(f"attempt {attempt}: margin below {MARGIN_FLOOR} in tables {sorted(bad)}: re-seeded")
    else:
        raise SystemExit("no seed met the margin condition")
    for i, (name, fixture, report, margin) in enumerate(results):
        np.savez_compressed(OUT / f"sel_{i:02d}.npz", **fixture)
        print(f"sel_{i:02d} {name}: {len(report.selected_frames)} of {report.eligible_frame_count} eligible / {report.total_frame_count} frames, "
              f"{report.orientation_count} bins, coverage {report.coverage_fraction:.2f} edge {report.edge_coverage_fraction:.2f} corner "
              f"{report.corner_coverage_fraction:.2f}, min margin {margin:.3g}, orient tol {fixture['orient_tol']}")
    print("largest orientation difference between the two solves:", np.max([r[1]["orient_tol"] for r in results], axis=0))
    if timing:
        df = table(900, 200, rows=6, cols=9, keep=lambda rng, n: int(rng.integers(6, n + 1)))
        t0 = time.perf_counter()
        rep = fs.select_calibration_frames(ImagePoints(df), CAM, SIZE)
        print(f"reference selector with the stand-in homography, 200 frames / {len(df)} rows, one camera: {time.perf_counter() - t0:.2f} s "
              f"({len(rep.selected_frames)} frames selected)")


if __name__ == "__main__":
    main(sys.argv[1], "--time" in sys.argv[2:])
