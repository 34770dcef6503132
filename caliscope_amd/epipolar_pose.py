"""Initial camera poses of a 2-D-only session (no object geometry: body keypoints, tracker output) from essential-matrix RANSAC
and resection on the MI355X.

Host-side mirror of the reference's ``core/bootstrap_pose/epipolar_pose_builder.py`` with the same names and constants.  Each
camera pair's matches, pooled over every shared frame, give an essential matrix (metric only up to the pair's baseline);
one pair, the scaffold, is triangulated into a cloud in its first camera's frame, and every other camera is resected
against that cloud.  The scaffold is the candidate whose cloud the third views fit best: score ``(n_failures, worst median
reprojection error, -cheirality inliers)``, lexicographic minimum, the first candidate on ties.

Where the stages run:

  pooled correspondences of every pair          numpy, one sort of all rows on (sync_index, object_id, keypoint_id)
  undistortion, essential RANSAC of all pairs   device, ``cba_pose_essential_batch`` (one call for every pair with >= 8)
  scaffold clouds, matching cameras to them     numpy, ``searchsorted`` on the group index of (sync_index, object_id, keypoint_id)
  resection of every (candidate, camera) job    device, ``cba_pose_resect_batch`` (one call for every job with >= 50 points)
  scores, winner, anchor-relative StereoPairs   host; then ``estimate_pnp_paired_pose_network`` (stereo RMSE on the device)

The arithmetic (``csrc/epipolar_math.h``) is a linear 8-point fit per hypothesis (not Nister's five-point solver: it needs
more hypotheses at low inlier ratios and is degenerate for coplanar points, as are 2-D-only sessions of a flat target),
Sampson scoring with cv2's rule, recoverPose's cheirality test, and Levenberg-Marquardt on the inliers; the answer is
judged against ground truth, not against cv2's bits or sample sequence.

There is no CPU fallback: without the library or a GPU the device stages raise ``BackendError``.  ``_epi`` replaces the
device calls (an object with ``essential_batch``, ``resect_batch`` and ``pair_rmse``, as :class:`DeviceEpipolar`) — the CPU
test-suite passes a g++ build of the same arithmetic.
"""

from __future__ import annotations

import ctypes as C
import logging
import time
from types import SimpleNamespace

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.exceptions import CalibrationError
from caliscope_amd.pose_network import (
    DevicePnP, PairedPoseNetwork, StereoPair, _group_starts, _intrinsic_tables, _pairs_within_groups, common_observations,
    estimate_pnp_paired_pose_network,
)

logger = logging.getLogger(__name__)

RANSAC_THRESHOLD_PX = 3.0  # essential-matrix inlier gate, pixels (converted to normalised units per camera)
RANSAC_PROB = 0.999  # (the reference's findEssentialMat confidence; the hypothesis count below is fixed instead)
MIN_RESECTION_POINTS = 50  # cloud points a camera must share to be resectioned
MIN_CORRESPONDENCES = 8  # an essential matrix needs 8 point correspondences
CONDITIONING_FLOOR = 0.5  # E singular-value ratio below this flags a near-degenerate (coplanar) pair
MAX_SCAFFOLD_CANDIDATES = 12  # cap third-view validation cost on large rigs
ESSENTIAL_HYPOTHESES = 1024  # 8-point samples per pair: a clean sample with p ~ 0.98 at an inlier ratio of 0.5
RESECTION_HYPOTHESES = 200  # the reference's solvePnPRansac iterationsCount
DEFAULT_SEED = 0
EPI_OK = 0


# ------------------------------------------------------------------------------------------------------------------------------
# C ABI of include/caliscope_pose.h

class EssentialDesc(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("cam_model", _lib.c_int32_p), ("cam_intr", _lib.c_double_p), ("n_obs", C.c_int64), ("obs_xy", _lib.c_double_p),
        ("obs_cam", _lib.c_int32_p), ("n_pairs", C.c_int64), ("pair_start", _lib.c_int64_p), ("corr_a", _lib.c_int64_p),
        ("corr_b", _lib.c_int64_p), ("threshold", _lib.c_double_p), ("n_hyp", C.c_int32), ("seed", C.c_uint64), ("float32_io", C.c_int32),
    ]


class ResectDesc(C.Structure):
    _fields_ = [
        ("n_jobs", C.c_int64), ("job_start", _lib.c_int64_p), ("obj", _lib.c_double_p), ("uv", _lib.c_double_p), ("threshold", _lib.c_double_p),
        ("n_hyp", C.c_int32), ("min_points", C.c_int32), ("seed", C.c_uint64),
    ]


EPI_SIGNATURES = {
    "cba_pose_essential_batch": (C.c_int, [C.POINTER(EssentialDesc), C.c_int32, _lib.c_double_p, _lib.c_int32_p, _lib.c_int64_p, _lib.c_int64_p,
                                           _lib.c_double_p, _lib.c_int32_p, _lib.c_uint8_p, _lib.c_double_p, _lib.c_double_p]),
    "cba_pose_resect_batch": (C.c_int, [C.POINTER(ResectDesc), C.c_int32, _lib.c_double_p, _lib.c_int32_p, _lib.c_int64_p, _lib.c_int32_p,
                                        _lib.c_double_p]),
}


class DeviceEpipolar:
    """The device calls of the epipolar bootstrap (``cba_pose_essential_batch``, ``cba_pose_resect_batch`` and the PnP path's
    ``cba_pose_pair_rmse``) on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def essential_batch(self, cam_model, cam_intr, obs_xy, obs_cam, pair_start, corr_a, corr_b, threshold, n_hyp, seed, float32_io=False):
        """Returns a dict: pose[n_pairs, 12], status, n_inliers, n_cheiral, conditioning, winner, flag[n_corr], xyz[n_corr, 3],
        undistorted[n_obs, 2]."""
        lib = _lib.bind(_lib.load(), EPI_SIGNATURES)
        cam_model = np.ascontiguousarray(cam_model, dtype=np.int32)
        cam_intr = np.ascontiguousarray(cam_intr, dtype=np.float64)
        obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
        obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32)
        pair_start = np.ascontiguousarray(pair_start, dtype=np.int64)
        corr_a = np.ascontiguousarray(corr_a, dtype=np.int64)
        corr_b = np.ascontiguousarray(corr_b, dtype=np.int64)
        threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        n_pairs, n_corr = len(pair_start) - 1, int(pair_start[-1])
        pose, status = np.zeros((n_pairs, 12)), np.zeros(n_pairs, dtype=np.int32)
        n_inl, n_chr = np.zeros(n_pairs, dtype=np.int64), np.zeros(n_pairs, dtype=np.int64)
        cond, winner = np.zeros(n_pairs), np.zeros(n_pairs, dtype=np.int32)
        flag, xyz, und = np.zeros(n_corr, dtype=np.uint8), np.zeros((n_corr, 3)), np.zeros_like(obs_xy)
        desc = EssentialDesc(n_cams=len(cam_model), cam_model=_lib.ptr(cam_model), cam_intr=_lib.ptr(cam_intr), n_obs=len(obs_xy),
                             obs_xy=_lib.ptr(obs_xy), obs_cam=_lib.ptr(obs_cam), n_pairs=n_pairs, pair_start=_lib.ptr(pair_start),
                             corr_a=_lib.ptr(corr_a), corr_b=_lib.ptr(corr_b), threshold=_lib.ptr(threshold), n_hyp=int(n_hyp),
                             seed=int(seed), float32_io=1 if float32_io else 0)
        rc = lib.cba_pose_essential_batch(C.byref(desc), self.device_id, _lib.ptr(pose), _lib.ptr(status), _lib.ptr(n_inl),
                                          _lib.ptr(n_chr), _lib.ptr(cond), _lib.ptr(winner), _lib.ptr(flag), _lib.ptr(xyz), _lib.ptr(und))
        _lib.check(lib, rc, "cba_pose_essential_batch")
        return dict(pose=pose, status=status, n_inliers=n_inl, n_cheiral=n_chr, conditioning=cond, winner=winner, flag=flag, xyz=xyz,
                    undistorted=und)

    def resect_batch(self, job_start, obj, uv, threshold, n_hyp, min_points, seed):
        """Returns a dict: pose[n_jobs, 12], status, n_inliers, winner, err[n]."""
        lib = _lib.bind(_lib.load(), EPI_SIGNATURES)
        job_start = np.ascontiguousarray(job_start, dtype=np.int64)
        obj = np.ascontiguousarray(obj, dtype=np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        n_jobs = len(job_start) - 1
        pose, status = np.zeros((n_jobs, 12)), np.zeros(n_jobs, dtype=np.int32)
        n_inl, winner, err = np.zeros(n_jobs, dtype=np.int64), np.zeros(n_jobs, dtype=np.int32), np.zeros(len(obj))
        desc = ResectDesc(n_jobs=n_jobs, job_start=_lib.ptr(job_start), obj=_lib.ptr(obj), uv=_lib.ptr(uv), threshold=_lib.ptr(threshold),
                          n_hyp=int(n_hyp), min_points=int(min_points), seed=int(seed))
        rc = lib.cba_pose_resect_batch(C.byref(desc), self.device_id, _lib.ptr(pose), _lib.ptr(status), _lib.ptr(n_inl),
                                       _lib.ptr(winner), _lib.ptr(err))
        _lib.check(lib, rc, "cba_pose_resect_batch")
        return dict(pose=pose, status=status, n_inliers=n_inl, winner=winner, err=err)

    def pair_rmse(self, pair_pose, pair_start, obs_a, obs_b):
        return DevicePnP(self.device_id).pair_rmse(pair_pose, pair_start, obs_a, obs_b)


# ------------------------------------------------------------------------------------------------------------------------------
def pooled_correspondences(df_a, df_b):
    """Matched pixels of one camera pair pooled over every shared frame: ``(keys[N, 3] = object_id, keypoint_id, sync_index;
    pixels_a[N, 2]; pixels_b[N, 2])``, rows with a non-finite pixel in either view dropped (reference semantics: an inner
    merge on (sync_index, object_id, keypoint_id), left order)."""
    on = ["sync_index", "object_id", "keypoint_id"]
    merged = df_a[on + ["img_loc_x", "img_loc_y"]].merge(df_b[on + ["img_loc_x", "img_loc_y"]], on=on, suffixes=("_a", "_b"))
    if merged.empty:
        return np.empty((0, 3), dtype=np.int64), np.empty((0, 2)), np.empty((0, 2))
    keys = merged[["object_id", "keypoint_id", "sync_index"]].to_numpy(dtype=np.int64)
    pix_a = merged[["img_loc_x_a", "img_loc_y_a"]].to_numpy(dtype=np.float64)
    pix_b = merged[["img_loc_x_b", "img_loc_y_b"]].to_numpy(dtype=np.float64)
    finite = np.isfinite(pix_a).all(axis=1) & np.isfinite(pix_b).all(axis=1)
    return keys[finite], pix_a[finite], pix_b[finite]


def _camera_tables(cameras):
    return _intrinsic_tables(SimpleNamespace(cameras=dict(enumerate(cameras))), list(range(len(cameras))))


def recover_pair_pose(pixels_a, pixels_b, *, camera_a, camera_b, n_hyp: int = ESSENTIAL_HYPOTHESES, seed: int = DEFAULT_SEED, _epi=None) -> dict:
    """Essential-matrix pose of camera b relative to camera a from matched pixels (one job of ``cba_pose_essential_batch``).
    The reference's dict keys (``rotation``, ``translation`` (unit), ``inlier_fraction``, ``n_inliers``, ``n_total``,
    ``cheirality_inliers``, ``conditioning``, ``norm_a``, ``norm_b``, ``inlier_index``) plus ``points``: the two-view point of
    every row (NaN unless a cheirality inlier).  Raises ``ValueError`` when the estimate fails."""
    backend = _epi or DeviceEpipolar()
    pixels_a = np.asarray(pixels_a, dtype=np.float64).reshape(-1, 2)
    pixels_b = np.asarray(pixels_b, dtype=np.float64).reshape(-1, 2)
    n = len(pixels_a)
    if n < MIN_CORRESPONDENCES or len(pixels_b) != n:
        raise ValueError(f"essential-matrix estimation needs {MIN_CORRESPONDENCES} matched points, got {n}")
    model, intr = _camera_tables([camera_a, camera_b])
    thr = RANSAC_THRESHOLD_PX / (0.5 * (camera_a.matrix[0, 0] + camera_b.matrix[0, 0]))
    out = backend.essential_batch(model, intr, np.vstack([pixels_a, pixels_b]), np.repeat(np.arange(2, dtype=np.int32), n),
                                  np.array([0, n], np.int64), np.arange(n), n + np.arange(n), np.array([thr]), n_hyp, seed)
    if out["status"][0] != EPI_OK:
        raise ValueError(f"essential-matrix estimation failed (status {int(out['status'][0])})")
    flag, und = out["flag"], out["undistorted"]
    return {
        "rotation": out["pose"][0, :9].reshape(3, 3).copy(),
        "translation": out["pose"][0, 9:].copy(),
        "inlier_fraction": float(out["n_inliers"][0] / n),
        "n_inliers": int(out["n_inliers"][0]),
        "n_total": int(n),
        "cheirality_inliers": int(out["n_cheiral"][0]),
        "conditioning": float(out["conditioning"][0]),
        "norm_a": und[:n].copy(),
        "norm_b": und[n:].copy(),
        "inlier_index": np.flatnonzero(flag == 2),
        "points": out["xyz"],
    }


def triangulate_scaffold(pair_pose: dict, keys) -> dict:
    """``{(object_id, keypoint_id, sync_index): xyz}``: the scaffold pair's cheirality inliers triangulated with A at
    [I | 0] and B at [R | t] (baseline 1); points at infinity (|w| <= 1e-12) are left out."""
    index = pair_pose["inlier_index"]
    pts = pair_pose["points"][index]
    ok = np.isfinite(pts).all(axis=1)
    return {(int(keys[i, 0]), int(keys[i, 1]), int(keys[i, 2])): pts[j] for j, i in enumerate(index) if ok[j]}


def resection_camera(cloud: dict, df_cam, camera, *, n_hyp: int = RESECTION_HYPOTHESES, seed: int = DEFAULT_SEED, _epi=None):
    """World-to-camera pose of one camera by RANSAC resection against ``cloud`` (one job of ``cba_pose_resect_batch``):
    ``(R, t, n_points, median normalised reprojection error)``.  Raises ``ValueError`` below MIN_RESECTION_POINTS matched
    points or when the resection fails."""
    backend = _epi or DeviceEpipolar()
    if not cloud:
        raise ValueError("scaffold cloud is empty")
    keys = np.array(list(cloud), dtype=np.int64).reshape(-1, 3)
    xyz = np.array(list(cloud.values()), dtype=np.float64).reshape(-1, 3)
    cam_keys = df_cam[["object_id", "keypoint_id", "sync_index"]].to_numpy(dtype=np.int64).reshape(-1, 3)
    pix = df_cam[["img_loc_x", "img_loc_y"]].to_numpy(dtype=np.float64)
    # (object_id, keypoint_id, sync_index) encoded as one int64 over the ranges both sides span, matched by searchsorted
    both = np.vstack([keys, cam_keys])
    lo, span = both.min(axis=0), both.max(axis=0) - both.min(axis=0) + 1
    code = lambda q: ((q[:, 0] - lo[0]) * span[1] + (q[:, 1] - lo[1])) * span[2] + (q[:, 2] - lo[2])  # noqa: E731
    ck = code(keys)
    order = np.argsort(ck, kind="stable")
    pos = np.searchsorted(ck[order], code(cam_keys))
    pos_c = np.minimum(pos, len(ck) - 1)
    rows = np.flatnonzero((pos < len(ck)) & (ck[order][pos_c] == code(cam_keys)))
    pts = order[pos_c[rows]]
    if len(rows):
        fin = np.isfinite(pix[rows]).all(axis=1)
        rows, pts = rows[fin], pts[fin]
    if len(rows) < MIN_RESECTION_POINTS:
        raise ValueError(f"only {len(rows)} cloud points to resection against")
    model, intr = _camera_tables([camera])
    # (the essential call with no pairs is the undistortion of its rows)
    uv = backend.essential_batch(model, intr, pix[rows], np.zeros(len(rows), np.int32), np.zeros(1, np.int64), np.zeros(0, np.int64),
                                 np.zeros(0, np.int64), np.zeros(0), 1, seed)["undistorted"]
    out = backend.resect_batch(np.array([0, len(rows)], np.int64), xyz[pts], uv, np.array([RANSAC_THRESHOLD_PX / camera.matrix[0, 0]]),
                               n_hyp, MIN_RESECTION_POINTS, seed)
    if out["status"][0] != EPI_OK:
        raise ValueError("resection failed")
    return out["pose"][0, :9].reshape(3, 3).copy(), out["pose"][0, 9:].copy(), int(len(rows)), float(np.median(out["err"]))


# ------------------------------------------------------------------------------------------------------------------------------
def pair_correspondences(cam, sync, obj, kp, min_count: int = MIN_CORRESPONDENCES):
    """Pooled correspondences of every camera pair in one sort of all rows on (sync_index, object_id, keypoint_id): the
    ``common_observations`` machinery, returning indices.  ``(pairs[(a, b)], pair_start, row_a, row_b, group)`` where rows are
    positions in the given arrays, pairs are ordered by (a, b), each pair's correspondences by key, and ``group`` holds the
    rank of every row's key (the point a correspondence belongs to)."""
    order = np.lexsort((cam, kp, obj, sync))
    starts = _group_starts(sync[order], obj[order], kp[order])
    group = np.empty(len(cam), dtype=np.int64)
    group[order] = np.repeat(np.arange(len(starts) - 1), np.diff(starts))
    i, j = _pairs_within_groups(starts, cam[order])
    ra, rb = order[i], order[j]  # cam[ra] < cam[rb]
    if len(ra) == 0:
        return [], np.zeros(1, np.int64), ra, rb, group
    base = int(cam.max()) + 1
    key = cam[ra] * base + cam[rb]
    o = np.argsort(key, kind="stable")
    ra, rb, key = ra[o], rb[o], key[o]
    st = _group_starts(key)
    keep = np.diff(st) >= min_count
    pairs = [(int(key[s] // base), int(key[s] % base)) for s in st[:-1][keep]]
    sel = np.repeat(keep, np.diff(st))
    ra, rb = ra[sel], rb[sel]
    sizes = np.diff(st)[keep]
    return pairs, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), ra, rb, group


def build_epipolar_pose_network(image_points, camera_array, *, n_hyp: int = ESSENTIAL_HYPOTHESES, seed: int = DEFAULT_SEED,
                                report: dict | None = None, _epi=None) -> PairedPoseNetwork:
    """The reference's ``build_epipolar_pose_network``, batched: one essential call for every pair, one resection call for
    every (scaffold candidate, other camera) job.  ``obj_loc`` is not read.  Raises ``CalibrationError`` for fewer than 2
    observed cameras or when no pair reaches MIN_CORRESPONDENCES shared correspondences.

    ``report`` (optional dict) receives ``scores`` (``(a, b, failures, worst median error, -cheirality)`` per candidate, in
    candidate order), ``scaffold``, the job counts and the wall time of every stage in seconds (``*_s``)."""
    backend = _epi or DeviceEpipolar()
    rep = report if report is not None else {}
    clock = [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        rep[name + "_s"] = now - clock[0]
        clock[0] = now

    df = image_points.df
    observed = set(int(c) for c in df["cam_id"].unique())
    cam_ids = sorted(c for c, cam in camera_array.cameras.items() if not cam.ignore and c in observed)
    if len(cam_ids) < 2:
        raise CalibrationError(f"Epipolar bootstrap needs at least 2 cameras with observations, found {len(cam_ids)}.")
    cam_all = df["cam_id"].to_numpy(dtype=np.int64)
    xy_all = df[["img_loc_x", "img_loc_y"]].to_numpy(dtype=np.float64)
    rows = np.flatnonzero(np.isin(cam_all, cam_ids) & np.isfinite(xy_all).all(axis=1))
    cam = cam_all[rows]
    sync = df["sync_index"].to_numpy(dtype=np.int64)[rows]
    obj = df["object_id"].to_numpy(dtype=np.int64)[rows]
    kp = df["keypoint_id"].to_numpy(dtype=np.int64)[rows]
    lut = {c: i for i, c in enumerate(cam_ids)}
    cam_idx = np.array([lut[c] for c in cam.tolist()], dtype=np.int32) if len(cam) else np.zeros(0, np.int32)
    model, intr = _intrinsic_tables(camera_array, cam_ids)
    fx = intr[:, 0]

    pairs, pair_start, ra, rb, group = pair_correspondences(cam, sync, obj, kp)
    lap("pooled_correspondences_host")
    if not pairs:
        raise CalibrationError(
            f"Insufficient camera overlap for epipolar bootstrap: no camera pair reached the {MIN_CORRESPONDENCES} shared "
            f"correspondences an essential matrix needs. Cameras must share observations of the moving subject across frames.")
    thr = np.array([RANSAC_THRESHOLD_PX / (0.5 * (fx[lut[a]] + fx[lut[b]])) for a, b in pairs])
    ess = backend.essential_batch(model, intr, xy_all[rows], cam_idx, pair_start, ra, rb, thr, n_hyp, seed)
    lap("essential_batch")
    rep.update(pairs=len(pairs), correspondences=int(pair_start[-1]))
    und = ess["undistorted"]

    pair_poses = {}
    for p, (a, b) in enumerate(pairs):
        s, e = int(pair_start[p]), int(pair_start[p + 1])
        if ess["status"][p] != EPI_OK:
            logger.warning(f"Pair {a}-{b}: essential-matrix recovery failed (status {int(ess['status'][p])})")
            continue
        pair_poses[(a, b)] = p
        cond = float(ess["conditioning"][p])
        logger.info(f"Pair {a}-{b}: {int(ess['n_inliers'][p])}/{e - s} inliers, {int(ess['n_cheiral'][p])} cheirality, E conditioning {cond:.3f}")
        if cond < CONDITIONING_FLOOR:
            logger.warning(f"Pair {a}-{b}: essential matrix poorly conditioned (singular-value ratio {cond:.3f} < {CONDITIONING_FLOOR}).")
    if not pair_poses:
        raise CalibrationError(
            f"Insufficient camera overlap for epipolar bootstrap: no camera pair reached the {MIN_CORRESPONDENCES} shared "
            f"correspondences an essential matrix needs (every essential estimate failed).")

    # scaffold candidates: the strongest pairs by cheirality inliers (stable: ties keep pair order)
    cand = sorted(pair_poses, key=lambda q: -int(ess["n_cheiral"][pair_poses[q]]))[:MAX_SCAFFOLD_CANDIDATES]

    # every row of a camera, sorted by its key's group (the match against a cloud is a searchsorted on the group index)
    rows_of = {}
    for c in cam_ids:
        r = np.flatnonzero(cam == c)
        rows_of[c] = r[np.argsort(group[r], kind="stable")]
    job_start, job_obj, job_uv, job_thr, job_of = [0], [], [], [], []
    clouds = []
    for ci, pair in enumerate(cand):
        p = pair_poses[pair]
        s, e = int(pair_start[p]), int(pair_start[p + 1])
        idx = s + np.flatnonzero((ess["flag"][s:e] == 2) & np.isfinite(ess["xyz"][s:e]).all(axis=1))
        g, first = np.unique(group[ra[idx]], return_index=True)  # one point per key (the first correspondence)
        pts = ess["xyz"][idx[first]]
        clouds.append(len(g))
        for c in cam_ids:
            if c in pair:
                continue
            r = rows_of[c]
            pos = np.searchsorted(g, group[r])
            hit = (pos < len(g)) & (g[np.minimum(pos, len(g) - 1)] == group[r]) if len(g) else np.zeros(len(r), bool)
            if int(hit.sum()) < MIN_RESECTION_POINTS:
                continue
            job_obj.append(pts[pos[hit]])
            job_uv.append(und[r[hit]])
            job_thr.append(RANSAC_THRESHOLD_PX / fx[lut[c]])
            job_start.append(job_start[-1] + int(hit.sum()))
            job_of.append((ci, c))
    lap("scaffold_clouds_host")
    rep.update(resection_jobs=len(job_of), resection_points=int(job_start[-1]))
    if job_of:
        res = backend.resect_batch(np.array(job_start, np.int64), np.concatenate(job_obj), np.concatenate(job_uv), np.array(job_thr),
                                   RESECTION_HYPOTHESES, MIN_RESECTION_POINTS, seed)
    resected = {}
    for jn, (ci, c) in enumerate(job_of):
        if res["status"][jn] == EPI_OK:
            s, e = job_start[jn], job_start[jn + 1]
            resected[(ci, c)] = (res["pose"][jn, :9].reshape(3, 3).copy(), res["pose"][jn, 9:].copy(), float(np.median(res["err"][s:e])))

    lap("resect_batch")
    best, best_score = None, None
    rep["scores"] = []
    for ci, pair in enumerate(cand):
        others = [c for c in cam_ids if c not in pair]
        errs = [resected[(ci, c)][2] for c in others if (ci, c) in resected]
        score = (len(others) - len(errs), max(errs) if errs else 0.0, -int(ess["n_cheiral"][pair_poses[pair]]))
        rep["scores"].append((pair[0], pair[1]) + score)
        logger.info(f"Scaffold candidate {pair[0]}-{pair[1]}: cloud of {clouds[ci]} points, score {score}")
        if best_score is None or score < best_score:
            best, best_score = ci, score
    pair = cand[best]
    anchor = pair[0]
    p = pair_poses[pair]
    poses = {pair[1]: (ess["pose"][p, :9].reshape(3, 3).copy(), ess["pose"][p, 9:].copy())}
    for c in cam_ids:
        if (best, c) in resected:
            poses[c] = resected[(best, c)][:2]
    logger.info(f"Selected scaffold {pair[0]}-{pair[1]} (failures={best_score[0]}, worst third-view reprojection={best_score[1]:.5f}); "
                f"posed {len(poses) + 1}/{len(cam_ids)} cameras, anchor = cam {anchor}")

    # anchor-relative StereoPairs (primary < secondary, as the PnP path keys them)
    aggregated = {}
    for c, (R, t) in poses.items():
        sp = StereoPair(primary_cam_id=anchor, secondary_cam_id=c, error_score=float("nan"), rotation=R, translation=t)
        if sp.primary_cam_id > sp.secondary_cam_id:
            sp = sp.inverted()
        aggregated[sp.pair] = sp
    undistorted = np.full((len(df), 2), np.nan)
    undistorted[rows] = und
    common = common_observations(image_points, camera_array, undistorted)
    rep["scaffold"] = pair
    lap("scaffold_choice_host")
    net = estimate_pnp_paired_pose_network(aggregated, common, _pnp=backend)
    lap("stereo_rmse_and_graph")
    return net


__all__ = [
    "RANSAC_THRESHOLD_PX", "RANSAC_PROB", "MIN_RESECTION_POINTS", "MIN_CORRESPONDENCES", "CONDITIONING_FLOOR", "MAX_SCAFFOLD_CANDIDATES",
    "DeviceEpipolar", "pooled_correspondences", "recover_pair_pose", "triangulate_scaffold", "resection_camera", "pair_correspondences",
    "build_epipolar_pose_network",
]
