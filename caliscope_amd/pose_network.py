"""Initial camera poses of an unposed board session: PnP per board view on the MI355X, then the stereo-pair graph.

Host-side mirror of the reference's PnP bootstrap (``core/bootstrap_pose/``: ``stereopairs.py``, ``paired_pose_network.py``,
``pose_network_builder.py``, ``build_paired_pose_network.py``), with the same public names:

* :class:`StereoPair` (``pair``, ``inverted()``, ``link()``), :class:`PairedPoseNetwork` (``from_raw_estimates``, ``get_pair``,
  ``apply_to``), :class:`PoseNetworkBuilder` (``estimate_camera_to_object_poses -> estimate_relative_poses -> filter_outliers ->
  build``, ``state``) and :func:`build_paired_pose_network`.

Where the stages run:

  undistortion + PnP of every (cam_id, sync_index, object_id) view      device, ``cba_pose_pnp_batch`` (one thread per view)
  relative poses T_B_A = T_B_obj T_A_obj^-1 per pair and (sync, object)  numpy, one pass per camera offset inside a view group
  IQR outlier rejection, quaternion average, mean translation           numpy, per camera pair
  common observations of each pair (>= 4)                               numpy, one sort on (sync_index, object_id, keypoint_id)
  stereo RMSE of each aggregated pair                                   device, ``cba_pose_pair_rmse`` (one workgroup per pair)
  graph: inversion, bridging, largest connected component, anchor       host (cameras^3 at most)

The PnP itself (``csrc/pnp_math.h``) is IPPE + Levenberg-Marquardt for planar boards and a DLT + Levenberg-Marquardt for
3-D targets: the least-squares pose, where the reference asks cv2 for SOLVEPNP_IPPE / SOLVEPNP_SQPNP.  Sessions without
object geometry (``obj_loc`` all NaN) take the essential-matrix bootstrap of :mod:`caliscope_amd.epipolar_pose`
(``build_paired_pose_network(method="epipolar" | "auto")``).

There is no CPU fallback: without the library or a GPU the device stages raise ``BackendError``.  ``_pnp`` replaces both
device calls (an object with ``pnp_batch`` and ``pair_rmse``, as :class:`DevicePnP`) — the CPU test-suite passes a g++
build of the same arithmetic.
"""

from __future__ import annotations

import ctypes as C
import logging
from collections import deque
from copy import deepcopy
from dataclasses import dataclass
from itertools import permutations
from typing import Dict, Tuple

import numpy as np
from scipy.spatial.transform import Rotation

from caliscope_amd import _lib

logger = logging.getLogger(__name__)

DEFAULT_MIN_PNP_POINTS = 4
DEFAULT_OUTLIER_THRESHOLD = 1.5
PNP_OK, PNP_TOO_FEW, PNP_FAILED = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------------------------
# C ABI of include/caliscope_pose.h (kept out of _lib.SIGNATURES, which mirrors include/caliscope_ba.h)

class PnpDesc(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("cam_model", _lib.c_int32_p), ("cam_intr", _lib.c_double_p), ("n_views", C.c_int64),
        ("view_start", _lib.c_int64_p), ("view_cam", _lib.c_int32_p), ("obs_xy", _lib.c_double_p), ("obs_obj", _lib.c_double_p),
        ("min_points", C.c_int32), ("float32_io", C.c_int32),
    ]


class PairDesc(C.Structure):
    _fields_ = [
        ("n_pairs", C.c_int64), ("pair_pose", _lib.c_double_p), ("pair_start", _lib.c_int64_p), ("obs_a", _lib.c_double_p),
        ("obs_b", _lib.c_double_p),
    ]


POSE_SIGNATURES = {
    "cba_pose_pnp_batch": (C.c_int, [C.POINTER(PnpDesc), C.c_int32, _lib.c_double_p, _lib.c_double_p, _lib.c_int32_p, _lib.c_double_p]),
    "cba_pose_pair_rmse": (C.c_int, [C.POINTER(PairDesc), C.c_int32, _lib.c_double_p, _lib.c_int64_p]),
}


class DevicePnP:
    """The two device calls of the bootstrap (``cba_pose_pnp_batch``, ``cba_pose_pair_rmse``) on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def pnp_batch(self, view_start, view_cam, cam_model, cam_intr, obs_xy, obs_obj, min_points, float32_io):
        """Returns ``(pose[n_views, 12], rmse[n_views], status[n_views], undistorted[n_obs, 2])``."""
        lib = _lib.bind(_lib.load(), POSE_SIGNATURES)
        view_start = np.ascontiguousarray(view_start, dtype=np.int64)
        view_cam = np.ascontiguousarray(view_cam, dtype=np.int32)
        cam_model = np.ascontiguousarray(cam_model, dtype=np.int32)
        cam_intr = np.ascontiguousarray(cam_intr, dtype=np.float64)
        obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64)
        obs_obj = np.ascontiguousarray(obs_obj, dtype=np.float64)
        n_views = len(view_start) - 1
        pose, rmse = np.zeros((n_views, 12)), np.zeros(n_views)
        status, und = np.zeros(n_views, dtype=np.int32), np.zeros_like(obs_xy)
        desc = PnpDesc(n_cams=len(cam_model), cam_model=_lib.ptr(cam_model), cam_intr=_lib.ptr(cam_intr), n_views=n_views,
                       view_start=_lib.ptr(view_start), view_cam=_lib.ptr(view_cam), obs_xy=_lib.ptr(obs_xy),
                       obs_obj=_lib.ptr(obs_obj), min_points=int(min_points), float32_io=1 if float32_io else 0)
        rc = lib.cba_pose_pnp_batch(C.byref(desc), self.device_id, _lib.ptr(pose), _lib.ptr(rmse), _lib.ptr(status), _lib.ptr(und))
        _lib.check(lib, rc, "cba_pose_pnp_batch")
        return pose, rmse, status, und

    def pair_rmse(self, pair_pose, pair_start, obs_a, obs_b):
        """Returns ``(rmse[n_pairs], count[n_pairs])``."""
        lib = _lib.bind(_lib.load(), POSE_SIGNATURES)
        pair_pose = np.ascontiguousarray(pair_pose, dtype=np.float64)
        pair_start = np.ascontiguousarray(pair_start, dtype=np.int64)
        obs_a = np.ascontiguousarray(obs_a, dtype=np.float64)
        obs_b = np.ascontiguousarray(obs_b, dtype=np.float64)
        n_pairs = len(pair_start) - 1
        rmse, count = np.zeros(n_pairs), np.zeros(n_pairs, dtype=np.int64)
        desc = PairDesc(n_pairs=n_pairs, pair_pose=_lib.ptr(pair_pose), pair_start=_lib.ptr(pair_start), obs_a=_lib.ptr(obs_a), obs_b=_lib.ptr(obs_b))
        rc = lib.cba_pose_pair_rmse(C.byref(desc), self.device_id, _lib.ptr(rmse), _lib.ptr(count))
        _lib.check(lib, rc, "cba_pose_pair_rmse")
        return rmse, count


# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class StereoPair:
    """Pose of the secondary camera in the primary camera's frame (X_secondary = R X_primary + t) and its error score."""

    primary_cam_id: int
    secondary_cam_id: int
    error_score: float
    translation: np.ndarray
    rotation: np.ndarray

    def __post_init__(self):
        object.__setattr__(self, "translation", np.squeeze(np.asarray(self.translation, dtype=np.float64)))
        object.__setattr__(self, "rotation", np.asarray(self.rotation, dtype=np.float64))
        if self.translation.shape != (3,):
            raise ValueError(f"Translation must be shape (3,) after squeezing, got {self.translation.shape}.")
        if self.rotation.shape != (3, 3):
            raise ValueError(f"Rotation must be shape (3,3), got {self.rotation.shape}")

    @property
    def pair(self) -> Tuple[int, int]:
        return (self.primary_cam_id, self.secondary_cam_id)

    @property
    def transformation(self) -> np.ndarray:
        T = np.eye(4)
        T[:3, :3] = self.rotation
        T[:3, 3] = self.translation
        return T

    def inverted(self) -> "StereoPair":
        """A -> B becomes B -> A (same error score)."""
        Ti = np.linalg.inv(self.transformation)
        return StereoPair(self.secondary_cam_id, self.primary_cam_id, self.error_score, Ti[0:3, 3], Ti[0:3, 0:3])

    def link(self, other: "StereoPair") -> "StereoPair":
        """(A -> B).link(B -> C) = A -> C; the error scores add up."""
        T = other.transformation @ self.transformation
        return StereoPair(self.primary_cam_id, other.secondary_cam_id, self.error_score + other.error_score, T[0:3, 3], T[0:3, 0:3])


@dataclass(frozen=True)
class PairedPoseNetwork:
    """Graph of stereo pairs between cameras (both directions of every link)."""

    _pairs: Dict[Tuple[int, int], StereoPair]

    @classmethod
    def from_raw_estimates(cls, raw_pairs: Dict[Tuple[int, int], StereoPair]) -> "PairedPoseNetwork":
        """Add the inverse of every pair, then fill missing pairs (A, C) by the bridge A -> X -> C of lowest summed error,
        round after round until the number of missing pairs stops changing (the reference's order: cameras sorted, candidate
        pairs in ``permutations`` order, bridges X in sorted order, a later bridge replaces only on a strictly lower error)."""
        all_pairs = dict(raw_pairs)
        all_pairs.update({(inv := p.inverted()).pair: inv for p in raw_pairs.values()})
        cam_ids = sorted({c for pair in all_pairs for c in pair})
        last = -1
        while True:
            missing = [pair for pair in permutations(cam_ids, 2) if pair not in all_pairs]
            if len(missing) == last or not missing:
                break
            last = len(missing)
            for a, c in missing:
                best = None
                for x in cam_ids:
                    ax, xc = all_pairs.get((a, x)), all_pairs.get((x, c))
                    if ax is not None and xc is not None:
                        bridge = ax.link(xc)
                        if best is None or best.error_score > bridge.error_score:
                            best = bridge
                if best is not None:
                    all_pairs[best.pair] = best
                    inv = best.inverted()
                    all_pairs[inv.pair] = inv
        logger.info(f"Paired pose network with {len(all_pairs)} directed pairs")
        return cls(_pairs=all_pairs)

    def get_pair(self, cam_id_a: int, cam_id_b: int) -> StereoPair | None:
        return self._pairs.get((cam_id_a, cam_id_b))

    def _find_largest_connected_component(self, cam_ids) -> set:
        if not self._pairs:
            return set()
        adj = {c: [] for c in cam_ids}
        for a, b in self._pairs:
            if a in adj:
                adj[a].append(b)
        visited, largest = set(), set()
        for c in cam_ids:
            if c in visited:
                continue
            comp, q = set(), deque([c])
            visited.add(c)
            while q:
                u = q.popleft()
                comp.add(u)
                for v in adj.get(u, []):
                    if v not in visited:
                        visited.add(v)
                        q.append(v)
            if len(comp) > len(largest):
                largest = comp
        return largest

    def _build_anchored_config(self, camera_array, anchor_cam_id: int):
        """Every camera unposed, the anchor at the origin, the others at the anchor's direct link; returns (summed error, cameras)."""
        configured = {}
        for cam_id, cam in camera_array.cameras.items():
            new = deepcopy(cam)
            new.rotation, new.translation = None, None
            configured[cam_id] = new
        configured[anchor_cam_id].rotation = np.eye(3, dtype=np.float64)
        configured[anchor_cam_id].translation = np.zeros(3, dtype=np.float64)
        total = 0.0
        for cam_id in sorted(camera_array.cameras):
            if cam_id == anchor_cam_id:
                continue
            p = self._pairs.get((anchor_cam_id, cam_id))
            if p is not None:
                configured[cam_id].translation = p.translation.flatten()
                configured[cam_id].rotation = p.rotation
                total += p.error_score
        return total, configured

    def get_best_anchored_camera_array(self, main_group_cam_ids, camera_array):
        best_anchor, lowest, best_config = -1, float("inf"), None
        for cam_id in main_group_cam_ids:  # (a set, iterated as the reference does)
            score, config = self._build_anchored_config(camera_array, cam_id)
            if score < lowest:
                lowest, best_anchor, best_config = score, cam_id, config
        if best_anchor == -1:
            return None, camera_array.cameras
        return best_anchor, best_config

    def apply_to(self, camera_array, anchor_cam: int | None = None) -> None:
        """Pose ``camera_array`` in place from the graph: the anchor (given, or the camera of the largest connected component
        with the lowest summed error to the others) at the origin; cameras outside that component stay unposed."""
        cam_ids = sorted(camera_array.cameras)
        main = self._find_largest_connected_component(cam_ids)
        if anchor_cam is not None:
            _, config = self._build_anchored_config(camera_array, anchor_cam)
        else:
            anchor_cam, config = self.get_best_anchored_camera_array(main, camera_array)
            logger.info(f"Selected camera {anchor_cam} as anchor, yielding lowest initial error.")
        for cam_id, cam in config.items():
            camera_array.cameras[cam_id] = cam
        unposed = [c for c in cam_ids if c not in main]
        if unposed:
            logger.warning(f"Cameras not in the main group remain unposed: {unposed}")


# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ViewPoses:
    """Camera-to-object poses of the successful views, one row per (cam_id, sync_index, object_id), sorted by that key."""

    cam_id: np.ndarray
    sync_index: np.ndarray
    object_id: np.ndarray
    rotation: np.ndarray  # (k, 3, 3)
    translation: np.ndarray  # (k, 3)
    rmse: np.ndarray

    def __len__(self):
        return len(self.cam_id)

    def as_dict(self) -> dict:
        """``{(cam_id, sync_index, object_id): (R, t, rmse)}`` as the reference's ``compute_camera_to_object_poses_pnp`` returns."""
        return {(int(c), int(s), int(o)): (R, t, float(e)) for c, s, o, R, t, e in
                zip(self.cam_id, self.sync_index, self.object_id, self.rotation, self.translation, self.rmse)}


@dataclass(frozen=True)
class RelativePoses:
    """T_B_A of every camera pair (a < b) that sees one (sync_index, object_id) in both of its views."""

    cam_a: np.ndarray
    cam_b: np.ndarray
    sync_index: np.ndarray
    object_id: np.ndarray
    rotation: np.ndarray
    translation: np.ndarray


def _intrinsic_tables(camera_array, cam_ids):
    model = np.zeros(len(cam_ids), dtype=np.int32)
    intr = np.zeros((len(cam_ids), 9))
    for i, c in enumerate(cam_ids):
        cam = camera_array.cameras[c]
        K = np.asarray(cam.matrix, dtype=np.float64)
        d = np.asarray(cam.distortions, dtype=np.float64).ravel()
        model[i] = 1 if cam.fisheye else 0
        intr[i, :4] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        intr[i, 4 : 4 + min(len(d), 5)] = d[:5]
    return model, intr


def _group_starts(*keys):
    """Starts of the runs of equal key tuples in sorted arrays, with the end appended."""
    n = len(keys[0])
    brk = np.zeros(max(n - 1, 0), dtype=bool)
    for k in keys:
        brk |= np.diff(k) != 0
    return np.concatenate([[0], np.flatnonzero(brk) + 1, [n]]).astype(np.int64)


def _pairs_within_groups(starts, cam):
    """Index pairs (i, j), i < j, of the rows of each group (rows sorted by camera inside a group): one pass per offset."""
    size = np.diff(starts)
    n = int(starts[-1])
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    group_of = np.repeat(np.arange(len(size)), size)
    ii, jj = [], []
    for d in range(1, int(size.max()) if len(size) else 1):
        i = np.arange(n - d)
        ok = group_of[i] == group_of[i + d]
        ii.append(i[ok])
        jj.append(i[ok] + d)
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    i, j = np.concatenate(ii), np.concatenate(jj)
    keep = cam[i] != cam[j]  # (a camera seen twice under one key is not a pair)
    return i[keep], j[keep]


def compute_camera_to_object_poses_pnp(image_points, camera_array, min_points: int = DEFAULT_MIN_PNP_POINTS, *, float32_io: bool = True,
                                       _pnp=None):
    """PnP of every (cam_id, sync_index, object_id) view on the device.  Returns ``(ViewPoses, undistorted)`` where
    ``undistorted`` holds the normalised image point of every row of ``image_points.df`` (NaN for rows not solved)."""
    df = image_points.df
    backend = _pnp or DevicePnP()
    cam_ids = [c for c, cam in camera_array.cameras.items() if cam.matrix is not None and cam.distortions is not None]
    for c, cam in camera_array.cameras.items():
        if c not in cam_ids:
            logger.warning(f"Camera {c} missing intrinsics, skipping")
    cam_all = df["cam_id"].to_numpy(dtype=np.int64)
    rows = np.flatnonzero(np.isin(cam_all, cam_ids))
    undistorted = np.full((len(df), 2), np.nan)
    empty = ViewPoses(*(np.zeros(0, np.int64),) * 3, np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0))
    if rows.size == 0:
        raise ValueError("No valid camera data found for PnP")
    cam = cam_all[rows]
    sync = df["sync_index"].to_numpy(dtype=np.int64)[rows]
    obj = df["object_id"].to_numpy(dtype=np.int64)[rows]
    order = np.lexsort((obj, sync, cam))  # the reference's groupby(["cam_id", "sync_index", "object_id"]); stable inside a view
    rows, cam, sync, obj = rows[order], cam[order], sync[order], obj[order]
    starts = _group_starts(cam, sync, obj)
    index_of = {c: i for i, c in enumerate(sorted(set(cam_ids)))}
    model, intr = _intrinsic_tables(camera_array, sorted(index_of))
    lut = np.zeros(max(index_of) + 1 if index_of else 1, dtype=np.int32)
    for c, i in index_of.items():
        lut[c] = i
    first = starts[:-1]
    xy = np.column_stack([df["img_loc_x"].to_numpy(dtype=np.float64)[rows], df["img_loc_y"].to_numpy(dtype=np.float64)[rows]])
    xyz = np.column_stack([df[c].to_numpy(dtype=np.float64)[rows] for c in ("obj_loc_x", "obj_loc_y", "obj_loc_z")])
    pose, rmse, status, und = backend.pnp_batch(starts, lut[cam[first]], model, intr, xy, xyz, min_points, float32_io)
    undistorted[rows] = und
    ok = status == PNP_OK
    n_fail = int((~ok).sum())
    logger.info(f"PnP complete: {int(ok.sum())} successes, {n_fail} failures")
    if not ok.any():
        return empty, undistorted
    vp = ViewPoses(cam[first][ok], sync[first][ok], obj[first][ok], pose[ok, :9].reshape(-1, 3, 3).copy(), pose[ok, 9:].copy(), rmse[ok])
    return vp, undistorted


def compute_relative_poses(view_poses: ViewPoses, camera_array) -> RelativePoses:
    """T_B_A = T_B_obj T_A_obj^-1 for every pair of non-ignored cameras a < b seeing one (sync_index, object_id)."""
    active = [c for c, cam in camera_array.cameras.items() if not cam.ignore]
    keep = np.isin(view_poses.cam_id, active)
    cam, sync, obj = view_poses.cam_id[keep], view_poses.sync_index[keep], view_poses.object_id[keep]
    R, t = view_poses.rotation[keep], view_poses.translation[keep]
    order = np.lexsort((cam, obj, sync))
    cam, sync, obj, R, t = cam[order], sync[order], obj[order], R[order], t[order]
    i, j = _pairs_within_groups(_group_starts(sync, obj), cam)
    Ra_T = np.transpose(R[i], (0, 2, 1))
    R_rel = R[j] @ Ra_T
    t_rel = t[j] - np.einsum("kij,kj->ki", R_rel, t[i])
    return RelativePoses(cam[i], cam[j], sync[i], obj[i], R_rel, t_rel)


def quaternion_average(quaternions: np.ndarray) -> np.ndarray:
    """Largest eigenvector of sum q q^T, sign so that w >= 0 (quaternions as (w, x, y, z))."""
    if len(quaternions) == 0:
        raise ValueError("Cannot average empty quaternion array")
    if len(quaternions) == 1:
        return quaternions[0]
    Q = np.asarray(quaternions).T
    _, vecs = np.linalg.eigh(Q @ Q.T)
    avg = vecs[:, -1]
    if avg[0] < 0:
        avg = -avg
    norm = np.linalg.norm(avg)
    if norm < 1e-10:
        logger.warning("Quaternion average failed, returning first quaternion")
        return quaternions[0]
    return avg / norm


def _wxyz(R):
    return np.roll(Rotation.from_matrix(R).as_quat(), 1, axis=-1)


def _from_wxyz(q):
    return Rotation.from_quat(np.roll(q, -1, axis=-1)).as_matrix()


def _pair_groups(rel: RelativePoses):
    """{(a, b): row indices of rel} in first-seen pair order."""
    if len(rel.cam_a) == 0:
        return {}
    key = rel.cam_a * (int(max(rel.cam_b.max(), rel.cam_a.max())) + 1) + rel.cam_b
    order = np.argsort(key, kind="stable")
    starts = _group_starts(key[order])
    return {(int(rel.cam_a[order[s]]), int(rel.cam_b[order[s]])): order[s:e] for s, e in zip(starts[:-1], starts[1:])}


def reject_outliers(rel: RelativePoses, threshold: float = DEFAULT_OUTLIER_THRESHOLD, rotation_threshold_multiplier: float | None = None,
                    translation_threshold_multiplier: float | None = None) -> dict:
    """IQR rejection per camera pair: ``{(a, b): kept row indices of rel}``.  Pairs with fewer than 5 valid samples are kept
    whole; otherwise |t| must lie within [q1 - k iqr, q3 + k iqr] and the angle to the average rotation must be at most
    q3 + k iqr (degrees; linear percentiles)."""
    rot_k = rotation_threshold_multiplier if rotation_threshold_multiplier is not None else threshold
    t_k = translation_threshold_multiplier if translation_threshold_multiplier is not None else threshold
    out = {}
    for pair, idx in _pair_groups(rel).items():
        R, t = rel.rotation[idx], rel.translation[idx]
        valid = ~(np.isnan(R).any(axis=(1, 2)) | np.isnan(t).any(axis=1))
        idx, R, t = idx[valid], R[valid], t[valid]
        if len(idx) < 5:
            logger.warning(f"Pair {pair} has only {len(idx)} samples, skipping outlier rejection")
            out[pair] = idx
            continue
        t_mag = np.linalg.norm(t, axis=1)
        q1, q3 = np.percentile(t_mag, [25, 75])
        iqr = q3 - q1
        t_bad = (t_mag < q1 - t_k * iqr) | (t_mag > q3 + t_k * iqr)
        R_avg = _from_wxyz(quaternion_average(_wxyz(R)))
        tr = np.clip(np.einsum("kij,ij->k", R, R_avg), -1.0, 3.0)  # trace(R R_avg^T)
        ang = np.degrees(np.arccos((tr - 1) / 2))
        r1, r3 = np.percentile(ang, [25, 75])
        r_bad = ang > r3 + rot_k * (r3 - r1)
        out[pair] = idx[~(t_bad | r_bad)]
        logger.info(f"Pair {pair}: {int((t_bad | r_bad).sum())}/{len(idx)} outliers rejected")
    return out


def aggregate_poses(rel: RelativePoses, kept: dict) -> Dict[Tuple[int, int], StereoPair]:
    """One StereoPair per pair: quaternion average of the kept rotations, mean of the kept translations (error NaN)."""
    out = {}
    for pair, idx in kept.items():
        if len(idx) == 0:
            logger.warning(f"No valid poses for pair {pair} after outlier rejection")
            continue
        if len(idx) == 1:
            out[pair] = StereoPair(pair[0], pair[1], float("nan"), rel.translation[idx[0]], rel.rotation[idx[0]])
            continue
        R_avg = _from_wxyz(quaternion_average(_wxyz(rel.rotation[idx])))
        out[pair] = StereoPair(pair[0], pair[1], float("nan"), np.mean(rel.translation[idx], axis=0), R_avg)
    return out


def common_observations(image_points, camera_array, undistorted, min_common: int = DEFAULT_MIN_PNP_POINTS) -> dict:
    """``{(a, b): (obs_a[m, 2], obs_b[m, 2])}``: the undistorted points both cameras (non-ignored, a < b) have of one
    (sync_index, object_id, keypoint_id), for pairs with at least ``min_common`` of them — one sort of all rows."""
    df = image_points.df
    active = [c for c, cam in camera_array.cameras.items() if not cam.ignore]
    cam = df["cam_id"].to_numpy(dtype=np.int64)
    rows = np.flatnonzero(np.isin(cam, active) & np.isfinite(undistorted).all(axis=1))
    cam = cam[rows]
    sync = df["sync_index"].to_numpy(dtype=np.int64)[rows]
    obj = df["object_id"].to_numpy(dtype=np.int64)[rows]
    kp = df["keypoint_id"].to_numpy(dtype=np.int64)[rows]
    order = np.lexsort((cam, kp, obj, sync))
    rows, cam = rows[order], cam[order]
    i, j = _pairs_within_groups(_group_starts(sync[order], obj[order], kp[order]), cam)
    rel = RelativePoses(cam[i], cam[j], np.zeros(len(i), np.int64), np.zeros(len(i), np.int64), np.zeros((len(i), 3, 3)), np.zeros((len(i), 3)))
    out = {}
    for pair, idx in _pair_groups(rel).items():
        if len(idx) >= min_common:
            idx = np.sort(idx)
            out[pair] = (undistorted[rows[i[idx]]], undistorted[rows[j[idx]]])
    return out


def estimate_pnp_paired_pose_network(aggregated: Dict[Tuple[int, int], StereoPair], common: dict, _pnp=None) -> PairedPoseNetwork:
    """Stereo RMSE of every aggregated pair (device: one launch for all pairs), then the bridged graph."""
    backend = _pnp or DevicePnP()
    pairs = [p for p in aggregated if p in common]
    for p in aggregated:
        if p not in common:
            logger.warning(f"Insufficient common points for RMSE calc on pair {p}, skipping")
    if not pairs:
        return PairedPoseNetwork.from_raw_estimates({})
    pose = np.stack([np.concatenate([aggregated[p].rotation.ravel(), aggregated[p].translation]) for p in pairs])
    sizes = np.array([len(common[p][0]) for p in pairs], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    obs_a = np.concatenate([common[p][0] for p in pairs])
    obs_b = np.concatenate([common[p][1] for p in pairs])
    rmse, _ = backend.pair_rmse(pose, start, obs_a, obs_b)
    raw = {}
    for p, e in zip(pairs, rmse):
        sp = aggregated[p]
        raw[p] = StereoPair(sp.primary_cam_id, sp.secondary_cam_id, float(e), sp.translation, sp.rotation)
        logger.info(f"Pair {p}: RMSE = {float(e):.6f}")
    return PairedPoseNetwork.from_raw_estimates(raw)


class PoseNetworkBuilder:
    """``PoseNetworkBuilder(cameras, image_points).estimate_camera_to_object_poses().estimate_relative_poses()
    .filter_outliers().build()`` -> :class:`PairedPoseNetwork` (reference ``pose_network_builder.py``)."""

    def __init__(self, camera_array, image_points, *, float32_io: bool = True, _pnp=None):
        self.camera_array = camera_array
        self._image_points = image_points
        self._float32_io = float32_io
        self._pnp = _pnp
        self._camera_to_object_poses: ViewPoses | None = None
        self._undistorted = None
        self._relative_poses: RelativePoses | None = None
        self._filtered_poses: dict | None = None
        self._aggregated_poses: dict | None = None
        self._pnp_network: PairedPoseNetwork | None = None
        self._state = "initialized"

    @property
    def state(self) -> str:
        return self._state

    def estimate_camera_to_object_poses(self, min_points: int = DEFAULT_MIN_PNP_POINTS) -> "PoseNetworkBuilder":
        self._relative_poses = self._filtered_poses = self._aggregated_poses = self._pnp_network = None
        self._camera_to_object_poses, self._undistorted = compute_camera_to_object_poses_pnp(
            self._image_points, self.camera_array, min_points, float32_io=self._float32_io, _pnp=self._pnp)
        self._state = "camera_poses_estimated"
        return self

    def estimate_relative_poses(self) -> "PoseNetworkBuilder":
        if self._camera_to_object_poses is None:
            raise RuntimeError("Must call estimate_camera_to_object_poses() first")
        self._relative_poses = compute_relative_poses(self._camera_to_object_poses, self.camera_array)
        self._state = "relative_poses_estimated"
        return self

    def filter_outliers(self, threshold: float = DEFAULT_OUTLIER_THRESHOLD, rotation_threshold_multiplier: float | None = None,
                        translation_threshold_multiplier: float | None = None) -> "PoseNetworkBuilder":
        if self._relative_poses is None:
            raise RuntimeError("Must call estimate_relative_poses() first")
        self._filtered_poses = reject_outliers(self._relative_poses, threshold, rotation_threshold_multiplier, translation_threshold_multiplier)
        self._state = "filtered"
        return self

    def build(self) -> PairedPoseNetwork:
        if self._filtered_poses is None:
            raise RuntimeError("Must call filter_outliers() first")
        self._aggregated_poses = aggregate_poses(self._relative_poses, self._filtered_poses)
        common = common_observations(self._image_points, self.camera_array, self._undistorted)
        self._pnp_network = estimate_pnp_paired_pose_network(self._aggregated_poses, common, _pnp=self._pnp)
        self._state = "built"
        return self._pnp_network


def has_object_geometry(image_points) -> bool:
    cols = [c for c in ("obj_loc_x", "obj_loc_y", "obj_loc_z") if c in image_points.df.columns]
    return bool(cols) and not image_points.df[cols].isna().all().all()


POSE_METHODS = ("pnp", "epipolar", "auto")


def build_paired_pose_network(image_points, camera_array, *, method: str = "pnp", _pnp=None, _epi=None) -> PairedPoseNetwork:
    """The reference's entry point.  ``method="pnp"`` (default): the PnP path (outlier threshold 1.5), which needs object
    geometry and raises ``ValueError`` without it.  ``"epipolar"``: the essential-matrix path of
    :mod:`caliscope_amd.epipolar_pose` (``obj_loc`` not read).  ``"auto"``: the reference's branching — PnP with object
    geometry, epipolar when ``obj_loc`` is all NaN."""
    if method not in POSE_METHODS:
        raise ValueError(f"method must be one of {POSE_METHODS}, got {method!r}")
    if method == "epipolar" or (method == "auto" and not has_object_geometry(image_points)):
        from caliscope_amd.epipolar_pose import build_epipolar_pose_network

        logger.info("Using the epipolar bootstrap (essential matrix per camera pair).")
        return build_epipolar_pose_network(image_points, camera_array, _epi=_epi)
    if not has_object_geometry(image_points):
        raise ValueError("No object geometry (obj_loc all NaN): the PnP path cannot run and the essential-matrix bootstrap "
                         "was not requested; pass method='epipolar' or 'auto', or supply board observations with obj_loc.")
    builder = PoseNetworkBuilder(camera_array, image_points, _pnp=_pnp)
    return builder.estimate_camera_to_object_poses().estimate_relative_poses().filter_outliers(threshold=1.5).build()


__all__ = [
    "StereoPair", "PairedPoseNetwork", "PoseNetworkBuilder", "build_paired_pose_network", "DevicePnP", "ViewPoses", "RelativePoses",
    "compute_camera_to_object_poses_pnp", "compute_relative_poses", "reject_outliers", "aggregate_poses", "quaternion_average",
    "common_observations", "estimate_pnp_paired_pose_network",
]
