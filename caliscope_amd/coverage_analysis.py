"""Camera-pair coverage of a calibration session, the check a user runs before ``calibrate_extrinsics``: which camera pairs share
observations, whether the rig is one connected network, and which cameras hang on a single link.

Host-side mirror of the reference's ``core/coverage_analysis.py`` under the same names: :class:`LinkQuality`,
:class:`WarningSeverity`, :class:`StructuralWarning`, :class:`ExtrinsicCoverageReport`, :func:`compute_coverage_matrix`,
:func:`analyze_multi_camera_coverage`, :func:`classify_link_quality` and :func:`detect_structural_warnings`, with the reference's
thresholds, warning texts and ordering.

Where the work runs: the matrix is the Gram matrix of the binary table keys x cameras, a key being one (``sync_index``,
``object_id``, ``keypoint_id``).  :func:`coverage_keys` turns the three columns into one key index with numpy, and one device call,
``cba_coverage_counts`` (``csrc/coverage_math.h``, ``csrc/coverage_lib.hip``), sets a bit per (camera, key) and sums
``popcount(row_i & row_j)`` per camera pair: no sort, no per-key Python.  Isolated cameras, connected components and leaf cameras
are O(cameras^2) numpy on the returned matrix.  There is no CPU fallback: without the library or a GPU the call raises
``BackendError``.  ``_solver`` replaces the device call (an object with ``coverage_counts``, as :class:`DeviceCoverageCounts`) —
the CPU test-suite passes a g++ build of the same enumeration.

As in the reference, the diagonal counts the distinct keys of a camera (a repeated row counts once), rows of a ``cam_id`` that the
map does not hold are left out, and :func:`analyze_multi_camera_coverage` takes the cameras from the data.  The indices of
``cam_id_to_index`` must be distinct values in ``[0, len(map))`` (``ValueError`` otherwise).
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from enum import Enum

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError

GOOD_OBSERVATION_THRESHOLD = 200
MARGINAL_OBSERVATION_THRESHOLD = 50

# The key index is computed directly from the three columns while their range holds at most max(DENSE_KEYS_PER_ROW * rows,
# DENSE_KEYS_FLOOR) keys (a bit per key and camera: 2**20 keys are 128 KiB per camera); beyond, the keys are compressed first.
DENSE_KEYS_PER_ROW = 8
DENSE_KEYS_FLOOR = 2**20


class LinkQuality(Enum):
    """How well a camera pair is linked, by its number of shared observations."""

    GOOD = "good"  # at least GOOD_OBSERVATION_THRESHOLD
    MARGINAL = "marginal"  # at least MARGINAL_OBSERVATION_THRESHOLD
    INSUFFICIENT = "insufficient"


class WarningSeverity(Enum):
    CRITICAL = "critical"  # the calibration will fail
    WARNING = "warning"  # it may cause trouble
    INFO = "info"


_SEVERITY_RANK = {WarningSeverity.CRITICAL: 0, WarningSeverity.WARNING: 1, WarningSeverity.INFO: 2}


@dataclass(frozen=True)
class StructuralWarning:
    """One structural problem of the camera network."""

    severity: WarningSeverity
    message: str


@dataclass(frozen=True)
class ExtrinsicCoverageReport:
    """Pairwise coverage of a session for the extrinsic calibration: the symmetric count matrix (the heat map), the ``cam_id`` of
    every camera without any shared observation, the number of connected components (1 for a rig that can be calibrated) and the
    cameras with exactly one link as (cam_id, linked cam_id, shared observations)."""

    pairwise_observations: np.ndarray
    isolated_cameras: list[int]
    n_connected_components: int
    leaf_cameras: list[tuple[int, int, int]]

    @property
    def n_cameras(self) -> int:
        return len(self.pairwise_observations)

    @property
    def has_critical_issues(self) -> bool:
        """True when the calibration cannot succeed: an isolated camera, or more than one component."""
        return bool(self.isolated_cameras) or self.n_connected_components > 1


class CoverageDesc(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_keys", C.c_int64), ("n_obs", C.c_int64), ("obs_key", _lib.c_int64_p), ("obs_cam", _lib.c_int32_p),
                ("slab_words", C.c_int64)]


COVERAGE_SIGNATURES = {
    "cba_coverage_counts": (C.c_int, [C.POINTER(CoverageDesc), C.c_int32, _lib.c_int64_p]),
}


def check_coverage_arguments(obs_key, obs_cam, n_cams, n_keys, slab_words):
    """The arrays of a ``coverage_counts`` call in the layout of ``cba_coverage_desc`` (``ValueError`` for mismatched lengths or a
    negative size; the range of every key and camera index is the library's check)."""
    obs_key = np.ascontiguousarray(obs_key, dtype=np.int64).reshape(-1)
    obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    if len(obs_key) != len(obs_cam):
        raise ValueError("coverage_counts: obs_key and obs_cam differ in length")
    if int(n_cams) < 0 or int(n_keys) < 0 or int(slab_words) < 0:
        raise ValueError("coverage_counts: n_cams, n_keys and slab_words must not be negative")
    return obs_key, obs_cam, int(n_cams), int(n_keys), int(slab_words)


class DeviceCoverageCounts:
    """The device call ``cba_coverage_counts`` on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def coverage_counts(self, obs_key, obs_cam, n_cams, n_keys, slab_words=0) -> np.ndarray:
        """``counts[n_cams, n_cams]`` (int64, symmetric): keys in ``[0, n_keys)`` shared by camera i and camera j over the rows
        (``obs_key``, ``obs_cam``); camera -1 is skipped.  ``slab_words``: 64-bit words of the key range per pass (0: the library's
        default); the result does not depend on it."""
        obs_key, obs_cam, n_cams, n_keys, slab_words = check_coverage_arguments(obs_key, obs_cam, n_cams, n_keys, slab_words)
        lib = _lib.bind(_lib.load(), COVERAGE_SIGNATURES)
        counts = np.zeros((n_cams, n_cams), dtype=np.int64)
        desc = CoverageDesc(n_cams=n_cams, n_keys=n_keys, n_obs=len(obs_key), obs_key=_lib.ptr(obs_key),
                            obs_cam=_lib.ptr(obs_cam), slab_words=slab_words)
        _lib.check(lib, lib.cba_coverage_counts(C.byref(desc), self.device_id, _lib.ptr(counts)), "cba_coverage_counts")
        return counts


def coverage_keys(sync_index, object_id, keypoint_id, *, force_unique: bool = False):
    """One key index per row for the triples (sync_index, object_id, keypoint_id): ``(key[rows] int64, n_keys, path)``.

    ``path == "dense"``: ``((sync - s_min) * n_obj + (obj - o_min)) * n_kp + (kp - k_min)`` with the spans of the three columns,
    taken when that range holds at most ``max(DENSE_KEYS_PER_ROW * rows, DENSE_KEYS_FLOOR)`` keys (the spans are Python ints: the
    product cannot overflow unseen).  ``path == "unique"``: the rank of the row's triple among the distinct triples
    (``np.unique``), for tables whose ids are far apart.  Equal triples get equal keys and different triples different keys on
    both paths, which is all the count needs."""
    sync = np.asarray(sync_index, dtype=np.int64).reshape(-1)
    obj = np.asarray(object_id, dtype=np.int64).reshape(-1)
    kp = np.asarray(keypoint_id, dtype=np.int64).reshape(-1)
    rows = len(sync)
    if rows == 0:
        return np.zeros(0, dtype=np.int64), 0, "dense"
    s_min, o_min, k_min = int(sync.min()), int(obj.min()), int(kp.min())
    n_sync, n_obj, n_kp = int(sync.max()) - s_min + 1, int(obj.max()) - o_min + 1, int(kp.max()) - k_min + 1
    total = n_sync * n_obj * n_kp
    if not force_unique and total <= max(DENSE_KEYS_PER_ROW * rows, DENSE_KEYS_FLOOR):
        return ((sync - s_min) * n_obj + (obj - o_min)) * n_kp + (kp - k_min), total, "dense"
    distinct, inverse = np.unique(np.column_stack([sync, obj, kp]), axis=0, return_inverse=True)
    return np.ascontiguousarray(inverse, dtype=np.int64).reshape(-1), len(distinct), "unique"


def _camera_index(cam_id, cam_id_to_index) -> np.ndarray:
    """Matrix index of every row's camera (int32), -1 for a ``cam_id`` outside the map."""
    n = len(cam_id_to_index)
    ids = np.fromiter(cam_id_to_index.keys(), dtype=np.int64, count=n)
    index = np.fromiter(cam_id_to_index.values(), dtype=np.int64, count=n)
    if n and (index.min() < 0 or index.max() >= n or len(np.unique(index)) != n):
        raise ValueError(f"cam_id_to_index must map to distinct indices in [0, {n})")
    by_id = np.argsort(ids, kind="stable")
    ids, index = ids[by_id], index[by_id]
    cam_id = np.asarray(cam_id, dtype=np.int64)
    pos = np.minimum(np.searchsorted(ids, cam_id), n - 1)
    return np.where(ids[pos] == cam_id, index[pos], -1).astype(np.int32)


def compute_coverage_matrix(image_points, cam_id_to_index: dict[int, int], *, device_id: int = 0, _solver=None) -> np.ndarray:
    """The (n, n) symmetric int64 matrix of a session, n = ``len(cam_id_to_index)``: entry [i, j] counts the (sync_index,
    object_id, keypoint_id) triples seen by both the camera at index i and the camera at index j, the diagonal the distinct
    triples of a camera.  Rows of a ``cam_id`` that is not in the map are left out.  One device call; an empty table or an empty
    map returns zeros without one."""
    n = len(cam_id_to_index)
    if n == 0 or len(image_points) == 0:
        return np.zeros((n, n), dtype=np.int64)
    cols = image_points.arrays()
    obs_cam = _camera_index(cols["cam_id"], cam_id_to_index)
    key, n_keys, _ = coverage_keys(cols["sync_index"], cols["object_id"], cols["keypoint_id"])
    backend = _solver or DeviceCoverageCounts(device_id)
    counts = np.asarray(backend.coverage_counts(key, obs_cam, n, n_keys), dtype=np.int64)
    if counts.shape != (n, n):
        raise BackendError(f"coverage_counts returned shape {counts.shape}, expected {(n, n)}")
    return counts


def connected_component_count(linked: np.ndarray) -> int:
    """Number of connected components of the graph with the symmetric boolean adjacency ``linked``: every node takes the smallest
    label among itself and its neighbours, then the label of its label, until nothing changes (whole-matrix steps, no per-node
    loop)."""
    n = len(linked)
    label = np.arange(n)
    while n:
        seen = np.where(linked, label[None, :], n).min(axis=1)
        new = np.minimum(label, seen)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    return len(np.unique(label))


def analyze_multi_camera_coverage(image_points, *, device_id: int = 0, _solver=None) -> ExtrinsicCoverageReport:
    """Pairwise coverage of every camera that occurs in ``image_points`` (sorted ``cam_id``; row and column k of the matrix belong
    to the k-th of them).  The lists of the report name cameras by ``cam_id``."""
    cam_ids = np.unique(image_points.arrays()["cam_id"]) if len(image_points) else np.zeros(0, dtype=np.int64)
    ids = [int(c) for c in cam_ids]
    counts = compute_coverage_matrix(image_points, {c: k for k, c in enumerate(ids)}, device_id=device_id, _solver=_solver)
    linked = counts > 0
    np.fill_diagonal(linked, False)
    degree = linked.sum(axis=1)
    leaf = np.flatnonzero(degree == 1)
    partner = linked[leaf].argmax(axis=1) if len(leaf) else np.zeros(0, dtype=np.int64)
    return ExtrinsicCoverageReport(
        pairwise_observations=counts,
        isolated_cameras=[ids[k] for k in np.flatnonzero(degree == 0)],
        n_connected_components=connected_component_count(linked),
        leaf_cameras=[(ids[k], ids[p], int(counts[k, p])) for k, p in zip(leaf.tolist(), partner.tolist())],
    )


def classify_link_quality(observation_count: int) -> LinkQuality:
    """GOOD from 200 shared observations, MARGINAL from 50, INSUFFICIENT below."""
    if observation_count >= GOOD_OBSERVATION_THRESHOLD:
        return LinkQuality.GOOD
    if observation_count >= MARGINAL_OBSERVATION_THRESHOLD:
        return LinkQuality.MARGINAL
    return LinkQuality.INSUFFICIENT


def detect_structural_warnings(report: ExtrinsicCoverageReport, n_cameras: int, min_leaf_observations: int = 100) -> list[StructuralWarning]:
    """The structural problems of a report a user can act on, critical ones first: every isolated camera and a network of several
    groups are CRITICAL; in a rig of more than two cameras (in one of two both are leaves by necessity) a leaf camera is a WARNING
    below ``min_leaf_observations`` shared observations and an INFO from there on.  Within a severity the order is that of the
    report's lists."""
    found = [StructuralWarning(WarningSeverity.CRITICAL, f"Camera C{cam_id} has no shared observations with any other camera")
             for cam_id in report.isolated_cameras]
    if report.n_connected_components > 1:
        found.append(StructuralWarning(WarningSeverity.CRITICAL, f"Camera network has {report.n_connected_components} disconnected groups"))
    if n_cameras > 2:
        for cam_id, linked_to, count in report.leaf_cameras:
            if count < min_leaf_observations:
                found.append(StructuralWarning(WarningSeverity.WARNING, f"Camera C{cam_id} only connected to C{linked_to} ({count} obs)"))
            else:
                found.append(StructuralWarning(WarningSeverity.INFO, f"Camera C{cam_id} connects only through C{linked_to}"))
    return sorted(found, key=lambda w: _SEVERITY_RANK[w.severity])  # stable


__all__ = ["LinkQuality", "WarningSeverity", "StructuralWarning", "ExtrinsicCoverageReport", "DeviceCoverageCounts", "compute_coverage_matrix",
           "analyze_multi_camera_coverage", "classify_link_quality", "detect_structural_warnings", "coverage_keys", "connected_component_count",
           "GOOD_OBSERVATION_THRESHOLD", "MARGINAL_OBSERVATION_THRESHOLD"]
