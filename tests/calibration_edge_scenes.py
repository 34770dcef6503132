"""Scenes for the launch and tie edges of frame selection (k_frame_features, k_frame_select) and intrinsic calibration
(k_intrinsics), built from tests/intrinsic_scenes.camera_scene.  TEST INFRASTRUCTURE: scenes only, seeded and cached; the checks
are in tests/test_calibration_edge_scenes.py (g++ build) and tests/test_calibration_kernel_edges_gpu.py (device).

Frame selection.  k_frame_select runs SELECT_BLOCK = 256 threads per camera: thread t takes frames t, t + 256, ... and the
workgroup argmax folds 64-lane waves first and the four waves after.  A camera of nf frames that holds base[i % 64] at frame i puts
bit-identical twins of every frame into other waves (f + 64, f + 128, f + 192) and into later passes of the same thread (f + 256,
f + 512); "lowest frame on ties" then decides every round.  k_frame_features runs one thread per frame in blocks of 64.

Intrinsic calibration.  k_intrinsics runs REFINE_BLOCK = 128 threads per camera: thread t takes views t, t + 128, ... of the
camera's list; 127 / 128 / 129 views leave the last lane empty, fill it, and wrap to a second pass, 257 views give lane 0 three.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle.camera_model import project_pinhole, rodrigues
from tests import intrinsic_scenes as S

K_BASE = 64                                   # distinct base frames of a twin camera
TWIN_COUNTS = (64, 63, 65, 255, 256, 257, 513)
TWIN_TARGETS = (1, 5, 8, 30, 200)
ELIGIBILITY_COUNTS = (255, 256, 257)
CUT_CORNERS = 5                               # below min_corners = 6
SEL_SEED = 101                                # (re-seeded when a scene breaks the margin condition, never the floor lowered)
FRONTAL_SEED = 7
HALF_SEED = 11
PINHOLE_SEED, FISHEYE_SEED = 201, 202
INTR_BOARD = dict(rows=4, cols=5, spacing=0.06, min_corners=8, noise=0.3)
PINHOLE_COUNTS = (127, 128, 129, 257)
FISHEYE_COUNTS = (127, 128, 129)


# ---- frame selection ------------------------------------------------------------------------------------------------------------------

@dataclass
class SelCall:
    """One select_frames call: the CSR arguments, and per frame the identity of its content (frames with equal ``content`` hold the
    same rows bit for bit)."""

    labels: list
    cam_frame_start: np.ndarray
    cam_size: np.ndarray
    frame_start: np.ndarray
    obs_xy: np.ndarray
    obs_obj: np.ndarray
    content: np.ndarray

    @property
    def args(self):
        return self.cam_frame_start, self.cam_size, self.frame_start, self.obs_xy, self.obs_obj

    @property
    def corners(self):
        return np.diff(self.frame_start)

    def camera(self, label):
        """(first frame, end frame) of the camera ``label``."""
        c = self.labels.index(label)
        return int(self.cam_frame_start[c]), int(self.cam_frame_start[c + 1])


@dataclass(frozen=True)
class Frame:
    key: int            # identity of the content
    xy: np.ndarray      # [n, 2] pixels
    obj: np.ndarray     # [n, 2] board x, y


def sel_call(cameras) -> SelCall:
    """``cameras``: list of (label, [Frame])."""
    frames = [f for _, fs in cameras for f in fs]
    counts = [len(fs) for _, fs in cameras]
    sizes = [len(f.xy) for f in frames]
    return SelCall([label for label, _ in cameras], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                   np.tile(np.array(S.SIZE, float), (len(cameras), 1)), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                   np.concatenate([f.xy for f in frames]) if frames else np.zeros((0, 2)),
                   np.concatenate([f.obj for f in frames]) if frames else np.zeros((0, 2)), np.array([f.key for f in frames], np.int64))


@functools.cache
def base_scene():
    return S.camera_scene(SEL_SEED, n_views=K_BASE, noise=0.3)


@functools.cache
def base_frames():
    """The 64 distinct frames (6 x 9 board, 0.3 px noise); frame k has content key k."""
    return tuple(Frame(k, uv.copy(), X[:, :2].copy()) for k, (X, uv, _, _) in enumerate(base_scene().views))


def cut(frame: Frame, n=CUT_CORNERS) -> Frame:
    """The frame with n corners left: its first three and its last n - 3 (two board rows, so the homography still has a fit)."""
    idx = np.r_[0:3, len(frame.xy) - (n - 3):len(frame.xy)]
    return Frame(frame.key + 1000, frame.xy[idx].copy(), frame.obj[idx].copy())


@functools.cache
def frontal_frame() -> Frame:
    """A near-frontal board on the optical axis (the recipe of the selection fixtures' "frontal only" table: tilt 0.004 rad, noise
    0.05 px): tilt magnitude far below FSEL_MIN_TILT, so it falls into no tilt bin."""
    rng = np.random.default_rng(FRONTAL_SEED)
    sc = base_scene()
    grid = S.board()
    rv = rng.normal(0, 0.004, 3)
    t = np.array([0.0, 0.0, 0.8]) - rodrigues(rv) @ grid.mean(0)
    K = np.array([[sc.intr[0], 0.0, sc.intr[2]], [0.0, sc.intr[1], sc.intr[3]], [0.0, 0.0, 1.0]])
    uv, _ = project_pinhole(grid, rv, t, K, sc.dist)
    return Frame(2000, uv + rng.normal(0, 0.05, uv.shape), grid[:, :2].copy())


def most_tilted_base() -> int:
    """The base frame whose true rotation tilts the board most (about x and y)."""
    return int(np.argmax([np.hypot(rv[0], rv[1]) for _, _, rv, _ in base_scene().views]))


def twin_camera(nf):
    base = base_frames()
    return [base[i % K_BASE] for i in range(nf)]


@functools.cache
def twin_call() -> SelCall:
    """The cameras nf = 64, 63, 65, 255, 256, 257, 513 with an empty camera between them: 1473 = 23 * 64 + 1 frames."""
    cams = [(f"twin{nf}", twin_camera(nf)) for nf in TWIN_COUNTS]
    cams.insert(3, ("empty", []))
    return sel_call(cams)


@functools.cache
def block_call() -> SelCall:
    """The 64-frame camera alone: a frame total of exactly one block of k_frame_features."""
    return sel_call([("twin64", twin_camera(64))])


@functools.cache
def late_call() -> SelCall:
    """late257: 256 copies of the frontal frame, then the only tilted frame.  late513: 449 copies of the frontal frame, then the
    64 base frames at 449..512.  one257: 257 copies of one tilted frame.  An empty camera and a camera whose frames are all below
    min_corners sit between them."""
    dull, base = frontal_frame(), base_frames()
    tilted = base[most_tilted_base()]
    return sel_call([("late257", [dull] * 256 + [tilted]), ("empty", []), ("one257", [tilted] * 257),
                     ("ineligible", [cut(f) for f in twin_camera(66)]), ("late513", [dull] * 449 + list(base))])


@functools.cache
def eligibility_call() -> SelCall:
    """The 255 / 256 / 257 twin cameras with every frame of a seeded random half cut to 5 corners, an empty and an all-ineligible
    camera between them (run with min_corners 6 and 0)."""
    rng = np.random.default_rng(HALF_SEED)
    cams = []
    for nf in ELIGIBILITY_COUNTS:
        half = set(rng.permutation(nf)[:nf // 2].tolist())
        cams.append((f"half{nf}", [cut(f) if i in half else f for i, f in enumerate(twin_camera(nf))]))
    cams.insert(1, ("empty", []))
    cams.insert(3, ("ineligible", [cut(f) for f in twin_camera(70)]))
    return sel_call(cams)


# ---- intrinsic calibration -------------------------------------------------------------------------------------------------------------

@functools.cache
def pinhole_scene():
    return S.camera_scene(PINHOLE_SEED, n_views=257, **INTR_BOARD)


@functools.cache
def fisheye_scene():
    return S.camera_scene(FISHEYE_SEED, n_views=129, fisheye=True, **INTR_BOARD)


def with_views(scene, views):
    return S.CameraScene(scene.fisheye, scene.size, scene.intr, scene.dist, list(views))


def prefix(scene, n):
    return with_views(scene, scene.views[:n])


def cut_view(view, idx):
    X, uv, rv, t = view
    idx = np.asarray(idx)
    return X[idx].copy(), uv[idx].copy(), rv, t


def with_cut(scene, which, n=3):
    """The scene with the views ``which`` cut to their first n corners (n = 3: PNP_TOO_FEW)."""
    views = list(scene.views)
    for v in which:
        views[v] = cut_view(views[v], np.arange(n))
    return with_views(scene, views)


def moved_fisheye(scene, v=128):
    """The fisheye scene with view v shifted along x until its farthest corner lies at 1.6 (> INTR_MAX_THETA_D = 1.5) start focal
    lengths from the start principal point: the view keeps all its corners and is left out by the theta screen (PNP_FAILED)."""
    w, h = scene.size
    f0, cx, cy = max(w, h) / np.pi, 0.5 * w - 0.5, 0.5 * h - 0.5   # intr_start of intrinsic_math.h
    X, uv, rv, t = scene.views[v]
    far = int(np.argmax(uv[:, 0]))
    dy = (uv[far, 1] - cy) / f0
    shift = cx + f0 * np.sqrt(1.6 ** 2 - dy ** 2) - uv[far, 0]
    views = list(scene.views)
    views[v] = (X, uv + np.array([shift, 0.0]), rv, t)
    return with_views(scene, views)


def two_row_corners(view, n):
    """Indices of n corners of a view from two board rows (the first corners of one row are collinear and the PnP then fails):
    ceil(n / 2) from the view's first row and the rest from its last."""
    X = view[0]
    first, last = np.flatnonzero(np.isclose(X[:, 1], X[0, 1])), np.flatnonzero(np.isclose(X[:, 1], X[-1, 1]))
    a = (n + 1) // 2
    assert len(first) >= a and len(last) >= n - a and not np.isclose(X[0, 1], X[-1, 1])
    return np.r_[first[:a], last[:n - a]]


def boundary_camera(scene, total):
    """Three views of ``scene`` cut to ``total`` corners together (each at least 4, from two board rows)."""
    per = [total - 2 * (total // 3), total // 3, total // 3]
    full = [v for v in scene.views if len(v[0]) == 20][:3]
    return with_views(scene, [cut_view(v, two_row_corners(v, n)) for v, n in zip(full, per)])


@functools.cache
def size_scenes():
    """Pinhole cameras of 127, 128, 129 and 257 views and fisheye cameras of 127, 128 and 129: prefixes of the two scenes."""
    return tuple([prefix(pinhole_scene(), n) for n in PINHOLE_COUNTS] + [prefix(fisheye_scene(), n) for n in FISHEYE_COUNTS])


@functools.cache
def screened_scenes():
    """(labels, scenes, {camera: expected non-zero view statuses {view: status}}).  Each 129-view camera with view 127, view 128 and
    views 0 + 128 cut to 3 corners; the fisheye camera with view 127 or 128 moved beyond the theta
    screen; a camera without views and a
    2-view camera between them."""
    pin, fish = prefix(pinhole_scene(), 129), fisheye_scene()
    labels, scenes, expect = [], [], {}
    for name, sc in (("pinhole", pin), ("fisheye", fish)):
        for which in ((127,), (128,), (0, 128)):
            expect[len(scenes)] = {v: 1 for v in which}
            labels.append(f"{name} cut {which}")
            scenes.append(with_cut(sc, which))
        if name == "pinhole":
            labels += ["no views", "two views"]
            scenes += [with_views(pin, []), prefix(pin, 2)]
    for v in (127, 128):  # (all but one view have 20 corners, so these sit on the last lane and on the wrap of the sorted list too)
        expect[len(scenes)] = {v: 2}
        labels.append(f"fisheye moved {v}")
        scenes.append(moved_fisheye(fish, v))
    return labels, tuple(scenes), expect


@functools.cache
def boundary_scenes():
    """(labels, scenes): 3-view cameras at the too-few boundary 2 * corners = NI + 6 * 3 (pinhole NI = 9: 13 corners too few, 14
    not; fisheye NI = 8: 12 too few, 13 not), a 3-view camera with one view screened out, and a healthy 3-view camera."""
    pin, fish = pinhole_scene(), fisheye_scene()
    return (["pinhole 13", "pinhole 14", "fisheye 12", "fisheye 13", "pinhole 3 views, one cut", "pinhole 3 views"],
            (boundary_camera(pin, 13), boundary_camera(pin, 14), boundary_camera(fish, 12), boundary_camera(fish, 13),
             with_cut(prefix(pin, 3), (1,)), prefix(pin, 3)))


def pack_permuted(scenes, seed):
    """``intrinsic_scenes.pack`` with the views of all cameras in a seeded random order (``view_cam`` unsorted, a camera's views
    interleaved with the others'): the same call by the C ABI.  Returns (pack arguments, perm) with packed view i = view perm[i] of
    the contiguous packing."""
    model, size, start, cam, xy, obj = S.pack(scenes)
    perm = np.random.default_rng(seed).permutation(len(cam))
    n = np.diff(start)
    new_start = np.concatenate([[0], np.cumsum(n[perm])]).astype(np.int64)
    rows = np.concatenate([np.arange(start[v], start[v + 1]) for v in perm]) if len(perm) else np.zeros(0, np.int64)
    return (model, size, new_start, cam[perm], xy[rows], obj[rows]), perm


def too_few_rule(scenes, vcam, vstart, view_status):
    """INTR_TOO_FEW per camera by the rule of intrinsic_math.h on the returned view statuses: with ``usable`` the camera's views of
    status 0 and ``corners`` their corner total, ``usable < 3 or 2 * corners < NI + 6 * usable`` (NI 9 pinhole, 8 fisheye)."""
    n = np.diff(vstart)
    out = []
    for c, sc in enumerate(scenes):
        ok = (np.asarray(vcam) == c) & (np.asarray(view_status) == 0)
        usable, corners, ni = int(ok.sum()), int(n[ok].sum()), 8 if sc.fisheye else 9
        out.append(usable < 3 or 2 * corners < ni + 6 * usable)
    return np.array(out)
