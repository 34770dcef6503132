"""Inputs for the four pose-bootstrap calls (cba_pose_pnp_batch, cba_pose_pair_rmse, cba_pose_essential_batch,
cba_pose_resect_batch) at the shape edges of their kernels, in the CSR form of the C ABI and built from ground-truth poses, and
plain-numpy references (np.longdouble, no shared header) for what the calls return.  Sizes follow the kernels' constants, read
from the sources: tests/test_pose_edge_scenes.py checks the scenes' properties on the g++ build,
tests/test_pose_kernel_edges_gpu.py runs them on the device."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LD = np.longdouble


def _constants():
    out = {}
    for path, names in ((ROOT / "caliscope_amd" / "csrc" / "pose_lib.hip", ("POSE_BLOCK", "PAIR_BLOCK", "HYP_BLOCK", "SCORE_BLOCK", "SCORE_PER_LANE",
                                                                          "SCORE_CHUNK")),
                        (ROOT / "caliscope_amd" / "csrc" / "epipolar_math.h", ("EPI_REDUCE_NT", "EPI_SAMPLE", "RES_SAMPLE"))):
        text = path.read_text()
        for name in names:
            m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", text)
            if m is None:
                raise RuntimeError(f"{path.name} no longer defines `constexpr int {name} = <number>;`: the edge scenes take their sizes from it")
            out[name] = int(m.group(1))
    return out


K = _constants()
POSE_BLOCK, PAIR_BLOCK, HYP_BLOCK = K["POSE_BLOCK"], K["PAIR_BLOCK"], K["HYP_BLOCK"]
SCORE_BLOCK, SCORE_PER_LANE, SCORE_CHUNK = K["SCORE_BLOCK"], K["SCORE_PER_LANE"], K["SCORE_CHUNK"]
EPI_REDUCE_NT, EPI_SAMPLE, RES_SAMPLE = K["EPI_REDUCE_NT"], K["EPI_SAMPLE"], K["RES_SAMPLE"]
TILE = SCORE_BLOCK * SCORE_PER_LANE  # items of one job that one k_score workgroup takes
GRID_Y_MAX = 65535                   # jobs beyond it are reached by the `j += gridDim.y` loop
DIST_THRESH = 50.0                   # epi_in_front: depth in (0, 50) in both views
GATE_BAND = 1e-6                     # relative distance from a gate inside which two builds may decide differently

# camera table: a distorted pinhole, a fisheye and an ideal pinhole camera, all f ~ 1600
CAM_MODEL = np.array([0, 1, 0], dtype=np.int32)
CAM_INTR = np.array([[1600.0, 1590.0, 960.0, 540.0, 0.1, -0.2, 0.001, 0.002, 0.05],
                     [1600.0, 1600.0, 970.0, 530.0, 0.05, -0.01, 0.002, -0.0005, 0.0],
                     [1610.0, 1600.0, 950.0, 545.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
FOCAL = 1600.0
ESS_THR = 3.0 / FOCAL    # the product's 3-pixel Sampson gate
RES_THR = 3.0 / 1000.0   # the gate of tests/test_epipolar_bootstrap_gpu.py's resection jobs
IDENTITY_POSE = np.concatenate([np.eye(3).ravel(), np.zeros(3)])


def rotations(rvec):
    """Rodrigues: rvec[..., 3] -> R[..., 3, 3]."""
    rvec = np.asarray(rvec, dtype=np.float64)
    th = np.linalg.norm(rvec, axis=-1)[..., None, None]
    k = rvec / np.maximum(np.linalg.norm(rvec, axis=-1, keepdims=True), 1e-300)
    Kx = np.zeros(rvec.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def to_pixels(model, k9, xy):
    """Normalised points through the camera's distortion model (0: k1 k2 p1 p2 k3, 1: fisheye k1..k4) to pixels."""
    x, y = xy[:, 0], xy[:, 1]
    fx, fy, cx, cy = k9[:4]
    if model == 0:
        k1, k2, p1, p2, k3 = k9[4:9]
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2**2 + k3 * r2**3
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    else:
        k1, k2, k3, k4 = k9[4:8]
        r = np.hypot(x, y)
        th = np.arctan(r)
        thd = th * (1 + k1 * th**2 + k2 * th**4 + k3 * th**6 + k4 * th**8)
        s = np.where(r > 1e-12, thd / np.maximum(r, 1e-12), 1.0)
        xd, yd = x * s, y * s
    return np.column_stack([fx * xd + cx, fy * yd + cy])


def random_motion(rng):
    """(R, unit t) of camera B in camera A's frame: a sideways baseline with a moderate turn."""
    R = rotations(rng.normal(0, 0.25, 3))
    t = np.array([1.0, 0.0, 0.0]) + rng.normal(0, 0.25, 3)
    return R, t / np.linalg.norm(t)


def _view_points(rng, n):
    return np.column_stack([rng.uniform(-1.3, 1.3, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 7.0, n)])


def _two_views(X, R, t):
    Xb = X @ R.T + t
    return X[:, :2] / X[:, 2:], Xb[:, :2] / Xb[:, 2:]


def essential_pair(rng, n, cams, noise_px=0.5, outliers=0.0, kind="rigid"):
    """One camera pair: normalised points of both views (before the camera models), its cameras and its true motion.
    kind: "rigid", "random" (no geometry at all) or "same" (one correspondence repeated n times)."""
    R, t = random_motion(rng)
    a, b = _two_views(_view_points(rng, n), R, t)
    if kind == "random":
        a, b = rng.uniform(-0.35, 0.35, (n, 2)), rng.uniform(-0.35, 0.35, (n, 2))
    elif kind == "same":
        a, b = np.repeat(a[:1], n, axis=0), np.repeat(b[:1], n, axis=0)
        noise_px = 0.0
    bad = rng.random(n) < outliers
    b[bad] = rng.uniform(-0.35, 0.35, (int(bad.sum()), 2))
    return dict(a=a, b=b, cams=cams, noise=rng.normal(0, 1.0, (2, n, 2)) * noise_px, R=R, t=t, kind=kind, outlier=bad)


def essential_call(pairs):
    """Pairs -> the arguments of essential_batch up to `threshold` (each pair has observation rows of its own: view A's, then
    view B's) and the list of truths."""
    xy, cam, ca, cb, start, row = [], [], [], [], [0], 0
    for p in pairs:
        n = len(p["a"])
        for k, (side, c) in enumerate(zip(("a", "b"), p["cams"])):
            xy.append(to_pixels(CAM_MODEL[c], CAM_INTR[c], p[side]) + p["noise"][k])
            cam.append(np.full(n, c, dtype=np.int32))
        ca.append(np.arange(row, row + n)); cb.append(np.arange(row + n, row + 2 * n))
        row += 2 * n
        start.append(start[-1] + n)
    cat = lambda parts, dt, shape: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dtype=dt)  # noqa: E731
    return (CAM_MODEL, CAM_INTR, cat(xy, np.float64, (0, 2)), cat(cam, np.int32, 0), np.array(start, dtype=np.int64), cat(ca, np.int64, 0),
            cat(cb, np.int64, 0), np.full(len(pairs), ESS_THR))


CAM_PAIRS = [(0, 1), (1, 2), (0, 2), (2, 1), (1, 0), (1, 1)]
MIXED_SIZES = [0, 7, 8, 9, 127, 128, 129, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE - 3]
MIXED_N_HYP = (1, 63, 128, 129, 300)
MIXED_SEED = 7


# An 8-point fit to 8 or 9 points with 0.5 px noise, projected onto the essential manifold, seldom keeps all of them inside the
# 3 px gate (about one draw in thirty does): the draws of these two pairs are chosen so that it does, and
# tests/test_pose_edge_scenes.py asserts that they end with status 0.
MIXED_SUBSEED = {2: 3, 3: 3}


def mixed_essential_scene(seed=11, subseed=None, upto=None):
    """Pairs of every size around the kernels' block sizes in one call, a pair of random points and a pair of one repeated
    correspondence (both must fail), the largest pair last.  0.5 px noise; 20 % gross outliers from 127 correspondences up."""
    sub = dict(MIXED_SUBSEED if subseed is None else subseed)
    rng = lambda i: np.random.default_rng([seed, i, sub.get(i, 0)])  # noqa: E731
    sizes = MIXED_SIZES[:upto]
    pairs = [essential_pair(rng(i), n, CAM_PAIRS[i % len(CAM_PAIRS)], outliers=0.2 if n >= 127 else 0.0) for i, n in enumerate(sizes)]
    if upto is None:
        k = len(pairs)
        pairs.append(essential_pair(rng(k), 40, (0, 1), kind="random"))
        pairs.append(essential_pair(rng(k + 1), 50, (1, 2), kind="same"))
        pairs.append(essential_pair(rng(k + 2), 3 * TILE + 517, (0, 1), outliers=0.2))
    args = essential_call(pairs)
    sizes = np.diff(args[4])
    return dict(args=args, pairs=pairs, sizes=sizes, too_few=np.flatnonzero(sizes < EPI_SAMPLE), failed=np.array([len(MIXED_SIZES), len(MIXED_SIZES) + 1]),
                good=np.array([j for j, p in enumerate(pairs) if sizes[j] >= 127 and p["kind"] == "rigid"]))


# ---- "the tail decides" ------------------------------------------------------------------------------------------------------
TAIL_N, TAIL_A, TAIL_N_HYP = 2000, 900, 1024


def _tail_layout(rng):
    """is_a[TAIL_N]: TAIL_A items of motion A shuffled into the first TILE items, every other item motion B."""
    is_a = np.zeros(TAIL_N, dtype=bool)
    is_a[rng.permutation(TILE)[:TAIL_A]] = True
    return is_a


MOTION_A = (rotations(np.array([0.05, -0.30, 0.10])), np.array([0.96, 0.10, 0.26]) / np.linalg.norm([0.96, 0.10, 0.26]))
MOTION_B = (rotations(np.array([-0.10, 0.35, -0.05])), np.array([0.90, -0.30, -0.31]) / np.linalg.norm([0.90, -0.30, -0.31]))
TAIL_ESS = dict(seed=7, shuffle=0, noise_px=0.3)
TAIL_RES = dict(seed=3, shuffle=1, noise=3e-4)
RES_MOTION_A = (rotations(np.array([0.3, -0.2, 0.1])), np.array([0.2, -0.1, 5.0]))
RES_MOTION_B = (rotations(np.array([-0.25, 0.3, -0.4])), np.array([-0.3, 0.2, 5.5]))


def tail_essential_scene(shuffle=None, noise_px=None):
    """One pair of TAIL_N correspondences of two rigid motions: A has the majority inside the first TILE items, B overall."""
    shuffle = TAIL_ESS["shuffle"] if shuffle is None else shuffle
    noise_px = TAIL_ESS["noise_px"] if noise_px is None else noise_px
    rng = np.random.default_rng(1000 + shuffle)
    is_a = _tail_layout(rng)
    X = _view_points(rng, TAIL_N)
    a, bA = _two_views(X, *MOTION_A)
    _, bB = _two_views(X, *MOTION_B)
    pair = dict(a=a, b=np.where(is_a[:, None], bA, bB), cams=(0, 1), noise=rng.normal(0, 1.0, (2, TAIL_N, 2)) * noise_px, R=MOTION_B[0],
                t=MOTION_B[1], kind="rigid")
    return dict(args=essential_call([pair]), is_a=is_a, n_hyp=TAIL_N_HYP, seed=TAIL_ESS["seed"])


def tail_resection_scene(shuffle=None, noise=None):
    shuffle = TAIL_RES["shuffle"] if shuffle is None else shuffle
    noise = TAIL_RES["noise"] if noise is None else noise
    rng = np.random.default_rng(2000 + shuffle)
    is_a = _tail_layout(rng)
    X = rng.uniform(-1, 1, (TAIL_N, 3))
    uv = np.zeros((TAIL_N, 2))
    for sel, (R, t) in ((is_a, RES_MOTION_A), (~is_a, RES_MOTION_B)):
        Y = X[sel] @ R.T + t
        uv[sel] = Y[:, :2] / Y[:, 2:]
    uv += rng.normal(0, noise, uv.shape)
    args = (np.array([0, TAIL_N], dtype=np.int64), X, uv, np.array([RES_THR]))
    return dict(args=args, is_a=is_a, n_hyp=TAIL_N_HYP, seed=TAIL_RES["seed"], min_points=6)


def pure_draws(is_a, n_hyp, seed, k):
    """(hypotheses drawn from A only, from B only) of job 0."""
    from tests.epipolar_native import sample

    draws = np.array([is_a[sample(seed, 0, h, len(is_a), k)].sum() for h in range(n_hyp)])
    return np.flatnonzero(draws == k), np.flatnonzero(draws == 0)


# ---- many small jobs ---------------------------------------------------------------------------------------------------------
MANY_JOBS = 70_000
MANY_N_HYP = 4


def many_resection_jobs(n_jobs=MANY_JOBS, seed=21):
    """n_jobs resection jobs of 8 clean points each (more jobs than the grid's y extent)."""
    rng = np.random.default_rng(seed)
    n = 8
    X = rng.uniform(-1, 1, (n_jobs, n, 3))
    R = rotations(rng.normal(0, 0.5, (n_jobs, 3)))
    t = np.array([0.0, 0.0, 5.0]) + rng.normal(0, 0.3, (n_jobs, 3))
    Y = np.einsum("jrc,jnc->jnr", R, X) + t[:, None, :]
    uv = Y[..., :2] / Y[..., 2:] + rng.normal(0, 1e-4, (n_jobs, n, 2))
    start = np.arange(n_jobs + 1, dtype=np.int64) * n
    return dict(args=(start, X.reshape(-1, 3), uv.reshape(-1, 2), np.full(n_jobs, RES_THR)), R=R, t=t, n_hyp=MANY_N_HYP, min_points=6, seed=5)


def many_essential_pairs(n_pairs=MANY_JOBS, seed=22):
    """n_pairs pairs of 8 to 12 exact correspondences (no noise: a minimal fit to noisy points seldom keeps them all inside the gate
    once projected onto the manifold), cameras 0 (pinhole) and 1 (fisheye)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(8, 13, n_pairs)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    job = np.repeat(np.arange(n_pairs), sizes)
    R = rotations(rng.normal(0, 0.25, (n_pairs, 3)))
    t = np.array([1.0, 0.0, 0.0]) + rng.normal(0, 0.25, (n_pairs, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    X = _view_points(rng, len(job))
    Xb = np.einsum("nrc,nc->nr", R[job], X) + t[job]
    a, b = X[:, :2] / X[:, 2:], Xb[:, :2] / Xb[:, 2:]
    n = len(job)
    xy = np.concatenate([to_pixels(0, CAM_INTR[0], a), to_pixels(1, CAM_INTR[1], b)])
    cam = np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)])
    args = (CAM_MODEL, CAM_INTR, xy, cam, start, np.arange(n, dtype=np.int64), np.arange(n, 2 * n, dtype=np.int64), np.full(n_pairs, ESS_THR))
    return dict(args=args, R=R, t=t, n_hyp=MANY_N_HYP, seed=9)


# ---- resection edges -----------------------------------------------------------------------------------------------------------
RES_MIN_POINTS = 20
RES_SIZES = [5, 6, 7, RES_MIN_POINTS - 1, RES_MIN_POINTS, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
RES_N_HYP = (1, 100, 200)


def resection_edge_scene(seed=31):
    """Jobs below RES_SAMPLE, between it and min_points, at min_points, around one and several tiles (20 % outliers from TILE - 1
    up), a job of coincident points and a job of random points (both must fail), mixed in one call."""
    rng = np.random.default_rng(seed)
    objs, uvs, truth = [], [], []
    for n in RES_SIZES + [40, 60]:
        X = rng.uniform(-1, 1, (n, 3))
        R, t = rotations(rng.normal(0, 0.5, 3)), np.array([0, 0, 5.0]) + rng.normal(0, 0.3, 3)
        kind = "rigid" if len(objs) < len(RES_SIZES) else ("same" if len(objs) == len(RES_SIZES) else "random")
        if kind == "same":
            X = np.repeat(X[:1], n, axis=0)
        Y = X @ R.T + t
        uv = Y[:, :2] / Y[:, 2:] + rng.normal(0, 3e-4, (n, 2))
        if kind == "random":
            uv = rng.uniform(-0.3, 0.3, (n, 2))
        if n >= TILE - 1:
            bad = rng.random(n) < 0.2
            uv[bad] += rng.uniform(-0.1, 0.1, (int(bad.sum()), 2))
        objs.append(X); uvs.append(uv); truth.append((R, t))
    sizes = np.array([len(o) for o in objs])
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    nr = len(RES_SIZES)
    return dict(args=(start, np.concatenate(objs), np.concatenate(uvs), np.full(len(sizes), RES_THR)), truth=truth, sizes=sizes,
                min_points=RES_MIN_POINTS, seed=3, too_few=np.flatnonzero(sizes[:nr] < RES_MIN_POINTS), failed=np.array([nr, nr + 1]),
                good=np.flatnonzero(sizes[:nr] >= RES_MIN_POINTS))


# ---- PnP batch and pair RMSE -----------------------------------------------------------------------------------------------------
PNP_VIEW_COUNTS = (1, POSE_BLOCK - 1, POSE_BLOCK, POSE_BLOCK + 1, 1000)
PNP_INTR = np.array([[1400.0, 1390.0, 960.0, 540.0, 0.1, -0.2, 0.001, 0.002, 0.05], [900.0, 900.0, 640.0, 360.0, 0.05, 0.01, 0.02, -0.01, 0.0],
                     [1100.0, 1100.0, 960.0, 540.0, 0.05, -0.01, 0.002, -0.0005, 0.0]])
PNP_MODEL = np.array([0, 0, 1], dtype=np.int32)


def pnp_views(n_views, seed=3, big=None, empty=None):
    """Board views as tests/test_pose_bootstrap_gpu.py builds them (planar at z = 0 / z = const, non-planar, too few,
    collinear) over a camera table whose third entry is a fisheye camera, plus planar views of 5 points (solved with
    min_points = 4, too few with 6); view `empty` has no observation, view `big` 5000.
    Returns the arguments of pnp_batch up to obs_obj and the true (R, t) of every view."""
    rng = np.random.default_rng(seed)
    sizes, obj, xy, cam, truth, kinds = [], [], [], [], [], []
    for v in range(n_views):
        kind = v % 5 if n_views > 1 else 0
        n = 3 if v % 10 == 7 else int(rng.integers(8, 60))
        if v % 10 == 2 and n_views > 1:
            n = 5  # a planar view between min_points = 4 and 6
        if v == big:
            n, kind = 5000, 3
        if v == empty:
            n = 0
        if kind == 3:
            P = rng.uniform(-0.2, 0.2, (n, 3))
        else:
            P = np.column_stack([rng.uniform(0, 0.3, (n, 2)), np.full(n, 0.006 * (kind == 1))])
        if kind == 4:
            P[:, 1] = 0.0  # collinear
        R = rotations(rng.normal(0, 0.5, 3))
        t = np.array([0.0, 0.0, 1.5]) - R @ (P.mean(0) if n else np.zeros(3))
        Xc = P @ R.T + t
        uv = Xc[:, :2] / Xc[:, 2:] + rng.normal(0, 5e-4, (n, 2))
        c = v % 3
        sizes.append(n); obj.append(P); xy.append(to_pixels(PNP_MODEL[c], PNP_INTR[c], uv)); cam.append(c); truth.append((R, t)); kinds.append(kind)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return dict(args=(start, np.array(cam, np.int32), PNP_MODEL, PNP_INTR, np.concatenate(xy), np.concatenate(obj)), truth=truth,
                kinds=np.array(kinds), sizes=np.array(sizes))


PAIR_SIZES = (0, PAIR_BLOCK - 1, PAIR_BLOCK, PAIR_BLOCK + 1, 4, 1000, 0)


def pair_rmse_scene(seed=8):
    rng = np.random.default_rng(seed)
    poses, A, B = [], [], []
    for m in PAIR_SIZES:
        R = rotations(rng.normal(0, 0.4, 3))
        t = np.array([0.8, 0.05, 0.1]) + rng.normal(0, 0.05, 3)
        X = rng.uniform(-0.3, 0.3, (m, 3)) + [0, 0, 2.0]
        a = X[:, :2] / X[:, 2:] + rng.normal(0, 1e-3, (m, 2))
        Xb = X @ R.T + t
        b = Xb[:, :2] / Xb[:, 2:] + rng.normal(0, 1e-3, (m, 2))
        poses.append(np.concatenate([R.ravel(), t])); A.append(a); B.append(b)
    start = np.concatenate([[0], np.cumsum(PAIR_SIZES)]).astype(np.int64)
    return dict(args=(np.stack(poses), start, np.concatenate(A), np.concatenate(B)), A=A, B=B)


# ---- plain numpy references ------------------------------------------------------------------------------------------------------
def rotation_angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def direction_angle_deg(ta, tb):
    c = float(ta @ tb) / (np.linalg.norm(ta) * np.linalg.norm(tb))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def sampson_ld(pose, a, b):
    """Squared Sampson distances under E = [t]x R, in np.longdouble (a, b: [n, 2] normalised)."""
    R, t = pose[:9].reshape(3, 3).astype(LD), pose[9:].astype(LD)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], dtype=LD)
    E = tx @ R
    xa = np.column_stack([a.astype(LD), np.ones(len(a), dtype=LD)])
    xb = np.column_stack([b.astype(LD), np.ones(len(b), dtype=LD)])
    Ea, Etb = xa @ E.T, xb @ E
    num = np.sum(xb * Ea, axis=1)
    den = Ea[:, 0] ** 2 + Ea[:, 1] ** 2 + Etb[:, 0] ** 2 + Etb[:, 1] ** 2
    return num * num / den


def two_view_points(pose, a, b):
    """The two-view DLT point of every correspondence by np.linalg.svd of its 4 x 4 system (float64), A at [I | 0], B at
    [R | t]: (X[n, 3], depth in A, depth in B)."""
    R, t = pose[:9].reshape(3, 3), pose[9:]
    P1, P2 = np.hstack([np.eye(3), np.zeros((3, 1))]), np.hstack([R, t[:, None]])
    A = np.stack([a[:, :1] * P1[2] - P1[0], a[:, 1:] * P1[2] - P1[1], b[:, :1] * P2[2] - P2[0], b[:, 1:] * P2[2] - P2[1]], axis=1)
    if len(A) == 0:
        return np.zeros((0, 3)), np.zeros(0), np.zeros(0)
    w = np.linalg.svd(A)[2][:, -1, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        X = w[:, :3] / w[:, 3:]
    return X, X[:, 2], X @ R[2] + t[2]


def essential_reference(args, out, p):
    """What the outputs of pair p must be, from its returned pose alone.  Returns a dict: `inlier` (Sampson distance within the
    gate), `band` (items within GATE_BAND of the gate: either flag is right), `front` (inlier with both depths in (0, 50)),
    `band2` (band, or a depth within GATE_BAND of a bound), `xyz` (SVD points)."""
    start, ca, cb, thr = args[4], args[5], args[6], args[7]
    s, e = start[p], start[p + 1]
    und = out["undistorted"]
    a, b = und[ca[s:e]], und[cb[s:e]]
    d = sampson_ld(out["pose"][p], a, b)
    thr2 = LD(thr[p]) ** 2
    band = np.abs(d / thr2 - 1) < GATE_BAND
    inlier = d <= thr2
    X, za, zb = two_view_points(out["pose"][p], a, b)
    with np.errstate(invalid="ignore"):
        front = inlier & (za > 0) & (za < DIST_THRESH) & (zb > 0) & (zb < DIST_THRESH)
        near = np.zeros(len(a), dtype=bool)
        for z in (za, zb):
            near |= (np.abs(z) < GATE_BAND) | (np.abs(z / DIST_THRESH - 1) < GATE_BAND) | ~np.isfinite(z)
    return dict(inlier=inlier, band=band, front=front, band2=band | (inlier & near), xyz=X)


def resection_errors_ld(pose, obj, uv):
    """(|uv - proj(R X + t)|, depth) of every point in np.longdouble."""
    R, t = pose[:9].reshape(3, 3).astype(LD), pose[9:].astype(LD)
    Y = obj.astype(LD) @ R.T + t
    r = Y[:, :2] / Y[:, 2:] - uv.astype(LD)
    return np.sqrt(np.sum(r * r, axis=1)), Y[:, 2]


def numpy_pair_rmse(rt, a, b):
    """tests/test_pose_bootstrap_gpu.py's _numpy_pair_rmse, batched; 0 for an empty pair."""
    if len(a) == 0:
        return 0.0
    R, t = rt[:9].reshape(3, 3), rt[9:]
    X, _, _ = two_view_points(rt, a, b)
    pb = X @ R.T + t
    err = np.concatenate([(a - X[:, :2] / X[:, 2:]) ** 2, (b - pb[:, :2] / pb[:, 2:]) ** 2], axis=1)
    return float(np.sqrt(err.sum() / (2 * len(a))))


# ---- checks shared by the CPU-build and the device tests -------------------------------------------------------------------------
def check_essential_outputs(args, out, pairs=None):
    """The outputs of an essential call against plain numpy from its returned poses alone: flags, counts, two-view points for
    the pairs with status 0; identity pose, zero flags and counts, NaN points, conditioning 0 for the others.  Returns
    (items left out as too close to a gate, items, largest relative distance of `xyz` from the SVD point)."""
    start = args[4]
    left_out, worst = 0, 0.0
    for p in (range(len(start) - 1) if pairs is None else pairs):
        s, e = start[p], start[p + 1]
        fl, xyz = out["flag"][s:e], out["xyz"][s:e]
        if out["status"][p] != 0:
            assert np.array_equal(out["pose"][p], IDENTITY_POSE), p
            assert out["n_inliers"][p] == 0 and out["n_cheiral"][p] == 0 and out["conditioning"][p] == 0.0, p
            assert not fl.any() and np.isnan(xyz).all(), p
            assert out["winner"][p] == -1 or e - s >= EPI_SAMPLE, p
            continue
        ref = essential_reference(args, out, p)
        sure, sure2 = ~ref["band"], ~ref["band2"]
        assert np.array_equal(fl[sure] >= 1, ref["inlier"][sure]), (p, np.flatnonzero((fl >= 1) != ref["inlier"]))
        assert np.array_equal(fl[sure2] == 2, ref["front"][sure2]), (p, np.flatnonzero((fl == 2) != ref["front"]))
        lo = int(ref["inlier"][sure].sum())
        assert lo <= out["n_inliers"][p] <= lo + int(ref["band"].sum()) and out["n_inliers"][p] == int((fl >= 1).sum()), p
        lo2 = int(ref["front"][sure2].sum())
        assert lo2 <= out["n_cheiral"][p] <= lo2 + int(ref["band2"].sum()) and out["n_cheiral"][p] == int((fl == 2).sum()), p
        assert 0.0 < out["conditioning"][p] <= 1.0, p
        m = fl == 2
        assert np.isnan(xyz[~m]).all() and np.isfinite(xyz[m]).all(), p
        if m.any():
            worst = max(worst, float((np.linalg.norm(xyz[m] - ref["xyz"][m], axis=1) / np.linalg.norm(ref["xyz"][m], axis=1)).max()))
        left_out += int(ref["band2"].sum())
    return left_out, int(start[-1]), worst


def check_resection_outputs(args, out, min_points):
    """As check_essential_outputs for a resection call: `err` and `n_inliers` from the returned pose in np.longdouble.
    Returns (points left out as too close to the gate, points)."""
    start, obj, uv, thr = args
    left_out = 0
    for j in range(len(start) - 1):
        s, e = start[j], start[j + 1]
        if out["status"][j] != 0:
            assert np.array_equal(out["pose"][j], IDENTITY_POSE) and out["n_inliers"][j] == 0 and np.isnan(out["err"][s:e]).all(), j
            assert (out["status"][j] == 1) == (e - s < max(RES_SAMPLE, min_points)), j
            assert out["winner"][j] == -1 or out["status"][j] == 2, j
            continue
        err, z = resection_errors_ld(out["pose"][j], obj[s:e], uv[s:e])
        np.testing.assert_allclose(out["err"][s:e], err.astype(np.float64), rtol=0, atol=1e-12, err_msg=str(j))
        band = (np.abs((err / LD(thr[j])) ** 2 - 1) < GATE_BAND) | (np.abs(z) < GATE_BAND)
        lo = int(((err <= thr[j]) & (z > 0) & ~band).sum())
        assert lo <= out["n_inliers"][j] <= lo + int(band.sum()), j
        left_out += int(band.sum())
    return left_out, int(start[-1])


def pairs_on_the_gate(args, cpu):
    """Pairs of an essential call with a correspondence within GATE_BAND of the Sampson gate at the CPU build's pose."""
    return [p for p in range(len(args[4]) - 1) if cpu["status"][p] == 0 and essential_reference(args, cpu, p)["band"].any()]


def jobs_on_the_gate(args, cpu):
    start, obj, uv, thr = args
    out = []
    for j in np.flatnonzero(cpu["status"] == 0):
        err, _ = resection_errors_ld(cpu["pose"][j], obj[start[j]:start[j + 1]], uv[start[j]:start[j + 1]])
        if np.any(np.abs((err / LD(thr[j])) ** 2 - 1) < GATE_BAND):
            out.append(int(j))
    return out


def pnp_rmse_ld(pose, obj, und, f32):
    """sqrt(mean |und - proj(R X + t)|^2) of one view in np.longdouble (object points rounded to float32 when `f32`, as the
    call reads them)."""
    R, t = pose[:9].reshape(3, 3).astype(LD), pose[9:].astype(LD)
    Y = (obj.astype(np.float32) if f32 else obj).astype(LD) @ R.T + t
    r = Y[:, :2] / Y[:, 2:] - und.astype(LD)
    return np.sqrt(np.sum(r * r) / len(obj))


def motion_errors(pose, R, t, unit=False):
    """(rotation angle in degrees, translation direction angle in degrees if `unit` else |t - t_true|)."""
    rot = rotation_angle_deg(pose[:9].reshape(3, 3), R)
    return rot, (direction_angle_deg(pose[9:], t) if unit else float(np.linalg.norm(pose[9:] - t)))


def many_essential_counts_ld(args, out):
    """Vectorised over a call of many small pairs: (inliers of every pair from its returned pose, items within GATE_BAND)."""
    start, ca, cb, thr = args[4], args[5], args[6], args[7]
    job = np.repeat(np.arange(len(start) - 1), np.diff(start))
    R, t = out["pose"][:, :9].reshape(-1, 3, 3).astype(LD), out["pose"][:, 9:].astype(LD)
    tx = np.zeros_like(R)
    tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0], tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
    E = np.matmul(tx, R)
    und = out["undistorted"].astype(LD)
    one = np.ones((len(job), 1), dtype=LD)
    xa, xb = np.hstack([und[ca], one]), np.hstack([und[cb], one])
    Ej = E[job]
    Ea = np.sum(Ej * xa[:, None, :], axis=2)
    Etb = np.sum(Ej * xb[:, :, None], axis=1)
    num = np.sum(xb * Ea, axis=1)
    den = Ea[:, 0] ** 2 + Ea[:, 1] ** 2 + Etb[:, 0] ** 2 + Etb[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(den > 0, num * num / den, LD(1e300))
    thr2 = thr[job].astype(LD) ** 2
    inl = (d <= thr2) & (out["status"][job] == 0)
    band = (np.abs(d / thr2 - 1) < GATE_BAND) & (out["status"][job] == 0)
    return np.add.reduceat(inl.astype(np.int64), start[:-1]), band


def many_resection_ld(args, out):
    """Vectorised over a call of many small jobs: (err of every point, inliers of every job, points within GATE_BAND)."""
    start, obj, uv, thr = args
    job = np.repeat(np.arange(len(start) - 1), np.diff(start))
    R, t = out["pose"][:, :9].reshape(-1, 3, 3).astype(LD), out["pose"][:, 9:].astype(LD)
    Y = np.sum(R[job] * obj.astype(LD)[:, None, :], axis=2) + t[job]
    r = Y[:, :2] / Y[:, 2:] - uv.astype(LD)
    err = np.sqrt(np.sum(r * r, axis=1))
    ok = out["status"][job] == 0
    thr_j = thr[job].astype(LD)
    inl = ok & (err <= thr_j) & (Y[:, 2] > 0)
    band = ok & ((np.abs((err / thr_j) ** 2 - 1) < GATE_BAND) | (np.abs(Y[:, 2]) < GATE_BAND))
    return np.where(ok, err, np.nan).astype(np.float64), np.add.reduceat(inl.astype(np.int64), start[:-1]), band


def check_pnp_outputs(sc, outs, f32):
    """The outputs of a PnP call against plain numpy: `undistorted` put back through the camera model gives the pixels (to the
    float32 rounding of pixels and points when `f32`: 2^-24 of 2000 px each, twice; otherwise to what the fixed number of
    undistortion iterations leaves), `rmse` is the reprojection error of the returned pose, views without status 0 hold the
    identity and rmse 0."""
    pose, rmse, st, und = outs
    start, cam, model, intr, xy, obj = sc["args"]
    for v in range(len(start) - 1):
        s, e = start[v], start[v + 1]
        back = to_pixels(model[cam[v]], intr[cam[v]], und[s:e])
        assert e == s or np.abs(back - xy[s:e]).max() < (1e-3 if f32 else 1e-5), (v, np.abs(back - xy[s:e]).max())
        if st[v] != 0:
            assert np.array_equal(pose[v], IDENTITY_POSE) and rmse[v] == 0.0, v
            continue
        ref = float(pnp_rmse_ld(pose[v], obj[s:e], und[s:e], f32))
        assert abs(rmse[v] - ref) <= 1e-9 * ref + 1e-15, (v, rmse[v], ref)


def motion_errors_many(pose, R, t, unit=False):
    """motion_errors for stacked poses: (rotation angles in degrees, direction angles in degrees if `unit` else |t - t_true|)."""
    c = (np.einsum("nij,nij->n", pose[:, :9].reshape(-1, 3, 3), R) - 1.0) / 2.0
    rot = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
    if not unit:
        return rot, np.linalg.norm(pose[:, 9:] - t, axis=1)
    ct = np.sum(pose[:, 9:] * t, axis=1) / (np.linalg.norm(pose[:, 9:], axis=1) * np.linalg.norm(t, axis=1))
    return rot, np.degrees(np.arccos(np.clip(ct, -1.0, 1.0)))
