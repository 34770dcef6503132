"""Scenes for the skeleton adjustment (include/caliscope/trajectory_skeleton.h), shared by the CPU and the GPU tests.  Each is built
once per process and not changed.  Noise: 1 mm across and 1 to 2 cm deep on 0.3 m segments of sigma 5 mm, a given length within one
sigma of the truth: where the oracle's undamped Gauss-Newton converges (tests/trajectory_skeleton_oracle.py)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

SEG = 0.3      # segment length, world units (metres)
SIGMA = 5e-3   # how rigid a segment is


@dataclass
class Scene:
    n_frames: int
    n_traj: int
    xyz: np.ndarray        # [n_slots, 3] NaN where unmeasured
    cov: np.ndarray        # [n_slots, 6]
    measured: np.ndarray   # [n_slots] uint8
    seg_traj: np.ndarray   # [n_seg, 2] int32
    seg_length: np.ndarray
    seg_sigma: np.ndarray
    trim: float = 3.0
    truth: np.ndarray | None = None   # [n_slots, 3]
    marks: dict = field(default_factory=dict)


def oracle_args(sc: Scene):
    return sc.n_frames, sc.n_traj, sc.xyz, sc.cov, sc.measured, sc.seg_traj, sc.seg_length, sc.seg_sigma, sc.trim


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _covariances(rng, n, lateral, deep_lo, deep_hi):
    """n covariances of standard deviation `lateral` across and deep_lo .. deep_hi along a random direction, and their Cholesky factors."""
    R, L = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    for i in range(n):
        Q = _rotation(rng)
        R[i] = Q @ np.diag([lateral ** 2, lateral ** 2, rng.uniform(deep_lo, deep_hi) ** 2]) @ Q.T
        R[i] = 0.5 * (R[i] + R[i].T)
        L[i] = np.linalg.cholesky(R[i])
    return R, L


def _rows6(R):
    return np.stack([R[:, 0, 0], R[:, 0, 1], R[:, 0, 2], R[:, 1, 1], R[:, 1, 2], R[:, 2, 2]], axis=1)


def _moving(rng, base, n_frames):
    """base [m, 3] carried through n_frames by a slow rigid motion: lengths stay what they are."""
    out = np.zeros((n_frames, len(base), 3))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    centre = base.mean(axis=0)
    for f in range(n_frames):
        a = 0.004 * f
        Rot = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        out[f] = (base - centre) @ Rot.T + centre + 0.002 * f * np.array([1.0, 0.3, 0.0])
    return out


def _assemble(rng, truth, meas, seg_traj, seg_length, lateral=1e-3, deep=(1e-2, 1.5e-2), sigma=SIGMA, **marks) -> Scene:
    n_frames, n_traj = meas.shape
    n_slots = n_frames * n_traj
    R, L = _covariances(rng, n_slots, lateral, *deep)
    Z = truth.reshape(n_slots, 3) + np.einsum("ijk,ik->ij", L, rng.normal(size=(n_slots, 3)))
    measured = meas.reshape(n_slots).astype(np.uint8)
    xyz, cov = np.where(measured[:, None] == 1, Z, np.nan), np.where(measured[:, None] == 1, _rows6(R), np.nan)
    seg_traj = np.asarray(seg_traj, dtype=np.int32).reshape(-1, 2)
    return Scene(n_frames, n_traj, xyz, cov, measured, seg_traj, np.asarray(seg_length, dtype=np.float64), np.full(len(seg_traj), sigma), truth=truth.reshape(n_slots, 3),
                 marks=marks)


@functools.cache
def edge() -> Scene:
    """257 frames (a second pass of a 256-thread stride has one live element) of, in one call: a pair (trajectories 0, 1); a 22-point
    chain (2 .. 23: n = 66, past one wave's width); a 12-point cycle (24 .. 35) with a star of three leaves (36, 37, 38) on vertex 24; a
    54-point random tree (39 .. 92) measured in 8 frames only; trajectory 93 in no segment.  Segments in shuffled order, every other
    one of the chain written from its higher end.
    Segments: chain (2, 3) has a given length and an even count of co-measured frames (256), chain (12, 13) an odd one (255); the
    leaf 37 is measured in frame 3 alone (one co-measured frame); the leaf 38 never (none, no given length: NaN, inactive); the pair
    is co-measured in 9 frames of which five carry the same bytes (ties at the median, mad == 0).
    Frames: 0 has nothing measured; in 5 the chain misses point 12 and falls in two; in 7 the chain's point 5 is measured and its
    neighbours 4 and 6 are not (status 2, the input's bytes); in 9 the ends of the pair coincide."""
    rng = np.random.default_rng(20240611)
    n_frames, n_traj = 257, 94
    base = np.zeros((n_traj, 3))
    base[0], base[1] = [0.0, 0.0, 2.0], [SEG, 0.0, 2.0]
    for i in range(22):  # a zigzag
        base[2 + i] = [1.0 + 0.5 * SEG * i, (i % 2) * SEG * np.sqrt(0.75) * np.cos(0.3 * i), (i % 2) * SEG * np.sqrt(0.75) * np.sin(0.3 * i)]
    radius = 0.5 * SEG / np.sin(np.pi / 12)
    for i in range(12):
        base[24 + i] = [-2.0 + radius * np.cos(2 * np.pi * i / 12), radius * np.sin(2 * np.pi * i / 12), 1.0]
    for i, d in enumerate(([0.6, 0.0, 0.8], [0.6, 0.48, -0.64], [0.8, -0.6, 0.0])):
        base[36 + i] = base[24] + SEG * np.array(d)
    parent = {}
    base[39] = [0.0, 3.0, 0.0]
    for i in range(40, 93):
        parent[i] = int(rng.integers(39, i))
        d = rng.normal(size=3)
        base[i] = base[parent[i]] + SEG * d / np.linalg.norm(d)
    base[93] = [5.0, 5.0, 5.0]
    truth = _moving(rng, base, n_frames)
    segs = [(0, 1)] + [((2 + i, 3 + i) if i % 2 == 0 else (3 + i, 2 + i)) for i in range(21)] + [(24 + i, 24 + (i + 1) % 12) for i in range(12)]
    segs += [(24, 36), (37, 24), (24, 38)] + [(parent[i], i) for i in range(40, 93)]
    order = rng.permutation(len(segs))
    segs = [segs[i] for i in order]
    given = np.full(len(segs), np.nan)
    given[segs.index((2, 3))] = SEG + SIGMA
    meas = np.zeros((n_frames, n_traj), dtype=bool)
    pair_frames = [9, 20, 21, 22, 23, 24, 30, 31, 32]
    meas[pair_frames, 0] = meas[pair_frames, 1] = True
    meas[1:, 2:24] = True
    meas[5, 12] = False
    meas[7, 4] = meas[7, 6] = False
    meas[1:41, 24:37] = True
    meas[256, 24:37] = True
    meas[3, 37] = True
    meas[1:9, 39:93] = True
    meas[1:, 93] = True
    sc = _assemble(rng, truth, meas, segs, given, pair=segs.index((0, 1)), chain_given=segs.index((2, 3)), chain_odd=segs.index((12, 13)),
                   single=segs.index((37, 24)), never=segs.index((24, 38)), hole_frame=5, lonely=(7, 5), coincident_frame=9, nothing_frame=0, loner=93)
    for f in (21, 22, 23, 24):  # the pair's bytes of frame 20 again
        for j in (0, 1):
            sc.xyz[f * n_traj + j], sc.cov[f * n_traj + j] = sc.xyz[20 * n_traj + j], sc.cov[20 * n_traj + j]
    sc.xyz[9 * n_traj + 1] = sc.xyz[9 * n_traj + 0]
    for a in (sc.xyz, sc.cov, sc.measured, sc.seg_traj, sc.seg_length, sc.seg_sigma):
        a.setflags(write=False)
    return sc


@functools.cache
def one() -> Scene:
    """One frame, two points, one segment of a given length."""
    rng = np.random.default_rng(7)
    truth = np.array([[[0.0, 0.0, 1.0], [SEG, 0.0, 1.0]]])
    return _assemble(rng, truth, np.ones((1, 2), dtype=bool), [(0, 1)], [SEG + SIGMA])


@functools.cache
def too_large() -> Scene:
    """A chain of 55 points behind three trajectories of a pair and a loner: the component of trajectory 3 is refused."""
    rng = np.random.default_rng(8)
    base = np.zeros((58, 3))
    base[:, 0] = SEG * np.arange(58)
    segs = [(0, 1)] + [(3 + i, 4 + i) for i in range(54)]
    return _assemble(rng, _moving(rng, base, 2), np.ones((2, 58), dtype=bool), segs, np.full(len(segs), np.nan))


@functools.cache
def wrong_length() -> Scene:
    """A chain of five points in six frames whose given lengths are 20 sigma off: Levenberg-Marquardt territory, no oracle."""
    rng = np.random.default_rng(9)
    base = np.zeros((5, 3))
    base[:, 0] = SEG * np.arange(5)
    base[:, 1] = 0.1 * (np.arange(5) % 2)
    length = np.linalg.norm(base[1] - base[0]) + 20 * SIGMA
    return _assemble(rng, _moving(rng, base, 6), np.ones((6, 5), dtype=bool), [(i, i + 1) for i in range(4)], np.full(4, length))


@functools.cache
def statistical() -> Scene:
    """Tracks drawn from the model: a tree of 10 points in 400 frames, the length of segment s in a frame L_s + N(0, sigma_s^2) with
    sigma_s = 3 mm, the samples the true points + N(0, R_i) with 0.3 mm across and 1 to 3 mm deep: at most 1 % of the 0.3 m
    segments, so that the curvature bias stays far inside the bounds.  The lengths L_s are given."""
    rng = np.random.default_rng(10)
    n_frames, m, sigma = 400, 10, 3e-3
    parent = [0] + [int(rng.integers(0, i)) for i in range(1, m)]
    dirs = rng.normal(size=(m, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    truth = np.zeros((n_frames, m, 3))
    for f in range(n_frames):
        truth[f, 0] = [0.001 * f, 0.0, 1.0]
        for i in range(1, m):
            truth[f, i] = truth[f, parent[i]] + dirs[i] * (SEG + sigma * rng.normal())
    segs = [(parent[i], i) for i in range(1, m)]
    return _assemble(rng, truth, np.ones((n_frames, m), dtype=bool), segs, np.full(m - 1, SEG), lateral=3e-4, deep=(1e-3, 3e-3), sigma=sigma)
