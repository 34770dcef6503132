"""Seeded scenes of the trajectory smoother tests: the arrays of cba_smooth_trajectories (points, their 3 x 3 covariances, measured
flags) with the launch and hole edges the issue lists, every one of which is asserted here from the scene's own tables."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from tests import trajectory_smooth_oracle as SO

FPS, ACCEL, SV0, MAX_GAP = 30.0, 2.0, 10.0, 3

# trajectories of EDGE with a pattern of their own (the others are measured at each frame with probability 0.8)
NONE, SINGLE, PAIR, HOLES, LONG, ENDS, FULL = 0, 1, 2, 3, 4, 5, 6
SINGLE_FRAME, PAIR_FRAMES = 17, (5, 20)
HOLES_MISSING = (5, 10, 11, 12, 20, 21, 22, 23)  # holes of 1, 3 and 4 frames
LONG_HOLE = (5, 35)                              # frames 5..34: 30 frames
ENDS_SPAN = (6, 34)                              # measured on [6, 34) alone


def random_covariances(rng, n):
    """[n, 6] rows of symmetric positive definite matrices with eigenvalues in 1e-6 .. 4e-4 (m^2), the largest at least 100 times the
    smallest, in a random orientation each."""
    lo = rng.uniform(1e-6, 4e-6, n)
    eig = np.column_stack([lo, lo * rng.uniform(1.0, 100.0, n), lo * 100.0])
    Qm = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    return SO.rows6(np.einsum("nij,nj,nkj->nik", Qm, eig, Qm))


def noisy_track(rng, n_frames, n_traj, cov_rows):
    """A sinusoidal truth per trajectory and its samples z = p + N(0, R)."""
    t = np.arange(n_frames)[:, None, None] / FPS
    centre, amp = rng.uniform(-1.0, 1.0, (1, n_traj, 3)), rng.uniform(0.05, 0.3, (1, n_traj, 3))
    omega, phase = rng.uniform(2.0, 8.0, (1, n_traj, 3)), rng.uniform(0.0, 6.28, (1, n_traj, 3))
    truth = centre + amp * np.sin(omega * t + phase)
    L = np.linalg.cholesky(SO.full3(cov_rows))
    noise = np.einsum("nij,nj->ni", L, rng.normal(size=(n_frames * n_traj, 3)))
    return truth.reshape(-1, 3), truth.reshape(-1, 3) + noise


def scene(n_frames, n_traj, xyz, meas_cov, measured, max_gap=MAX_GAP, sv0=SV0, accel=ACCEL):
    return SimpleNamespace(n_frames=n_frames, n_traj=n_traj, xyz=np.ascontiguousarray(xyz), meas_cov=np.ascontiguousarray(meas_cov),
                           measured=np.ascontiguousarray(measured, dtype=np.uint8), fps=FPS, accel=accel, sv0=sv0, max_gap=max_gap)


def oracle_args(sc):
    return (sc.n_frames, sc.n_traj, sc.xyz, sc.meas_cov, sc.measured, sc.fps, sc.accel, sc.sv0, sc.max_gap)


@functools.cache
def edge():
    n_frames, n_traj = 40, 257
    rng = np.random.default_rng(11)
    cov = random_covariances(rng, n_frames * n_traj)
    _, z = noisy_track(rng, n_frames, n_traj, cov)
    m = rng.uniform(size=(n_frames, n_traj)) < 0.8
    m[:, NONE] = False
    m[:, SINGLE] = False
    m[SINGLE_FRAME, SINGLE] = True
    m[:, PAIR] = False
    m[list(PAIR_FRAMES), PAIR] = True
    m[:, HOLES] = True
    m[list(HOLES_MISSING), HOLES] = False
    m[:, LONG] = True
    m[LONG_HOLE[0]:LONG_HOLE[1], LONG] = False
    m[:, ENDS] = False
    m[ENDS_SPAN[0]:ENDS_SPAN[1], ENDS] = True
    m[:, FULL] = True
    m[[0, 39], 64] = True
    m[[0, 39], 256] = True
    sc = scene(n_frames, n_traj, z, cov, m.reshape(-1))
    # the properties the tests rely on, from the tables themselves
    assert n_traj == 256 + 1 and n_traj > 4 * 64  # a second workgroup with one live thread; trajectory 64 opens the second wave
    eig = np.linalg.eigvalsh(SO.full3(cov))
    assert (eig[:, 0] > 0).all() and (eig[:, 2] / eig[:, 0] >= 100.0 * (1 - 1e-9)).all() and len(np.unique(cov[:, 0])) == len(cov)
    assert m[:, NONE].sum() == 0 and m[:, SINGLE].sum() == 1 and m[:, PAIR].sum() == 2 and m[:, FULL].all()
    holes = hole_lengths(m[:, HOLES])
    assert sorted(holes) == [1, 3, 4] and hole_lengths(m[:, LONG]) == [30] and sc.max_gap == 3
    assert not m[:ENDS_SPAN[0], ENDS].any() and not m[ENDS_SPAN[1]:, ENDS].any() and m[ENDS_SPAN[0]:ENDS_SPAN[1], ENDS].all()
    assert m[:, 64].any() and m[:, 256].any()
    return sc


def hole_lengths(meas):
    at = np.flatnonzero(meas)
    return [int(b - a - 1) for a, b in zip(at[:-1], at[1:]) if b - a > 1]


@functools.cache
def one():
    rng = np.random.default_rng(12)
    cov = random_covariances(rng, 1)
    return scene(1, 1, rng.normal(size=(1, 3)), cov, np.ones(1))


@functools.cache
def drawn_from_the_model(seed=5, n_traj=512, n_frames=41, sv0=1.0):
    """Tracks drawn from the model itself: v0 ~ N(0, sv0^2), the white-noise acceleration of density ACCEL, z = p + N(0, R_t), all
    measured.  Returns (scene, truth positions [n_slots, 3])."""
    rng = np.random.default_rng(seed)
    dt, F, Q = SO.model(FPS, ACCEL)
    LQ = np.linalg.cholesky(Q)
    cov = random_covariances(rng, n_frames * n_traj)
    x = np.concatenate([rng.uniform(-1.0, 1.0, (n_traj, 3)), sv0 * rng.normal(size=(n_traj, 3))], axis=1)
    truth = np.empty((n_frames, n_traj, 3))
    for f in range(n_frames):
        if f:
            x = x @ F.T + rng.normal(size=(n_traj, 6)) @ LQ.T
        truth[f] = x[:, :3]
    L = np.linalg.cholesky(SO.full3(cov))
    z = truth.reshape(-1, 3) + np.einsum("nij,nj->ni", L, rng.normal(size=(n_frames * n_traj, 3)))
    return scene(n_frames, n_traj, z, cov, np.ones(n_frames * n_traj), sv0=sv0), truth.reshape(-1, 3)


def model_statistics(sc, truth, out):
    """(mean of d^T P_pos^-1 d at the middle frame, mean nis over the measured frames that have one)."""
    mid = (sc.n_frames // 2) * sc.n_traj + np.arange(sc.n_traj)
    d = out.pos[mid] - truth[mid]
    m2 = np.einsum("ni,nij,nj->n", d, np.linalg.inv(SO.full3(out.pos_cov[mid])), d)
    nis = out.nis[~np.isnan(out.nis)]
    assert len(nis) == (sc.n_frames - 1) * sc.n_traj
    return float(m2.mean()), float(nis.mean())


@functools.cache
def sinusoid():
    """One noisy sinusoidal track per trajectory, all measured: (scene, truth)."""
    rng = np.random.default_rng(21)
    n_frames, n_traj = 120, 4
    cov = random_covariances(rng, n_frames * n_traj)
    truth, z = noisy_track(rng, n_frames, n_traj, cov)
    return scene(n_frames, n_traj, z, cov, np.ones(n_frames * n_traj)), truth


__all__ = ["ACCEL", "FPS", "MAX_GAP", "SV0", "drawn_from_the_model", "edge", "model_statistics", "one", "oracle_args", "sinusoid"]
