"""Two independent numpy restatements of the fixed-interval smoother of include/caliscope/trajectory_smoother.h.

``sequential``: the forward Kalman filter and the modified Bryson-Frazier backward pass on the filtered pairs, written with full 6 x 6
matrices (the recursion of csrc/trajectory_smooth_math.h, which holds them as blocks).  ``joint``: the posterior of a whole trajectory as one
whitened least-squares problem solved by QR, the marginal covariances from the inverse of its triangular factor; no recursion, no
innovation, no gain.  ``disagreement`` is the measure both are held to each other with, and the build to them."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
from scipy.linalg import solve_triangular

try:  # many small factorisations: a BLAS thread pool only gets in their way (ten times slower on eight threads)
    from threadpoolctl import threadpool_limits
except ImportError:  # pragma: no cover
    from contextlib import nullcontext as threadpool_limits

SYM = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])  # rows xx xy xz yy yz zz


def full3(rows):
    rows = np.asarray(rows, dtype=np.float64)
    return rows[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(rows.shape[:-1] + (3, 3))


def rows6(m):
    return np.asarray(m)[..., SYM[0], SYM[1]]


def model(fps, q):
    dt = 1.0 / fps
    I3 = np.eye(3)
    F = np.block([[I3, dt * I3], [np.zeros((3, 3)), I3]])
    Q = q * q * np.block([[dt ** 3 / 3 * I3, dt ** 2 / 2 * I3], [dt ** 2 / 2 * I3, dt * I3]])
    return dt, F, Q


def empty(n_slots):
    nan = np.nan
    return SimpleNamespace(pos=np.full((n_slots, 3), nan), vel=np.full((n_slots, 3), nan), pos_cov=np.full((n_slots, 6), nan),
                           vel_cov=np.full((n_slots, 6), nan), nis=np.full(n_slots, nan), status=np.zeros(n_slots, dtype=np.uint8))


def statuses(meas, max_gap):
    """[n_frames] status of one trajectory from its measured flags: 1 measured, 2 inside a hole of at most max_gap frames between two
    measured frames, 0 otherwise."""
    st = np.zeros(len(meas), dtype=np.uint8)
    at = np.flatnonzero(meas)
    st[at] = 1
    for a, b in zip(at[:-1], at[1:]):
        if 0 < b - a - 1 <= max_gap:
            st[a + 1:b] = 2
    return st


def _tracks(n_frames, n_traj, xyz, meas_cov, measured):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(n_frames, n_traj, 3)
    R = full3(np.asarray(meas_cov, dtype=np.float64).reshape(n_frames, n_traj, 6))
    m = np.asarray(measured).reshape(n_frames, n_traj) == 1
    return xyz, R, m


def sequential(n_frames, n_traj, xyz, meas_cov, measured, fps, q, sv0, max_gap):
    dt, F, Q = model(fps, q)
    H = np.hstack([np.eye(3), np.zeros((3, 3))])
    xyz, R, m = _tracks(n_frames, n_traj, xyz, meas_cov, measured)
    out = empty(n_frames * n_traj)
    for j in range(n_traj):
        at = np.flatnonzero(m[:, j])
        if at.size == 0:
            continue
        f0, f1 = int(at[0]), int(at[-1])
        st = statuses(m[:, j], max_gap)
        x = np.concatenate([xyz[f0, j], np.zeros(3)])
        P = np.zeros((6, 6))
        P[:3, :3], P[3:, 3:] = R[f0, j], sv0 * sv0 * np.eye(3)
        xs, Ps, us, Sis, Gs = {f0: x}, {f0: P}, {}, {}, {}
        for f in range(f0 + 1, f1 + 1):  # forward: the filtered pair of every frame; u = S^-1 y, S^-1 and (I - K H)^T of the measured ones
            x, P = F @ x, F @ P @ F.T + Q
            if m[f, j]:
                A, B, Cv = P[:3, :3], P[:3, 3:], P[3:, 3:]
                y = xyz[f, j] - x[:3]
                Si = np.linalg.inv(A + R[f, j])
                Si = 0.5 * (Si + Si.T)
                u = Si @ y
                out.nis[f * n_traj + j] = y @ u
                # I - K H = [[I - A Si, 0], [-B^T Si, I]] with I - Si A = Si R: products, no difference of nearly equal matrices
                M, N = Si @ R[f, j], -Si @ B
                G = np.block([[M, N], [np.zeros((3, 3)), np.eye(3)]])
                x = x + P[:, :3] @ u
                P = np.block([[M.T @ A, M.T @ B], [(M.T @ B).T, Cv - B.T @ Si @ B]])
                P = 0.5 * (P + P.T)
                us[f], Sis[f], Gs[f] = u, Si, G
            xs[f], Ps[f] = x, P
        lam, Lam = np.zeros(6), np.zeros((6, 6))
        for f in range(f1, f0 - 1, -1):  # backward: the adjoint pair, smoothed = filtered - P (adjoint)
            x, P = xs[f], Ps[f]
            if st[f]:
                s = f * n_traj + j
                xm, Pm = x - P @ lam, P - P @ Lam @ P
                out.pos[s], out.vel[s], out.pos_cov[s], out.vel_cov[s], out.status[s] = xm[:3], xm[3:], rows6(Pm[:3, :3]), rows6(Pm[3:, 3:]), st[f]
            if f in us:
                G = Gs[f]
                lam = G @ lam - H.T @ us[f]
                Lam = G @ Lam @ G.T + H.T @ Sis[f] @ H
            lam, Lam = F.T @ lam, F.T @ Lam @ F
    return out


def joint(*args):
    """No nis (there is no innovation here)."""
    with threadpool_limits(1):
        return _joint(*args)


def _joint(n_frames, n_traj, xyz, meas_cov, measured, fps, q, sv0, max_gap):
    dt, F, Q = model(fps, q)
    LQi = np.linalg.inv(np.linalg.cholesky(Q))
    xyz, R, m = _tracks(n_frames, n_traj, xyz, meas_cov, measured)
    out = empty(n_frames * n_traj)
    scale = np.concatenate([np.ones(3), np.full(3, 1.0 / dt)])  # the unknown of a velocity column is v dt
    Fs = F * scale[None, :]
    for j in range(n_traj):
        at = np.flatnonzero(m[:, j])
        if at.size == 0:
            continue
        f0, f1 = int(at[0]), int(at[-1])
        T = f1 - f0 + 1
        st = statuses(m[:, j], max_gap)
        z0 = xyz[f0, j]
        rows, rhs = [], []
        for f in at:
            Li = np.linalg.inv(np.linalg.cholesky(R[f, j]))
            blk = np.zeros((3, 6 * T))
            blk[:, 6 * (f - f0):6 * (f - f0) + 3] = Li
            rows.append(blk)
            rhs.append(Li @ (xyz[f, j] - z0))
        for t in range(T - 1):
            blk = np.zeros((6, 6 * T))
            blk[:, 6 * t:6 * t + 6] = -LQi @ Fs
            blk[:, 6 * t + 6:6 * t + 12] = LQi * scale[None, :]
            rows.append(blk)
            rhs.append(np.zeros(6))
        blk = np.zeros((3, 6 * T))
        blk[:, 3:6] = np.eye(3) / (sv0 * dt)
        rows.append(blk)
        rhs.append(np.zeros(3))
        A, b = np.vstack(rows), np.concatenate(rhs)
        Rb = np.linalg.qr(np.column_stack([A, b]), mode="r")  # (Q is not formed: Q^T b is the last column of the factor of [A b])
        Rf = Rb[:6 * T, :6 * T]
        sol = solve_triangular(Rf, Rb[:6 * T, 6 * T])
        Ri = solve_triangular(Rf, np.eye(6 * T))
        for f in range(f0, f1 + 1):
            if not st[f]:
                continue
            s, t = f * n_traj + j, f - f0
            out.pos[s], out.vel[s] = sol[6 * t:6 * t + 3] + z0, sol[6 * t + 3:6 * t + 6] / dt
            out.pos_cov[s] = rows6(Ri[6 * t:6 * t + 3] @ Ri[6 * t:6 * t + 3].T)
            out.vel_cov[s] = rows6(Ri[6 * t + 3:6 * t + 6] @ Ri[6 * t + 3:6 * t + 6].T) / (dt * dt)
            out.status[s] = st[f]
    return out


def disagreement(a, b):
    """(means, covariances): the largest |a - b| of the smoothed position and velocity in units of the slot's own smoothed standard
    deviation sqrt(tr P) (of b), and the largest relative Frobenius distance of the two covariances, over the slots b has."""
    at = np.flatnonzero(b.status > 0)
    if at.size == 0:
        return 0.0, 0.0
    Pp, Pv = full3(b.pos_cov[at]), full3(b.vel_cov[at])
    mean = max(float((np.linalg.norm(a.pos[at] - b.pos[at], axis=1) / np.sqrt(np.trace(Pp, axis1=1, axis2=2))).max()),
               float((np.linalg.norm(a.vel[at] - b.vel[at], axis=1) / np.sqrt(np.trace(Pv, axis1=1, axis2=2))).max()))
    cov = max(float((np.linalg.norm(full3(a.pos_cov[at]) - Pp, axis=(1, 2)) / np.linalg.norm(Pp, axis=(1, 2))).max()),
              float((np.linalg.norm(full3(a.vel_cov[at]) - Pv, axis=(1, 2)) / np.linalg.norm(Pv, axis=(1, 2))).max()))
    return mean, cov


__all__ = ["disagreement", "empty", "full3", "joint", "model", "rows6", "sequential", "statuses"]
