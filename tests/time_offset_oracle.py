"""A numpy restatement of cba_estimate_time_offsets, written from include/caliscope/time_offsets.h and not from the header of the
arithmetic: the joint problem in (X, delta) with its dense Jacobian, Gauss-Newton by `lstsq` on the stacked system (no Schur
complement), the same rounds and the same freezing of V, the same safeguard.  It works on the rows of the grid, not on a dense grid.

`estimate(grid, dtype)` runs in float64 or in longdouble.  In longdouble the state, the residuals and the Jacobian are longdouble; the
step is `lstsq` of their float64 copies (numpy's LAPACK has no longdouble), which is relatively accurate to 1e-16 times the condition,
so that the iteration converges to the fixed point of the longdouble residuals: the Gauss-Newton loop is its own iterative refinement.
The start is a DLT of its own (Newton inversion of the lens to convergence, `svd`), which the synchronous start makes immaterial.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg

RESOLVE, PRED_ROW, MAX_INNER, MAX_HALVINGS, TOL_FRACTION = 1e-10, 1e-18, 30, 10, 1e-6


@dataclass
class OracleResult:
    offsets: np.ndarray
    sigma: np.ndarray
    status: np.ndarray
    rms_before: np.ndarray
    rms_after: np.ndarray
    rows: np.ndarray
    sigma0_px: float
    rounds: int
    converged: bool
    xyz: np.ndarray
    valid: np.ndarray
    velocity: np.ndarray
    frame_time: np.ndarray
    row_xy: np.ndarray
    row_used: np.ndarray
    unit_offset: np.ndarray  # [n_cams] sqrt((S^-1)_cc), 0 where the camera is not estimated
    unit_xyz: np.ndarray     # [n_slots, 3] sqrt(diag H^-1), NaN without a point
    changes: list            # max |delta - delta of the round before| per round
    F: float = 0.0


def lens(model, d, x, y):
    """(xd, yd, 2 x 2 derivative as four arrays) of normalised points, any float dtype."""
    r2 = x * x + y * y
    if model == 0:
        k1, k2, p1, p2, k3 = d[:5]
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        drad = k1 + r2 * (2 * k2 + 3 * k3 * r2)  # d rad / d r2
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return (xd, yd, rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x, 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y,
                2 * x * y * drad + 2 * p1 * x + 2 * p2 * y, rad + 2 * y * y * drad + 6 * p1 * y + 2 * p2 * x)
    k1, k2, k3, k4 = d[:4]
    r = np.sqrt(r2)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    dthd = 1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4)))
    s = thd / r
    ds = (dthd / (1 + r2) - s) / r2  # (d s / d r) / r
    return x * s, y * s, s + x * x * ds, x * y * ds, x * y * ds, s + y * y * ds


def project(model, intr, P, X):
    """pixels [n, 2] and d pixel / d X [n, 2, 3] of world points X [n, 3]; intr = fx fy cx cy d0..d4, P = [R | t] row-major."""
    T = X.dtype
    intr, P = intr.astype(T), P.astype(T).reshape(3, 4)
    R, t = P[:, :3], P[:, 3]
    Xc = X @ R.T + t
    iz = 1 / Xc[:, 2]
    x, y = Xc[:, 0] * iz, Xc[:, 1] * iz
    xd, yd, dxx, dxy, dyx, dyy = lens(model, intr[4:], x, y)
    uv = np.stack([intr[2] + intr[0] * xd, intr[3] + intr[1] * yd], axis=1)
    # d (x, y) / d Xc = [[1, 0, -x], [0, 1, -y]] / Z
    G = np.zeros((len(X), 2, 3), dtype=T)
    G[:, 0, 0], G[:, 0, 1], G[:, 0, 2] = intr[0] * dxx * iz, intr[0] * dxy * iz, -intr[0] * (dxx * x + dxy * y) * iz
    G[:, 1, 0], G[:, 1, 1], G[:, 1, 2] = intr[1] * dyx * iz, intr[1] * dyy * iz, -intr[1] * (dyx * x + dyy * y) * iz
    return uv, G @ R


def undistort(model, intr, uv):
    """Normalised undistorted points by Newton on the lens, to convergence (float64)."""
    x0, y0 = (uv[:, 0] - intr[2]) / intr[0], (uv[:, 1] - intr[3]) / intr[1]
    x, y = x0.copy(), y0.copy()
    for _ in range(30):
        xd, yd, a, b, c, d = lens(model, intr[4:], x, y)
        det = a * d - b * c
        ex, ey = xd - x0, yd - y0
        x, y = x - (d * ex - b * ey) / det, y - (-c * ex + a * ey) / det
    return x, y


def dlt(grid, rows, n_slots):
    """[n_slots, 3] float64 (NaN without two posed views) from the rows `rows` of posed cameras."""
    A = [[] for _ in range(n_slots)]
    for c in np.unique(grid.row_cam[rows]):
        at = rows[grid.row_cam[rows] == c]
        x, y = undistort(int(grid.cam_model[c]), grid.cam_intr[c], grid.row_xy[at])
        P = grid.cam_P[c].reshape(3, 4)
        for s, xi, yi in zip(grid.row_slot[at], x, y):
            A[s] += [xi * P[2] - P[0], yi * P[2] - P[1]]
    out = np.full((n_slots, 3), np.nan)
    for s, a in enumerate(A):
        if len(a) >= 4:
            w = np.linalg.svd(np.array(a))[2][-1]
            out[s] = w[:3] / w[3]
    return out


class Problem:
    """The rows in use, the residuals and the dense Jacobian of the joint problem in dtype T."""

    def __init__(self, grid, T, huber_px):
        self.g, self.T, self.huber = grid, T, huber_px
        g = grid
        self.n_slots = g.n_frames * g.n_traj
        posed = np.flatnonzero(g.cam_posed[g.row_cam] == 1)
        views = np.bincount(g.row_slot[posed], minlength=self.n_slots)
        self.valid = views >= 2
        self.rows = posed[self.valid[g.row_slot[posed]]]          # rows in use, grid order
        self.cam, self.slot = g.row_cam[self.rows], g.row_slot[self.rows]
        self.uv = g.row_xy[self.rows].astype(T)
        frame = g.row_slot // g.n_traj
        count = np.bincount(frame, minlength=g.n_frames)
        total = np.zeros(g.n_frames, dtype=T)
        np.add.at(total, frame, g.row_time.astype(T))
        with np.errstate(invalid="ignore", divide="ignore"):
            self.tau = np.where(count > 0, total / np.maximum(count, 1), T(np.nan))
        self.stamp = g.row_time[self.rows].astype(T) - self.tau[self.slot // g.n_traj]
        self.point = np.cumsum(self.valid) - 1                      # slot -> index among the points
        self.n_points = int(self.valid.sum())

    def evaluate(self, X, delta, V):
        """residuals [m, 2], B [m, 2, 3], a = B V [m, 2], weights [m], F."""
        g, T = self.g, self.T
        lag = self.stamp + delta[self.cam]
        r = np.zeros((len(self.rows), 2), dtype=T)
        B = np.zeros((len(self.rows), 2, 3), dtype=T)
        for c in np.unique(self.cam):
            at = np.flatnonzero(self.cam == c)
            P = X[self.slot[at]] + V[self.slot[at]] * lag[at, None]
            uv, J = project(int(g.cam_model[c]), g.cam_intr[c], g.cam_P[c], P)
            r[at], B[at] = uv - self.uv[at], J
        norm = np.sqrt((r * r).sum(axis=1))
        if self.huber is None:
            w, rho = np.ones(len(r), dtype=T), norm * norm
        else:
            k = T(self.huber)
            out = norm > k
            w = np.where(out, k / np.where(out, norm, 1), 1).astype(T)
            rho = np.where(out, k * (2 * norm - k), norm * norm)
        a = np.einsum("mij,mj->mi", B, V[self.slot])
        return r, B, a, w, rho.sum() / 2

    def step(self, X, delta, V, free):
        """Gauss-Newton step (dX [n_slots, 3], ddelta [n_cams], predicted decrease), F, and the float64 system for the report."""
        r, B, a, w, F = self.evaluate(X, delta, V)
        m, n = len(self.rows), 3 * self.n_points
        col = {int(c): n + k for k, c in enumerate(free)}
        J = np.zeros((2 * m, n + len(free)))
        sw = np.sqrt(w).astype(np.float64)
        p = self.point[self.slot]
        for i in range(2):
            for k in range(3):
                J[2 * np.arange(m) + i, 3 * p + k] = (B[:, i, k]).astype(np.float64) * sw
            for c, at in col.items():
                mine = np.flatnonzero(self.cam == c)
                J[2 * mine + i, at] = a[mine, i].astype(np.float64) * sw[mine]
        rhs = -(r.astype(np.float64) * sw[:, None]).reshape(-1)
        dx = scipy.linalg.lstsq(J, rhs, lapack_driver="gelsy", check_finite=False)[0]  # (QR with column pivoting)
        pred = 0.5 * float(np.sum((J @ dx) ** 2))
        dX = np.zeros((self.n_slots, 3), dtype=self.T)
        dX[self.valid] = dx[:n].reshape(-1, 3)
        dd = np.zeros(self.g.n_cams, dtype=self.T)
        for c, at in col.items():
            dd[c] = dx[at]
        return dX, dd, pred, F, J

    def inner(self, X, delta, V, free, max_offset):
        pred_floor = PRED_ROW * len(self.g.row_cam)
        for _ in range(MAX_INNER):
            dX, dd, pred, F, _ = self.step(X, delta, V, free)
            alpha, kept = 1.0, False
            for _ in range(MAX_HALVINGS + 1):
                Xt = X + self.T(alpha) * dX
                dt = np.clip(delta + self.T(alpha) * dd, -max_offset, max_offset)
                Ft = self.evaluate(Xt, dt, V)[4]
                if np.isfinite(Ft) and Ft <= F + RESOLVE * (1 + F):
                    X, delta, kept = Xt, dt, True
                    break
                alpha /= 2
            if not kept or pred <= pred_floor:
                break
        return X, delta

    def velocity(self, X, gap):
        g = self.g
        V = np.zeros_like(X)
        valid = self.valid.reshape(g.n_frames, g.n_traj)
        Xg = X.reshape(g.n_frames, g.n_traj, 3)
        for f in range(g.n_frames):
            for j in range(g.n_traj):
                if not valid[f, j]:
                    continue
                before = next((f - k for k in range(1, gap + 1) if f - k >= 0 and valid[f - k, j]), None)
                after = next((f + k for k in range(1, gap + 1) if f + k < g.n_frames and valid[f + k, j]), None)
                if before is not None and after is not None:
                    V[f * g.n_traj + j] = (Xg[after, j] - Xg[before, j]) / (self.tau[after] - self.tau[before])
        return V


def estimate(grid, dtype=np.float64, *, reference_cam=None, huber_px=None, max_offset=None, max_neighbour_gap=1, min_rows=30, tol=None,
             max_rounds=10) -> OracleResult:
    """`reference_cam`: index into the cameras of the grid."""
    T = dtype
    pr = Problem(grid, T, huber_px)
    g, n_slots = grid, pr.n_slots
    with_rows = [c for c in range(g.n_cams) if g.cam_posed[c] and (g.row_cam == c).any()]
    ref = with_rows[0] if reference_cam is None else reference_cam
    have = np.flatnonzero(~np.isnan(pr.tau.astype(np.float64)))
    steps = np.sort((np.diff(pr.tau[have]) / np.diff(have)).astype(np.float64))
    interval = steps[(len(steps) - 1) // 2]
    max_offset = T(interval if max_offset is None else max_offset)
    tol = TOL_FRACTION * interval if tol is None else tol

    X = dlt(g, pr.rows, n_slots).astype(T)
    delta = np.zeros(g.n_cams, dtype=T)
    V = np.zeros((n_slots, 3), dtype=T)
    X, delta = pr.inner(X, delta, V, [], max_offset)               # the synchronous start
    r0 = pr.evaluate(X, delta, V)[0]
    V = pr.velocity(X, max_neighbour_gap)
    # (the call asks V != 0, and gets exact zeros where the pixels of neighbouring frames are equal: it solves slot by slot.  The dense
    # solve here returns such points equal to rounding only; the speeds of the scenes are zero or above 0.1 m/s)
    moving = np.sqrt((V * V).sum(axis=1).astype(np.float64)) > 1e-9
    used = np.bincount(pr.cam, minlength=g.n_cams)
    in_motion = np.bincount(pr.cam[moving[pr.slot]], minlength=g.n_cams)
    free = [c for c in range(g.n_cams) if g.cam_posed[c] and c != ref and in_motion[c] >= min_rows]

    rounds, converged, changes = 0, False, []
    prev = delta.copy()
    for k in range(max_rounds):
        if k > 0:
            V = pr.velocity(X, max_neighbour_gap)
        X, delta = pr.inner(X, delta, V, free, max_offset)
        changes.append(float(np.max(np.abs(delta - prev))))
        prev, rounds = delta.copy(), k + 1
        if changes[-1] < tol:
            converged = True
            break

    delta = np.where(np.abs(delta) < tol, T(0), delta)             # below tol: zero
    r, B, a, w, F = pr.evaluate(X, delta, V)
    J = pr.step(X, delta, V, free)[4]
    unit = np.zeros(g.n_cams)
    if free:
        R22 = np.linalg.qr(J, mode="r")[-len(free):, -len(free):]
        inv = np.linalg.inv(R22)
        unit[free] = np.sqrt((inv * inv).sum(axis=1))
    dof = 2 * len(pr.rows) - 3 * pr.n_points - len(free)
    sigma0 = float(np.sqrt(2 * F / dof)) if dof > 0 else float("nan")
    H = np.zeros((n_slots, 3, 3))
    np.add.at(H, pr.slot, np.einsum("m,mij,mik->mjk", w, B, B).astype(np.float64))
    unit_xyz = np.full((n_slots, 3), np.nan)
    unit_xyz[pr.valid] = np.sqrt(np.diagonal(np.linalg.inv(H[pr.valid]), axis1=1, axis2=2))

    offsets, sigma, status = np.full(g.n_cams, np.nan, dtype=T), np.full(g.n_cams, np.nan), np.zeros(g.n_cams, dtype=np.uint8)
    for c in range(g.n_cams):
        if not g.cam_posed[c] or used[c] == 0:
            continue
        if c == ref:
            offsets[c], sigma[c], status[c] = 0, 0.0, 1
        elif c not in free:
            status[c] = 4
        else:
            offsets[c], sigma[c], status[c] = delta[c], sigma0 * unit[c], 3 if abs(delta[c]) >= max_offset else 2
    rms = lambda res: np.array([float(np.sqrt((res[pr.cam == c] ** 2).sum() / used[c])) if g.cam_posed[c] and used[c] else np.nan for c in range(g.n_cams)])
    row_xy, row_used = g.row_xy.astype(T).copy(), np.zeros(len(g.row_cam), dtype=np.uint8)
    still = pr.evaluate(X, delta, np.zeros_like(V))[0]  # pi_c(X) - u: without V the lag moves nothing
    row_xy[pr.rows] = pr.uv - (r - still)
    row_used[pr.rows] = 1
    xyz = np.where(pr.valid[:, None], X, T(np.nan))
    return OracleResult(offsets=offsets, sigma=sigma, status=status, rms_before=rms(r0), rms_after=rms(r), rows=np.where(g.cam_posed == 1, used, 0).astype(np.int64),
                        sigma0_px=sigma0, rounds=rounds, converged=converged, xyz=xyz, valid=pr.valid.astype(np.uint8), velocity=V, frame_time=pr.tau,
                        row_xy=row_xy, row_used=row_used, unit_offset=unit, unit_xyz=unit_xyz, changes=changes, F=float(F))



@dataclass
class Units:
    unit_offset: np.ndarray
    unit_xyz: np.ndarray


def units(grid, res, huber_px=None) -> Units:
    """sqrt((S^-1)_cc) [n_cams] and sqrt(diag H^-1) [n_slots, 3] of the problem at the iterate of a result `res` (of the call or of
    `estimate`): one evaluation and one QR, for scenes whose full run here takes too long."""
    pr = Problem(grid, np.float64, huber_px)
    X = np.where(pr.valid[:, None], np.asarray(res.xyz, dtype=np.float64), 0.0)
    V = np.asarray(res.velocity, dtype=np.float64)
    free = [c for c in range(grid.n_cams) if res.status[c] in (2, 3)]
    delta = np.where(np.isfinite(np.asarray(res.offsets, dtype=np.float64)), np.asarray(res.offsets, dtype=np.float64), 0.0)
    r, B, a, w, F = pr.evaluate(X, delta, V)
    J = pr.step(X, delta, V, free)[4]
    unit = np.zeros(grid.n_cams)
    if free:
        inv = np.linalg.inv(np.linalg.qr(J, mode="r")[-len(free):, -len(free):])
        unit[free] = np.sqrt((inv * inv).sum(axis=1))
    H = np.zeros((pr.n_slots, 3, 3))
    np.add.at(H, pr.slot, np.einsum("m,mij,mik->mjk", w, B, B))
    unit_xyz = np.full((pr.n_slots, 3), np.nan)
    unit_xyz[pr.valid] = np.sqrt(np.diagonal(np.linalg.inv(H[pr.valid]), axis1=1, axis2=2))
    return Units(unit, unit_xyz)
