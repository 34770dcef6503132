"""numpy restatements of include/caliscope/trajectory_skeleton.h for the tests: the lengths with np.sort, and the adjustment of a
(frame, component) twice, by routes that share no linear algebra:

    gauss_newton   Gauss-Newton on the whitened, stacked Jacobian by QR (np.linalg.lstsq), the covariance from R^-1 R^-T of its QR factor
    scipy_newton   scipy.optimize.least_squares, then Newton steps on the normal equations (np.linalg.solve), the covariance inv(J^T J)

Both iterate until the decrement -g^T delta stops falling: the rounding floor, not a tolerance.  Neither is damped, so they are
oracles only where plain Gauss-Newton converges: noise at most 10 % of a segment's length and given lengths within 3 sigma of the
truth (further out the contraction rises above 0.5 and with noise comparable with the segments the two end in different minima).
`adjust` asserts that contraction on every problem it solves."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.optimize import least_squares

MAD_SCALE = 1.4826


def full(rows):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    return rows[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def rows6(mats):
    mats = np.asarray(mats).reshape(-1, 3, 3)
    return np.stack([mats[:, 0, 0], mats[:, 0, 1], mats[:, 0, 2], mats[:, 1, 1], mats[:, 1, 2], mats[:, 2, 2]], axis=1)


def components(n_traj, seg_traj):
    """(n_comp, traj_comp): union-find, the components numbered by their smallest trajectory, -1 for a trajectory in no segment."""
    parent = np.arange(n_traj)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    used = np.zeros(n_traj, dtype=bool)
    for a, b in np.asarray(seg_traj).reshape(-1, 2):
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
        used[a] = used[b] = True
    comp = np.full(n_traj, -1, dtype=np.int32)
    n_comp = 0
    for j in range(n_traj):
        if used[j]:
            r = find(j)
            if r == j:
                comp[j] = n_comp
                n_comp += 1
            else:
                comp[j] = comp[r]
    return n_comp, comp


def lower_median(v):
    return np.sort(v)[(len(v) - 1) // 2]


def unit(a, b):
    d = a - b
    n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])  # (one product, one sum at a time: the bits of the library's)
    return n, (d / n if n > 0 else np.zeros(3))


def lengths(n_frames, n_traj, xyz, cov, measured, seg_traj, seg_length, trim):
    """length, med, mad, frames per segment."""
    xyz = xyz.reshape(n_frames, n_traj, 3)
    R = full(cov).reshape(n_frames, n_traj, 3, 3)
    meas = measured.reshape(n_frames, n_traj) == 1
    n_seg = len(seg_traj)
    length, med, mad, frames = np.full(n_seg, np.nan), np.full(n_seg, np.nan), np.full(n_seg, np.nan), np.zeros(n_seg, dtype=np.int64)
    for s, (a, b) in enumerate(seg_traj):
        fs = np.flatnonzero(meas[:, a] & meas[:, b])
        frames[s] = len(fs)
        length[s] = seg_length[s]
        if not len(fs):
            continue
        d, v = np.zeros(len(fs)), np.zeros(len(fs))
        for i, f in enumerate(fs):
            d[i], u = unit(xyz[f, a], xyz[f, b])
            S = R[f, a] + R[f, b]
            v[i] = u @ S @ u if d[i] > 0 else np.trace(S) / 3.0
        med[s] = lower_median(d)
        mad[s] = lower_median(np.abs(d - med[s]))
        if np.isnan(seg_length[s]):
            keep = d == med[s] if mad[s] == 0 else np.abs(d - med[s]) <= trim * MAD_SCALE * mad[s]
            length[s] = np.sum(d[keep] / v[keep]) / np.sum(1.0 / v[keep])
    return length, med, mad, frames


class Problem:
    """One (frame, component): Z [m, 3], R [m, 3, 3], segs [(a, b, L, sigma)] over the m unknowns.  The whitened residual vector is
    (W_i (X_i - Z_i))_i, W_i = chol(R_i)^-1, then ((|X_a - X_b| - L) / sigma)_s; F = |r|^2."""

    def __init__(self, Z, R, segs):
        self.Z, self.segs, self.m = Z, segs, len(Z)
        self.W = np.linalg.inv(np.linalg.cholesky(R))
        self.a, self.b = np.array([s[0] for s in segs]), np.array([s[1] for s in segs])
        self.L, self.sg = np.array([s[2] for s in segs]), np.array([s[3] for s in segs])
        self.J0 = np.zeros((3 * self.m + len(segs), 3 * self.m))
        for i in range(self.m):
            self.J0[3 * i:3 * i + 3, 3 * i:3 * i + 3] = self.W[i]

    def _units(self, X):
        d = X[self.a] - X[self.b]
        n = np.sqrt(np.sum(d * d, axis=1))
        return n, d / np.where(n > 0, n, 1.0)[:, None]  # (coincident ends: d = 0, so u = 0)

    def residuals(self, x):
        X = x.reshape(self.m, 3)
        return np.concatenate([np.einsum("ijk,ik->ij", self.W, X - self.Z).reshape(-1), (self._units(X)[0] - self.L) / self.sg])

    def jacobian(self, x):
        J = self.J0.copy()
        u = self._units(x.reshape(self.m, 3))[1] / self.sg[:, None]
        rows = 3 * self.m + np.arange(len(self.segs))
        for c in range(3):
            J[rows, 3 * self.a + c] = u[:, c]
            J[rows, 3 * self.b + c] = -u[:, c]
        return J


def _iterate(prob, x, step):
    """x <- x + step(J, r) until the decrement |J delta|^2 stops falling; returns x and the largest contraction
    sqrt(dec_k / dec_{k-1}) seen while dec_{k-1} is above the rounding floor."""
    last, contraction = np.inf, 0.0
    for _ in range(100):
        r, J = prob.residuals(x), prob.jacobian(x)
        delta = step(J, r)
        dec = float((J @ delta) @ (J @ delta))
        if dec >= last or dec == 0.0:
            if dec == 0.0:
                x = x + delta
            break
        if last < np.inf and last > 1e-20:
            contraction = max(contraction, np.sqrt(dec / last))
        x, last = x + delta, dec
    else:
        raise AssertionError("the oracle's Gauss-Newton did not reach its floor in 100 steps")
    return x, contraction


def gauss_newton(prob):
    x, contraction = _iterate(prob, prob.Z.reshape(-1).copy(), lambda J, r: np.linalg.lstsq(J, -r, rcond=None)[0])
    Rq = np.linalg.qr(prob.jacobian(x), mode="r")
    Ri = np.linalg.inv(Rq)
    return x, Ri @ Ri.T, contraction


def scipy_newton(prob):
    x0 = prob.Z.reshape(-1).copy()
    sol = least_squares(prob.residuals, x0, jac=prob.jacobian, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale="jac")
    x, contraction = _iterate(prob, sol.x, lambda J, r: np.linalg.solve(J.T @ J, -(J.T @ r)))
    J = prob.jacobian(x)
    return x, np.linalg.inv(J.T @ J), contraction


@dataclass
class Adjusted:
    pos: np.ndarray
    pos_cov: np.ndarray
    status: np.ndarray
    length: np.ndarray
    med: np.ndarray
    mad: np.ndarray
    frames: np.ndarray
    len_before: np.ndarray
    w_before: np.ndarray
    len_after: np.ndarray
    chi2: np.ndarray
    rows: np.ndarray
    active: np.ndarray   # [n_frames, n_comp] whether anything is active
    contraction: float


def adjust(method, n_frames, n_traj, xyz, cov, measured, seg_traj, seg_length, seg_sigma, trim, max_contraction=0.5):
    """The whole call by `method` (gauss_newton or scipy_newton)."""
    seg_traj = np.asarray(seg_traj).reshape(-1, 2)
    n_seg, n_slots = len(seg_traj), n_frames * n_traj
    n_comp, comp = components(n_traj, seg_traj)
    length, med, mad, frames = lengths(n_frames, n_traj, xyz, cov, measured, seg_traj, seg_length, trim)
    meas = measured.reshape(n_frames, n_traj) == 1
    Zall, Rall = xyz.reshape(n_frames, n_traj, 3), full(cov).reshape(n_frames, n_traj, 3, 3)
    pos, pos_cov = np.full((n_slots, 3), np.nan), np.full((n_slots, 6), np.nan)
    pos[measured == 1], pos_cov[measured == 1] = xyz[measured == 1], cov[measured == 1]
    status = np.where(measured == 1, 2, 0).astype(np.uint8)
    out = Adjusted(pos, pos_cov, status, length, med, mad, frames, np.full((n_frames, n_seg), np.nan), np.full((n_frames, n_seg), np.nan),
                   np.full((n_frames, n_seg), np.nan), np.zeros((n_frames, n_comp)), np.zeros((n_frames, n_comp), dtype=np.int32),
                   np.zeros((n_frames, n_comp), dtype=bool), 0.0)
    seg_comp = comp[seg_traj[:, 0]] if n_seg else np.zeros(0, dtype=np.int32)
    for f in range(n_frames):
        act = meas[f, seg_traj[:, 0]] & meas[f, seg_traj[:, 1]] & np.isfinite(length) if n_seg else np.zeros(0, dtype=bool)
        for k in range(n_comp):
            ss = np.flatnonzero(act & (seg_comp == k))
            if not len(ss):
                continue
            trajs = np.unique(seg_traj[ss])
            loc = {int(t): i for i, t in enumerate(trajs)}
            segs = [(loc[int(seg_traj[s, 0])], loc[int(seg_traj[s, 1])], length[s], seg_sigma[s]) for s in ss]
            prob = Problem(Zall[f, trajs], Rall[f, trajs], segs)
            x, P, contraction = method(prob)
            assert contraction < max_contraction, f"frame {f} component {k}: Gauss-Newton contraction {contraction:.2f}"
            out.contraction = max(out.contraction, contraction)
            X = x.reshape(-1, 3)
            slots = f * n_traj + trajs
            out.pos[slots] = X
            out.pos_cov[slots] = rows6(np.stack([P[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(len(trajs))]))
            out.status[slots] = 1
            r = prob.residuals(x)
            out.chi2[f, k], out.rows[f, k], out.active[f, k] = r @ r, len(ss), True
            for (a, b, L, sg), s in zip(segs, ss):
                d, u = unit(prob.Z[a], prob.Z[b])
                out.len_before[f, s] = d
                out.w_before[f, s] = (d - L) / np.sqrt(sg * sg + u @ (Rall[f, trajs[a]] + Rall[f, trajs[b]]) @ u)
                out.len_after[f, s] = unit(X[a], X[b])[0]
    return out


def disagreement(a, b):
    """(means in sqrt(tr P) of the slot, covariances as relative Frobenius distance), the largest over the adjusted slots of b."""
    at = b.status == 1
    if not at.any():
        return 0.0, 0.0
    Pa, Pb = full(a.pos_cov[at]), full(b.pos_cov[at])
    mean = np.linalg.norm(a.pos[at] - b.pos[at], axis=1) / np.sqrt(np.trace(Pb, axis1=1, axis2=2))
    cov = np.linalg.norm((Pa - Pb).reshape(-1, 9), axis=1) / np.linalg.norm(Pb.reshape(-1, 9), axis=1)
    return float(mean.max()), float(cov.max())
