"""What cba_reconstruct_trajectories_uncertain is held to: the formula of include/caliscope/trajectory_uncertainty.h evaluated densely
per slot with numpy.linalg, B_c and A_c from the analytic Jacobians of `oracle.camera_model.project_pinhole` / `project_fisheye`
(cv2's column layout) mapped to the bundle-adjustment parameterisation (rvec, tvec and, for a 9-wide camera, s, k1, k2 with
d/ds = fx0 d/dfx + fy0 d/dfy).  None of it is ba_math.h or the code under test."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import refine_oracle as RO


@dataclass
class OracleCovariance:
    cov: np.ndarray        # [n_slots, 6] xx xy xz yy yz zz, NaN where nothing was computed
    cov_calib: np.ndarray  # [n_slots, 6] (zeros where cam_cov is None)
    cov_noise: np.ndarray  # [n_slots, 6]
    cond: np.ndarray       # [n_slots] cond_2(V)
    computed: np.ndarray   # [n_slots] bool


def jacobians(model, X, width):
    """B (2 x 3) and A (2 x width) of one camera of `refine_oracle.camera_models` at X, in pixels."""
    project, rvec, tvec, K, dist, R, fisheye = model
    _, J = project(np.asarray(X, dtype=np.float64).reshape(1, 3), rvec, tvec, K, dist, jacobian=True)
    d_rvec, d_tvec = (J[:, 8:11], J[:, 11:14]) if fisheye else (J[:, 0:3], J[:, 3:6])
    A = [d_rvec, d_tvec]
    if width == 9:
        assert not fisheye
        A.append(np.column_stack([K[0, 0] * J[:, 6] + K[1, 1] * J[:, 7], J[:, 10], J[:, 11]]))  # s (at s = 1: fx = fx0), k1, k2
    return d_tvec @ R, np.hstack(A)


def rows6(S):
    return np.array([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])


def covariance_grid(grid, camera_array, tables, xyz, used, at) -> OracleCovariance:
    """The oracle on the slots `at`: `xyz` [n_slots, 3] the points of the call, `used` [n_cams, n_slots] bool its views in use,
    `tables` the UncertaintyTables of the call (widths, offsets, cam_cov, sigma_px)."""
    models = RO.camera_models(grid, camera_array)
    n = grid.n_slots
    out = OracleCovariance(cov=np.full((n, 6), np.nan), cov_calib=np.full((n, 6), np.nan), cov_noise=np.full((n, 6), np.nan), cond=np.full(n, np.nan),
                           computed=np.zeros(n, dtype=bool))
    ncp = 0 if tables.cam_cov is None else tables.cam_cov.shape[0]
    for s in at:
        V, parts = np.zeros((3, 3)), []
        for c in np.flatnonzero(used[:, s]):
            B, A = jacobians(models[c], xyz[s], int(tables.cam_nparams[c]))
            V += B.T @ B
            parts.append((c, B, A))
        Vinv = np.linalg.inv(V)
        M = np.zeros((3, ncp))
        for c, B, A in parts:
            off = int(tables.cam_offset[c])
            if tables.cam_cov is not None and off >= 0:
                M[:, off:off + A.shape[1]] = Vinv @ B.T @ A
        calib = M @ tables.cam_cov @ M.T if tables.cam_cov is not None else np.zeros((3, 3))
        noise = tables.sigma_px**2 * Vinv
        out.cov[s], out.cov_calib[s], out.cov_noise[s], out.cond[s], out.computed[s] = rows6(noise + calib), rows6(calib), rows6(noise), np.linalg.cond(V, 2), True
    return out
