"""What cba_reconstruct_trajectories_refined is held to: `scipy.optimize.least_squares` per slot on the pixel residuals of
`oracle.camera_model.project_pinhole` / `project_fisheye`, with the same loss and f_scale, from the call's own DLT point, tolerances
at 1e-14, and the rejection rounds of include/caliscope/trajectory_refine.h restated around it in Python.  None of it is the code
under test."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from scipy.optimize import least_squares

from caliscope_amd.cameras import matrix_to_rvec
from oracle import camera_model as cm


@dataclass
class OracleResult:
    xyz: np.ndarray         # [n_slots, 3] (the start point where nothing was refined)
    view_state: np.ndarray  # [n_cams, n_slots] uint8
    views: np.ndarray       # [n_slots]
    rms_px: np.ndarray
    max_px: np.ndarray
    status: np.ndarray      # 0 no point, 1 refined, 3 kept the DLT point (the oracle has no iteration cap)
    jac_norm: np.ndarray    # [n_slots] the largest ||d e_c / d X||_2 over the views in use at the end
    decisions: list = field(default_factory=list)  # (slot, [camera ranks in use], [d_c], rank dropped or None) per rejection decision


def camera_models(grid, camera_array):
    """Per camera rank: None (unposed) or (project, rvec, tvec, K, dist, R)."""
    out = []
    for cid, posed in zip(grid.cam_ids, grid.cam_posed):
        cam = camera_array.cameras[int(cid)]
        if not posed:
            out.append(None)
            continue
        R = np.asarray(cam.rotation, dtype=np.float64)
        out.append((cm.project_fisheye if cam.fisheye else cm.project_pinhole, matrix_to_rvec(R), np.asarray(cam.translation, dtype=np.float64).ravel(),
                    np.asarray(cam.matrix, dtype=np.float64), np.asarray(cam.distortions, dtype=np.float64).ravel(), R, bool(cam.fisheye)))
    return out


def _residual_and_jacobian(X, views):
    """e [2 n] and d e / d X [2 n, 3] of the views (model, u, v) at X."""
    e, J = [], []
    for (project, rvec, tvec, K, dist, R, fisheye), u, v in views:
        px, jac = project(X.reshape(1, 3), rvec, tvec, K, dist, jacobian=True)
        e.append(px[0] - (u, v))
        J.append(jac[:, 11:14] @ R if fisheye else jac[:, 3:6] @ R)  # d pixel / d tvec = d pixel / d X_cam
    return np.concatenate(e), np.vstack(J)


def refine_slot(models, ranks, pixels, x0, loss, f_scale, reject_px, max_reject, min_views):
    """(x, {rank: state}, d of the views in use, jac_norm, status, decisions) of one slot; `ranks` the posed cameras with a cell,
    ascending, `pixels` their cells."""
    used = list(ranks)
    uv = {c: p for c, p in zip(ranks, pixels)}
    state = {c: 1 for c in ranks}
    depth = [(models[c][5] @ x0 + models[c][2])[2] for c in used]
    if min(depth) <= 0.0:
        return x0, state, None, np.nan, 3, []
    x, decisions, rounds = np.array(x0, dtype=np.float64), [], 0
    while True:
        views = [(models[c], *uv[c]) for c in used]
        sol = least_squares(lambda p: _residual_and_jacobian(p, views)[0], x, jac=lambda p: _residual_and_jacobian(p, views)[1], loss=loss,
                            f_scale=f_scale, xtol=1e-14, ftol=1e-14, gtol=1e-14, method="trf", max_nfev=500)
        x = sol.x
        e, J = _residual_and_jacobian(x, views)
        d = np.sqrt((e.reshape(-1, 2) ** 2).sum(axis=1))
        if not reject_px > 0.0:
            break
        worst = int(np.argmax(d))  # the first of equals: the lowest rank
        drop = rounds < max_reject and d[worst] > reject_px and len(used) - 1 >= min_views
        if rounds < max_reject:
            decisions.append((list(used), d.copy(), used[worst] if drop else None))
        if not drop:
            break
        state[used[worst]] = 2
        used.pop(worst)
        rounds += 1
    jac_norm = max(np.linalg.norm(J[2 * i:2 * i + 2], 2) for i in range(len(used)))
    return x, state, d, jac_norm, 1, decisions


def refine_grid(grid, camera_array, xy, start, valid, loss="huber", f_scale=2.0, reject_px=0.0, max_reject=2, min_views=2) -> OracleResult:
    """The oracle over a grid: `xy` [n_cams, n_slots, 2] the observation grid of the call, `start` [n_slots, 3] and `valid` [n_slots]
    its unrefined points."""
    models = camera_models(grid, camera_array)
    n_slots = grid.n_slots
    out = OracleResult(xyz=np.array(start, dtype=np.float64), view_state=np.zeros((grid.n_cams, n_slots), dtype=np.uint8),
                       views=np.zeros(n_slots, dtype=np.int64), rms_px=np.full(n_slots, np.nan), max_px=np.full(n_slots, np.nan),
                       status=np.zeros(n_slots, dtype=np.int64), jac_norm=np.full(n_slots, np.nan))
    for s in np.flatnonzero(valid == 1):
        ranks = [c for c in range(grid.n_cams) if models[c] is not None and not np.isnan(xy[c, s, 0])]
        x, state, d, jac_norm, status, decisions = refine_slot(models, ranks, [xy[c, s] for c in ranks], start[s], loss, f_scale, reject_px,
                                                               max_reject, min_views)
        out.xyz[s], out.status[s], out.jac_norm[s] = x, status, jac_norm
        for c, v in state.items():
            out.view_state[c, s] = v
        out.views[s] = sum(1 for v in state.values() if v == 1)
        if d is not None:
            out.rms_px[s], out.max_px[s] = np.sqrt(np.mean(d**2)), d.max()
        out.decisions += [(int(s), *dec) for dec in decisions]
    return out


def objective(grid, camera_array, xy, view_state, xyz, loss, f_scale) -> np.ndarray:
    """F [n_slots] of include/caliscope/trajectory_refine.h at `xyz` over the views with view_state == 1 (NaN where there are none):
    scipy's rho per scalar residual, written out from its documentation."""
    models = camera_models(grid, camera_array)
    F = np.full(grid.n_slots, np.nan)
    for s in range(grid.n_slots):
        views = [(models[c], *xy[c, s]) for c in range(grid.n_cams) if view_state[c, s] == 1]
        if not views:
            continue
        z = (_residual_and_jacobian(xyz[s], views)[0] / f_scale) ** 2
        rho = {"linear": z, "huber": np.where(z <= 1, z, 2 * np.sqrt(z) - 1), "soft_l1": 2 * (np.sqrt(1 + z) - 1), "cauchy": np.log1p(z),
               "arctan": np.arctan(z)}[loss]
        F[s] = 0.5 * f_scale**2 * rho.sum()
    return F
