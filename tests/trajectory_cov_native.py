"""g++ build of caliscope_amd/csrc/trajectory_cov_math.h with trajectory_refine_math.h and trajectory_math.h
(tests/native/trajectory_cov_harness.cpp), the `_solver` hook that runs on it, the calibration report the covariance tests share and
the comparison with tests/trajectory_cov_oracle.py that the CPU and the GPU tests make."""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.reconstruction import TrajDesc, TrajOut
from caliscope_amd.trajectory_refinement import RefineOptions, TrajQuality, TrajRefine
from caliscope_amd.trajectory_uncertainty import (CovarianceOptions, TrajCovOut, TrajectoryCovariance, TrajUncertainty, UncertaintyTables, full_matrices,
                                                  run_uncertain_call, uncertainty_tables)
from tests import trajectory_cov_oracle as CO
from tests import trajectory_refine_native as RN
from tests.native_build import CSRC, NATIVE, load_native

WIDTHS = {0: 9, 1: 9, 2: 6, 3: 6, 4: 9, 5: 6}  # cam_id -> parameters in the report of the shared scene (cam_id 2 is the fisheye)
REFINED = dict(loss="huber", reject_px=5.0)
SIGMA_PX = 0.3


@functools.cache
def harness():
    lib = load_native(NATIVE / "trajectory_cov_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.tch_last_error.restype = C.c_char_p
    lib.tch_reconstruct_trajectories_uncertain.restype = C.c_int
    lib.tch_reconstruct_trajectories_uncertain.argtypes = [C.POINTER(TrajDesc), C.POINTER(TrajRefine), C.POINTER(TrajUncertainty), C.POINTER(TrajOut),
                                                           C.POINTER(TrajQuality), C.POINTER(TrajCovOut)]
    lib.tch_cov_grid.restype = None
    lib.tch_cov_grid.argtypes = [C.c_int32, C.c_int64, _lib.c_uint8_p, _lib.c_int32_p, C.POINTER(TrajUncertainty), _lib.c_double_p, _lib.c_uint8_p,
                                 _lib.c_uint8_p, _lib.c_double_p, C.POINTER(TrajCovOut)]
    return lib


class HarnessUncertainSolver(RN.HarnessRefinedSolver):
    """The `_solver` hook on the g++ build, with `reconstruct_uncertain` as caliscope_amd.trajectory_uncertainty.DeviceUncertainTrajectorySolver."""

    def reconstruct_uncertain(self, grid, options, refine=None, *, camera_array=None, xy_gap=0, xyz_gap=0, filt=None, float32_io=True, want_grids=False):
        self.calls += 1
        lib = harness()
        tables = options if isinstance(options, UncertaintyTables) else uncertainty_tables(grid, camera_array, options)
        return run_uncertain_call(lib.tch_reconstruct_trajectories_uncertain, grid, tables, refine, xy_gap, xyz_gap, filt, float32_io, self.memory_limit,
                                  want_grids, "cba_reconstruct_trajectories_uncertain", lambda: lib.tch_last_error().decode())


def cov_grid(grid, tables: UncertaintyTables, result, quality) -> TrajectoryCovariance:
    """k_traj_cov's thread body over the points and the views of a call made with want_grids=True and without xyz_gap (`quality`
    None: the plain call): what the g++ build computes from the very numbers the device computed from."""
    n_slots = grid.n_slots
    cam_cov = None if tables.cam_cov is None else np.ascontiguousarray(tables.cam_cov, dtype=np.float64)
    keep = [np.ascontiguousarray(tables.cam_nparams, dtype=np.int32), np.ascontiguousarray(tables.cam_const), np.ascontiguousarray(tables.cam_x),
            np.ascontiguousarray(tables.cam_offset, dtype=np.int64)]
    u = TrajUncertainty(cam_nparams=_lib.ptr(keep[0]), cam_const=_lib.ptr(keep[1]), cam_x=_lib.ptr(keep[2]), cam_offset=_lib.ptr(keep[3]),
                        ncp=0 if cam_cov is None else cam_cov.shape[0], cam_cov=_lib.ptr(cam_cov), sigma_px=float(tables.sigma_px))
    out = TrajectoryCovariance(cov=np.full((n_slots, 6), np.nan), cov_calib=None if cam_cov is None else np.full((n_slots, 6), np.nan),
                               cov_status=np.zeros(n_slots, dtype=np.uint8))
    co = TrajCovOut(cov=_lib.ptr(out.cov), cov_calib=_lib.ptr(out.cov_calib), cov_status=_lib.ptr(out.cov_status))
    valid = np.ascontiguousarray((result.valid == 1).astype(np.uint8))
    harness().tch_cov_grid(grid.n_cams, n_slots, _lib.ptr(grid.cam_posed), _lib.ptr(grid.cam_model), C.byref(u), _lib.ptr(np.ascontiguousarray(result.xy_filled)),
                           None if quality is None else _lib.ptr(quality.view_state), _lib.ptr(valid), _lib.ptr(np.ascontiguousarray(result.xyz)), C.byref(co))
    return out


def report(widths: dict, seed: int = 3, scale: float = 1e-8):
    """What `uncertainty_tables` reads of an UncertaintyReport, for cameras `widths` (cam_id -> 6 or 9, in this order): cam_cov_full a
    dense random PSD matrix G G^T * scale, so that cross-camera blocks and offsets matter."""
    ncp = sum(widths.values())
    G = np.random.default_rng(seed).normal(size=(ncp, ncp))
    full = G @ G.T * scale
    full = 0.5 * (full + full.T)
    cameras, at = {}, 0
    for cam_id, w in widths.items():
        cameras[cam_id] = SimpleNamespace(cam_id=cam_id, param_cov=full[at:at + w, at:at + w].copy())
        at += w
    return SimpleNamespace(cameras=cameras, cam_cov_full=full)


@functools.cache
def wide_rig(n_cams: int, n_frames: int = 8, n_traj: int = 5, seed: int = 7):
    """(ImagePoints, CameraArray, report) of a rig on either side of the size at which k_traj_cov stops staging its camera tables in
    LDS: `n_cams` posed pinhole ring cameras, every third one 9-wide in the report, and `n_traj` landmarks of which landmark j is seen
    by the cameras with cam_id % n_traj == j alone (so whole stretches of the camera loops are skipped), 0.3 px of noise."""
    import pandas as pd

    from caliscope_amd.cameras import matrix_to_rvec
    from caliscope_amd.point_data import ImagePoints
    from caliscope_amd.synthetic import ring_camera_array
    from oracle import camera_model as cm

    rng = np.random.default_rng(seed)
    cams = ring_camera_array(n_cams)
    truth = np.array([0.0, 0.0, 0.6]) + rng.uniform(-0.3, 0.3, (n_frames, n_traj, 3))
    rows = []
    for cid, cam in cams.cameras.items():
        j = cid % n_traj
        uv = cm.project_pinhole(truth[:, j], matrix_to_rvec(cam.rotation), cam.translation, cam.matrix, cam.distortions)[0] + rng.normal(0.0, 0.3, (n_frames, 2))
        rows.append(pd.DataFrame({"sync_index": np.arange(n_frames), "cam_id": cid, "object_id": 0, "keypoint_id": j, "img_loc_x": uv[:, 0],
                                  "img_loc_y": uv[:, 1], "frame_time": np.arange(n_frames) / 30.0}))
    return ImagePoints(pd.concat(rows, ignore_index=True)), cams, report({cid: 9 if cid % 3 == 0 else 6 for cid in cams.cameras}, scale=1e-9)


def used_views(grid, result, quality):
    """[n_cams, n_slots] bool: the views in use of a call made with want_grids=True (quality None: the plain call)."""
    if quality is not None:
        return quality.view_state == 1
    return (grid.cam_posed[:, None] == 1) & ~np.isnan(result.xy_filled[:, :, 0]) & (result.valid[None, :] == 1)


def expected_ok(result, quality):
    """Slots whose covariance must be there: a point, and (refined) status converged or iteration cap."""
    ok = result.valid == 1
    return ok & np.isin(quality.status, (1, 2)) if quality is not None else ok


def compare_with_oracle(what, cov, oracle, at, calib: bool):
    """The bar of the issue per slot of `at`: ||cov - oracle||_F <= 1e-12 cond_2(V) ||cov_oracle||_F on the full 3 x 3 matrices, cov_calib
    held to the same figure.  Prints and returns the largest ratio to the bar."""
    bar = 1e-12 * oracle.cond[at] * np.linalg.norm(full_matrices(oracle.cov[at]), axis=(1, 2))
    err = np.linalg.norm(full_matrices(cov.cov[at]) - full_matrices(oracle.cov[at]), axis=(1, 2))
    worst = float((err / bar).max())
    line = f"{what}: {len(at)} slots, cond_2(V) up to {oracle.cond[at].max():.3e}, largest ||cov - oracle||_F / bar = {worst:.3e}"
    if calib:
        err_c = np.linalg.norm(full_matrices(cov.cov_calib[at]) - full_matrices(oracle.cov_calib[at]), axis=(1, 2))
        worst = max(worst, float((err_c / bar).max()))
        line += f", of cov_calib {float((err_c / bar).max()):.3e}"
    print(line)
    assert np.isfinite(cov.cov[at]).all() and (cov.cov_status[at] == 1).all(), what
    assert np.all(err <= bar), what
    if calib:
        assert np.all(err_c <= bar), what
    return worst


def check_scene_against_oracle(solver, grid, cameras, options: CovarianceOptions, refine, what, xyz_gap=0):
    """One call of `solver` on `grid` held against the oracle at the call's own points and views; the rows without a covariance are
    NaN with status 0 or 2.  Returns (result, quality, cov, tables)."""
    tables = uncertainty_tables(grid, cameras, options)
    result, quality, cov = solver.reconstruct_uncertain(grid, tables, RefineOptions(**refine) if refine else None, xyz_gap=xyz_gap, want_grids=True)
    ok = expected_ok(result, quality)
    assert ok.sum() > 0 and (cov.cov_status[ok] == 1).all(), what
    at = np.flatnonzero(cov.cov_status == 1)
    oracle = CO.covariance_grid(grid, cameras, tables, result.xyz, used_views(grid, result, quality), at)
    calib = options.calibration is not None
    compare_with_oracle(what, cov, oracle, at, calib)
    rest = cov.cov_status != 1
    assert np.isnan(cov.cov[rest]).all() and np.isin(cov.cov_status[rest], (0, 2)).all(), what
    assert (cov.cov_status[result.valid == 0] == 0).all() and (cov.cov_status[result.valid == 2] == 2).all(), what
    if calib:
        assert np.isnan(cov.cov_calib[rest]).all(), what
    else:
        assert cov.cov_calib is None, what
    return result, quality, cov, tables


__all__ = ["HarnessUncertainSolver", "REFINED", "SIGMA_PX", "WIDTHS", "check_scene_against_oracle", "compare_with_oracle", "expected_ok", "harness",
           "report", "used_views", "wide_rig"]
