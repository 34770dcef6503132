"""g++ build of caliscope_amd/csrc/trajectory_refine_math.h and trajectory_math.h (tests/native/trajectory_refine_harness.cpp), the
`_solver` hook that runs on it, k_traj_refine alone on a grid given by hand, and the comparisons with tests/refine_oracle.py that
the CPU and the GPU tests share."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.reconstruction import TrajDesc, TrajOut
from caliscope_amd.trajectory_refinement import LOSSES, RefineOptions, TrajectoryQuality, TrajQuality, TrajRefine, refine_struct, run_refined_call
from tests import trajectory_native as N
from tests.native_build import CSRC, NATIVE, load_native


@functools.cache
def harness():
    lib = load_native(NATIVE / "trajectory_refine_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.trh_last_error.restype = C.c_char_p
    lib.trh_reconstruct_trajectories_refined.restype = C.c_int
    lib.trh_reconstruct_trajectories_refined.argtypes = [C.POINTER(TrajDesc), C.POINTER(TrajRefine), C.POINTER(TrajOut), C.POINTER(TrajQuality)]
    lib.trh_refine_grid.restype = None
    lib.trh_refine_grid.argtypes = [C.c_int32, C.c_int64, _lib.c_uint8_p, _lib.c_int32_p, _lib.c_double_p, _lib.c_double_p, _lib.c_double_p,
                                    C.POINTER(TrajRefine), _lib.c_uint8_p, _lib.c_double_p, C.POINTER(TrajQuality)]
    return lib


class HarnessRefinedSolver(N.HarnessTrajectorySolver):
    """The `_solver` hook on the g++ build, with `reconstruct_refined` as caliscope_amd.trajectory_refinement.DeviceRefinedTrajectorySolver."""

    def reconstruct_refined(self, grid, options, *, xy_gap=0, xyz_gap=0, filt=None, float32_io=True, want_grids=False):
        self.calls += 1
        lib = harness()
        return run_refined_call(lib.trh_reconstruct_trajectories_refined, grid, options, xy_gap, xyz_gap, filt, float32_io, self.memory_limit,
                                want_grids, "cba_reconstruct_trajectories_refined", lambda: lib.trh_last_error().decode())


def empty_quality(n_cams: int, n_slots: int):
    """(TrajectoryQuality, its cba_traj_quality)."""
    q = TrajectoryQuality(views=np.zeros(n_slots, dtype=np.int32), rms_px=np.full(n_slots, np.nan), max_px=np.full(n_slots, np.nan),
                          iterations=np.zeros(n_slots, dtype=np.int32), status=np.zeros(n_slots, dtype=np.uint8),
                          view_state=np.zeros((n_cams, n_slots), dtype=np.uint8))
    return q, TrajQuality(views=_lib.ptr(q.views), rms_px=_lib.ptr(q.rms_px), max_px=_lib.ptr(q.max_px), iterations=_lib.ptr(q.iterations),
                          status=_lib.ptr(q.status), view_state=_lib.ptr(q.view_state))


def refine_grid(cam_model, cam_intr, cam_P, xy, start, options: RefineOptions | TrajRefine, cam_posed=None, valid=None):
    """k_traj_refine's thread body over a grid given by hand (no host check in front): xy [n_cams, n_slots, 2], start [n_slots, 3].
    Returns (xyz, TrajectoryQuality)."""
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    n_cams, n_slots = xy.shape[:2]
    cam_model, cam_intr, cam_P = np.ascontiguousarray(cam_model, dtype=np.int32), np.ascontiguousarray(cam_intr, dtype=np.float64), np.ascontiguousarray(cam_P, dtype=np.float64)
    cam_posed = np.ones(n_cams, dtype=np.uint8) if cam_posed is None else np.ascontiguousarray(cam_posed, dtype=np.uint8)
    valid = np.ones(n_slots, dtype=np.uint8) if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    xyz = np.array(start, dtype=np.float64).reshape(n_slots, 3)
    r = options if isinstance(options, TrajRefine) else refine_struct(options)
    q, cq = empty_quality(n_cams, n_slots)
    harness().trh_refine_grid(n_cams, n_slots, _lib.ptr(cam_posed), _lib.ptr(cam_model), _lib.ptr(cam_intr), _lib.ptr(cam_P), _lib.ptr(xy), C.byref(r),
                              _lib.ptr(valid), _lib.ptr(xyz), C.byref(cq))
    return xyz, q


def compare_with_oracle(what, xyz, quality, oracle, at):
    """The agreement the issue asks for, on the slots `at` (refined by both): positions within 1e-6 m, the rejected sets identical,
    rms_px and max_px within (position difference x the largest ||d e_c / d X||_2 of the oracle) + 1e-9.  Prints the largest figures."""
    diff = np.linalg.norm(xyz[at] - oracle.xyz[at], axis=1)
    bound = diff * oracle.jac_norm[at] + 1e-9
    rms, top = np.abs(quality.rms_px[at] - oracle.rms_px[at]), np.abs(quality.max_px[at] - oracle.max_px[at])
    print(f"{what}: {len(at)} slots, max |x - oracle| = {diff.max():.3e} m (bar 1e-6), max |rms - oracle| = {rms.max():.3e} px, "
          f"max |max_px - oracle| = {top.max():.3e} px, smallest bound {bound.min():.3e}, status counts {np.bincount(quality.status, minlength=4).tolist()}, "
          f"evaluations {int(quality.iterations.sum())}")
    assert np.array_equal(quality.view_state, oracle.view_state), what
    assert np.array_equal(quality.views, oracle.views), what
    assert diff.max() <= 1e-6, what
    assert np.all(rms <= bound) and np.all(top <= bound), what


def check_placement(solver, options):
    """The one call with xyz_gap = 3 and a filter against WorldPoints.fill_gaps(3).smooth(..) of the host chain on the refined table
    of a call without either, bit for bit (the line of pandas and the recurrence of scipy in their own order of operations, as in
    tests/test_reconstruction.py); what the 3-D fill added has no views and no reprojection error.  `solver`: both hooks."""
    from caliscope_amd.reconstruction import reconstruct_trajectories
    from caliscope_amd.trajectory_refinement import QUALITY_COLUMNS
    from tests import refine_scenes as RS

    sc, smooth, opt = RS.scene(), (30.0, 6.0, 2), RefineOptions(**options)
    base, base_q = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, refine=opt, return_quality=True, _solver=solver)
    got, got_q = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, xyz_gap_fill=3, smooth=smooth, refine=opt, return_quality=True,
                                          _solver=solver)
    plain = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, _solver=solver)
    want = base.fill_gaps(3).smooth(*smooth)
    assert len(want) == len(base) + 6
    assert list(got.df.columns) == N.WORLD_COLS == list(plain.df.columns) and list(got_q.columns) == list(QUALITY_COLUMNS)
    assert np.array_equal(N.keyed(got.df), N.keyed(want.df), equal_nan=True)
    assert not np.array_equal(N.keyed(base.df)[:, 3:6], N.keyed(plain.df)[:, 3:6])  # (the refinement moved the points)
    keys = ["sync_index", "object_id", "keypoint_id"]
    assert np.array_equal(got_q[keys].to_numpy(), got.df[keys].to_numpy()) and np.array_equal(base_q[keys].to_numpy(), base.df[keys].to_numpy())
    merged = got_q.merge(base_q[keys].assign(was=True), on=keys, how="left")
    filled = merged["was"].isna().to_numpy()
    assert filled.sum() == 6 and (got_q["n_views"][filled] == 0).all() and got_q["reproj_rms_px"][filled].isna().all()
    assert got_q["reproj_max_px"][filled].isna().all() and (got_q["n_rejected"][filled] == 0).all() and (got_q["status"][filled] == 0).all()
    kept = got_q[~filled].reset_index(drop=True)
    assert kept.drop(columns=keys).equals(base_q.drop(columns=keys))  # the quality is that of the refinement, whatever follows it
    f = 8  # the table of rejected cameras names cam_ids
    row = base_q[(base_q["sync_index"] == f + RS.SYNC0) & (base_q["object_id"] == 0) & (base_q["keypoint_id"] == 0)].iloc[0]
    assert row["rejected_cam_ids"] == (f % 6, (f + 3) % 6) and row["n_rejected"] == 2 and row["n_views"] == 4 and row["status"] in (1, 2)


def check_point_behind_a_camera(solver):
    """tests/refine_scenes.behind_camera_case through the whole call: status 3, the bits of the unrefined call, no error."""
    from caliscope_amd.reconstruction import trajectory_grid
    from tests import refine_scenes as RS

    ip, cams, point = RS.behind_camera_case()
    grid = trajectory_grid(ip, cams)
    base = solver.reconstruct(grid)
    res, q = solver.reconstruct_refined(grid, RefineOptions(reject_px=5.0))
    depth = grid.cam_P.reshape(3, 3, 4)[:, 2, :3] @ base.xyz[0] + grid.cam_P.reshape(3, 3, 4)[:, 2, 3]
    assert base.valid.tolist() == [1] and np.allclose(base.xyz[0], point, atol=1e-6) and depth[2] < -0.29 and (depth[:2] > 1.0).all()
    assert res.valid.tolist() == [1] and q.status.tolist() == [3] and N.bits(res.xyz).tolist() == N.bits(base.xyz).tolist()
    assert q.views.tolist() == [3] and q.iterations.tolist() == [1] and np.isnan(q.rms_px[0]) and np.isnan(q.max_px[0])
    assert q.view_state[:, 0].tolist() == [1, 1, 1]


def check_slot_count(solver, n_slots, whole, options):
    """A grid of exactly `n_slots` slots (tests/refine_scenes.relabelled) against the first `n_slots` slots of the scene's own call
    `whole` = (result, quality): the same cells, the same cameras, so the same bits."""
    from caliscope_amd.reconstruction import trajectory_grid
    from tests import refine_scenes as RS

    grid = trajectory_grid(RS.relabelled(RS.scene(), n_slots), RS.scene().cameras)
    assert (grid.n_traj, grid.n_frames, grid.n_slots, grid.n_cams) == (1, n_slots, n_slots, 7)
    res, q = solver.reconstruct_refined(grid, RefineOptions(**options))
    full, full_q = whole
    assert res.valid.tobytes() == full.valid[:n_slots].tobytes() and res.xyz.tobytes() == full.xyz[:n_slots].tobytes()
    for name in ("views", "rms_px", "max_px", "iterations", "status"):
        assert getattr(q, name).tobytes() == getattr(full_q, name)[:n_slots].tobytes(), name
    assert np.array_equal(q.view_state, full_q.view_state[:, :n_slots]) and (q.view_state == 2).any()


__all__ = ["HarnessRefinedSolver", "LOSSES", "compare_with_oracle", "empty_quality", "harness", "refine_grid"]
