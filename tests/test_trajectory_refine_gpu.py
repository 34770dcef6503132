"""cba_reconstruct_trajectories_refined on the device (k_traj_refine of csrc/trajectory_lib.hip) on the recording of
tests/refine_scenes.py — 300 slots, two workgroups, the second partly filled — against scipy (tests/refine_oracle.py) started from the
device's own DLT points, the place of the refinement in the call against the host chain, and the entry point that was restructured
around it against what it returned before.  The checks are those of tests/test_trajectory_refine.py, where they run on the g++ build."""
import functools

import numpy as np
import pytest

from caliscope_amd.reconstruction import DeviceTrajectorySolver, filter_coefficients, reconstruct_trajectories, trajectory_grid
from caliscope_amd.trajectory_refinement import DeviceRefinedTrajectorySolver, RefineOptions
from tests import refine_oracle as RO
from tests import refine_scenes as RS
from tests import trajectory_native as N
from tests import trajectory_refine_native as RN
from tests.trajectory_native import _compare, _time_bound_after_fill

pytestmark = pytest.mark.gpu

OPTIONS = dict(f_scale=1.0, reject_px=5.0)


class DeviceSolver(DeviceTrajectorySolver, DeviceRefinedTrajectorySolver):
    """Both hooks on the device."""


@functools.cache
def _grid():
    sc = RS.scene()
    return trajectory_grid(sc.image_points, sc.cameras)


@functools.cache
def _base():
    return DeviceSolver().reconstruct(_grid(), want_grids=True)


@functools.cache
def _oracle(loss):
    base = _base()
    return RO.refine_grid(_grid(), RS.scene().cameras, base.xy_filled, base.xyz, base.valid, loss=loss, **OPTIONS)


@functools.cache
def _refined(loss="huber"):
    return DeviceSolver().reconstruct_refined(_grid(), RefineOptions(loss=loss, **OPTIONS))


@pytest.mark.parametrize("loss", ["linear", "huber", "soft_l1"])
def test_refinement_agrees_with_scipy(loss):
    (res, q), orc, base = _refined(loss), _oracle(loss), _base()
    at = np.flatnonzero(base.valid == 1)
    assert np.array_equal(res.valid, base.valid) and (orc.status[at] == 1).all()
    RN.compare_with_oracle(f"device, {loss}", res.xyz, q, orc, at)


def test_view_state_and_quality():
    """What compare_with_oracle does not look at: the slots without a point, the unposed camera, statuses and evaluations; and the
    g++ build of the same routine, which contracts its products differently (the points agree to rounding, the decisions exactly)."""
    (res, q), base = _refined("huber"), _base()
    at, off = np.flatnonzero(base.valid == 1), np.flatnonzero(base.valid == 0)
    assert len(off) == 6 and (q.views[off] == 0).all() and (q.status[off] == 0).all() and (q.iterations[off] == 0).all()
    assert (q.view_state[:, off] == 0).all() and np.isnan(q.rms_px[off]).all() and np.isnan(q.max_px[off]).all() and np.isnan(res.xyz[off]).all()
    assert (q.view_state[6] == 0).all() and np.isin(q.status[at], (1, 2)).all() and (q.iterations[at] >= 2).all()
    assert np.array_equal(q.views, (q.view_state == 1).sum(axis=0)) and (q.view_state == 2).sum() == RS.scene().outlier[:6].sum()
    cpu, cpu_q = RN.HarnessRefinedSolver().reconstruct_refined(_grid(), RefineOptions(**OPTIONS))
    assert np.array_equal(q.view_state, cpu_q.view_state) and np.allclose(res.xyz[at], cpu.xyz[at], rtol=0, atol=1e-8)
    assert np.allclose(q.rms_px[at], cpu_q.rms_px[at], rtol=0, atol=1e-5) and np.allclose(q.max_px[at], cpu_q.max_px[at], rtol=0, atol=1e-5)


def test_the_fill_and_the_filter_run_on_the_refined_points():
    RN.check_placement(DeviceSolver(), OPTIONS)


def test_two_calls_return_the_same_bytes():
    kw = dict(xy_gap=0, xyz_gap=2, filt=filter_coefficients((30.0, 6.0, 2)), want_grids=True)
    (a, qa), (b, qb) = (DeviceSolver().reconstruct_refined(_grid(), RefineOptions(**OPTIONS), **kw) for _ in range(2))
    for name in ("xyz", "valid", "slot_time", "frame_time", "xy_filled", "ft_filled"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    for name in ("views", "rms_px", "max_px", "iterations", "status", "view_state"):
        assert getattr(qa, name).tobytes() == getattr(qb, name).tobytes(), name
    assert set(np.unique(a.valid)) == {0, 1, 2} and set(np.unique(qa.view_state)) == {0, 1, 2}


def test_the_entry_point_without_refinement_still_equals_the_host_chain():
    """The comparison of tests/test_reconstruction_gpu.py on this scene: cba_reconstruct_trajectories now runs through the function it
    shares with the refined call, and must launch and return what it did."""
    sc = RS.scene()
    filled = sc.image_points.fill_gaps(3)
    base = filled.triangulate(sc.cameras)
    got = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=3)
    assert list(got.df.columns) == N.WORLD_COLS and len(got) == 300  # (the 2-D fill closes every hole of the scene)
    _compare(got, base, N.frame_time_bound(filled.df, N.keyed(base.df)[:, 0].astype(np.int64)), "xy_gap 3")
    smooth = (30.0, 6.0, 2)
    base = sc.image_points.triangulate(sc.cameras)
    got = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, xyz_gap_fill=3, smooth=smooth)
    want = base.fill_gaps(3)
    assert len(base) == 294 and len(want) == 300
    _compare(got, want.smooth(*smooth), _time_bound_after_fill(sc.image_points.df, base), "xy_gap 0, xyz_gap 3, filter")


def test_a_dlt_point_behind_a_camera_goes_through_the_call_unchanged():
    """A valid input whose handling is defined (status 3, the DLT bits, no error): nothing here is out of bounds or undefined, the
    thread stops after its first pass over the cameras."""
    RN.check_point_behind_a_camera(DeviceSolver())


@pytest.mark.parametrize("n_slots", [256, 257])
def test_a_grid_of_one_workgroup_and_of_one_thread_more(n_slots):
    RN.check_slot_count(DeviceSolver(), n_slots, _refined("huber"), OPTIONS)
