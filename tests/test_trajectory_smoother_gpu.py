"""cba_smooth_trajectories and cba_reconstruct_trajectories_smoothed on the device (k_traj_smooth of csrc/trajectory_lib.hip): the
scenes of tests/trajectory_smooth_scenes.py — EDGE with 257 trajectories, a second workgroup with one live thread and a second wave
that opens at trajectory 64 — against the two numpy restatements of tests/trajectory_smooth_oracle.py and against the g++ build of the
same thread body fed the same arrays, the tracks drawn from the model, and the smoothed reconstruction of the tests/refine_scenes.py
recording.  The bar is that of tests/trajectory_smooth_native.py: ten times the disagreement of the two restatements."""
import functools

import numpy as np
import pytest

from caliscope_amd.reconstruction import trajectory_grid
from caliscope_amd.trajectory_refinement import RefineOptions
from caliscope_amd.trajectory_smoother import DeviceTrajectorySmoother, SmootherOptions
from caliscope_amd.trajectory_uncertainty import CovarianceOptions, DeviceUncertainTrajectorySolver
from tests import refine_scenes as RS
from tests import trajectory_cov_native as CN
from tests import trajectory_smooth_native as SN
from tests import trajectory_smooth_scenes as SC
from tests.test_trajectory_smoother import OPTIONS, check_model_statistics, check_smoothed_reconstruction

pytestmark = pytest.mark.gpu


class DeviceSolver(DeviceTrajectorySmoother, DeviceUncertainTrajectorySolver):
    """The smoother and the call it extends on the device."""


@functools.cache
def _device(name: str):
    return SN.run_scene(DeviceSolver(), getattr(SC, name)())


@pytest.mark.parametrize("name", ["edge", "one"])
def test_device_matches_both_restatements(name):
    """Largest disagreement observed on an MI355X, EDGE: against the joint least-squares solve 4.5e-13 sqrt(tr P) and 3.0e-10 (0.13 and
    0.06 of the bar), against the recursion in numpy 5.3e-13 and 5.5e-10 (0.15, 0.11); nis to 1.6e-13.  ONE: 0 and 2e-15."""
    got = _device(name)
    seq, jnt = SN.oracles(name)
    SN.compare(f"device, {name}, against the joint solve", got, jnt)
    SN.compare(f"device, {name}, against the recursion", got, seq)
    SN.compare_nis(f"device, {name}", got, seq)


def test_device_matches_the_host_build_of_the_thread_body():
    """The g++ build fed the same arrays: the same statuses and NaN pattern, the rest within the bar (observed on an MI355X: 6.2e-13
    sqrt(tr P) and 4.4e-10, 0.17 and 0.09 of the bar: the two builds differ by contraction and by the reciprocal square root)."""
    sc = SC.edge()
    got = _device("edge")
    cpu = SN.thread_body(sc.n_frames, sc.n_traj, sc.xyz, sc.meas_cov, sc.measured, SN.options_of(sc))
    assert np.array_equal(np.isnan(got.nis), np.isnan(cpu.nis))
    ratios = SN.compare("device against the g++ build, edge", got, cpu)
    SN.compare_nis("device against the g++ build, edge", got, cpu)
    print(f"ratio to the bar: means {ratios[0]:.3f}, covariances {ratios[1]:.3f}")
    st = got.status.reshape(sc.n_frames, sc.n_traj)
    assert (st[:, SC.NONE] == 0).all() and st[:, SC.SINGLE].sum() == 1 and st[0, 64] == 1 and st[39, 256] == 1
    s = SC.SINGLE_FRAME * sc.n_traj + SC.SINGLE
    assert np.array_equal(got.pos[s], sc.xyz[s]) and np.array_equal(got.pos_cov[s], sc.meas_cov[s]) and np.array_equal(got.vel[s], np.zeros(3))


def test_two_calls_return_the_same_bytes():
    again = SN.run_scene(DeviceSolver(), SC.edge())
    for name in SN.FIELDS:
        assert getattr(again, name).tobytes() == getattr(_device("edge"), name).tobytes(), name


def test_covariance_and_nis_describe_tracks_drawn_from_the_model():
    check_model_statistics(lambda sc: SN.run_scene(DeviceSolver(), sc))


@pytest.mark.parametrize("refined", [True, False], ids=["refined", "plain"])
@pytest.mark.parametrize("full", [True, False], ids=["full", "noise-only"])
def test_smoothed_reconstruction_on_the_device(refined, full):
    grid, result, cov, sm = check_smoothed_reconstruction(DeviceSolver(), RefineOptions(**CN.REFINED) if refined else None, full,
                                                          f"device, {'refined' if refined else 'plain'}, {'full' if full else 'noise-only'}")
    st = sm.status.reshape(grid.n_frames, grid.n_traj)
    assert (cov.cov_status == 1).sum() == 294 and (st == 1).sum() == 294 and (st == 2).sum() == 6


def test_a_sample_without_a_covariance_is_unmeasured():
    """The one-slot recording whose point lies behind a camera: cov_status 2, so the smoother has nothing to smooth (its kernel runs:
    the call has rows)."""
    ip, cams, _ = RS.behind_camera_case()
    grid = trajectory_grid(ip, cams)
    options = CovarianceOptions(CN.SIGMA_PX, CN.report({0: 9, 1: 9, 3: 6}))
    for refine in (RefineOptions(reject_px=5.0), None):
        result, _, cov, sm = DeviceSolver().reconstruct_smoothed(grid, options, OPTIONS, refine, camera_array=cams)
        assert result.valid.tolist() == [1] and cov.cov_status.tolist() == [2] and sm.status.tolist() == [0]
        assert all(np.isnan(getattr(sm, name)).all() for name in ("pos", "vel", "pos_cov", "vel_cov", "nis", "meas_cov"))


def test_host_checks_refuse_before_any_launch_and_the_device_is_fine_afterwards():
    sc = SC.edge()
    with pytest.raises(ValueError, match="fps must be finite and positive"):
        DeviceSolver().smooth(sc.n_frames, sc.n_traj, sc.xyz, sc.meas_cov, sc.measured, SmootherOptions(fps=0.0, accel_density=2.0))
    with pytest.raises(ValueError, match="bytes of device memory, 100000 are available"):
        SN.run_scene(DeviceSolver(memory_limit=100000), sc)
    none = DeviceSolver().smooth(sc.n_frames, sc.n_traj, sc.xyz, sc.meas_cov, np.zeros_like(sc.measured), SN.options_of(sc))
    assert (none.status == 0).all() and np.isnan(none.pos).all()
    again = SN.run_scene(DeviceSolver(), sc)
    assert again.pos.tobytes() == _device("edge").pos.tobytes()
