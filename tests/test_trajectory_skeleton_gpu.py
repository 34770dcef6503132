"""cba_adjust_skeleton on the device (k_skel_length and k_skel_adjust of csrc/skeleton_lib.hip): the scenes of
tests/trajectory_skeleton_scenes.py — EDGE with 257 frames, a second pass of the 256-thread stride with one live frame, components of
2, 15, 22 and 54 points in one call — against the two numpy restatements of tests/trajectory_skeleton_oracle.py and against the g++
build of the same arithmetic fed the same arrays, the tracks drawn from the model, the refusal of 55 points and the
tests/refine_scenes.py recording adjusted and then smoothed.  The bar is that of tests/trajectory_skeleton_native.py."""
import functools

import numpy as np
import pytest

from caliscope_amd.trajectory_skeleton import DeviceSkeletonAdjuster
from caliscope_amd.trajectory_smoother import DeviceTrajectorySmoother, SmootherOptions, smooth_trajectories
from caliscope_amd.trajectory_uncertainty import DeviceUncertainTrajectorySolver
from tests import trajectory_skeleton_native as KN
from tests import trajectory_skeleton_scenes as KS
from tests.test_trajectory_skeleton import check_recording

pytestmark = pytest.mark.gpu


@functools.cache
def _device(name: str):
    return KN.run_scene(DeviceSkeletonAdjuster(), getattr(KS, name)())


@pytest.mark.parametrize("name", ["edge", "one"])
def test_device_matches_both_restatements(name):
    """Largest disagreement observed on an MI355X, EDGE: against Gauss-Newton by QR 2.1e-12 sqrt(tr P) and 1.58e-13 (0.021 and 0.50
    of the bar), against scipy and Newton the same to two digits; chi2 to 3.1e-14 (1 + chi2), the trimmed mean to 1.3e-15, medians
    bit for bit.  The covariance figure is the tolerance, not arithmetic: the covariance is a function of the iterate, and a run that
    stops at tol = 1e-11 leaves the chain's slowest frame that far from its minimum.  ONE: 5.2e-14 and 2.5e-14 (0.001, 0.08).
    (Printed by a run with workgroups of 64 threads; the measurement of DESIGN.md found the positions and covariances of 64 and 256 the same bytes.)"""
    sc, got = getattr(KS, name)(), _device(name)
    gn, sp = KN.oracles(name)
    KN.compare(f"device, {name}, against Gauss-Newton by QR", got, gn)
    KN.compare(f"device, {name}, against scipy and Newton", got, sp)
    KN.compare_lengths(f"device, {name}", sc, got, gn)
    active = got.comp_status != 0
    assert np.array_equal(active, gn.active) and (got.comp_status[active] == 1).all() and got.iterations.max() < KN.MAX_ITER


def test_device_matches_the_host_build():
    """The g++ build fed the same arrays: the same statuses, NaN pattern, counts, medians and given lengths bit for bit, the rest
    within the bar (observed on an MI355X: 1.6e-13 sqrt(tr P) and 3.7e-14, 0.002 and 0.12 of the bar, 20 iterations at most in
    both: the two builds differ by contraction and by the reciprocal square root)."""
    sc, got = KS.edge(), _device("edge")
    cpu = KN.run_scene(KN.HarnessSkeletonAdjuster(), sc)
    ratios = KN.compare("device against the g++ build, edge", got, cpu)
    KN.compare_lengths("device against the g++ build, edge", sc, got, cpu)
    print(f"ratio to the bar: means {ratios[0]:.3f}, covariances {ratios[1]:.3f}; iterations device {got.iterations.max()}, g++ {cpu.iterations.max()}")
    assert np.array_equal(got.comp_status, cpu.comp_status) and np.array_equal(got.rows, cpu.rows)
    f, j = sc.marks["lonely"]
    s = f * sc.n_traj + j
    assert got.status[s] == 2 and got.pos[s].tobytes() == sc.xyz[s].tobytes() and got.pos_cov[s].tobytes() == sc.cov[s].tobytes()


def test_two_calls_return_the_same_bytes():
    again = KN.run_scene(DeviceSkeletonAdjuster(), KS.edge())
    for name in KN.FIELDS:
        assert getattr(again, name).tobytes() == getattr(_device("edge"), name).tobytes(), name


def test_chi2_and_covariance_describe_tracks_drawn_from_the_model():
    """Observed on an MI355X: sum chi2 3730.3 for 3600 rows (0.31 of the bound), mean distance from the truth 3.0107 (0.02 of the bound)."""
    sc = KS.statistical()
    got = KN.run_scene(DeviceSkeletonAdjuster(), sc)
    KN.check_statistics("device on tracks drawn from the model", sc, got)
    assert (got.comp_status == 1).all()


def test_55_points_are_refused_without_a_launch_and_the_device_is_fine_afterwards():
    sc = KS.too_large()
    with pytest.raises(ValueError, match="the component of trajectory 3 has 55 trajectories, at most 54"):
        KN.run_scene(DeviceSkeletonAdjuster(), sc)
    with pytest.raises(ValueError, match=r"bytes of device memory \(154 per slot, 32 per \(frame, segment\), 17 per \(frame, component\)\), 100000 are"):
        KN.run_scene(DeviceSkeletonAdjuster(memory_limit=100000), KS.edge())
    one = KS.one()
    none = DeviceSkeletonAdjuster().adjust(one.n_frames, one.n_traj, one.xyz, one.cov, np.zeros_like(one.measured), one.seg_traj, one.seg_length, one.seg_sigma)
    assert (none.status == 0).all() and np.isnan(none.pos).all()
    again = KN.run_scene(DeviceSkeletonAdjuster(), one)
    assert again.pos.tobytes() == _device("one").pos.tobytes()


class _Device(DeviceTrajectorySmoother, DeviceUncertainTrajectorySolver):
    """The reconstruction with its covariances and the smoother on the device."""


def test_recording_adjusted_and_smoothed_on_the_device():
    res, world, frame = check_recording(_Device(), DeviceSkeletonAdjuster(), "device")
    smoothed = smooth_trajectories(res.world, res.covariance_frame, SmootherOptions(fps=100.0, accel_density=5.0))
    assert len(smoothed) >= len(world._df) and np.isfinite(smoothed[["x", "y", "z"]].to_numpy()).all()
