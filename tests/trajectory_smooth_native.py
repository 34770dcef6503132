"""g++ build of caliscope_amd/csrc/trajectory_smooth_math.h with the trajectory headers it stands on
(tests/native/trajectory_smooth_harness.cpp), the `_solver` hook that runs on it, the bar of the comparison with
tests/trajectory_smooth_oracle.py and the comparison itself, which the CPU and the GPU tests share.

The bar.  The yardstick is the largest disagreement of the oracle's two restatements (the recursion in numpy; the whitened joint
least-squares problem by QR) on the scenes of tests/trajectory_smooth_scenes.py, the smoothed means in units of the slot's own
smoothed standard deviation sqrt(tr P), the covariances as relative Frobenius distance per slot: 3.6e-13 and 4.9e-10 on EDGE (the
covariances of interpolated frames in a hole right behind a trajectory's first sample, where P - P Lambda P takes a velocity variance
of 100 down to 1e-2), 0 and 2e-15 on ONE.  The bar for the g++ build and for the device is ten times the yardstick of EDGE, computed
here from the two restatements, not from the code under test; it is asserted to lie below 1e-11 / 1e-8 so that an oracle gone wrong
does not widen it unseen."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.trajectory_smoother import (SmoothDesc, SmootherOptions, TrajSmoother, TrajSmoothOut, run_smooth_call, run_smoothed_call)
from caliscope_amd.reconstruction import TrajDesc, TrajOut
from caliscope_amd.trajectory_refinement import TrajQuality, TrajRefine
from caliscope_amd.trajectory_uncertainty import TrajCovOut, TrajUncertainty, UncertaintyTables, uncertainty_tables
from tests import trajectory_cov_native as CN
from tests import trajectory_smooth_oracle as SO
from tests import trajectory_smooth_scenes as SC
from tests.native_build import CSRC, NATIVE, load_native

FIELDS = ("pos", "vel", "pos_cov", "vel_cov", "nis", "status")


@functools.cache
def harness():
    lib = load_native(NATIVE / "trajectory_smooth_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.tsh_last_error.restype = C.c_char_p
    lib.tsh_smooth_trajectories.restype = C.c_int
    lib.tsh_smooth_trajectories.argtypes = [C.POINTER(SmoothDesc), C.POINTER(TrajSmoothOut)]
    lib.tsh_smooth_threads.restype = None
    lib.tsh_smooth_threads.argtypes = [C.POINTER(SmoothDesc), C.POINTER(TrajSmoothOut)]
    lib.tsh_reconstruct_trajectories_smoothed.restype = C.c_int
    lib.tsh_reconstruct_trajectories_smoothed.argtypes = [C.POINTER(TrajDesc), C.POINTER(TrajRefine), C.POINTER(TrajUncertainty), C.POINTER(TrajSmoother),
                                                          C.POINTER(TrajOut), C.POINTER(TrajQuality), C.POINTER(TrajCovOut), C.POINTER(TrajSmoothOut)]
    return lib


class HarnessSmoother(CN.HarnessUncertainSolver):
    """The `_solver` hook on the g++ build, with `smooth` and `reconstruct_smoothed` as caliscope_amd.trajectory_smoother.DeviceTrajectorySmoother."""

    def smooth(self, n_frames, n_traj, xyz, meas_cov, measured, options):
        self.calls += 1
        lib = harness()
        return run_smooth_call(lib.tsh_smooth_trajectories, n_frames, n_traj, xyz, meas_cov, measured, options, self.memory_limit,
                               lambda: lib.tsh_last_error().decode())

    def reconstruct_smoothed(self, grid, covariance, options, refine=None, *, camera_array=None, xy_gap=0, xyz_gap=0, filt=None, float32_io=True,
                             want_grids=False):
        self.calls += 1
        lib = harness()
        tables = covariance if isinstance(covariance, UncertaintyTables) else uncertainty_tables(grid, camera_array, covariance)
        return run_smoothed_call(lib.tsh_reconstruct_trajectories_smoothed, grid, tables, options, refine, xy_gap, xyz_gap, filt, float32_io,
                                 self.memory_limit, want_grids, lambda: lib.tsh_last_error().decode())


def thread_body(n_frames, n_traj, xyz, meas_cov, measured, options):
    """k_traj_smooth's thread body over arrays given by hand, no check in front: what the g++ build computes from the very numbers the
    device computed from."""
    return run_smooth_call(lambda d, o: harness().tsh_smooth_threads(d, o) or 0, n_frames, n_traj, xyz, meas_cov, measured, options, 0, lambda: "")


def options_of(sc) -> SmootherOptions:
    return SmootherOptions(fps=sc.fps, accel_density=sc.accel, velocity_prior_std=sc.sv0, max_gap=sc.max_gap)


def run_scene(solver, sc):
    return solver.smooth(sc.n_frames, sc.n_traj, sc.xyz, sc.meas_cov, sc.measured, options_of(sc))


def _scene(name: str):
    sc = getattr(SC, name)()
    return sc[0] if isinstance(sc, tuple) else sc


@functools.cache
def sequential(name: str):
    """The recursion in numpy on the scene `name` of tests/trajectory_smooth_scenes.py, computed once and not changed."""
    return SO.sequential(*SC.oracle_args(_scene(name)))


@functools.cache
def oracles(name: str):
    """(sequential, joint) of the scene `name`, computed once and not changed."""
    return sequential(name), SO.joint(*SC.oracle_args(_scene(name)))


@functools.cache
def bar():
    """(means in sqrt(tr P), covariances relative): ten times the disagreement of the two restatements on EDGE."""
    seq, jnt = oracles("edge")
    assert np.array_equal(seq.status, jnt.status)
    mean, cov = SO.disagreement(seq, jnt)
    print(f"yardstick on EDGE (sequential against joint): means {mean:.3e} sqrt(tr P), covariances {cov:.3e} relative; the bar is ten times that")
    assert 0.0 < mean < 1e-12 and 0.0 < cov < 1e-9
    return 10.0 * mean, 10.0 * cov


def same_pattern(what, got, ref):
    """Statuses equal; rows of status 0 NaN, the others finite; nis NaN exactly where the sequential restatement has none."""
    assert np.array_equal(got.status, ref.status), what
    none = got.status == 0
    for name in FIELDS[:4]:
        a = getattr(got, name)
        assert np.isnan(a[none]).all() and np.isfinite(a[~none]).all(), (what, name)


def compare(what, got, ref):
    """`got` against a restatement `ref` (or against the g++ build) within the bar; prints and returns the ratios to it."""
    same_pattern(what, got, ref)
    mean, cov = SO.disagreement(got, ref)
    bm, bc = bar()
    print(f"{what}: means {mean:.3e} sqrt(tr P) ({mean / bm:.3f} of the bar), covariances {cov:.3e} relative ({cov / bc:.3f} of the bar)")
    assert mean <= bm and cov <= bc, what
    return mean / bm, cov / bc


def compare_nis(what, got, seq):
    """nis against the sequential restatement: NaN in the same slots, and 1e-9 (1 + nis) elsewhere (y^T S^-1 y with S^-1 good to
    cond(S) eps, cond(S) at most a few 1e5 on the scenes, and y itself the difference of two positions known to 1e-12 of its size)."""
    assert np.array_equal(np.isnan(got.nis), np.isnan(seq.nis)), what
    at = ~np.isnan(seq.nis)
    err = np.abs(got.nis[at] - seq.nis[at]) / (1.0 + seq.nis[at])
    print(f"{what}: nis at {int(at.sum())} slots, largest |nis - oracle| / (1 + nis) = {err.max() if at.any() else 0.0:.3e}")
    assert (err <= 1e-9).all(), what


__all__ = ["FIELDS", "HarnessSmoother", "bar", "compare", "compare_nis", "harness", "options_of", "oracles", "run_scene", "same_pattern", "sequential", "thread_body"]
