"""g++ build of caliscope_amd/csrc/trajectory_skeleton_math.h (tests/native/trajectory_skeleton_harness.cpp), the `_solver` hook that
runs on it, the bar of the comparison with tests/trajectory_skeleton_oracle.py and the comparison itself, which the CPU and the GPU
tests share.

The bar.  The yardstick is the largest disagreement of the oracle's two restatements (Gauss-Newton by QR; scipy's least_squares and
Newton steps on the normal equations) on the EDGE scene of tests/trajectory_skeleton_scenes.py, the adjusted means in units of the
slot's own sqrt(tr P), the covariances as relative Frobenius distance per slot.  The bar for the g++ build and for the device is ten
times the yardstick for the covariances; for the means ten times the larger of the yardstick and the `tol` the tests run with
(TOL = 1e-11: with the oracle's contraction below 0.5 the distance left after a step shorter than tol, in those units, is below
tol).  It is computed here from the two restatements, never from the code under test, and asserted to lie below 1e-9 / 1e-9 so that
an oracle gone wrong does not widen it unseen."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.trajectory_skeleton import SkeletonDesc, SkeletonOut, run_skeleton_call, skeleton_components
from tests import trajectory_skeleton_oracle as KO
from tests import trajectory_skeleton_scenes as KS
from tests.native_build import CSRC, NATIVE, load_native

TOL = 1e-11
MAX_ITER = 60
FIELDS = ("pos", "pos_cov", "status", "length", "med", "mad", "frames", "len_before", "w_before", "len_after", "chi2", "rows", "iterations", "comp_status")


@functools.cache
def harness():
    lib = load_native(NATIVE / "trajectory_skeleton_harness.cpp", flags=("-Wno-unknown-pragmas",), include=(CSRC,))
    lib.tkh_last_error.restype = C.c_char_p
    lib.tkh_adjust_skeleton.restype = C.c_int
    lib.tkh_adjust_skeleton.argtypes = [C.POINTER(SkeletonDesc), C.POINTER(SkeletonOut)]
    return lib


class HarnessSkeletonAdjuster:
    """The `_solver` hook on the g++ build, with `adjust` as caliscope_amd.trajectory_skeleton.DeviceSkeletonAdjuster.  The components
    that size the outputs come from the real library's host code, as on the device path."""

    def __init__(self, memory_limit: int = 0):
        self.memory_limit = memory_limit
        self.calls = 0

    def adjust(self, n_frames, n_traj, xyz, meas_cov, measured, seg_traj, seg_length, seg_sigma, *, trim=3.0, max_iter=30, tol=1e-9):
        self.calls += 1
        lib = harness()
        return run_skeleton_call(lib.tkh_adjust_skeleton, skeleton_components, n_frames, n_traj, xyz, meas_cov, measured, seg_traj, seg_length,
                                 seg_sigma, trim, max_iter, tol, self.memory_limit, lambda: lib.tkh_last_error().decode())


def run_scene(solver, sc, max_iter=MAX_ITER, tol=TOL):
    return solver.adjust(sc.n_frames, sc.n_traj, sc.xyz, sc.cov, sc.measured, sc.seg_traj, sc.seg_length, sc.seg_sigma, trim=sc.trim, max_iter=max_iter,
                         tol=tol)


@functools.cache
def oracles(name: str):
    """(gauss_newton, scipy_newton) of the scene `name`, computed once and not changed; both assert their contraction below 0.5."""
    sc = getattr(KS, name)()
    return KO.adjust(KO.gauss_newton, *KS.oracle_args(sc)), KO.adjust(KO.scipy_newton, *KS.oracle_args(sc))


@functools.cache
def bar():
    """(means in sqrt(tr P), covariances relative) from the two restatements on EDGE."""
    gn, sp = oracles("edge")
    assert np.array_equal(gn.status, sp.status)
    mean, cov = KO.disagreement(gn, sp)
    print(f"yardstick on EDGE (Gauss-Newton by QR against scipy and Newton): means {mean:.3e} sqrt(tr P), covariances {cov:.3e} relative; "
          f"contraction {max(gn.contraction, sp.contraction):.3f}")
    bm, bc = 10.0 * max(mean, TOL), 10.0 * cov
    assert 0.0 < mean and 0.0 < cov and bm < 1e-9 and bc < 1e-9
    return bm, bc


def same_pattern(what, got, ref):
    """Statuses equal; unmeasured rows NaN, the others finite; the per-(frame, segment) outputs NaN in the same cells."""
    assert np.array_equal(got.status, ref.status), what
    none = got.status == 0
    assert np.isnan(got.pos[none]).all() and np.isnan(got.pos_cov[none]).all(), what
    assert np.isfinite(got.pos[~none]).all() and np.isfinite(got.pos_cov[~none]).all(), what
    for name in ("len_before", "w_before", "len_after"):
        assert np.array_equal(np.isnan(getattr(got, name)), np.isnan(getattr(ref, name))), (what, name)
    assert np.array_equal(got.rows, ref.rows), what


def compare(what, got, ref):
    """`got` against a restatement `ref` (or against the g++ build) within the bar; prints and returns the ratios to it."""
    same_pattern(what, got, ref)
    mean, cov = KO.disagreement(got, ref)
    bm, bc = bar()
    chi = float(np.max(np.abs(got.chi2 - ref.chi2) / (1.0 + ref.chi2))) if ref.chi2.size else 0.0
    at = ~np.isnan(ref.len_before)
    seg = max((float(np.max(np.abs(getattr(got, n)[at] - getattr(ref, n)[at]) / (1.0 + np.abs(getattr(ref, n)[at])))) if at.any() else 0.0)
              for n in ("len_before", "w_before", "len_after"))
    print(f"{what}: means {mean:.3e} sqrt(tr P) ({mean / bm:.3f} of the bar), covariances {cov:.3e} relative ({cov / bc:.3f} of the bar), "
          f"chi2 {chi:.3e} of 1 + chi2 ({chi / 1e-9:.3f} of the bar), per-segment lengths and w {seg:.3e}")
    assert mean <= bm and cov <= bc and chi <= 1e-9 and seg <= 1e-9, what
    return mean / bm, cov / bc


def compare_lengths(what, sc, got, ref):
    """med, mad and a given length as equal bits, the count equal, the trimmed mean to 1e-13 relative; NaN in the same places."""
    assert np.array_equal(got.frames, ref.frames), what
    for name in ("med", "mad"):
        a, b = getattr(got, name), getattr(ref, name)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)].view(np.uint64), b[~np.isnan(b)].view(np.uint64)), (what, name)
    assert np.array_equal(np.isnan(got.length), np.isnan(ref.length)), what
    given = ~np.isnan(sc.seg_length)
    assert np.array_equal(got.length[given].view(np.uint64), sc.seg_length[given].view(np.uint64)), what
    at = ~np.isnan(ref.length)
    err = float(np.max(np.abs(got.length[at] - ref.length[at]) / ref.length[at])) if at.any() else 0.0
    print(f"{what}: {len(ref.length)} segments, med and mad equal bits, largest |length - oracle| / length = {err:.3e}")
    assert err <= 1e-13, what


def statistics(sc, got):
    """(sum chi2, sum rows, its bound, mean Mahalanobis distance of the adjusted points from the truth, its bound) of tracks drawn
    from the model.  chi2 of a (frame, component) is chi-square with `rows` degrees of freedom, so the sum is within
    5 sqrt(2 dof) of dof.  (X - truth)^T P^-1 (X - truth) of a slot is chi-square with 3, variance 6; the slots of one frame are
    correlated, the frames are independent, and the variance of a frame's mean is at most 6, so the standard error of the mean over
    all slots is at most sqrt(6 / frames)."""
    dof = int(got.rows.sum())
    at = got.status == 1
    e = got.pos[at] - sc.truth[at]
    q = np.einsum("ij,ijk,ik->i", e, np.linalg.inv(KO.full(got.pos_cov[at])), e)
    return float(got.chi2.sum()), dof, 5.0 * np.sqrt(2.0 * dof), float(q.mean()), 5.0 * np.sqrt(6.0 / sc.n_frames)


def check_statistics(what, sc, got):
    chi2, dof, bound, q, q_bound = statistics(sc, got)
    print(f"{what}: sum chi2 {chi2:.1f} for {dof} rows (within {bound:.1f}: {abs(chi2 - dof) / bound:.3f} of the bound); mean Mahalanobis "
          f"distance from the truth {q:.4f} (3 within {q_bound:.3f}: {abs(q - 3.0) / q_bound:.3f} of the bound)")
    assert abs(chi2 - dof) <= bound and abs(q - 3.0) <= q_bound, what


__all__ = ["FIELDS", "HarnessSkeletonAdjuster", "MAX_ITER", "TOL", "bar", "check_statistics", "compare", "compare_lengths", "harness", "oracles",
           "run_scene", "same_pattern", "statistics"]
