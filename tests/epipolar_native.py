"""g++ build of caliscope_amd/csrc/epipolar_math.h (tests/native/epipolar_harness.cpp) and an `_epi` hook for
caliscope_amd.epipolar_pose that runs on it — the CPU side of the epipolar-bootstrap tests."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests.native_build import CSRC, NATIVE, load_native
from tests.pnp_native import HarnessPnP

D = C.POINTER(C.c_double)
I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)
U8 = C.POINTER(C.c_uint8)


def _p(a, t=D):
    return a.ctypes.data_as(t)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "epipolar_harness.cpp", include=(CSRC,))
    lib.eh_sample.restype = None
    lib.eh_sample.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int, I64]
    lib.eh_sampson.restype = C.c_double
    lib.eh_sampson.argtypes = [D, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.eh_decompose.restype = C.c_int
    lib.eh_decompose.argtypes = [D, C.c_int64, D, D, I64]
    lib.eh_essential_batch.restype = None
    lib.eh_essential_batch.argtypes = [C.c_int32, I32, D, C.c_int64, D, I32, C.c_int64, I64, I64, I64, D, C.c_int32, C.c_uint64, C.c_int32,
                                       D, I32, I64, I64, D, I32, U8, D, D]
    lib.eh_resect_batch.restype = None
    lib.eh_resect_batch.argtypes = [C.c_int64, I64, D, D, D, C.c_int32, C.c_int32, C.c_uint64, D, I32, I64, I32, D]
    lib.eh_essential_counts.restype = None
    lib.eh_essential_counts.argtypes = [D, I64, I64, C.c_int64, C.c_int64, C.c_double, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, I64, I64]
    lib.eh_resect_counts.restype = None
    lib.eh_resect_counts.argtypes = [D, D, C.c_int64, C.c_int64, C.c_double, C.c_int32, C.c_uint64, C.c_int64, C.c_int64, I64, I64]
    return lib


def essential_counts(und, corr_a, corr_b, s, n, thr, n_hyp, seed, job, items):
    """Inlier count of every hypothesis of the job holding correspondences s .. s + n - 1 (batch index ``job``) over
    ``items`` (offsets into the job); ``und`` are the undistorted rows."""
    und = np.ascontiguousarray(und, dtype=np.float64)
    corr_a, corr_b = np.ascontiguousarray(corr_a, dtype=np.int64), np.ascontiguousarray(corr_b, dtype=np.int64)
    items = np.ascontiguousarray(items, dtype=np.int64)
    count = np.zeros(int(n_hyp), dtype=np.int64)
    harness().eh_essential_counts(_p(und), _p(corr_a, I64), _p(corr_b, I64), int(s), int(n), float(thr), int(n_hyp), int(seed), int(job),
                                  len(items), _p(items, I64), _p(count, I64))
    return count


def resect_counts(obj, uv, s, n, thr, n_hyp, seed, job, items):
    """As ``essential_counts`` for a resection job of points s .. s + n - 1."""
    obj, uv = np.ascontiguousarray(obj, dtype=np.float64), np.ascontiguousarray(uv, dtype=np.float64)
    items = np.ascontiguousarray(items, dtype=np.int64)
    count = np.zeros(int(n_hyp), dtype=np.int64)
    harness().eh_resect_counts(_p(obj), _p(uv), int(s), int(n), float(thr), int(n_hyp), int(seed), int(job), len(items), _p(items, I64),
                               _p(count, I64))
    return count


def sample(seed, job, h, n, k):
    idx = np.zeros(k, dtype=np.int64)
    harness().eh_sample(seed, job, h, n, k, _p(idx, I64))
    return idx


def sampson(E, xa, ya, xb, yb):
    E = np.ascontiguousarray(E, dtype=np.float64).ravel()
    return harness().eh_sampson(_p(E), xa, ya, xb, yb)


def decompose(E, a, b):
    """(picked candidate, rt[4, 12], in-front counts[4]) for correspondences a, b (normalised [n, 2])."""
    E = np.ascontiguousarray(E, dtype=np.float64).ravel()
    c = np.ascontiguousarray(np.hstack([a, b]), dtype=np.float64)
    rt, cnt = np.zeros((4, 12)), np.zeros(4, dtype=np.int64)
    k = harness().eh_decompose(_p(E), len(c), _p(c), _p(rt), _p(cnt, I64))
    return k, rt, cnt


class HarnessEpipolar:
    """The `_epi` hook of caliscope_amd.epipolar_pose on the g++ build: same arguments and results as the device calls
    (``pair_rmse`` is the PnP harness's)."""

    def essential_batch(self, cam_model, cam_intr, obs_xy, obs_cam, pair_start, corr_a, corr_b, threshold, n_hyp, seed, float32_io=False):
        cam_model = np.ascontiguousarray(cam_model, dtype=np.int32)
        cam_intr = np.ascontiguousarray(cam_intr, dtype=np.float64)
        obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
        obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32)
        pair_start = np.ascontiguousarray(pair_start, dtype=np.int64)
        corr_a = np.ascontiguousarray(corr_a, dtype=np.int64)
        corr_b = np.ascontiguousarray(corr_b, dtype=np.int64)
        threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        n_pairs, n_corr = len(pair_start) - 1, int(pair_start[-1])
        pose, status = np.zeros((n_pairs, 12)), np.zeros(n_pairs, dtype=np.int32)
        n_inl, n_chr = np.zeros(n_pairs, dtype=np.int64), np.zeros(n_pairs, dtype=np.int64)
        cond, winner = np.zeros(n_pairs), np.zeros(n_pairs, dtype=np.int32)
        flag, xyz, und = np.zeros(n_corr, dtype=np.uint8), np.zeros((n_corr, 3)), np.zeros_like(obs_xy)
        harness().eh_essential_batch(len(cam_model), _p(cam_model, I32), _p(cam_intr), len(obs_xy), _p(obs_xy), _p(obs_cam, I32), n_pairs,
                                     _p(pair_start, I64), _p(corr_a, I64), _p(corr_b, I64), _p(threshold), int(n_hyp), int(seed),
                                     1 if float32_io else 0, _p(pose), _p(status, I32), _p(n_inl, I64), _p(n_chr, I64), _p(cond),
                                     _p(winner, I32), _p(flag, U8), _p(xyz), _p(und))
        return dict(pose=pose, status=status, n_inliers=n_inl, n_cheiral=n_chr, conditioning=cond, winner=winner, flag=flag, xyz=xyz,
                    undistorted=und)

    def resect_batch(self, job_start, obj, uv, threshold, n_hyp, min_points, seed):
        job_start = np.ascontiguousarray(job_start, dtype=np.int64)
        obj = np.ascontiguousarray(obj, dtype=np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        n_jobs = len(job_start) - 1
        pose, status = np.zeros((n_jobs, 12)), np.zeros(n_jobs, dtype=np.int32)
        n_inl, winner, err = np.zeros(n_jobs, dtype=np.int64), np.zeros(n_jobs, dtype=np.int32), np.zeros(len(obj))
        harness().eh_resect_batch(n_jobs, _p(job_start, I64), _p(obj), _p(uv), _p(threshold), int(n_hyp), int(min_points), int(seed), _p(pose),
                                  _p(status, I32), _p(n_inl, I64), _p(winner, I32), _p(err))
        return dict(pose=pose, status=status, n_inliers=n_inl, winner=winner, err=err)

    def pair_rmse(self, pair_pose, pair_start, obs_a, obs_b):
        return HarnessPnP().pair_rmse(pair_pose, pair_start, obs_a, obs_b)
