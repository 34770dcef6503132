"""g++ build of caliscope_amd/csrc/scale_math.h (tests/native/scale_harness.cpp) and a `_solver` hook for the scale report
(caliscope_amd.scale_accuracy, CaptureVolume.compute_volumetric_scale_accuracy) that runs on it — the CPU side of the anchoring tests."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests.native_build import CSRC, NATIVE, load_native

D = C.POINTER(C.c_double)
I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)


@functools.cache
def harness():
    """Compile (once per process) and load the harness.  -ffp-contract=off: the per-pair arithmetic is written without fused
    multiply-adds, as the device build keeps it."""
    lib = load_native(NATIVE / "scale_harness.cpp", flags=("-ffp-contract=off",), include=(CSRC,))
    lib.sh_last_error.restype = C.c_char_p
    lib.sh_constants.restype = None
    lib.sh_constants.argtypes = [I32]
    lib.sh_lane_pairs.restype = C.c_int64
    lib.sh_lane_pairs.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, I32, I32]
    lib.sh_scale_errors.restype = C.c_int
    lib.sh_scale_errors.argtypes = [C.c_int64, D, C.c_int64, I64, I64, D, D, I32]
    return lib


def constants() -> dict:
    out = np.zeros(6, dtype=np.int32)
    harness().sh_constants(out.ctypes.data_as(I32))
    return dict(zip(("small_max", "lds_small", "lds_large", "max_group", "block", "nstat"), out.tolist()))


def lane_pairs(n: int, lane: int, stride: int):
    """(i[], j[]) of the pairs lane `lane` of `stride` visits in a group of n entries, in the order it visits them."""
    cap = n * (n - 1) // 2 // stride + 2
    i, j = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    k = harness().sh_lane_pairs(n, lane, stride, cap, i.ctypes.data_as(I32), j.ctypes.data_as(I32))
    assert k <= cap
    return i[:k], j[:k]


class HarnessError(Exception):
    def __init__(self, code, message):
        super().__init__(f"code {code}: {message}")
        self.code, self.message = code, message


class HarnessScaleErrors:
    """The `_solver` hook on the g++ build: same arguments and result as caliscope_amd.scale_accuracy.DeviceScaleErrors.  `bins` holds
    the path every group of the last call took (0 thread per group, 1 / 2 staged workgroup, 3 unstaged workgroup)."""

    bins = None

    def scale_errors(self, world_xyz, group_start, ent_world, ent_obj):
        world_xyz = np.ascontiguousarray(world_xyz, dtype=np.float64).reshape(-1, 3)
        group_start = np.ascontiguousarray(group_start, dtype=np.int64)
        ent_world = np.ascontiguousarray(ent_world, dtype=np.int64)
        ent_obj = np.ascontiguousarray(ent_obj, dtype=np.float64).reshape(-1, 3)
        n_groups = len(group_start) - 1
        stats = np.zeros((n_groups, 8))
        self.bins = np.zeros(n_groups, dtype=np.int32)
        rc = harness().sh_scale_errors(len(world_xyz), world_xyz.ctypes.data_as(D), n_groups, group_start.ctypes.data_as(I64),
                                       ent_world.ctypes.data_as(I64), ent_obj.ctypes.data_as(D), stats.ctypes.data_as(D),
                                       self.bins.ctypes.data_as(I32))
        if rc:
            raise HarnessError(rc, harness().sh_last_error().decode())
        return stats
