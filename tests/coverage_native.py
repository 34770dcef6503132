"""g++ build of caliscope_amd/csrc/coverage_math.h (tests/native/coverage_harness.cpp), a `_solver` hook for
caliscope_amd.coverage_analysis that runs on it, and the tables and the brute force the coverage tests share."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from caliscope_amd.coverage_analysis import check_coverage_arguments
from caliscope_amd.exceptions import BackendError
from tests.native_build import CSRC, NATIVE, load_native

I32 = C.POINTER(C.c_int32)
I64 = C.POINTER(C.c_int64)


@functools.cache
def harness():
    """Compile (once per process) and load the harness."""
    lib = load_native(NATIVE / "coverage_harness.cpp", include=(CSRC,))
    lib.ch_last_error.restype = C.c_char_p
    lib.ch_constants.restype = None
    lib.ch_constants.argtypes = [I32]
    lib.ch_plan.restype = None
    lib.ch_plan.argtypes = [C.c_int32, C.c_int64, C.c_int64, I64]
    lib.ch_tile_pair.restype = None
    lib.ch_tile_pair.argtypes = [C.c_int64, C.c_int32, I32]
    lib.ch_coverage_counts.restype = C.c_int
    lib.ch_coverage_counts.argtypes = [C.c_int32, C.c_int64, C.c_int64, I64, I32, C.c_int64, I64]
    return lib


def constants() -> dict:
    out = np.zeros(6, dtype=np.int32)
    harness().ch_constants(out.ctypes.data_as(I32))
    return dict(zip(("tile", "block", "stage_words", "lds_stride", "target_wg", "max_cams"), out.tolist()))


def plan(n_cams: int, n_keys: int, slab_words: int = 0) -> dict:
    """The enumeration of a call: words of a row, words per slab, slabs, row stride, words per chunk, chunks, tiles, tile pairs."""
    out = np.zeros(8, dtype=np.int64)
    harness().ch_plan(n_cams, n_keys, slab_words, out.ctypes.data_as(I64))
    return dict(zip(("n_words", "slab_words", "n_slabs", "stride", "chunk_words", "n_chunks", "n_tiles", "n_tile_pairs"), out.tolist()))


def tile_pair(p: int, n_tiles: int) -> tuple[int, int]:
    out = np.zeros(2, dtype=np.int32)
    harness().ch_tile_pair(p, n_tiles, out.ctypes.data_as(I32))
    return int(out[0]), int(out[1])


class HarnessCoverageCounts:
    """The `_solver` hook on the g++ build: same arguments, checks, result and error type as
    caliscope_amd.coverage_analysis.DeviceCoverageCounts.  `slab_words` set on the object overrides the argument (the public
    functions always pass the default)."""

    def __init__(self, slab_words=None):
        self.slab_words = slab_words
        self.calls = 0

    def coverage_counts(self, obs_key, obs_cam, n_cams, n_keys, slab_words=0):
        obs_key, obs_cam, n_cams, n_keys, slab_words = check_coverage_arguments(obs_key, obs_cam, n_cams, n_keys, slab_words)
        if self.slab_words is not None:
            slab_words = self.slab_words
        self.calls += 1
        counts = np.zeros((n_cams, n_cams), dtype=np.int64)
        rc = harness().ch_coverage_counts(n_cams, n_keys, len(obs_key), obs_key.ctypes.data_as(I64), obs_cam.ctypes.data_as(I32), slab_words,
                                          counts.ctypes.data_as(I64))
        if rc:
            raise BackendError(f"cba_coverage_counts failed (code {rc}): {harness().ch_last_error().decode()}")
        return counts


# ---- tables and the brute force ------------------------------------------------------------------------------------------------------

def random_rows(n_keys: int, n_cams: int, seed: int, density: float = 0.3):
    """(obs_key, obs_cam, M): a random boolean table M[n_keys, n_cams] (every camera and, where there are enough cameras, the first
    and the last key occupied), its rows shuffled, 10 % of them repeated and 5 % more rows with camera -1 at random keys."""
    rng = np.random.default_rng(seed)
    M = rng.random((n_keys, n_cams)) < density
    M[rng.integers(0, n_keys, n_cams), np.arange(n_cams)] = True
    M[0, 0] = M[n_keys - 1, n_cams - 1] = True
    key, cam = np.nonzero(M)
    again = rng.integers(0, len(key), max(1, len(key) // 10))
    outside = max(1, len(key) // 20)
    key = np.concatenate([key, key[again], rng.integers(0, n_keys, outside)])
    cam = np.concatenate([cam, cam[again], np.full(outside, -1)])
    order = rng.permutation(len(key))
    return key[order].astype(np.int64), cam[order].astype(np.int32), M


def brute_force(M) -> np.ndarray:
    """M.T @ M of the boolean table keys x cameras."""
    m = np.asarray(M, dtype=np.int64)
    return m.T @ m


def table_from_rows(obs_key, obs_cam, n_cams: int) -> np.ndarray:
    """The boolean table keys x cameras of a row list, camera -1 left out (for tables that are given as rows)."""
    obs_key, obs_cam = np.asarray(obs_key), np.asarray(obs_cam)
    keep = obs_cam >= 0
    M = np.zeros((int(obs_key.max()) + 1 if len(obs_key) else 0, n_cams), dtype=bool)
    M[obs_key[keep], obs_cam[keep]] = True
    return M


def edge_grid():
    """n_keys x cameras at the word and tile edges: (n_keys, n_cams) pairs."""
    tile = constants()["tile"]
    return [(k, c) for k in (1, 63, 64, 65, 4097) for c in (1, 2, tile - 1, tile, tile + 1, 65, 200)]
