"""The compact Schur record of six-parameter cameras on the host (csrc/ba_math.h ``rec6_*``, csrc/cba_kernels.h ``SchurRec<6>``), without a GPU.

A six-parameter record keeps ten doubles, (Y = R X, 1/Zc, Q_row0, Q_row1), where the kernels kept twelve, (Y, Q = G^T Z): Q's third row is
-(x Q_row0 + y Q_row1), and a reader rebuilds the normalised point x = (Y0 + t0) / Zc, y = (Y1 + t1) / Zc from its camera's translation with
``project_factors``' own expression (bit for bit what the record's G was formed with).

``tests/native/compact_records_check.cpp`` — a stand-alone program, built here with ``-fsanitize=address,undefined`` — evaluates the twelve values in
long double and compares pack / expand, a camera-pair block and a diagonal block (all four quarters, and the rotation-rotation quarter relative to
its own size), a right-hand side and the back-substitution terms of BOTH the full double path ("old") and the compact path ("new", with the
arithmetic of the kernels) with them.  Cases: pinhole and fisheye rows; t = 0; |t| = 100 with the points one unit in front of the camera
(Yc = Y + t cancels two digits); depth 2 (the synthetic scenes' cameras stand on a 3 m ring around points within 0.6 m of the axis: depths from
2.3) and depth 0.2.

Bound: four times the OLD path's own error against the same long double values, per case and quantity.  Measured on the CPU (g++ -O2, x86-64;
errors relative to the largest entry of the group), old / new:

    case                    rec                 blk                 rot                 rhs                 step
    pinhole_t0              2.99e-16 2.99e-16   1.19e-16 1.19e-16   8.36e-17 6.92e-17   1.92e-16 1.92e-16   2.92e-16 3.36e-16
    pinhole_t100_depth1     9.39e-15 9.39e-15   8.57e-15 8.65e-15   5.56e-15 5.56e-15   1.33e-14 1.35e-14   8.08e-15 8.08e-15
    pinhole_ring_depth2     3.16e-16 3.16e-16   2.25e-16 2.44e-16   2.25e-16 2.44e-16   1.42e-15 1.42e-15   5.54e-16 5.28e-16
    pinhole_ring_depth0.2   5.02e-14 5.03e-14   3.30e-14 3.30e-14   3.14e-14 3.16e-14   3.32e-14 3.35e-14   2.24e-13 2.24e-13
    fisheye_t0              2.82e-16 2.82e-16   5.20e-16 5.20e-16   2.95e-16 2.95e-16   2.76e-16 2.76e-16   4.31e-16 4.07e-16
    fisheye_t100_depth1     9.96e-15 9.96e-15   3.13e-15 3.13e-15   3.13e-15 3.13e-15   4.02e-15 3.95e-15   1.17e-14 1.17e-14
    fisheye_ring_depth2     3.44e-16 3.44e-16   1.33e-15 1.33e-15   3.66e-16 3.24e-16   3.11e-16 3.11e-16   1.60e-15 8.35e-16
    fisheye_ring_depth0.2   2.14e-15 2.21e-15   2.32e-15 2.32e-15   1.50e-15 1.16e-15   1.98e-15 1.98e-15   5.64e-15 5.75e-15

The second half replays the pair kernel's plan (csrc/schur_plan.h) with the layout numbers of the compact record — 80 slots per wave, records
5 pieces apart in runs of 448, 320 slots per chunk; a ``static_assert`` behind ``Reg3Cfg`` in csrc/cba_kernels.h holds the kernel to these — the way
tests/test_schur_plan.py does with the numbers of the twelve-double record: every camera-pair block must receive exactly its pairs, and the coloured
slots must still spread the LDS bank groups."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.native_build import CSRC, NATIVE, compile_native, load_native
from tests.test_schur_plan import _expected, _visibility

# the old path's error per case: (rec, blk, rot, rhs, step), from the table above
QUANTITIES = ("rec", "blk", "rot", "rhs", "step")
OLD_ERROR = {
    "pinhole_t0": (2.988e-16, 1.188e-16, 8.364e-17, 1.924e-16, 2.915e-16),
    "pinhole_t100_depth1": (9.388e-15, 8.567e-15, 5.560e-15, 1.334e-14, 8.077e-15),
    "pinhole_ring_depth2": (3.160e-16, 2.253e-16, 2.253e-16, 1.423e-15, 5.542e-16),
    "pinhole_ring_depth0.2": (5.024e-14, 3.298e-14, 3.141e-14, 3.319e-14, 2.239e-13),
    "fisheye_t0": (2.818e-16, 5.201e-16, 2.946e-16, 2.764e-16, 4.313e-16),
    "fisheye_t100_depth1": (9.956e-15, 3.127e-15, 3.127e-15, 4.022e-15, 1.169e-14),
    "fisheye_ring_depth2": (3.444e-16, 1.325e-15, 3.661e-16, 3.109e-16, 1.599e-15),
    "fisheye_ring_depth0.2": (2.141e-15, 2.320e-15, 1.495e-15, 1.983e-15, 5.640e-15),
}


@pytest.fixture(scope="module")
def figures():
    exe = compile_native(NATIVE / "compact_records_check.cpp", flags=("-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined"),
                         include=(CSRC,), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-4000:], proc.stderr[-3000:])
    assert proc.returncode == 0 and "all cases ran" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-3000:]
    out = {}
    for line in proc.stdout.splitlines():
        f = line.split()
        if f and f[0] == "case":
            assert f[2::3] == list(QUANTITIES), line
            out[f[1]] = dict(old=tuple(float(v) for v in f[3::3]), new=tuple(float(v) for v in f[4::3]))
    return out


def test_every_case_ran(figures):
    assert sorted(figures) == sorted(OLD_ERROR)


@pytest.mark.parametrize("case", list(OLD_ERROR))
def test_compact_path_against_long_double(figures, case):
    """pack / expand, the blocks, the right-hand side and the back-substitution term formed from the ten values: within four times the full
    double path's own error (OLD_ERROR, measured once) against the long double values."""
    fig = figures[case]
    for what, old_now, new, old in zip(QUANTITIES, fig["old"], fig["new"], OLD_ERROR[case]):
        print(f"{case} {what}: compact {new:.3e}, full double path {old_now:.3e} (recorded {old:.3e}), bound {4 * old:.3e}")
        assert new <= 4.0 * old, (case, what, new, old)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the plan with the compact record's layout (Reg3Cfg<6>: EPW, SchurRec<6>::LST, WAVE_PIECES, SCHUNK)
I32P, F64P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_long)
EPW, LST, WP, CAP = 80, 5, 448, 320


@pytest.fixture(scope="module")
def harness():
    lib = load_native(NATIVE / "plan_harness.cpp", flags=("-pthread",))
    lib.plan_replay.restype = C.c_int
    lib.plan_replay.argtypes = [C.c_int] * 17 + [I32P, I32P, F64P, F64P, I64P]
    return lib


def test_layout_numbers_follow_the_record():
    """What Reg3Cfg<6> derives from a 5-piece record: seven 64-lane loads per wave and chunk, runs padded to whole loads and to whole rounds of the
    16 bank groups (the plan's colouring wants slot mod 16 to decide a record's bank group: an odd stride, and runs that start at a multiple of 16)."""
    nld = -(-EPW * LST // 64)
    assert nld == 7 and WP == nld * 64 and WP % 16 == 0 and EPW % 16 == 0 and LST % 2 == 1 and CAP == 4 * EPW
    assert len({(LST * s) % 16 for s in range(16)}) == 16
    assert 2 * (4 * WP + LST + 1) * 16 <= 64 * 1024  # both chunk buffers with their zero records: two workgroups per CU with room to spare


def _check(lib, rng, n_cams, n_points, k_lo, k_hi, *, cheap=False, chunk_cap=CAP, region_chunks=64, **vis):
    nc, gmax, threads = 6, 16, 256
    hcam, hps = _visibility(rng, n_cams, n_points, k_lo, k_hi, **vis)
    T = np.zeros((hps[-1], 18))
    T[:] = rng.normal(size=T.shape)
    G = -(-n_cams // gmax)
    g = -(-n_cams // G)
    rep = threads // (g * g) if g * g <= threads // 2 else 1
    nT = G * (G + 1) // 2
    acc = np.zeros((nT, threads, nc * nc))
    stats = np.zeros(10, dtype=np.int64)
    rc = lib.plan_replay(n_cams, len(hps) - 1, G, g, rep, nc, T.shape[1], chunk_cap, EPW, LST, WP, region_chunks, 0, 4, threads // 64, 0, int(cheap),
                         hcam.ctypes.data_as(I32P), hps.ctypes.data_as(I32P), T.ctypes.data_as(F64P), acc.ctypes.data_as(F64P), stats.ctypes.data_as(I64P))
    assert rc == 0, rc
    real, helper = _expected(n_cams, hcam, hps, T, nc, G, g)
    nblk = g * g
    blocks = np.zeros((nT, nblk, nc * nc))
    for s in range(rep):
        blocks += acc[:, s * nblk:(s + 1) * nblk]
    assert np.all(acc[:, rep * nblk:] == 0.0)
    t = 0
    for a in range(G):
        na = min(g, n_cams - a * g)
        for b in range(a, G):
            got = blocks[t].reshape(nblk, nc, nc)
            for li in range(g):
                for lj in range(g):
                    if not (a == b and lj <= li):
                        np.testing.assert_allclose(got[li * g + lj], real[t, li * g + lj], rtol=1e-12, atol=1e-12)
            if a == b:
                tot = np.zeros((g, nc, nc))
                k = 0
                for li in range(g):
                    for lj in range(li + 1):
                        tot[k % max(na, 1)] += got[li * g + lj]
                        k += 1
                np.testing.assert_allclose(tot, helper[a], rtol=1e-12, atol=1e-12)
            t += 1
    return stats, int(hps[-1])


@pytest.mark.parametrize("cheap", [False, True])
def test_plan_replay_with_the_compact_layout(harness, cheap):
    rng = np.random.default_rng(41)
    _check(harness, rng, 64, 900, 2, 10, cheap=cheap)                                 # four groups of 16, ten tiles
    _check(harness, rng, 17, 300, 2, 12, cheap=cheap, duplicates=0.1)                 # two ragged groups, a camera seeing a point twice
    _check(harness, rng, 8, 300, 2, 8, cheap=cheap)                                   # one small group: rep = 4
    # one tile with more slots than one chunk: 16 cameras, 200 points of 6 views = 1200 slots, four chunks of 320
    stats, n_obs = _check(harness, rng, 16, 200, 6, 6, cheap=cheap)
    assert n_obs == 1200 > CAP
    _check(harness, rng, 48, 700, 2, 12, cheap=cheap, chunk_cap=64, region_chunks=4)  # many small chunks and regions


def test_bank_spread_at_the_bench_shape(harness):
    """64 cameras, ten views per point (the flagship's shape at a twentieth of its size): the coloured slots of 5-piece records stay below 1.7
    cycles per 16-lane group, the bound tests/test_schur_plan.py holds the 7-piece layout to, and the lanes stay as busy."""
    rng = np.random.default_rng(9)
    stats, _ = _check(harness, rng, 64, 10000, 10, 10)
    n_pairs, lane_iters, groups, cycles, arrival = stats[1], stats[2], stats[5], stats[6], stats[7]
    print(f"lane fill {n_pairs / lane_iters:.3f}, cycles per group {cycles / groups:.3f} (arrival order {arrival / groups:.3f})")
    assert n_pairs == 10000 * 55 and n_pairs / lane_iters > 0.68
    assert cycles / groups < 1.7 and arrival / groups > 2.2, (cycles / groups, arrival / groups)
