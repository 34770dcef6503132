"""cba_reconstruct_trajectories on the device at the edges of its launches, its holes and its filter, on the two scenes of
tests/trajectory_scenes.py (which asserts from its tables what makes them these edges):

* WIDE, 86 trajectories x 40 frames: k_traj_filtfilt runs 258 threads, so its strided scratch column gets a second workgroup and
  trajectory 85 has its coordinates in two of them; one trajectory reaches the filter with 3 samples and is left alone at every
  order, one with 28, the fewest that order 8 filters;
* LONG, 2 trajectories x 257 frames: k_traj_frame_time gets a second workgroup with one live thread, and without the 2-D fill there
  are frames without a row from any camera — traj_frame_mean returns NaN there and the 3-D fill draws its line of times across them.

On them: every filter order from 1 to CBA_TRAJ_MAX_ORDER (traj_lfilter_step is other code per order, and its bits depend on hipcc
contracting nothing in it), `float32_io = 0`, and the entry point's own host code (a call without rows, the explicit memory limit).

The rules are those of tests/test_reconstruction_gpu.py (`_compare`, tests/trajectory_native.py): xyz and the filled grids bit for bit
against the host chain — `ImagePoints.fill_gaps(g).triangulate(cameras)`, `WorldPoints.fill_gaps`, `WorldPoints.smooth` — and
frame_time within n 2^-52 max|frame_time|.  tests/test_reconstruction.py runs the same scenes on the g++ build of the same routines:
where a test fails here and passes there, the difference is the device's.

Wall time of this file on an MI355X: 35 tests in 2.7 s; the slowest, 0.65 s, is the first to ask for the host references of WIDE,
which the others share.
"""
import dataclasses
import functools

import numpy as np
import pytest

from caliscope_amd.reconstruction import DeviceTrajectorySolver, filter_coefficients, reconstruct_trajectories, trajectory_grid
from caliscope_amd.triangulation import triangulate
from tests import trajectory_native as N
from tests import trajectory_scenes as S
from tests.trajectory_native import _compare, _time_bound_after_fill

pytestmark = pytest.mark.gpu

OUTPUTS = ("xyz", "valid", "slot_time", "frame_time", "xy_filled", "ft_filled")
both_scenes = pytest.mark.parametrize("name", ["WIDE", "LONG"])


def _scene(name):
    sc = S.SCENES[name]()
    return sc.image_points, sc.cameras


@functools.lru_cache(maxsize=None)
def _grid(name):
    return trajectory_grid(*_scene(name))


@functools.lru_cache(maxsize=None)
def _host_triangulated(name, xy_gap):
    """(filled ImagePoints table, host WorldPoints) — computed once, read by every test that needs it."""
    ip, cams = _scene(name)
    filled = ip.fill_gaps(xy_gap)
    return filled.df, filled.triangulate(cams)


@functools.lru_cache(maxsize=None)
def _host_unsmoothed(name):
    return _host_triangulated(name, S.GAP)[1].fill_gaps(S.GAP)


@both_scenes
@pytest.mark.parametrize("xy_gap", [0, 3])
def test_fill_and_triangulation_equal_the_host_chain(name, xy_gap):
    ip, cams = _scene(name)
    filled, want = _host_triangulated(name, xy_gap)
    got = reconstruct_trajectories(ip, cams, xy_gap_fill=xy_gap)
    assert list(got.df.columns) == N.WORLD_COLS
    rows = _compare(got, want, N.frame_time_bound(filled, N.keyed(want.df)[:, 0].astype(np.int64)), f"{name} xy_gap {xy_gap}")
    assert np.array_equal(got.df[N.WORLD_COLS[:3]].to_numpy(), rows[:, :3].astype(np.int64))  # sorted by (sync, object, keypoint)
    if xy_gap:
        assert len(want) > len(_host_triangulated(name, 0)[1])  # the 2-D fill made slots triangulable


@both_scenes
@pytest.mark.parametrize("xy_gap,xyz_gap", [(0, 1), (0, 3), (3, 3)])
def test_the_3d_fill_equals_the_host_chain(name, xy_gap, xyz_gap):
    ip, cams = _scene(name)
    filled, base = _host_triangulated(name, xy_gap)
    want = base.fill_gaps(xyz_gap)
    assert len(want) > len(base)
    got = reconstruct_trajectories(ip, cams, xy_gap_fill=xy_gap, xyz_gap_fill=xyz_gap)
    _compare(got, want, _time_bound_after_fill(filled, base), f"{name} xy_gap {xy_gap} xyz_gap {xyz_gap}")
    if name == "LONG" and xy_gap == 0:  # points, and times, in frames that have no row: the line ran across them
        rows = set(ip.df["sync_index"])
        assert len(set(got.df["sync_index"]) - rows) >= 2 and not set(base.df["sync_index"]) - rows
        assert np.isfinite(got.df["frame_time"].to_numpy()).all()


@both_scenes
@pytest.mark.parametrize("order", range(1, 9))
def test_the_filter_equals_the_host_chain(name, order):
    ip, cams = _scene(name)
    filled, base = _host_triangulated(name, S.GAP)
    unsmoothed = _host_unsmoothed(name)
    counts = unsmoothed.df.groupby(["object_id", "keypoint_id"]).size().to_numpy()
    assert np.array_equal(counts, S.samples(S.SCENES[name]()))
    want = unsmoothed.smooth(30.0, 6.0, order)
    got = reconstruct_trajectories(ip, cams, xy_gap_fill=S.GAP, xyz_gap_fill=S.GAP, smooth=(30.0, 6.0, order))
    rows = _compare(got, want, _time_bound_after_fill(filled, base), f"{name} order {order}")
    plain = N.keyed(unsmoothed.df)
    traj = (rows[:, 1] * 7 + rows[:, 2]).astype(np.int64)
    changed = np.array([not np.array_equal(rows[traj == j, 3:6], plain[traj == j, 3:6]) for j in range(len(counts))])
    assert np.array_equal(changed, counts > 3 * order)
    if name == "WIDE":
        assert counts[0] == 3 and counts[84] == 3 * (8 + 1) + 1 and counts[85] == 40
        assert np.array_equal(N.bits(rows[traj == 0, 3:6]), N.bits(plain[traj == 0, 3:6]))  # left alone
        assert changed[84] and changed[85]                                                   # (order 8: 28 samples are just enough)


@both_scenes
@pytest.mark.parametrize("xy_gap", [0, 3])
def test_the_device_and_the_harness_fill_the_same_grid(name, xy_gap):
    grid = _grid(name)
    dev = DeviceTrajectorySolver().reconstruct(grid, xy_gap=xy_gap, xyz_gap=3, want_grids=True)
    cpu = N.HarnessTrajectorySolver().reconstruct(grid, xy_gap=xy_gap, xyz_gap=3, want_grids=True)
    assert np.array_equal(dev.xy_filled, cpu.xy_filled, equal_nan=True) and np.array_equal(dev.ft_filled, cpu.ft_filled, equal_nan=True)
    assert np.array_equal(np.isnan(dev.xy_filled), np.isnan(cpu.xy_filled)) and np.array_equal(np.isnan(dev.ft_filled), np.isnan(cpu.ft_filled))
    assert np.array_equal(np.isnan(dev.frame_time), np.isnan(cpu.frame_time))
    assert np.array_equal(N.bits(dev.frame_time), N.bits(cpu.frame_time))  # the same sum in the same order, the same NaN
    empty = np.isnan(dev.frame_time)
    print(f"{name} xy_gap {xy_gap}: {int(empty.sum())} of {grid.n_frames} frames without a time")
    if name == "LONG" and xy_gap == 0:
        assert empty.sum() >= 2 and (np.diff(np.flatnonzero(empty)) == 1).any()
    if name == "WIDE":
        assert not empty.any()
    assert np.array_equal(dev.valid, cpu.valid) and {1, 2} <= set(np.unique(dev.valid))
    # the harness triangulates without fused multiply-adds: the points agree to rounding, not to the bit
    at = np.flatnonzero(dev.valid)
    assert np.allclose(dev.xyz[at], cpu.xyz[at], rtol=0, atol=1e-9)
    assert np.isnan(dev.xyz[dev.valid == 0]).all() and np.isnan(dev.slot_time[dev.valid == 0]).all()
    assert np.array_equal(np.isnan(dev.slot_time), np.isnan(cpu.slot_time))


@functools.lru_cache(maxsize=None)
def _recording():
    ip, cams, _ = N.recording()
    return ip, cams


@pytest.mark.parametrize("name", ["recording", "WIDE"])
def test_float64_io_has_the_bits_of_k_triangulate(name):
    """`float32_io = 0`: undistort_one keeps the pixels in double.  The same switch of cba_triangulate is the reference, and the
    result differs from that of the default, so the switch arrived."""
    ip, cams = _recording() if name == "recording" else _scene(name)
    filled = ip.fill_gaps(S.GAP)
    want = triangulate(filled, cams, float32_io=False)
    got = reconstruct_trajectories(ip, cams, xy_gap_fill=S.GAP, float32_io=False)
    rows = _compare(got, want, N.frame_time_bound(filled.df, N.keyed(want.df)[:, 0].astype(np.int64)), f"{name} float32_io 0")
    single = N.keyed(reconstruct_trajectories(ip, cams, xy_gap_fill=S.GAP, float32_io=True).df)
    assert np.array_equal(single[:, :3], rows[:, :3]) and not np.array_equal(single[:, 3:6], rows[:, 3:6])
    print(f"{name}: max |float64_io - float32_io| = {np.max(np.abs(single[:, 3:6] - rows[:, 3:6])):.3e}")


def test_a_grid_without_rows_comes_back_empty():
    """The `n_rows == 0` path of the entry point, which no kernel runs: NaN everywhere, no slot valid, as the harness has it."""
    grid = _grid("WIDE")
    bare = dataclasses.replace(grid, row_cam=grid.row_cam[:0].copy(), row_slot=grid.row_slot[:0].copy(), row_xy=grid.row_xy[:0].copy(),
                               row_time=grid.row_time[:0].copy())
    assert (bare.n_cams, bare.n_traj, bare.n_frames, len(bare.row_cam)) == (4, 86, 40, 0)
    kw = dict(xy_gap=3, xyz_gap=3, filt=filter_coefficients((30.0, 6.0, 2)), want_grids=True)
    dev, cpu = DeviceTrajectorySolver().reconstruct(bare, **kw), N.HarnessTrajectorySolver().reconstruct(bare, **kw)
    for name in OUTPUTS:
        a = getattr(dev, name)
        assert a.shape == getattr(cpu, name).shape and np.array_equal(a, getattr(cpu, name), equal_nan=True), name
        assert not a.any() if name == "valid" else np.isnan(a).all(), name
    assert dev.xyz.shape == (3440, 3) and dev.xy_filled.shape == (4, 3440, 2) and dev.frame_time.shape == (40,)


def test_the_memory_limit_of_the_caller_refuses_and_the_next_call_runs():
    """4 cameras x 350 slots x 24 bytes alone are 33 600."""
    ip, cams = _recording()
    grid = trajectory_grid(ip, cams)
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory, 30000 are available") as dev:
        DeviceTrajectorySolver(memory_limit=30000).reconstruct(grid, xy_gap=3)
    with pytest.raises(ValueError) as cpu:
        N.HarnessTrajectorySolver(memory_limit=30000).reconstruct(grid, xy_gap=3)
    assert str(dev.value) == str(cpu.value)
    filled = ip.fill_gaps(3)
    want = filled.triangulate(cams)
    _compare(reconstruct_trajectories(ip, cams, xy_gap_fill=3), want, N.frame_time_bound(filled.df, N.keyed(want.df)[:, 0].astype(np.int64)),
             "after the refusal")


def test_two_calls_return_the_same_bytes():
    grid = _grid("WIDE")
    kw = dict(xy_gap=3, xyz_gap=3, filt=filter_coefficients((30.0, 6.0, 8)), want_grids=True)
    a, b = DeviceTrajectorySolver().reconstruct(grid, **kw), DeviceTrajectorySolver().reconstruct(grid, **kw)
    for name in OUTPUTS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert set(np.unique(a.valid)) == {0, 1, 2}
