"""caliscope_amd.reconstruction without a GPU: the routines of csrc/trajectory_math.h in their g++ build (tests/trajectory_native.py)
against pandas (`_fill_track_gaps`), scipy (`filtfilt`) and the reference's own tables, the whole call through `_solver`, and the
refusals.  The device kernels call the same routines: tests/test_reconstruction_gpu.py, and on the edge scenes of
tests/trajectory_scenes.py, which run here too, tests/test_reconstruction_edges_gpu.py."""
import functools
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from scipy.signal import butter, filtfilt

from caliscope_amd.point_data import ImagePoints, WorldPoints
from caliscope_amd.reconstruction import filter_coefficients, reconstruct_trajectories, reconstruct_xyz, trajectory_grid
from caliscope_amd.synthetic import ring_camera_array
from tests import trajectory_native as N
from tests import trajectory_scenes as S

TABLES = sorted((Path(__file__).parent / "golden" / "reference_host").glob("tables_*.npz"))


def _random_tracks(seed, n_cams=3, n_traj=4, n_frames=60, drop=0.35):
    rng = np.random.default_rng(seed)
    c, j, f = np.meshgrid(np.arange(n_cams), np.arange(n_traj), np.arange(n_frames), indexing="ij")
    keep = rng.random(c.shape) > drop
    c, j, f = c[keep], j[keep], f[keep]
    df = pd.DataFrame({"sync_index": f + 3, "cam_id": c * 2 + 1, "object_id": j // 2, "keypoint_id": (j % 2) * 5 + 2,
                       "img_loc_x": rng.uniform(0, 1920, len(f)), "img_loc_y": rng.uniform(0, 1080, len(f)), "frame_time": rng.uniform(0, 100, len(f))})
    return ImagePoints(df.iloc[rng.permutation(len(df))].reset_index(drop=True))


@pytest.mark.parametrize("gap", [0, 1, 3, 5])
@pytest.mark.parametrize("seed", [0, 1])
def test_the_2d_fill_equals_fill_track_gaps_bit_for_bit(seed, gap):
    ip = _random_tracks(seed)
    cams = ring_camera_array(8)  # cam_ids 1, 3, 5 of the table are posed
    grid = trajectory_grid(ip, cams)
    got = N.HarnessTrajectorySolver().reconstruct(grid, xy_gap=gap, want_grids=True)
    xy, ft, mean, filled = N.host_grid(ip, grid, gap)
    assert np.array_equal(np.isnan(got.xy_filled), np.isnan(xy)) and np.array_equal(np.isnan(got.ft_filled), np.isnan(ft))  # the keys
    assert np.array_equal(got.xy_filled, xy, equal_nan=True) and np.array_equal(got.ft_filled, ft, equal_nan=True)
    if gap:
        assert np.isnan(xy).sum() < np.isnan(N.host_grid(ip, grid, 0)[0]).sum()  # something was filled
    syncs = np.arange(grid.n_frames) + grid.sync_min
    assert np.all(np.abs(got.frame_time - mean) <= N.frame_time_bound(filled, syncs))


def test_the_fill_formula_is_the_one_of_fill_track_gaps():
    rng = np.random.default_rng(3)
    for _ in range(200):
        left, right, k = rng.normal(0, 500), rng.normal(0, 500), int(rng.integers(1, 9))
        for i in range(1, k + 1):
            assert N.harness().th_lerp(left, right, i, k) == left + (right - left) * (i / (k + 1.0))


@pytest.mark.parametrize("order,fps,cutoff", [(2, 30.0, 6.0), (3, 60.0, 4.0)])
@pytest.mark.parametrize("length", ["smallest", 64, 1000])
def test_the_filter_equals_scipy_filtfilt_bit_for_bit(order, fps, cutoff, length):
    n = 3 * (order + 1) + 1 if length == "smallest" else length
    rng = np.random.default_rng(n + order)
    x = np.cumsum(rng.normal(0, 0.01, n)) + 0.3 * np.sin(np.arange(n) * 0.11) + rng.normal(0, 0.002, n) + 1.5
    o, b, a, zi = filter_coefficients((fps, cutoff, order))
    y, filtered = N.filtfilt(x, o, b, a, zi)
    want = filtfilt(*butter(order, cutoff, btype="low", fs=fps, output="ba"), x)
    assert filtered
    assert np.array_equal(N.bits(y), N.bits(want)), float(np.max(np.abs(y - want)) / np.max(np.abs(x)))


@pytest.mark.parametrize("order", range(1, 9))
def test_the_filter_equals_scipy_filtfilt_at_every_order(order):
    """traj_lfilter_step keeps its state with fixed trip counts and a select per entry, so every order runs other code; the padding
    and both reflections depend on the order too.  Three pairs of frame rate and cutoff, the fewest samples the order filters, 64
    and 300."""
    for fps, cutoff in ((30.0, 6.0), (60.0, 4.0), (120.0, 10.0)):
        o, b, a, zi = filter_coefficients((fps, cutoff, order))
        assert o == order and len(b) == len(a) == order + 1 and len(zi) == order
        want_ba = butter(order, cutoff, btype="low", fs=fps, output="ba")
        for n in (3 * (order + 1) + 1, 64, 300):
            rng = np.random.default_rng(1000 * order + n)
            x = np.cumsum(rng.normal(0, 0.01, n)) + 0.3 * np.sin(np.arange(n) * 0.11) + rng.normal(0, 0.002, n) + 1.5
            y, filtered = N.filtfilt(x, o, b, a, zi)
            want = filtfilt(*want_ba, x)
            assert filtered and not np.array_equal(y, x)
            assert np.array_equal(N.bits(y), N.bits(want)), (fps, cutoff, n, float(np.max(np.abs(y - want)) / np.max(np.abs(x))))


@pytest.mark.parametrize("order", [1, 2, 3, 8])
def test_short_signals_are_left_alone(order):
    o, b, a, zi = filter_coefficients((30.0, 5.0, order))
    x = np.linspace(0.0, 1.0, 3 * order) ** 2
    y, filtered = N.filtfilt(x, o, b, a, zi)
    assert not filtered and np.array_equal(y, x)


def test_the_table_fixtures_are_there():
    assert len(TABLES) == 6


@pytest.mark.parametrize("path", TABLES, ids=lambda p: p.stem)
def test_world_stages_reproduce_the_reference_s_tables(path):
    """`world_filled_{gap}`, `world_smoothed` and `world_smoothed_o3` of the reference's own run, compared as tables sorted by
    (sync_index, object_id, keypoint_id) with the tolerance tests/test_reference_host_fixtures.py gives the host chain (1e-12
    absolute), and bit for bit against that host chain.  The fill works on sync indices and takes the tables as they are."""
    ref = np.load(path)
    wcols = [str(c) for c in ref["world_columns"]]
    wdf = pd.DataFrame(ref["world"], columns=N.WORLD_COLS).astype({"sync_index": "int64", "object_id": "int64", "keypoint_id": "int64"})
    wp = WorldPoints(wdf)

    def same(mine, theirs, host):
        mine, host = N.keyed(mine), N.keyed(host)
        theirs = theirs[np.lexsort((theirs[:, 2], theirs[:, 1], theirs[:, 0]))]
        assert mine.shape == theirs.shape and np.array_equal(mine[:, :3], theirs[:, :3])
        assert np.array_equal(np.isnan(mine), np.isnan(theirs))
        assert np.allclose(mine, theirs, rtol=0, atol=1e-12, equal_nan=True), float(np.nanmax(np.abs(mine - theirs)))
        assert np.array_equal(mine, host, equal_nan=True)

    for gap in (1, 3, 5):
        cols = [str(c) for c in ref[f"world_filled_{gap}_columns"]]
        same(N.world_stages(wdf, gap), ref[f"world_filled_{gap}"][:, [cols.index(c) for c in wcols]], wp.fill_gaps(gap).df)
    # The reference filters a trajectory's samples in table order, and these tables are shuffled.  On the grid the order of the samples
    # is the order of the frames, so every row is laid at the frame of its position within its trajectory; `smooth` keeps the rows
    # where they are, so the same positions key the reference's output.
    rank = wdf.groupby(["object_id", "keypoint_id"]).cumcount().to_numpy()
    assert not np.all(np.diff(wdf["sync_index"].to_numpy()[np.argsort(wdf["object_id"].to_numpy() * 1000 + wdf["keypoint_id"].to_numpy(), kind="stable")]) >= 0)
    laid = wdf.assign(sync_index=rank)
    for key, args in (("world_smoothed", (30.0, 6.0, 2)), ("world_smoothed_o3", (60.0, 4.0, 3))):
        theirs = ref[key].copy()
        assert np.array_equal(theirs[:, :3], wdf[N.WORLD_COLS[:3]].to_numpy(dtype=np.float64))
        theirs[:, 0] = rank
        same(N.world_stages(laid, 0, filter_coefficients(args)), theirs, wp.smooth(*args).df.assign(sync_index=rank))


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    return N.recording()


@pytest.mark.parametrize("gap", [0, 1, 3])
def test_the_whole_call_on_the_harness(scene, gap):
    """Filled grids and per-frame times against the host chain; the slots that hold a point are those with two posed views in the
    host chain's filled table; the points sit near the ground truth.  That last check is one of geometry, not of precision: 0.3 px of
    noise are 4 mm across the ray at five sigma (1.5 px / 1394.6 px x 3.6 m), and the two posed cameras that are 144 degrees apart see a
    point under 36 degrees, which stretches that by 1 / sin 36 = 1.7 along their bisector: 7 mm; 1 cm is asked."""
    ip, cams, truth = scene
    grid = trajectory_grid(ip, cams)
    assert (grid.n_cams, grid.n_traj, grid.n_frames, grid.sync_min) == (4, 5, N.N_FRAMES, N.SYNC0) and grid.cam_posed.tolist() == [1, 1, 0, 1]
    got = N.HarnessTrajectorySolver().reconstruct(grid, xy_gap=gap, want_grids=True)
    xy, ft, mean, filled = N.host_grid(ip, grid, gap)
    assert np.array_equal(got.xy_filled, xy, equal_nan=True) and np.array_equal(got.ft_filled, ft, equal_nan=True)
    assert np.all(np.abs(got.frame_time - mean) <= N.frame_time_bound(filled, np.arange(grid.n_frames) + grid.sync_min))
    views = (~np.isnan(xy[grid.cam_posed.astype(bool), :, 0])).sum(axis=0)
    assert np.array_equal(got.valid, (views >= 2).astype(np.uint8))
    at = np.flatnonzero(got.valid)
    if gap == 0:  # (filled rows lie on a chord of the true curve, and in the long hole far from it)
        assert np.max(np.abs(got.xyz[at] - truth.reshape(-1, 3)[at])) < 1e-2
    assert np.isnan(got.xyz[got.valid == 0]).all() and np.isnan(got.slot_time[got.valid == 0]).all()
    assert np.array_equal(got.slot_time[at], got.frame_time[at // grid.n_traj])
    valid = got.valid.reshape(N.N_FRAMES, 5)
    assert valid[:, 0].all() and valid[:6, 1].all() and not valid[6:, 1].any()  # one posed + the unposed camera: no point
    assert valid[50:52, 2].all() == (gap >= 2) and not valid[20 + gap:50, 3].any() and valid[20:20 + gap, 3].all()


@pytest.mark.parametrize("xy_gap,xyz_gap,smooth,short", [(0, 1, None, 10), (0, 3, None, 10), (3, 3, None, 10), (3, 3, (30.0, 6.0, 2), 10),
                                                         (3, 3, (60.0, 4.0, 3), 13), (0, 0, (30.0, 6.0, 2), 10)])
def test_the_3d_stages_of_the_whole_call_equal_the_host_chain(xy_gap, xyz_gap, smooth, short):
    """`reconstruct_trajectories(.., xyz_gap_fill, smooth)` against `WorldPoints.fill_gaps` / `.smooth` of its own triangulated table
    (the harness triangulates), bit for bit: the same line, the same recurrence."""
    ip, cams, _ = N.recording(short=short)
    solver = N.HarnessTrajectorySolver()
    base = reconstruct_trajectories(ip, cams, xy_gap_fill=xy_gap, _solver=solver)
    got = reconstruct_trajectories(ip, cams, xy_gap_fill=xy_gap, xyz_gap_fill=xyz_gap, smooth=smooth, _solver=solver)
    want = base.fill_gaps(xyz_gap) if xyz_gap else base
    assert len(want) > len(base) or not xyz_gap
    if smooth:
        counts = want.df.groupby(["object_id", "keypoint_id"]).size()
        assert counts.loc[(1, 7)] == 3 * (smooth[2] + 1) + 1 and counts.loc[(0, 1)] <= 3 * smooth[2]
        want = want.smooth(*smooth)
        untouched = got.df[(got.df["object_id"] == 0) & (got.df["keypoint_id"] == 1)]
        assert np.array_equal(N.keyed(untouched), N.keyed(base.df[(base.df["object_id"] == 0) & (base.df["keypoint_id"] == 1)]))
    assert list(got.df.columns) == N.WORLD_COLS and solver.calls == 2
    assert np.array_equal(N.keyed(got.df), N.keyed(want.df), equal_nan=True)
    assert np.array_equal(got.df[N.WORLD_COLS[:3]].to_numpy(), N.keyed(got.df)[:, :3].astype(np.int64))  # sorted by (sync, object, keypoint)


# ---- the edge scenes of tests/trajectory_scenes.py (on the device: tests/test_reconstruction_edges_gpu.py) --------------------------------

@pytest.mark.parametrize("gap", [0, 3])
@pytest.mark.parametrize("name", ["WIDE", "LONG"])
def test_the_edge_scenes_fill_the_grids_of_the_host_chain(name, gap):
    """Grids bit for bit, the per-frame mean within frame_time_bound, and a frame without a row from any camera NaN here exactly
    where the pandas mean has no entry (LONG without the 2-D fill has such frames, two of them in a row)."""
    sc = S.SCENES[name]()
    ip, cams = sc.image_points, sc.cameras
    grid = trajectory_grid(ip, cams)
    got = N.HarnessTrajectorySolver().reconstruct(grid, xy_gap=gap, want_grids=True)
    xy, ft, mean, filled = N.host_grid(ip, grid, gap)
    assert np.array_equal(np.isnan(got.xy_filled), np.isnan(xy)) and np.array_equal(np.isnan(got.ft_filled), np.isnan(ft))
    assert np.array_equal(got.xy_filled, xy, equal_nan=True) and np.array_equal(got.ft_filled, ft, equal_nan=True)
    if gap:
        assert np.isnan(xy).sum() < np.isnan(N.host_grid(ip, grid, 0)[0]).sum()
    empty = np.isnan(mean)
    assert np.array_equal(np.isnan(got.frame_time), empty)
    assert np.array_equal(empty, np.isnan(ft).all(axis=0).reshape(grid.n_frames, grid.n_traj).all(axis=1))
    if name == "LONG" and gap == 0:
        assert empty.sum() >= 2 and (np.diff(np.flatnonzero(empty)) == 1).any() and empty[[128, 129]].all()
    if name == "WIDE":
        assert not empty.any()
    syncs = (np.arange(grid.n_frames) + grid.sync_min)[~empty]
    assert np.all(np.abs(got.frame_time[~empty] - mean[~empty]) <= N.frame_time_bound(filled, syncs))
    views = (~np.isnan(xy[grid.cam_posed.astype(bool), :, 0])).sum(axis=0)
    assert np.array_equal(got.valid, (views >= 2).astype(np.uint8))
    assert np.isnan(got.slot_time[got.valid == 0]).all() and np.isfinite(got.slot_time[got.valid == 1]).all()


@functools.lru_cache(maxsize=None)
def _edge_base(name, xy_gap):
    """The harness's own triangulated table of a scene: what its 3-D stages are compared from."""
    sc = S.SCENES[name]()
    return reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=xy_gap, _solver=N.HarnessTrajectorySolver())


@pytest.mark.parametrize("xy_gap,xyz_gap", [(0, 1), (0, 3), (3, 3)])
@pytest.mark.parametrize("name", ["WIDE", "LONG"])
def test_the_edge_scenes_fill_the_3d_holes_of_the_host_chain(name, xy_gap, xyz_gap):
    """On LONG without the 2-D fill the line of the times runs across frames that have no time of their own."""
    sc = S.SCENES[name]()
    base = _edge_base(name, xy_gap)
    want = base.fill_gaps(xyz_gap)
    assert len(want) > len(base)
    got = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=xy_gap, xyz_gap_fill=xyz_gap, _solver=N.HarnessTrajectorySolver())
    assert np.array_equal(N.keyed(got.df), N.keyed(want.df)) and np.isfinite(N.keyed(got.df)).all()
    if name == "LONG" and xy_gap == 0:
        rows = set(sc.image_points.df["sync_index"])
        assert len(set(got.df["sync_index"]) - rows) >= 2 and not set(base.df["sync_index"]) - rows


@pytest.mark.parametrize("order", [1, 2, 5, 8])
@pytest.mark.parametrize("name", ["WIDE", "LONG"])
def test_the_edge_scenes_are_filtered_as_the_host_chain_filters_them(name, order):
    sc = S.SCENES[name]()
    unsmoothed = _edge_base(name, S.GAP).fill_gaps(S.GAP)
    counts = unsmoothed.df.groupby(["object_id", "keypoint_id"]).size().to_numpy()
    assert np.array_equal(counts, S.samples(sc))
    want = unsmoothed.smooth(30.0, 6.0, order)
    got = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=S.GAP, xyz_gap_fill=S.GAP, smooth=(30.0, 6.0, order),
                                   _solver=N.HarnessTrajectorySolver())
    rows, plain = N.keyed(got.df), N.keyed(unsmoothed.df)
    assert np.array_equal(N.bits(rows), N.bits(N.keyed(want.df)))
    traj = (rows[:, 1] * 7 + rows[:, 2]).astype(np.int64)
    changed = np.array([not np.array_equal(rows[traj == j, 3:6], plain[traj == j, 3:6]) for j in range(len(counts))])
    assert np.array_equal(changed, counts > 3 * order)
    if name == "WIDE":
        assert counts[0] == 3 and counts[84] == 3 * (8 + 1) + 1 and not changed[0] and changed[84] and changed[85]
        assert np.array_equal(N.bits(rows[traj == 0]), N.bits(plain[traj == 0]))


def test_reconstruct_xyz_writes_the_table_or_nothing(scene, tmp_path):
    ip, cams, _ = scene
    solver = N.HarnessTrajectorySolver()
    path = reconstruct_xyz(ip, cams, "walk", tmp_path, _solver=solver)
    assert path == tmp_path / "xyz_walk.csv" and path.exists()
    back, want = WorldPoints.from_csv(path), reconstruct_trajectories(ip, cams, xy_gap_fill=3, _solver=solver)
    assert np.array_equal(back.df[N.WORLD_COLS[:3]].to_numpy(), want.df[N.WORLD_COLS[:3]].to_numpy())
    assert np.allclose(back.df[N.WORLD_COLS[3:]].to_numpy(), want.df[N.WORLD_COLS[3:]].to_numpy(), rtol=0, atol=1e-6)
    assert reconstruct_xyz(ImagePoints(ip.df.iloc[:0]), cams, "none", tmp_path, _solver=solver) is None
    single = ImagePoints(ip.df[ip.df["cam_id"].isin([0, 3])])  # one posed view per slot
    assert reconstruct_xyz(single, cams, "single", tmp_path, _solver=solver) is None
    assert sorted(p.name for p in tmp_path.iterdir()) == ["xyz_walk.csv"]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(scene):
    from caliscope_amd.cameras import CameraArray

    ip, cams, _ = scene
    solver = N.HarnessTrajectorySolver()
    df = ip.df
    with pytest.raises(ValueError, match="duplicates"):
        reconstruct_trajectories(ImagePoints(pd.concat([df, df.iloc[[7]]], ignore_index=True)), cams, _solver=solver)
    negative = df.copy()
    negative.loc[3, "sync_index"] = -1
    with pytest.raises(ValueError, match="row 3 has the negative sync_index -1"):
        reconstruct_trajectories(ImagePoints(negative), cams, _solver=solver)
    infinite = df.copy()
    infinite.loc[11, "img_loc_y"] = np.inf
    with pytest.raises(ValueError, match="row 11 has a pixel position that is not finite"):
        reconstruct_trajectories(ImagePoints(infinite), cams, _solver=solver)
    with pytest.raises(ValueError, match="order must be in 1..8, got 9"):
        reconstruct_trajectories(ip, cams, smooth=(30.0, 6.0, 9), _solver=solver)
    assert solver.calls == 0
    # a trajectory of 8 samples at order 2: scipy raises in the host chain, the call refuses before anything runs
    eight, _, _ = N.recording(short=8)
    with pytest.raises(ValueError, match="trajectory 4 has 8 samples"):
        reconstruct_trajectories(eight, cams, smooth=(30.0, 6.0, 2), _solver=solver)
    with pytest.raises(ValueError):
        reconstruct_trajectories(eight, cams, _solver=solver).smooth(30.0, 6.0, 2)
    # empty table, no posed camera: an empty table with the frame_time column, no call
    calls = solver.calls
    for empty in (reconstruct_trajectories(ImagePoints(df.iloc[:0]), cams, _solver=solver),
                  reconstruct_trajectories(ip, CameraArray({3: cams.cameras[3]}), _solver=solver)):
        assert len(empty) == 0 and list(empty.df.columns) == N.WORLD_COLS
    assert solver.calls == calls
    # the grid against the memory figure handed to the check: 4 cameras x 350 slots x 24 bytes alone are 33 600
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory, 30000 are available"):
        reconstruct_trajectories(ip, cams, _solver=N.HarnessTrajectorySolver(memory_limit=30000))
    assert len(reconstruct_trajectories(ip, cams, _solver=N.HarnessTrajectorySolver(memory_limit=10**6))) > 0


def test_the_library_s_own_checks_name_the_row(scene):
    """What the C ABI refuses when it is called without reconstruction.py's marshalling: rows out of order, a duplicate, an index out
    of range, a pixel that is not finite."""
    import dataclasses

    ip, cams, _ = scene
    grid = trajectory_grid(ip, cams)
    solver = N.HarnessTrajectorySolver()

    def changed(**kw):
        return dataclasses.replace(grid, **{k: v.copy() for k, v in kw.items()})

    slot = grid.row_slot.copy()
    slot[[4, 5]] = slot[[5, 4]]
    with pytest.raises(ValueError, match="row 5: rows are not sorted"):
        solver.reconstruct(changed(row_slot=slot))
    slot = grid.row_slot.copy()
    slot[9] = slot[8]
    with pytest.raises(ValueError, match="row 9: duplicate of row 8"):
        solver.reconstruct(changed(row_slot=slot))
    slot = grid.row_slot.copy()
    slot[-1] = grid.n_slots
    with pytest.raises(ValueError, match=r"slot 350 out of range \[0, 350\)"):
        solver.reconstruct(changed(row_slot=slot))
    cam = grid.row_cam.copy()
    cam[0] = -1
    with pytest.raises(ValueError, match="row 0: camera -1 out of range"):
        solver.reconstruct(changed(row_cam=cam))
    xy = grid.row_xy.copy()
    xy[20, 0] = np.nan
    with pytest.raises(ValueError, match="row 20: pixel is not finite"):
        solver.reconstruct(changed(row_xy=xy))


def test_the_symbol_is_in_its_own_header_and_the_functions_are_exported():
    import caliscope_amd
    from caliscope_amd import _lib, build
    from caliscope_amd import reconstruction as R

    root = Path(__file__).resolve().parent.parent
    assert "cba_reconstruct_trajectories" in (root / "include" / "caliscope_trajectory.h").read_text()
    assert "cba_reconstruct_trajectories" not in (root / "include" / "caliscope_ba.h").read_text()
    assert list(R.TRAJECTORY_SIGNATURES) == ["cba_reconstruct_trajectories"] and "cba_reconstruct_trajectories" not in _lib.SIGNATURES
    assert caliscope_amd.reconstruct_trajectories is R.reconstruct_trajectories and caliscope_amd.reconstruct_xyz is R.reconstruct_xyz
    names = {p.name for p in build.SOURCES + build.DEPENDS}
    assert {"trajectory_lib.hip", "trajectory_math.h", "caliscope_trajectory.h"} <= names
