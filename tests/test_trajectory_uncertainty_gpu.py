"""cba_reconstruct_trajectories_uncertain on the device (k_traj_cov of csrc/trajectory_lib.hip) on the recording of
tests/refine_scenes.py — 300 slots, two workgroups, the second partly filled — against the numpy oracle of
tests/trajectory_cov_oracle.py at the device's own points and views, against the g++ build of the same thread body fed those points,
at the launch edges (256 and 257 slots), on either side of the rig size at which the camera tables leave LDS (128 and 129 cameras), at
the edges of the pair loop, and end to end behind parameter_uncertainty() of an optimised
volume.  The bar is that of tests/test_trajectory_uncertainty.py: 1e-12 cond_2(V) ||cov||_F per slot."""
import functools

import numpy as np
import pandas as pd
import pytest

from caliscope_amd.point_data import ImagePoints
from caliscope_amd.reconstruction import DeviceTrajectorySolver, filter_coefficients, reconstruct_trajectories, trajectory_grid
from caliscope_amd.trajectory_refinement import DeviceRefinedTrajectorySolver, RefineOptions
from caliscope_amd.trajectory_uncertainty import COVARIANCE_COLUMNS, CovarianceOptions, DeviceUncertainTrajectorySolver, full_matrices
from tests import refine_scenes as RS
from tests import trajectory_cov_native as CN
from tests import trajectory_cov_oracle as CO

pytestmark = pytest.mark.gpu

RESULT = ("xyz", "valid", "slot_time", "frame_time", "xy_filled", "ft_filled")
QUALITY = ("views", "rms_px", "max_px", "iterations", "status", "view_state")


class DeviceSolver(DeviceTrajectorySolver, DeviceRefinedTrajectorySolver, DeviceUncertainTrajectorySolver):
    """All three hooks on the device."""


def _options(full: bool) -> CovarianceOptions:
    return CovarianceOptions(CN.SIGMA_PX, CN.report(CN.WIDTHS) if full else None)


@functools.cache
def _grid():
    sc = RS.scene()
    return trajectory_grid(sc.image_points, sc.cameras)


@functools.cache
def _call(refined: bool, full: bool):
    """(result, quality, cov, tables) of the scene, held against the oracle once."""
    return CN.check_scene_against_oracle(DeviceSolver(), _grid(), RS.scene().cameras, _options(full), CN.REFINED if refined else None,
                                         f"device, {'refined' if refined else 'plain'}, {'full' if full else 'noise-only'}")


def _against_the_host_build(what, grid, cameras, result, quality, cov, tables):
    """The g++ build of the thread body on the device's own points and views: cov_status identical, covariances to the bar."""
    cpu = CN.cov_grid(grid, tables, result, quality)
    assert np.array_equal(cpu.cov_status, cov.cov_status), what
    at = np.flatnonzero(cov.cov_status == 1)
    full = tables.cam_cov is not None
    oracle = CO.covariance_grid(grid, cameras, tables, result.xyz, CN.used_views(grid, result, quality), at)  # (for cond_2(V))
    oracle.cov, oracle.cov_calib = cpu.cov, cpu.cov_calib if full else oracle.cov_calib  # the same bar, around the host build's figures
    CN.compare_with_oracle(f"device against the g++ build, {what}", cov, oracle, at, full)


@pytest.mark.parametrize("refined", [True, False], ids=["refined", "plain"])
@pytest.mark.parametrize("full", [True, False], ids=["full", "noise-only"])
def test_device_covariance_matches_the_oracle_and_the_host_build(refined, full):
    result, quality, cov, tables = _call(refined, full)
    assert (cov.cov_status == 1).sum() == 294 and (cov.cov_status == 0).sum() == 6
    _against_the_host_build(f"{'refined' if refined else 'plain'}, {'full' if full else 'noise-only'}", _grid(), RS.scene().cameras, result, quality, cov,
                            tables)


@pytest.mark.parametrize("n_cams", [128, 129])
def test_a_rig_at_the_size_where_the_camera_tables_leave_lds(n_cams):
    """128 cameras: the tables staged in LDS, all 48 KiB of them; 129: read from global memory.  Each landmark is seen by every fifth
    camera, so most cameras are skipped by every wave; 6- and 9-wide cameras alternate along the offsets."""
    image_points, cameras, rep = CN.wide_rig(n_cams)
    grid = trajectory_grid(image_points, cameras)
    assert grid.n_cams == n_cams and grid.n_slots == 40
    what = f"{n_cams} cameras"
    result, quality, cov, tables = CN.check_scene_against_oracle(DeviceSolver(), grid, cameras, CovarianceOptions(CN.SIGMA_PX, rep), CN.REFINED, f"device, {what}")
    assert (cov.cov_status == 1).all() and ((quality.view_state == 1).sum(axis=0) >= 25).all()
    _against_the_host_build(what, grid, cameras, result, quality, cov, tables)


def test_pair_loop_edges():
    """All six cameras (trajectory 0), the first four, the first and another (trajectory 2: cameras 0 and 4), a rejected view that must
    not contribute, the unposed camera 6 without a block — all in the scene's refined call, held against the oracle in _call; and a
    recording whose trajectory 0 is seen by the first and the last posed camera alone."""
    result, quality, cov, tables = _call(True, True)
    state = quality.view_state
    assert tables.cam_offset.tolist() == [0, 9, 18, 24, 30, 39, -1] and (state[6] == 0).all()
    ok = cov.cov_status == 1
    assert (ok & (state[:6] == 1).all(axis=0)).any() and (ok & (state == 2).any(axis=0)).sum() > 40
    assert (ok & (state[0] == 1) & (state[4] == 1) & ((state == 1).sum(axis=0) == 2)).sum() > 90
    sc = RS.scene()
    df = sc.image_points.df
    first_last = ImagePoints(df[~((df["object_id"] == 0) & (df["keypoint_id"] == 0) & df["cam_id"].isin([1, 2, 3, 4]))].reset_index(drop=True))
    grid = trajectory_grid(first_last, sc.cameras)
    result, quality, cov, _ = CN.check_scene_against_oracle(DeviceSolver(), grid, sc.cameras, _options(True), CN.REFINED, "device, cameras 0 and 5 alone")
    only = (quality.view_state[0] == 1) & (quality.view_state[5] == 1) & ((quality.view_state == 1).sum(axis=0) == 2)
    assert only[0::3].all() and (cov.cov_status[0::3] == 1).all()


def test_two_calls_return_the_same_bytes():
    kw = dict(xyz_gap=2, filt=filter_coefficients((30.0, 6.0, 2)), want_grids=True)
    tables = _call(True, True)[3]
    (a, qa, ca), (b, qb, cb) = (DeviceSolver().reconstruct_uncertain(_grid(), tables, RefineOptions(**CN.REFINED), **kw) for _ in range(2))
    for name in RESULT:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    for name in QUALITY:
        assert getattr(qa, name).tobytes() == getattr(qb, name).tobytes(), name
    for name in ("cov", "cov_calib", "cov_status"):
        assert getattr(ca, name).tobytes() == getattr(cb, name).tobytes(), name
    assert set(np.unique(ca.cov_status)) == {0, 1, 2} and (ca.cov_status[a.valid == 2] == 2).all() and (a.valid == 2).sum() == 5


def test_everything_else_is_the_call_it_extends():
    """xyz, valid, the times, the grids and the quality of the new entry point are the bytes of cba_reconstruct_trajectories_refined
    (of cba_reconstruct_trajectories in the plain call) on the same input, the fill and the filter included."""
    kw = dict(xy_gap=2, xyz_gap=3, filt=filter_coefficients((30.0, 6.0, 2)), want_grids=True)
    tables = _call(True, True)[3]
    refine = RefineOptions(**CN.REFINED)
    got, got_q, _ = DeviceSolver().reconstruct_uncertain(_grid(), tables, refine, **kw)
    want, want_q = DeviceSolver().reconstruct_refined(_grid(), refine, **kw)
    for name in RESULT:
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
    for name in QUALITY:
        assert getattr(got_q, name).tobytes() == getattr(want_q, name).tobytes(), name
    got, none, _ = DeviceSolver().reconstruct_uncertain(_grid(), tables, None, **kw)
    want = DeviceSolver().reconstruct(_grid(), **kw)
    assert none is None
    for name in RESULT:
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


@pytest.mark.parametrize("n_slots", [256, 257])
def test_a_grid_of_one_workgroup_and_of_one_thread_more(n_slots):
    """The first `n_slots` slots of the scene as a grid of their own: the same cells and cameras, so the same bytes."""
    sc = RS.scene()
    grid = trajectory_grid(RS.relabelled(sc, n_slots), sc.cameras)
    assert (grid.n_traj, grid.n_frames, grid.n_slots, grid.n_cams) == (1, n_slots, n_slots, 7)
    for refined in (True, False):
        _, _, whole, tables = _call(refined, True)
        _, _, cov = DeviceSolver().reconstruct_uncertain(grid, tables, RefineOptions(**CN.REFINED) if refined else None)
        for name in ("cov", "cov_calib", "cov_status"):
            assert getattr(cov, name).tobytes() == getattr(whole, name)[:n_slots].tobytes(), (name, refined)
        assert (cov.cov_status == 1).sum() >= n_slots - 6


def test_host_checks_refuse_before_any_launch_and_the_device_is_fine_afterwards():
    grid, tables = _grid(), _call(True, True)[3]
    bad = type(tables)(**{**tables.__dict__, "sigma_px": 0.0})
    with pytest.raises(ValueError, match="sigma_px"):
        DeviceSolver().reconstruct_uncertain(grid, bad, RefineOptions(**CN.REFINED))
    with pytest.raises(ValueError, match="bytes of device memory, 100000 are available"):
        DeviceSolver(memory_limit=100000).reconstruct_uncertain(grid, tables, None)
    again = DeviceSolver().reconstruct_uncertain(grid, tables, RefineOptions(**CN.REFINED))[2]
    assert again.cov.tobytes() == _call(True, True)[2].cov.tobytes()


def test_end_to_end_behind_the_uncertainty_report_of_an_optimised_volume():
    """parameter_uncertainty() of a volume solved by optimize(), then its own image points reconstructed with that report: the frame
    is row-aligned, the calibration has a share strictly between none and all, and cov - cov_noise is PSD to rounding."""
    from caliscope_amd.capture_volume import CaptureVolume
    from tests.helpers import small_problem

    sc, _, _ = small_problem(n_cams=4, n_points=30, k=3)
    vol = CaptureVolume.from_arrays(sc.cameras_init, sc.camera_indices, sc.image_coords, sc.obj_indices, sc.points_init).optimize()
    rep = vol.parameter_uncertainty()
    df = vol.image_points.df.copy()
    df["frame_time"] = 0.0
    image_points = ImagePoints(df)
    options = CovarianceOptions(0.5, rep)
    world, frame = reconstruct_trajectories(image_points, vol.camera_array, xy_gap_fill=0, refine=RefineOptions(loss="linear"), covariance=options)
    keys = ["sync_index", "object_id", "keypoint_id"]
    assert list(frame.columns) == list(COVARIANCE_COLUMNS) and len(frame) == len(world) == 30
    assert np.array_equal(frame[keys].to_numpy(), world.df[keys].to_numpy()) and (frame["cov_status"] == 1).all()
    assert ((frame["calib_share"] > 0.0) & (frame["calib_share"] < 1.0)).all()
    _, noise = reconstruct_trajectories(image_points, vol.camera_array, xy_gap_fill=0, refine=RefineOptions(loss="linear"), covariance=CovarianceOptions(0.5))
    cols = list(COVARIANCE_COLUMNS[3:9])
    total, alone = full_matrices(frame[cols].to_numpy()), full_matrices(noise[cols].to_numpy())
    lowest = np.linalg.eigvalsh(total - alone)[:, 0]
    print(f"calib_share {frame['calib_share'].min():.3f} .. {frame['calib_share'].max():.3f}; std_major {frame['std_major'].min() * 1e3:.3f} .. "
          f"{frame['std_major'].max() * 1e3:.3f} mm; lowest eigenvalue of cov - cov_noise / ||cov|| = {(lowest / np.linalg.norm(total, axis=(1, 2))).min():.3e}")
    assert (lowest >= -1e-12 * np.linalg.norm(total, axis=(1, 2))).all()
    assert isinstance(noise, pd.DataFrame) and noise["calib_share"].isna().all()
