"""cba_smooth_trajectories and cba_reconstruct_trajectories_smoothed on the g++ build of their thread body and checks
(tests/trajectory_smooth_native.py): the smoother against the two numpy restatements of tests/trajectory_smooth_oracle.py on the
scenes of tests/trajectory_smooth_scenes.py, what its numbers mean (tracks drawn from the model itself), the refusals, the Python
layer and the C ABI.  The device runs the same routine in tests/test_trajectory_smoother_gpu.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from caliscope_amd import _lib
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.reconstruction import TrajDesc, TrajOut, reconstruct_trajectories, reconstruct_xyz, trajectory_grid
from caliscope_amd.trajectory_refinement import RefineOptions
from caliscope_amd.trajectory_smoother import (SMOOTHED_COLUMNS, TRAJ_SMOOTHER_SIGNATURES, SmoothDesc, SmootherOptions, TrajSmoother, TrajSmoothOut,
                                               smooth_trajectories, smoothed_frame)
from caliscope_amd.trajectory_uncertainty import COVARIANCE_COLUMNS, CovarianceOptions, full_matrices, uncertainty_tables
from tests import refine_scenes as RS
from tests import trajectory_cov_native as CN
from tests import trajectory_smooth_native as SN
from tests import trajectory_smooth_oracle as SO
from tests import trajectory_smooth_scenes as SC

ROOT = Path(__file__).resolve().parent.parent
OPTIONS = SmootherOptions(fps=30.0, accel_density=2.0)  # of the refine_scenes recording (30 frames per second, 0.15 m sinusoids)
KEYS = ["sync_index", "object_id", "keypoint_id"]


# ---- 1. the recursion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge", "one"])
def test_scene_matches_both_restatements(name):
    """Largest disagreement observed on the g++ build, EDGE: against the joint least-squares solve 9.8e-13 sqrt(tr P) and 3.9e-10
    (0.27 and 0.08 of the bar), against the recursion in numpy 7.5e-13 and 8.3e-10 (0.21, 0.17); nis to 1.4e-13.  ONE: 0 and 2e-15."""
    sc = getattr(SC, name)()
    got = SN.run_scene(SN.HarnessSmoother(), sc)
    seq, jnt = SN.oracles(name)
    SN.compare(f"g++ build, {name}, against the joint solve", got, jnt)
    SN.compare(f"g++ build, {name}, against the recursion", got, seq)
    SN.compare_nis(f"g++ build, {name}", got, seq)


def test_edge_trajectories_get_the_status_the_model_gives_them():
    sc = SC.edge()
    got = SN.run_scene(SN.HarnessSmoother(), sc)
    st, m = got.status.reshape(sc.n_frames, sc.n_traj), sc.measured.reshape(sc.n_frames, sc.n_traj) == 1
    assert ((st == 1) == m).all()  # measured and smoothed are the same cells
    assert (st[:, SC.NONE] == 0).all()
    s = SC.SINGLE_FRAME * sc.n_traj + SC.SINGLE  # one sample: the measurement itself, P = R, the velocity at its prior
    assert st[:, SC.SINGLE].sum() == 1 and np.array_equal(got.pos[s], sc.xyz[s]) and np.array_equal(got.pos_cov[s], sc.meas_cov[s])
    assert np.array_equal(got.vel[s], np.zeros(3)) and np.array_equal(got.vel_cov[s], sc.sv0 ** 2 * np.array([1.0, 0, 0, 1, 0, 1])) and np.isnan(got.nis[s])
    a, b = SC.PAIR_FRAMES  # two samples 14 frames apart: both smoothed, nothing between them
    assert st[:, SC.PAIR].tolist() == [1 if f in (a, b) else 0 for f in range(sc.n_frames)]
    assert np.isnan(got.nis[a * sc.n_traj + SC.PAIR]) and np.isfinite(got.nis[b * sc.n_traj + SC.PAIR])
    assert st[:, SC.HOLES].tolist() == [0 if f in (20, 21, 22, 23) else 2 if f in SC.HOLES_MISSING else 1 for f in range(sc.n_frames)]
    assert (st[SC.LONG_HOLE[0]:SC.LONG_HOLE[1], SC.LONG] == 0).all() and (st[:SC.LONG_HOLE[0], SC.LONG] == 1).all() and (st[SC.LONG_HOLE[1]:, SC.LONG] == 1).all()
    assert (st[:SC.ENDS_SPAN[0], SC.ENDS] == 0).all() and (st[SC.ENDS_SPAN[1]:, SC.ENDS] == 0).all() and (st[SC.ENDS_SPAN[0]:SC.ENDS_SPAN[1], SC.ENDS] == 1).all()
    assert (st[:, SC.FULL] == 1).all() and st[0, 64] == 1 and st[39, 256] == 1
    # an interpolated frame is less certain than its measured neighbours, and the recursion went through the 30-frame hole: the
    # sample behind it has an innovation
    hole = got.pos_cov[5 * sc.n_traj + SC.HOLES, [0, 3, 5]].sum()
    assert hole > got.pos_cov[4 * sc.n_traj + SC.HOLES, [0, 3, 5]].sum() and hole > got.pos_cov[6 * sc.n_traj + SC.HOLES, [0, 3, 5]].sum()
    assert np.isfinite(got.nis[SC.LONG_HOLE[1] * sc.n_traj + SC.LONG])
    # every covariance that is returned is positive definite
    at = got.status > 0
    assert np.linalg.eigvalsh(full_matrices(got.pos_cov[at])).min() > 0 and np.linalg.eigvalsh(full_matrices(got.vel_cov[at])).min() > 0


def test_two_runs_return_the_same_bytes():
    sc = SC.edge()
    a, b = SN.run_scene(SN.HarnessSmoother(), sc), SN.run_scene(SN.HarnessSmoother(), sc)
    for name in SN.FIELDS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    alone = SN.thread_body(sc.n_frames, sc.n_traj, sc.xyz, sc.meas_cov, sc.measured, SN.options_of(sc))  # (what the GPU tests hold the device to)
    assert all(getattr(a, name).tobytes() == getattr(alone, name).tobytes() for name in SN.FIELDS)


# ---- 2. what the numbers mean ------------------------------------------------------------------------------------------------------------
def check_model_statistics(run):
    """512 tracks x 41 frames drawn from the model: the squared Mahalanobis distance of the smoothed position from the truth has mean
    3 at the middle frame (5 standard errors: 5 sqrt(6 / 512) = 0.55), and the nis has mean 3 over the 20 480 measured frames that
    have one (5 sqrt(6 / 20480) = 0.086).  The seed is one at which the oracle alone satisfies both: 2.999 and 2.991."""
    sc, truth = SC.drawn_from_the_model()
    assert sc.sv0 == 1.0 and sc.n_traj == 512 and sc.n_frames == 41 and (sc.measured == 1).all()
    m2, nis = SC.model_statistics(sc, truth, SN.sequential("drawn_from_the_model"))
    assert abs(m2 - 3.0) <= 5 * np.sqrt(6 / 512) and abs(nis - 3.0) <= 5 * np.sqrt(6 / 20480), (m2, nis)
    got = run(sc)
    m2, nis = SC.model_statistics(sc, truth, got)
    print(f"drawn from the model: mean d^T P^-1 d at the middle frame {m2:.4f}, mean nis {nis:.4f}")
    assert abs(m2 - 3.0) <= 5 * np.sqrt(6 / 512) and abs(nis - 3.0) <= 5 * np.sqrt(6 / 20480), (m2, nis)


def test_covariance_and_nis_describe_tracks_drawn_from_the_model():
    check_model_statistics(lambda sc: SN.run_scene(SN.HarnessSmoother(), sc))


def test_smoothing_a_noisy_sinusoid_brings_it_closer_to_the_truth():
    sc, truth = SC.sinusoid()
    got = SN.run_scene(SN.HarnessSmoother(), sc)
    raw, smooth = np.sqrt(((sc.xyz - truth) ** 2).sum(axis=1).mean()), np.sqrt(((got.pos - truth) ** 2).sum(axis=1).mean())
    print(f"RMS error of the samples {raw:.4e}, of the smoothed positions {smooth:.4e}")
    assert (got.status == 1).all() and smooth < raw


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------
def _small(**change):
    sc = SC.edge()
    n_frames, n_traj = 6, 3
    at = np.arange(n_frames * n_traj)
    arrays = dict(xyz=sc.xyz[at].copy(), meas_cov=sc.meas_cov[at].copy(), measured=np.ones(len(at), dtype=np.uint8))
    options = dict(fps=30.0, accel_density=2.0, velocity_prior_std=10.0, max_gap=3)
    for name, value in change.items():
        if callable(value):
            value(arrays[name])
        elif name in options:
            options[name] = value
        else:
            arrays[name] = value
    return n_frames, n_traj, arrays["xyz"], arrays["meas_cov"], arrays["measured"], SmootherOptions(**options)


def _set(index, value):
    def apply(a):
        a[index] = value
    return apply


MODEL_REFUSALS = [(dict(**{name: bad}), f"{name} must be finite and positive") for name in ("fps", "accel_density", "velocity_prior_std")
                  for bad in (0.0, -1.0, float("nan"), float("inf"))] + [(dict(max_gap=-1), "max_gap must not be negative, got -1")]


@pytest.mark.parametrize("change,words", MODEL_REFUSALS + [
    (dict(xyz=_set((7, 1), float("nan"))), "slot 7: xyz is not finite"),
    (dict(xyz=_set((17, 2), float("inf"))), "slot 17: xyz is not finite"),
    (dict(meas_cov=_set((4, 3), float("nan"))), "slot 4: meas_cov is not finite"),
    (dict(meas_cov=_set((5, 0), -1e-6)), "slot 5: meas_cov is not positive definite"),
    (dict(meas_cov=_set((9, slice(None)), [1.0, 2.0, 0.0, 1.0, 0.0, 1.0])), "slot 9: meas_cov is not positive definite"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_the_stand_alone_call_names_what_it_refuses(change, words):
    with pytest.raises(ValueError, match=re.escape(words)):
        SN.HarnessSmoother().smooth(*_small(**change))


def test_an_unmeasured_slot_may_hold_anything():
    def spoil(a):
        a[4] = np.nan
    args = _small(xyz=spoil, meas_cov=spoil, measured=_set(4, 0))
    got = SN.HarnessSmoother().smooth(*args)
    assert got.status.tolist() == [1] * 4 + [2] + [1] * 13 and np.isfinite(got.pos).all() and np.isnan(got.nis[4])
    flagged = SN.HarnessSmoother().smooth(*_small(xyz=spoil, meas_cov=spoil, measured=_set(4, 2)))  # (anything but 1 is "not measured")
    assert all(getattr(got, name).tobytes() == getattr(flagged, name).tobytes() for name in SN.FIELDS)


def test_memory_limits_count_the_buffers_of_the_smoother():
    args = _small()
    total = 586 * 18  # trajectory_smoother.h: xyz 24, meas_cov 48, measured 1, the outputs 153, the parked rows 360
    assert (SN.HarnessSmoother(total).smooth(*args).status == 1).all()
    with pytest.raises(ValueError, match=f"needs {total} bytes of device memory, {total - 1} are available"):
        SN.HarnessSmoother(total - 1).smooth(*args)
    sc = RS.scene()
    grid = trajectory_grid(sc.image_points, sc.cameras)
    tables = uncertainty_tables(grid, sc.cameras, CovarianceOptions(CN.SIGMA_PX, CN.report(CN.WIDTHS)))
    slots, cams, rows, ncp = grid.n_slots, grid.n_cams, len(grid.row_cam), tables.cam_cov.shape[0]
    plain = cams * slots * 24 + slots * 33 + grid.n_frames * 8 + rows * 36 + cams * 200  # caliscope_trajectory.h
    refined = cams * slots + slots * 25                                                    # trajectory_refine.h
    extra = slots * 49 + cams * 396 + 8 * ncp * ncp + slots * 48                           # trajectory_uncertainty.h
    for refine, total in ((RefineOptions(), plain + refined + extra + 561 * slots), (None, plain + extra + 561 * slots)):
        assert (SN.HarnessSmoother(total).reconstruct_smoothed(grid, tables, OPTIONS, refine)[3].status == 1).any()
        with pytest.raises(ValueError, match=f"and the smoother needs {total} bytes of device memory, {total - 1} are available"):
            SN.HarnessSmoother(total - 1).reconstruct_smoothed(grid, tables, OPTIONS, refine)


def test_the_smoothed_reconstruction_names_what_it_refuses():
    sc = RS.scene()
    grid = trajectory_grid(sc.image_points, sc.cameras)
    tables = uncertainty_tables(grid, sc.cameras, CovarianceOptions(CN.SIGMA_PX))
    solver = SN.HarnessSmoother()
    for change, words in MODEL_REFUSALS:
        with pytest.raises(ValueError, match=re.escape(words)):
            solver.reconstruct_smoothed(grid, tables, SmootherOptions(**{**dict(fps=30.0, accel_density=2.0), **change}))
    with pytest.raises(ValueError, match="xyz_gap 2 with the smoother"):
        solver.reconstruct_smoothed(grid, tables, OPTIONS, xyz_gap=2)
    from caliscope_amd.reconstruction import filter_coefficients
    with pytest.raises(ValueError, match="a Butterworth filter with the smoother"):
        solver.reconstruct_smoothed(grid, tables, OPTIONS, filt=filter_coefficients((30, 6, 2)))
    with pytest.raises(ValueError, match="sigma_px"):  # (the checks of the call it extends stand in front)
        solver.reconstruct_smoothed(grid, type(tables)(**{**tables.__dict__, "sigma_px": 0.0}), OPTIONS)
    lib = SN.harness()
    desc, out, sm, so = TrajDesc(), TrajOut(), TrajSmoother(fps=30.0, accel_density=2.0, velocity_prior_std=10.0, max_gap=3), TrajSmoothOut()
    assert lib.tsh_reconstruct_trajectories_smoothed(C.byref(desc), None, None, C.byref(sm), C.byref(out), None, None, C.byref(so)) == -1
    assert "uncertainty: null argument" in lib.tsh_last_error().decode()


def test_nothing_to_smooth_is_no_error():
    solver = SN.HarnessSmoother()
    none = solver.smooth(0, 5, np.zeros((0, 3)), np.zeros((0, 6)), np.zeros(0, dtype=np.uint8), OPTIONS)
    assert none.status.shape == (0,) and none.pos.shape == (0, 3)
    args = _small(measured=np.zeros(18, dtype=np.uint8), xyz=np.full((18, 3), np.nan))
    got = solver.smooth(*args)
    assert (got.status == 0).all() and all(np.isnan(getattr(got, name)).all() for name in SN.FIELDS[:5])
    sc = RS.scene()
    empty = reconstruct_trajectories(ImagePoints(sc.image_points.df.iloc[:0]), sc.cameras, covariance=CovarianceOptions(CN.SIGMA_PX), smoother=OPTIONS,
                                     _solver=solver)
    assert len(empty) == 3 and len(empty[0]) == 0 and list(empty[1].columns) == list(COVARIANCE_COLUMNS) and list(empty[2].columns) == list(SMOOTHED_COLUMNS)
    assert len(empty[2]) == 0


# ---- 4. the reconstruction with the smoother behind it, and the Python layer ------------------------------------------------------------------------
def check_smoothed_reconstruction(solver, refine, full, what):
    """One smoothed call on the refine_scenes recording: out, quality and cov_out the bytes of the uncertain call; meas_cov the noise
    term; the smoothed rows within the bar of the oracle fed the call's own xyz and meas_cov.  Returns (grid, result, cov, smoothed).
    Largest ratio to the bar observed: refined 0.18 (means) and 0.25 (covariances) on the g++ build, 0.19 and 0.12 on an MI355X; plain,
    where the 60 px outliers stay in the points and the innovations are hundreds of standard deviations, 0.36 and 0.16 on the g++
    build, 0.86 and 0.09 on an MI355X."""
    sc = RS.scene()
    grid = trajectory_grid(sc.image_points, sc.cameras)
    tables = uncertainty_tables(grid, sc.cameras, CovarianceOptions(CN.SIGMA_PX, CN.report(CN.WIDTHS) if full else None))
    result, quality, cov, sm = solver.reconstruct_smoothed(grid, tables, OPTIONS, refine, want_grids=True)
    base, base_q, base_cov = solver.reconstruct_uncertain(grid, tables, refine, want_grids=True)
    for name in ("xyz", "valid", "slot_time", "frame_time", "xy_filled", "ft_filled"):
        assert getattr(result, name).tobytes() == getattr(base, name).tobytes(), (what, name)
    for name in ("views", "rms_px", "max_px", "iterations", "status", "view_state"):
        assert quality is None or getattr(quality, name).tobytes() == getattr(base_q, name).tobytes(), (what, name)
    assert cov.cov.tobytes() == base_cov.cov.tobytes() and cov.cov_status.tobytes() == base_cov.cov_status.tobytes(), what
    ok = cov.cov_status == 1
    assert np.isnan(sm.meas_cov[~ok]).all() and np.isfinite(sm.meas_cov[ok]).all(), what
    if full:  # the noise term is what is left of cov without cov_calib, to the rounding of the sum
        assert cov.cov_calib.tobytes() == base_cov.cov_calib.tobytes(), what
        scale = np.abs(cov.cov[ok]).max(axis=1, keepdims=True)
        assert (np.abs(sm.meas_cov[ok] - (cov.cov[ok] - cov.cov_calib[ok])) <= 4 * np.finfo(float).eps * scale).all(), what
    else:
        assert cov.cov_calib is None and sm.meas_cov.tobytes() == cov.cov.tobytes(), what
    args = (grid.n_frames, grid.n_traj, result.xyz, sm.meas_cov, ok.astype(np.uint8), OPTIONS.fps, OPTIONS.accel_density, OPTIONS.velocity_prior_std,
            OPTIONS.max_gap)
    SN.compare(f"{what}, against the joint solve", sm, SO.joint(*args))
    seq = SO.sequential(*args)
    SN.compare(f"{what}, against the recursion", sm, seq)
    SN.compare_nis(what, sm, seq)
    return grid, result, cov, sm


@pytest.mark.parametrize("refined", [True, False], ids=["refined", "plain"])
@pytest.mark.parametrize("full", [True, False], ids=["full", "noise-only"])
def test_smoothed_reconstruction_on_the_host_build(refined, full):
    grid, result, cov, sm = check_smoothed_reconstruction(SN.HarnessSmoother(), RefineOptions(**CN.REFINED) if refined else None, full,
                                                          f"g++ build, {'refined' if refined else 'plain'}, {'full' if full else 'noise-only'}")
    st = sm.status.reshape(grid.n_frames, grid.n_traj)
    assert (cov.cov_status == 1).sum() == 294 and (st == 1).sum() == 294
    # trajectory 2 has no point in frames 10-12 and 20-21, trajectory 1 none in frame 50: holes of 3, 2 and 1 frames, all filled
    assert (st[10:13, 2] == 2).all() and (st[20:22, 2] == 2).all() and st[50, 1] == 2 and (st == 2).sum() == 6


def test_the_public_call_and_the_csv(tmp_path):
    sc = RS.scene()
    solver = SN.HarnessSmoother()
    options = CovarianceOptions(CN.SIGMA_PX, CN.report(CN.WIDTHS))
    kw = dict(xy_gap_fill=0, refine=RefineOptions(**CN.REFINED), return_quality=True, covariance=options, _solver=solver)
    world, quality, frame, smoothed = reconstruct_trajectories(sc.image_points, sc.cameras, smoother=OPTIONS, **kw)
    base, base_q, base_frame = reconstruct_trajectories(sc.image_points, sc.cameras, **kw)
    assert world.df.equals(base.df) and quality.equals(base_q) and frame.equals(base_frame)  # the smoother changes nothing else
    assert list(smoothed.columns) == list(SMOOTHED_COLUMNS) and len(smoothed) == 300 and (smoothed["smooth_status"] == 2).sum() == 6
    meas = smoothed["smooth_status"] == 1
    assert np.array_equal(smoothed.loc[meas, KEYS].to_numpy(), world.df[KEYS].to_numpy())
    S = full_matrices(smoothed[[f"cov_{c}" for c in ("xx", "xy", "xz", "yy", "yz", "zz")]].to_numpy())
    assert np.allclose(smoothed["std_major"] ** 2, np.linalg.eigvalsh(S)[:, -1], rtol=1e-12)
    assert np.allclose(smoothed[["std_x", "std_y", "std_z"]].to_numpy() ** 2, np.einsum("njj->nj", S), rtol=1e-12)
    # the calibration term of a sample passes through unchanged; an interpolated frame has none
    calib = smoothed[[f"cov_calib_{c}" for c in ("xx", "xy", "xz", "yy", "yz", "zz")]].to_numpy()
    share = frame["calib_share"].to_numpy() * frame[["cov_xx", "cov_yy", "cov_zz"]].sum(axis=1).to_numpy()
    assert np.isnan(calib[~meas.to_numpy()]).all() and np.allclose(calib[meas.to_numpy()][:, [0, 3, 5]].sum(axis=1), share, rtol=1e-12)
    # smoothing gains: the smoothed position of a sample is more certain than the sample, and closer to the truth over the recording
    noise = frame[["cov_xx", "cov_yy", "cov_zz"]].sum(axis=1).to_numpy() - share
    assert (smoothed.loc[meas, ["cov_xx", "cov_yy", "cov_zz"]].sum(axis=1).to_numpy() < noise).all()
    f, j = world.df["sync_index"].to_numpy() - RS.SYNC0, np.array([RS.TRAJ.index((int(o), int(k))) for o, k in zip(world.df["object_id"], world.df["keypoint_id"])])
    raw = np.sqrt(((world.df[["x_coord", "y_coord", "z_coord"]].to_numpy() - sc.truth[f, j]) ** 2).sum(axis=1).mean())
    smo = np.sqrt(((smoothed.loc[meas, ["x", "y", "z"]].to_numpy() - sc.truth[f, j]) ** 2).sum(axis=1).mean())
    assert smo < raw
    # the stand-alone call on the table and its covariance frame: with the noise term alone it is the same smoother on the same numbers
    plain_kw = dict(xy_gap_fill=0, covariance=CovarianceOptions(CN.SIGMA_PX), _solver=solver)
    table, cframe, sframe = reconstruct_trajectories(sc.image_points, sc.cameras, smoother=OPTIONS, **plain_kw)
    alone = smooth_trajectories(table, cframe, OPTIONS, _solver=solver)
    assert list(alone.columns) == list(SMOOTHED_COLUMNS) and alone.equals(sframe)
    path = reconstruct_xyz(RS.restricted(sc, 2, (0, 4)), sc.cameras, "take", tmp_path, smoother=OPTIONS, **plain_kw)
    written, cov_written = pd.read_csv(tmp_path / "xyz_take_smoothed.csv"), pd.read_csv(tmp_path / "xyz_take_covariance.csv")
    assert path == tmp_path / "xyz_take.csv" and list(written.columns) == list(SMOOTHED_COLUMNS) and len(cov_written) == len(pd.read_csv(path)) == 95
    assert len(written) == 100 and (written["smooth_status"] == 2).sum() == 5
    again = smooth_trajectories(type(table).from_csv(path), cov_written, OPTIONS, _solver=solver)  # an xyz csv with its covariance csv
    assert np.array_equal(again[KEYS].to_numpy(), written[KEYS].to_numpy()) and np.allclose(again[["x", "y", "z"]], written[["x", "y", "z"]], atol=1e-6)


def test_the_python_layer_names_its_conflicts():
    sc = RS.scene()
    solver = SN.HarnessSmoother()
    cov = CovarianceOptions(CN.SIGMA_PX)
    with pytest.raises(ValueError, match="smoother needs covariance"):
        reconstruct_trajectories(sc.image_points, sc.cameras, smoother=OPTIONS, _solver=solver)
    with pytest.raises(ValueError, match="smoother with xyz_gap_fill = 3"):
        reconstruct_trajectories(sc.image_points, sc.cameras, covariance=cov, xyz_gap_fill=3, smoother=OPTIONS, _solver=solver)
    with pytest.raises(ValueError, match="smoother with smooth"):
        reconstruct_trajectories(sc.image_points, sc.cameras, covariance=cov, smooth=(30, 6, 2), smoother=OPTIONS, _solver=solver)
    with pytest.raises(ValueError, match="smoother options are not numbers"):
        reconstruct_trajectories(sc.image_points, sc.cameras, covariance=cov, smoother=SmootherOptions("fast", 2.0), _solver=solver)
    with pytest.raises(ValueError, match="fps must be finite and positive"):
        reconstruct_trajectories(sc.image_points, sc.cameras, covariance=cov, smoother=SmootherOptions(0.0, 2.0), _solver=solver)
    assert solver.calls == 1  # (only the last one reached the library)
    table, frame = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, covariance=cov, _solver=solver)
    with pytest.raises(ValueError, match="294 rows and the covariance frame 293"):
        smooth_trajectories(table, frame.iloc[:-1], OPTIONS, _solver=solver)
    with pytest.raises(ValueError, match="keypoint_id differs"):
        smooth_trajectories(table, frame.assign(keypoint_id=frame["keypoint_id"].to_numpy()[::-1]), OPTIONS, _solver=solver)
    assert len(smooth_trajectories(type(table)(table.df.iloc[:0]), frame.iloc[:0], OPTIONS, _solver=solver)) == 0


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_header_the_table_and_the_build_agree():
    from caliscope_amd import build
    from caliscope_amd.reconstruction import TRAJECTORY_SIGNATURES
    from caliscope_amd.trajectory_refinement import REFINE_SIGNATURES
    from caliscope_amd.trajectory_uncertainty import TRAJ_UNCERTAINTY_SIGNATURES

    header = (ROOT / "include" / "caliscope" / "trajectory_smoother.h").read_text()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    names = {"cba_smooth_trajectories", "cba_reconstruct_trajectories_smoothed"}
    assert set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", text)) == set(TRAJ_SMOOTHER_SIGNATURES) == names
    for table in (TRAJECTORY_SIGNATURES, REFINE_SIGNATURES, TRAJ_UNCERTAINTY_SIGNATURES, _lib.SIGNATURES):
        assert not names & set(table)
    assert not (ROOT / "include" / "trajectory_smoother.h").exists()  # (the top level of include/ holds the headers of the first round alone)
    assert ROOT / "include" / "caliscope" / "trajectory_smoother.h" in build.DEPENDS and build.CSRC / "trajectory_smooth_math.h" in build.DEPENDS
    fields = lambda struct: re.findall(r"(\w+);", re.search(r"typedef struct \{([^}]*)\} " + struct + ";", text).group(1))
    assert fields("cba_traj_smoother") == [f[0] for f in TrajSmoother._fields_] and C.sizeof(TrajSmoother) == 32
    assert fields("cba_smooth_desc") == [f[0] for f in SmoothDesc._fields_] and C.sizeof(SmoothDesc) == 80
    assert fields("cba_traj_smooth_out") == [f[0] for f in TrajSmoothOut._fields_] and C.sizeof(TrajSmoothOut) == 56
    build.build(verbose=False)
    lib = _lib.bind(_lib.load(), TRAJ_SMOOTHER_SIGNATURES)
    for name in names:
        fn = getattr(lib, name)
        assert fn.restype == TRAJ_SMOOTHER_SIGNATURES[name][0] and fn.argtypes == TRAJ_SMOOTHER_SIGNATURES[name][1]
    assert b"k_traj_smooth" in build.OUT.read_bytes()  # the kernel is in the code object under its name
    # a refusal comes back before any device is asked for
    desc, out = SmoothDesc(n_frames=1, n_traj=1, fps=0.0, accel_density=2.0, velocity_prior_std=10.0, max_gap=3), TrajSmoothOut()
    assert lib.cba_smooth_trajectories(C.byref(desc), 0, C.byref(out)) == -1 and "fps must be finite and positive" in _lib.last_error(lib)
    smoothed = SN.run_scene(SN.HarnessSmoother(), SC.one())
    frame = smoothed_frame(type("G", (), dict(sync_min=7, n_traj=1, traj_object=np.array([2]), traj_keypoint=np.array([9])))(), smoothed)
    assert frame[KEYS].to_numpy().tolist() == [[7, 2, 9]] and frame["smooth_status"].tolist() == [1] and np.isnan(frame["cov_calib_xx"]).all()
