"""cba_estimate_time_offsets on the g++ build of csrc/time_offset_math.h (tests/native/time_offset_harness.cpp) against the numpy
restatement of tests/time_offset_oracle.py on the scenes of tests/time_offset_scenes.py, the recovery of known offsets, and the host
side of caliscope_amd/time_offsets.py: the options, the compensated table, `apply_time_offsets` and every refusal with its message.
The bars are those of tests/time_offset_native.py and of the docstrings below."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

from caliscope_amd.reconstruction import reconstruct_trajectories
from caliscope_amd.time_offsets import (STATUS_ESTIMATED, STATUS_NONE, STATUS_REFERENCE, STATUS_UNDETERMINED, TimeOffsetOptions, apply_time_offsets,
                                        estimate_time_offsets, options_struct, run_time_offset_call)
from caliscope_amd.trajectory_refinement import RefineOptions
from tests import time_offset_native as TN
from tests import time_offset_oracle as TO
from tests import time_offset_scenes as TS
from tests.trajectory_refine_native import HarnessRefinedSolver

HUBER_PX = 1.0


def relative_truth(sc, status):
    """[n_cams] the scene's offsets against the camera with status 1."""
    t = np.array([sc.offsets[int(c)] for c in sc.grid.cam_ids])
    return t - t[np.flatnonzero(np.asarray(status) == STATUS_REFERENCE)[0]]


def tol_of(sc):
    tau = sc.image_points.df.groupby("sync_index")["frame_time"].mean().to_numpy()
    return 1e-6 * float(np.median(np.diff(tau)))


def test_the_oracle_projects_as_the_camera_model_and_its_jacobian_is_the_derivative():
    """The restatement's lens against oracle/camera_model.py (1e-10 px: both are float64 evaluations of pixels up to 2000), and its
    analytic d pixel / d X against central differences in longdouble (step 1e-6 m: truncation 1e-12 x third derivative, rounding
    1e-19 / 1e-6 x 2000 px, against entries of 500 px/m: 1e-7 relative)."""
    from oracle import camera_model as cm
    from caliscope_amd.cameras import matrix_to_rvec

    sc = TS.edge()
    g = sc.grid
    rng = np.random.default_rng(1)
    X = np.array([0.3, -0.2, 0.5]) + rng.uniform(-0.4, 0.4, (50, 3))
    for c in np.flatnonzero(g.cam_posed):
        cam = sc.cameras.cameras[int(g.cam_ids[c])]
        uv, J = TO.project(int(g.cam_model[c]), g.cam_intr[c], g.cam_P[c], X)
        ref = (cm.project_fisheye if cam.fisheye else cm.project_pinhole)(X, matrix_to_rvec(cam.rotation), cam.translation, cam.matrix, cam.distortions)[0]
        assert np.abs(uv - ref).max() < 1e-10
        Xl = X.astype(np.longdouble)
        for k in range(3):
            h = np.zeros(3, dtype=np.longdouble)
            h[k] = 1e-6
            d = (TO.project(int(g.cam_model[c]), g.cam_intr[c], g.cam_P[c], Xl + h)[0] - TO.project(int(g.cam_model[c]), g.cam_intr[c], g.cam_P[c], Xl - h)[0]) / 2e-6
            assert np.abs(d.astype(np.float64) - J[:, :, k]).max() < 1e-7 * np.abs(J).max()


@pytest.mark.parametrize("name", ["edge", "exact"])
def test_host_build_matches_the_oracle(name):
    """Observed: EDGE against the longdouble run offsets 1.3e-14, positions 1.9e-13, pixels 3.6e-13 px (0.004, 0.007 and 0.012 of the bar);
    EXACT 3.3e-14, 2.0e-13 and 3.5e-13 px (0.011, 0.010, 0.011)."""
    got = TN.run_scene(TN.HarnessTimeOffsetSolver(), getattr(TS, name)())
    f64, ld = TN.oracles(name)
    TN.compare(f"g++ build, {name}, against the oracle in float64", name, got, f64)
    TN.compare(f"g++ build, {name}, against the oracle in longdouble", name, got, ld)
    tol = tol_of(getattr(TS, name)())
    assert got.converged and got.rounds < 10 and all(c > 2.0 * tol or c < 0.8 * tol for c in f64.changes), f64.changes  # (no round ends near the tolerance)


def test_edge_scene_statuses_and_what_is_left_alone():
    sc = TS.edge()
    g = sc.grid
    got = TN.run_scene(TN.HarnessTimeOffsetSolver(), sc)
    by_id = dict(zip(g.cam_ids.tolist(), got.status.tolist()))
    assert by_id == {0: STATUS_REFERENCE, 2: STATUS_ESTIMATED, 3: STATUS_NONE, 5: STATUS_UNDETERMINED, 7: STATUS_ESTIMATED}
    c5, c3 = int(np.searchsorted(g.cam_ids, 5)), int(np.searchsorted(g.cam_ids, 3))
    assert np.isnan(got.offsets[[c5, c3]]).all() and np.isnan(got.sigma[[c5, c3]]).all() and got.rows[c3] == 0 and got.rows[c5] == 47
    assert np.isfinite(got.rms_after[c5]) and np.isnan(got.rms_after[c3])
    assert got.valid.sum() == 256 and got.valid[50] == 0 and np.isnan(got.xyz[50]).all()
    assert not got.velocity[[49, 50, 51]].any() and got.velocity[48].any()          # frames 49 and 51 miss a neighbour
    # at rest from frame 202 on.  Equal pixels give equal points, bit for bit, and V = 0, but for two places: the stop itself, and frame 210,
    # from which camera 5 adds its rows to the sums; what they leave (below 1e-5 m/s) moves one frame further with every round
    still = 211 + got.rounds
    assert np.abs(got.velocity[203:]).max() < 1e-5 and not got.velocity[still:].any() and not got.velocity[0].any() and not got.velocity[256].any()
    unused = (g.row_cam == c3) | (g.row_slot == 50)
    assert np.array_equal(got.row_used, (~unused).astype(np.uint8))
    assert got.row_xy[unused].tobytes() == g.row_xy[unused].tobytes()
    at_rest = (g.row_slot >= still) & ~unused
    assert got.row_xy[at_rest].tobytes() == g.row_xy[at_rest].tobytes()               # V = 0: nothing to compensate
    assert np.abs(got.row_xy[~unused & ~at_rest] - g.row_xy[~unused & ~at_rest]).max() > 0.5


def test_edge17_fills_a_second_tile_row_and_column():
    """The 17 posed cameras of EDGE17: 16 free columns and the reference.  The offsets of the cameras it shares with EDGE agree with
    EDGE's to 2e-5 s (the kinks of the path are model error, seen from other sides), and every offset is within 2e-5 s of the truth."""
    sc = TS.edge17()
    got = TN.run_scene(TN.HarnessTimeOffsetSolver(), sc)
    assert (got.status == STATUS_ESTIMATED).sum() == 15 and (got.status == STATUS_UNDETERMINED).sum() == 1 and got.converged
    at = got.status == STATUS_ESTIMATED
    assert np.abs(got.offsets - relative_truth(sc, got.status))[at].max() < 2e-5


def test_exact_offsets_are_recovered_within_ten_tol():
    """The model holds exactly on EXACT, and "converged" means the last change was below tol: the truth is recovered within 10 tol.
    The oracle alone meets it (1.5e-9 s against 3.3e-7), then the g++ build."""
    sc = TS.exact()
    tol = tol_of(sc)
    f64 = TN.oracles("exact")[0]
    assert f64.converged and np.nanmax(np.abs(np.asarray(f64.offsets, dtype=np.float64) - relative_truth(sc, f64.status))) <= 10.0 * tol
    got = TN.run_scene(TN.HarnessTimeOffsetSolver(), sc)
    err = np.nanmax(np.abs(got.offsets - relative_truth(sc, got.status)))
    print(f"EXACT: largest |offset - truth| {err:.3e} s, tol {tol:.3e} s; positions {np.abs(got.xyz - sc.truth.reshape(-1, 3)).max():.3e} m; "
          f"rms before {got.rms_before.max():.3f} px, after {got.rms_after.max():.3e} px")
    assert got.converged and err <= 10.0 * tol
    assert np.abs(got.xyz - sc.truth.reshape(-1, 3)).max() < 1e-6 and got.rms_after.max() < 1e-4 < 0.1 < got.rms_before.min()


@pytest.fixture(scope="module")
def curved_bound():
    """(bias_c, 4 sigma_c + bias_c) by camera of the grid: the oracle's error on the noise-free copy is the model error (no
    acceleration term), not tuned away; sigma_c is the oracle's on CURVED."""
    clean, noisy = TS.curved_clean(), TS.curved()
    oc, on = TO.estimate(clean.grid), TO.estimate(noisy.grid)
    bias = np.abs(np.asarray(oc.offsets, dtype=np.float64) - relative_truth(clean, oc.status))
    return bias, 4.0 * on.sigma + bias, on


def sigma0_bounds(res, sigma_px):
    dof = 2 * int(res.rows.sum()) - 3 * int(np.asarray(res.valid).sum()) - int((np.asarray(res.status) == STATUS_ESTIMATED).sum())
    return sigma_px * np.sqrt(stats.chi2.ppf([0.0005, 0.9995], dof) / dof)


def test_curved_offsets_within_four_sigma_and_the_model_error(curved_bound):
    """|offset - truth| <= 4 sigma_c + bias_c, and sigma0 within the two-sided 0.1 % bounds of chi-square around the 0.3 px the rows
    were drawn with.  Observed: bias at most 9.5e-6 s, errors at most 0.29 of the bound, sigma0 0.3029 px in [0.2862, 0.3140]; the
    oracle passes both, then the g++ build (which agrees with it to 1e-16 s)."""
    bias, bound, on = curved_bound
    sc = TS.curved()
    lo, hi = sigma0_bounds(on, sc.sigma_px)
    for what, res in (("oracle", on), ("g++ build", TN.run_scene(TN.HarnessTimeOffsetSolver(), sc))):
        err = np.abs(np.asarray(res.offsets, dtype=np.float64) - relative_truth(sc, res.status))
        at = np.asarray(res.status) == STATUS_ESTIMATED
        print(f"CURVED, {what}: bias {bias[at].max():.3e} s, error / bound {np.max(err[at] / bound[at]):.3f}, sigma0 {res.sigma0_px:.4f} px in [{lo:.4f}, {hi:.4f}]")
        assert at.sum() == 4 and res.converged and (err[at] <= bound[at]).all() and lo <= res.sigma0_px <= hi


def test_gross_rows_move_the_offsets_unless_the_loss_is_huber(curved_bound):
    """OUTLIER against CURVED's bound.  Observed: with huber_px = 1 the errors are at most 0.47 of it; without, the largest is 14 times
    it (6.2e-3 s), so the scene is not too mild.  The restatement with the same loss agrees with the g++ build to 1e-9 s and in rounds."""
    _, bound, _ = curved_bound
    sc = TS.outlier()
    plain = TN.run_scene(TN.HarnessTimeOffsetSolver(), sc)
    huber = TN.run_scene(TN.HarnessTimeOffsetSolver(), sc, TimeOffsetOptions(huber_px=HUBER_PX))
    at = huber.status == STATUS_ESTIMATED
    e_plain, e_huber = (np.abs(r.offsets - relative_truth(sc, r.status))[at] for r in (plain, huber))
    print(f"OUTLIER: error / bound with Huber {np.max(e_huber / bound[at]):.3f}, without {np.max(e_plain / bound[at]):.3f}")
    assert (e_huber <= bound[at]).all() and (e_plain > bound[at]).any()
    o = TO.estimate(sc.grid, huber_px=HUBER_PX)
    assert np.nanmax(np.abs(huber.offsets - np.asarray(o.offsets, dtype=np.float64))) < 1e-9 and o.rounds == huber.rounds


def test_synchronous_cameras_get_their_rows_back_bit_for_bit():
    sc = TS.sync()
    res = estimate_time_offsets(sc.image_points, sc.cameras, _solver=TN.HarnessTimeOffsetSolver())
    assert res.converged and res.rounds == 1 and all(v == 0.0 for v in res.offsets.values())
    assert res.result.row_xy.tobytes() == sc.grid.row_xy.tobytes() and res.result.row_used.all()
    back = res.compensated(sc.image_points).df
    src = sc.image_points.df
    for col in ("img_loc_x", "img_loc_y", "frame_time", "sync_index", "cam_id", "object_id", "keypoint_id"):
        assert back[col].to_numpy().tobytes() == src[col].to_numpy().tobytes(), col


def test_compensated_table_and_apply_time_offsets():
    sc = TS.edge()
    res = estimate_time_offsets(sc.image_points, sc.cameras, _solver=TN.HarnessTimeOffsetSolver())
    assert res.status == {0: STATUS_REFERENCE, 2: STATUS_ESTIMATED, 3: STATUS_NONE, 5: STATUS_UNDETERMINED, 7: STATUS_ESTIMATED}
    assert res.offsets[0] == 0.0 and np.isnan(res.offsets[5]) and np.isnan(res.offsets[3]) and res.rows[3] == 0 and res.rows[7] == 256
    src, out = sc.image_points.df, res.compensated(sc.image_points).df
    assert list(out.columns) == list(src.columns) and len(out) == len(src)
    for col in ("sync_index", "cam_id", "object_id", "keypoint_id"):
        assert np.array_equal(out[col], src[col])
    tau = src.groupby("sync_index")["frame_time"].mean()
    assert np.abs(out["frame_time"].to_numpy() - tau.loc[src["sync_index"]].to_numpy()).max() < 1e-14
    unused = ((src["cam_id"] == 3) | (src["sync_index"] == TS.SYNC0 + 50)).to_numpy()
    xy_src, xy_out = src[["img_loc_x", "img_loc_y"]].to_numpy(), out[["img_loc_x", "img_loc_y"]].to_numpy()
    assert xy_out[unused].tobytes() == xy_src[unused].tobytes() and np.abs(xy_out - xy_src)[~unused].max() > 0.5
    # the grid's rows and the table's are the same cells
    g, r = res.grid, res.result
    key = lambda cam, sync: cam * 100000 + sync
    lookup = dict(zip(key(g.cam_ids[g.row_cam], g.row_slot // g.n_traj + g.sync_min).tolist(), range(len(g.row_cam))))
    at = np.array([lookup[k] for k in key(src["cam_id"].to_numpy(), src["sync_index"].to_numpy()).tolist()])
    assert xy_out.tobytes() == r.row_xy[at].tobytes()
    with pytest.raises(ValueError, match="the table has 480 rows, the one the offsets were estimated from 1073"):
        res.compensated(TS.exact().image_points)
    # world: the points at the nominal times, frame_time as reconstruct_trajectories returns it
    w = res.world._df
    assert len(w) == 256 and np.abs(w["frame_time"].to_numpy() - tau.loc[w["sync_index"]].to_numpy()).max() < 1e-14
    shifted = apply_time_offsets(sc.image_points, res).df
    want = src["frame_time"].to_numpy() + np.array([0.0 if np.isnan(res.offsets[int(c)]) else res.offsets[int(c)] for c in src["cam_id"]])
    assert np.array_equal(shifted["frame_time"].to_numpy(), want) and np.array_equal(shifted[["img_loc_x", "img_loc_y"]], src[["img_loc_x", "img_loc_y"]])
    assert np.array_equal(apply_time_offsets(sc.image_points, {2: 0.5}).df["frame_time"], src["frame_time"] + 0.5 * (src["cam_id"] == 2))


def rms_from_truth(sc, world):
    w = world._df
    f, j = w["sync_index"].to_numpy() - TS.SYNC0, (w["object_id"] * 2 + w["keypoint_id"]).to_numpy()
    return float(np.sqrt(np.mean(np.sum((w[["x_coord", "y_coord", "z_coord"]].to_numpy() - sc.truth[f, j]) ** 2, axis=1))))


def check_round_trip(estimate_solver, refine_solver, what):
    """CURVED, compensated and then through the existing refined reconstruction: closer to the true trajectory than the rows as they
    came.  Returns the compensated table."""
    sc = TS.curved()
    res = estimate_time_offsets(sc.image_points, sc.cameras, _solver=estimate_solver)
    comp = res.compensated(sc.image_points)
    refine = RefineOptions(loss="huber", f_scale=2.0)
    before = rms_from_truth(sc, reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, float32_io=False, refine=refine, _solver=refine_solver))
    after = rms_from_truth(sc, reconstruct_trajectories(comp, sc.cameras, xy_gap_fill=0, float32_io=False, refine=refine, _solver=refine_solver))
    own = rms_from_truth(sc, res.world)
    print(f"{what}: RMS distance from the true trajectory {before * 1e3:.3f} mm as recorded, {after * 1e3:.3f} mm compensated, {own * 1e3:.3f} mm the call's own points")
    assert after < 0.5 * before and abs(own - after) < 0.1 * after
    return sc, comp


def test_compensated_rows_reconstruct_closer_to_the_truth():
    """Observed: 1.592 mm as recorded, 0.641 mm compensated (0.3 px of noise is 0.6 mm at these distances)."""
    check_round_trip(TN.HarnessTimeOffsetSolver(), HarnessRefinedSolver(), "g++ builds")


def test_options():
    g = TS.exact().grid
    o = options_struct(TimeOffsetOptions(), g)
    assert (o.reference_cam, o.max_neighbour_gap, o.min_rows, o.max_rounds, o.huber_px, o.max_offset, o.tol) == (-1, 1, 30, 10, 0.0, 0.0, 0.0)
    o = options_struct(TimeOffsetOptions(reference_cam=2, huber_px=1.5, max_offset=0.02, tol=1e-7, max_neighbour_gap=2, min_rows=5, max_rounds=3), g)
    assert (o.reference_cam, o.max_neighbour_gap, o.min_rows, o.max_rounds, o.huber_px, o.max_offset, o.tol) == (2, 2, 5, 3, 1.5, 0.02, 1e-7)
    for field, value, message in (("huber_px", 0.0, "huber_px must be finite and positive, got 0.0"), ("max_offset", float("nan"), "max_offset must be finite and positive"),
                                  ("tol", -1e-6, "tol must be finite and positive, got -1e-06"), ("tol", "x", "tol is not a number"),
                                  ("max_neighbour_gap", 0, "max_neighbour_gap must be an integer of at least 1, got 0"),
                                  ("min_rows", 1.5, "min_rows must be an integer of at least 1, got 1.5"), ("max_rounds", -1, "max_rounds must be an integer of at least 1"),
                                  ("reference_cam", 9, "reference camera 9 has no rows")):
        with pytest.raises(ValueError, match=message):
            options_struct(TimeOffsetOptions(**{field: value}), g)
    empty = estimate_time_offsets(TS.exact().image_points.take(np.zeros(0, dtype=np.int64)), TS.exact().cameras, _solver=TN.HarnessTimeOffsetSolver())
    assert empty.offsets == {} and len(empty.world) == 0 and not empty.converged


def test_other_reference_camera_and_neighbour_gap():
    """The offsets against camera 2 are those against camera 0 shifted, to 5e-5 s: the gauge moves the nominal instants by 6.5 ms, and
    the points of EXACT's first and last frame, which have no V and were exposed at the mean of their stamps, are then off the line by
    V x 6.5 ms, and with them the V of their neighbours (observed: 1.8e-5 s).  A gap of 2 gives frames 49 and 51 of EDGE a velocity."""
    sc = TS.exact()
    a = TN.run_scene(TN.HarnessTimeOffsetSolver(), sc)
    b = TN.run_scene(TN.HarnessTimeOffsetSolver(), sc, TimeOffsetOptions(reference_cam=2))
    assert b.status.tolist() == [2, 2, 1, 2] and np.abs((b.offsets - b.offsets[0]) - a.offsets).max() < 5e-5
    wide = TN.run_scene(TN.HarnessTimeOffsetSolver(), TS.edge(), TimeOffsetOptions(max_neighbour_gap=2))
    assert wide.velocity[49].any() and wide.velocity[51].any() and not wide.velocity[50].any()


def raw_call(sc, options=TimeOffsetOptions(), memory_limit=0, **desc):
    """The harness with fields of the descriptor or of the options struct overwritten after the Python side filled them."""
    lib = TN.harness()
    opts = options_struct(options, sc.grid)

    def call(d, o, r):
        for k, v in desc.items():
            target = o._obj if hasattr(o._obj, k) else d._obj
            setattr(target, k, v)
        return lib.toh_estimate_time_offsets(d, o, r)

    return run_time_offset_call(call, sc.grid, opts, memory_limit, lambda: lib.toh_last_error().decode())


def with_rows(sc, edit):
    df = sc.image_points.df
    edit(df)
    from caliscope_amd.point_data import ImagePoints
    return ImagePoints(df)


def test_refusals_name_the_offender():
    sc = TS.exact()
    solver = TN.HarnessTimeOffsetSolver()
    for field, value, message in (("xy_gap", 2, r"xy_gap must be 0, got 2 \(this call fills no holes\)"), ("xyz_gap", 1, "xyz_gap must be 0, got 1"),
                                  ("huber_px", -1.0, "huber_px must be finite and not negative, got -1.0"), ("max_offset", float("inf"), "max_offset must be finite and not negative"),
                                  ("tol", float("nan"), "tol must be finite and not negative"), ("max_neighbour_gap", 0, "max_neighbour_gap must be at least 1, got 0"),
                                  ("min_rows", 0, "min_rows must be at least 1, got 0"), ("max_rounds", 0, "max_rounds must be at least 1, got 0"),
                                  ("reference_cam", 4, r"reference camera 4 out of range \[0, 4\)")):
        with pytest.raises(ValueError, match="cba_estimate_time_offsets: " + message):
            raw_call(sc, **{field: value})
    b, a = np.array([0.5, 0.5]), np.array([1.0, 0.0])
    with pytest.raises(ValueError, match="cba_estimate_time_offsets: a filter in the descriptor"):
        raw_call(sc, filter_b=b.ctypes.data_as(C.POINTER(C.c_double)), filter_a=a.ctypes.data_as(C.POINTER(C.c_double)),
                 filter_zi=b.ctypes.data_as(C.POINTER(C.c_double)), filter_order=1)
    # what traj_validate refuses, with its own words
    with pytest.raises(ValueError, match="cba_reconstruct_trajectories: negative size"):
        raw_call(sc, n_frames=-1)
    bad = with_rows(sc, lambda df: df.__setitem__("frame_time", df["frame_time"].where(df.index != 7, np.inf)))
    with pytest.raises(ValueError, match=r"cba_estimate_time_offsets: row \d+: row_time is not finite"):
        estimate_time_offsets(bad, sc.cameras, _solver=solver)
    late = with_rows(sc, lambda df: df.__setitem__("frame_time", df["frame_time"] + 0.1 * (df["sync_index"] == TS.SYNC0 + 4)))
    with pytest.raises(ValueError, match=r"cba_estimate_time_offsets: frame 5: its mean time 0\.16\d+ does not lie after that of frame 4, 0\.23\d+"):
        estimate_time_offsets(late, sc.cameras, _solver=solver)
    edge = TS.edge()
    with pytest.raises(ValueError, match="cba_estimate_time_offsets: reference camera 2 is unposed"):
        estimate_time_offsets(edge.image_points, edge.cameras, TimeOffsetOptions(reference_cam=3), _solver=solver)
    with pytest.raises(ValueError, match="estimate_time_offsets: reference camera 4 has no rows"):
        estimate_time_offsets(edge.image_points, edge.cameras, TimeOffsetOptions(reference_cam=4), _solver=solver)
    one = sc.image_points.take(np.flatnonzero((sc.image_points.df["sync_index"] == TS.SYNC0).to_numpy()))
    with pytest.raises(ValueError, match="one frame with rows: no frame interval to derive max_offset and tol from"):
        estimate_time_offsets(one, sc.cameras, _solver=solver)
    too_many = TS.many_cameras(65)
    with pytest.raises(ValueError, match="cba_estimate_time_offsets: 65 posed cameras: at most 64 are supported"):
        estimate_time_offsets(too_many.image_points, too_many.cameras, _solver=solver)
    with pytest.raises(ValueError, match=r"needs \d+ bytes of device memory \(96 per slot for the 4 columns of Q\), 10000 are available"):
        estimate_time_offsets(sc.image_points, sc.cameras, _solver=TN.HarnessTimeOffsetSolver(memory_limit=10000))


def test_cameras_without_a_pose_or_rows_succeed_without_a_launch():
    sc = TS.edge()
    only = sc.image_points.take(np.flatnonzero((sc.image_points.df["cam_id"] == 3).to_numpy()))
    res = estimate_time_offsets(only, sc.cameras, _solver=TN.HarnessTimeOffsetSolver())
    assert res.status == {3: STATUS_NONE} and np.isnan(res.offsets[3]) and res.rounds == 0 and len(res.world) == 0
    back = res.compensated(only).df
    assert back[["img_loc_x", "img_loc_y"]].to_numpy().tobytes() == only.df[["img_loc_x", "img_loc_y"]].to_numpy().tobytes()
