"""caliscope_amd.trajectory_refinement without a GPU: the thread body of k_traj_refine (csrc/trajectory_refine_math.h) in its g++ build
(tests/trajectory_refine_native.py) against scipy (tests/refine_oracle.py) on the recording of tests/refine_scenes.py, the rejection
and depth rules on grids made by hand, the place of the refinement in the call, the refusals and the ABI.  The device kernel calls the
same routine: tests/test_trajectory_refine_gpu.py."""
import ctypes as C
import dataclasses
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from caliscope_amd import _lib
from caliscope_amd.reconstruction import TRAJECTORY_SIGNATURES, reconstruct_trajectories, run_trajectory_call, trajectory_grid
from caliscope_amd.trajectory_refinement import LOSSES, QUALITY_COLUMNS, REFINE_SIGNATURES, RefineOptions, TrajRefine
from oracle import camera_model as cm
from tests import refine_oracle as RO
from tests import refine_scenes as RS
from tests import trajectory_native as N
from tests import trajectory_refine_native as RN

ROOT = Path(__file__).resolve().parent.parent
OPTIONS = dict(f_scale=1.0, reject_px=5.0)  # what the scene's margins are stated for


@functools.cache
def _grid():
    sc = RS.scene()
    return trajectory_grid(sc.image_points, sc.cameras)


@functools.cache
def _base():
    """The unrefined call with its grids: the DLT points every comparison starts from."""
    return RN.HarnessRefinedSolver().reconstruct(_grid(), want_grids=True)


@functools.cache
def _oracle(loss):
    base = _base()
    return RO.refine_grid(_grid(), RS.scene().cameras, base.xy_filled, base.xyz, base.valid, loss=loss, **OPTIONS)


@functools.cache
def _refined(loss="huber", **kw):
    return RN.HarnessRefinedSolver().reconstruct_refined(_grid(), RefineOptions(loss=loss, **{**OPTIONS, **kw}))


def _frames(trajectory):
    """Slot of every frame of a trajectory."""
    return np.arange(RS.N_FRAMES) * RS.N_TRAJ + trajectory


def test_the_scene_is_the_one_described():
    sc, grid, base = RS.scene(), _grid(), _base()
    assert (grid.n_cams, grid.n_traj, grid.n_frames, grid.sync_min) == (7, 3, 100, RS.SYNC0) and grid.n_slots == 300 > 256
    assert grid.cam_posed.tolist() == [1, 1, 1, 1, 1, 1, 0] and grid.cam_model.tolist() == [0, 0, 1, 0, 0, 0, 0]
    views = (~np.isnan(base.xy_filled[:6, :, 0])).sum(axis=0).reshape(100, 3)
    assert (views[:, 0] == 6).all() and set(np.unique(views[:, 1])) == {1, 3, 4} and set(np.unique(views[:, 2])) == {0, 1, 2}
    assert np.array_equal(base.valid.reshape(100, 3), (views >= 2).astype(np.uint8)) and (base.valid == 0).sum() == 6
    out = sc.outlier[:6].sum(axis=0)
    assert (out[::4, 0] == 2).all() and (out[1::4, 0] == 1).all() and (out[2::4, 0] == 0).all() and (out[3::4, 0] == 0).all()
    assert (out[::3, 1] == 1).all() and out[:, 1].sum() == 34 and out[:, 2].sum() == 0
    f = np.arange(0, 100, 4)
    assert sc.outlier[f % 6, f, 0].all() and sc.outlier[(f + 3) % 6, f, 0].all()


def test_the_margins_of_the_scene_hold_on_the_oracle():
    """At every rejection decision of the oracle (huber, f_scale 1, reject_px 5) every inlier is below reject_px / 2, every outlier above
    2 reject_px, and the view dropped is an outlier: no decision of the tests below hangs on the last digits."""
    sc, grid, orc = RS.scene(), _grid(), _oracle("huber")
    inlier, outlier, dropped = 0.0, np.inf, 0
    for s, used, d, drop in orc.decisions:
        is_out = sc.outlier[grid.cam_ids[used], s // 3, s % 3]
        inlier, outlier = max(inlier, d[~is_out].max()), min(outlier, d[is_out].min(initial=np.inf))
        assert drop is None or sc.outlier[grid.cam_ids[drop], s // 3, s % 3], (s, used, d, drop)
        dropped += drop is not None
    print(f"{len(orc.decisions)} decisions, {dropped} views dropped, largest inlier {inlier:.2f} px, smallest outlier {outlier:.2f} px")
    assert inlier < OPTIONS["reject_px"] / 2 and outlier > 2 * OPTIONS["reject_px"]
    assert dropped == sc.outlier[:6].sum()  # every outlier, nothing else


@pytest.mark.parametrize("loss", ["linear", "huber", "soft_l1"])
def test_refinement_agrees_with_scipy(loss):
    (res, q), orc, base = _refined(loss), _oracle(loss), _base()
    at = np.flatnonzero(base.valid == 1)
    assert np.array_equal(res.valid, base.valid) and (orc.status[at] == 1).all() and np.isin(q.status[at], (1, 2)).all()
    RN.compare_with_oracle(loss, res.xyz, q, orc, at)
    off = np.flatnonzero(base.valid == 0)
    assert (q.views[off] == 0).all() and (q.status[off] == 0).all() and (q.iterations[off] == 0).all() and (q.view_state[:, off] == 0).all()
    assert np.isnan(q.rms_px[off]).all() and np.isnan(q.max_px[off]).all() and np.isnan(res.xyz[off]).all()
    assert (q.view_state[6] == 0).all() and (q.iterations[at] >= 1).all()


def test_refined_points_are_nearer_the_truth_than_the_dlt_points():
    (res, _), base, truth = _refined("huber"), _base(), RS.scene().truth.reshape(-1, 3)
    at = np.concatenate([_frames(0), _frames(1)])
    at = at[base.valid[at] == 1]
    rms = [float(np.sqrt(np.mean(np.sum((x[at] - truth[at]) ** 2, axis=1)))) for x in (base.xyz, res.xyz)]
    print(f"RMS distance to the truth over {len(at)} slots: DLT {1e3 * rms[0]:.2f} mm, refined {1e3 * rms[1]:.2f} mm")
    assert rms[1] < rms[0]


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_no_loss_leaves_a_larger_objective_than_the_dlt_point(loss):
    """F(refined) <= F(DLT) in every slot, F written out in Python over the same views (no rejection).  A step is taken only when the
    routine's own F goes down; Python adds the same terms in another order, hence 64 ulp."""
    sc, grid, base = RS.scene(), _grid(), _base()
    res, q = RN.HarnessRefinedSolver().reconstruct_refined(grid, RefineOptions(loss=loss))
    assert not (q.view_state == 2).any()
    before = RO.objective(grid, sc.cameras, base.xy_filled, q.view_state, base.xyz, loss, 2.0)
    after = RO.objective(grid, sc.cameras, base.xy_filled, q.view_state, res.xyz, loss, 2.0)
    at = np.flatnonzero(base.valid == 1)
    print(f"{loss}: sum F {before[at].sum():.4f} -> {after[at].sum():.4f}, statuses {np.bincount(q.status, minlength=4).tolist()}")
    assert np.all(after[at] <= before[at] * (1 + 64 * 2.0**-52)) and after[at].sum() < before[at].sum()


# ---- the rejection rules ------------------------------------------------------------------------------------------------------------

def test_max_reject_1_drops_only_the_worse_of_two_outliers():
    sc, grid, orc = RS.scene(), _grid(), _oracle("huber")
    _, q = _refined("huber", max_reject=1)
    first = {}
    for s, used, d, drop in orc.decisions:
        first.setdefault(s, drop)
    for f in range(0, 100, 4):
        s = 3 * f
        rejected = np.flatnonzero(q.view_state[:, s] == 2)
        assert len(rejected) == 1 and rejected[0] == first[s] and rejected[0] in (f % 6, (f + 3) % 6) and q.views[s] == 5
        assert q.max_px[s] > 2 * OPTIONS["reject_px"]  # the other outlier is still in
    assert ((q.view_state == 2).sum(axis=0) <= 1).all()


def test_min_views_and_reject_px_0_stop_the_rejection():
    _, q = _refined("huber", min_views=6)
    assert not (q.view_state == 2).any() and (q.views[_frames(0)] == 6).all() and (q.max_px[_frames(0)[::4]] > 10).all()
    _, q = _refined("huber", min_views=4)  # trajectory 1 has four views at most: nothing goes there, trajectory 0 as before
    assert not (q.view_state[:, _frames(1)] == 2).any() and np.array_equal(q.view_state[:, _frames(0)], _refined("huber")[1].view_state[:, _frames(0)])
    _, q = _refined("huber", reject_px=0.0)
    assert not (q.view_state == 2).any() and q.max_px[0] > 10


def test_two_views_and_an_outlier_keep_both_views():
    sc = RS.scene()
    pair = RS.restricted(sc, 1, (0, 2))
    grid = trajectory_grid(pair, sc.cameras)
    assert (grid.n_cams, grid.n_traj, grid.n_frames) == (2, 1, 100)
    res, q = RN.HarnessRefinedSolver().reconstruct_refined(grid, RefineOptions(**OPTIONS))
    two = np.arange(100) != 50  # (camera 2 has no row in frame 50)
    assert np.array_equal(res.valid, two.astype(np.uint8)) and (q.views[two] == 2).all() and not (q.view_state == 2).any()
    hit = sc.outlier[0, :, 1] | sc.outlier[2, :, 1]
    assert not hit[50] and hit.sum() == 17 and (q.max_px[hit] > OPTIONS["reject_px"]).all() and (q.max_px[~hit & two] < OPTIONS["reject_px"] / 2).all()
    # trajectory 2 of the scene itself: two views, nothing to reject
    _, q = _refined("huber")
    at = _frames(2)[_base().valid[_frames(2)] == 1]
    assert (q.views[at] == 2).all() and (q.max_px[at] < OPTIONS["reject_px"] / 2).all()


def _mirror_pair(dv_a=0.0, dv_b=0.0):
    """Two cameras at x = -1 and x = +1 looking along z, principal point 0, no distortion, and the point (0, 0, 3): a half turn about
    the z axis swaps the cameras and negates the pixels, sign for sign in floating point.  Camera 0 sees (u, 30 + dv_a), camera 1
    (-u, -30 - dv_b): with dv_a == dv_b the two residuals are equal to the bit wherever on the axis the point is."""
    intr = np.tile([1000.0, 1000.0, 0.0, 0.0, 0, 0, 0, 0, 0], (2, 1))
    P = np.array([np.hstack([np.eye(3), [[1.0], [0.0], [0.0]]]).ravel(), np.hstack([np.eye(3), [[-1.0], [0.0], [0.0]]]).ravel()])
    u = 1000.0 / 3.0
    xy = np.array([[[u, 30.0 + dv_a]], [[-u, -30.0 - dv_b]]])
    return np.zeros(2, dtype=np.int32), intr, P, xy, np.array([[0.0, 0.0, 3.0]])


def test_a_tie_is_broken_by_camera_rank():
    """min_views = 1 reaches the routine only here, where no host check stands in front: with two views one of them can go."""
    r = TrajRefine(loss=0, max_iter=20, f_scale=1.0, reject_px=5.0, max_reject=1, min_views=1)
    _, q = RN.refine_grid(*_mirror_pair(), r)
    assert q.view_state[:, 0].tolist() == [2, 1] and q.views[0] == 1
    _, q = RN.refine_grid(*_mirror_pair(dv_b=1.0), r)  # not a tie: the larger residual goes, whatever its rank
    assert q.view_state[:, 0].tolist() == [1, 2]
    _, q = RN.refine_grid(*_mirror_pair(dv_a=1.0), r)
    assert q.view_state[:, 0].tolist() == [2, 1]
    r.reject_px = 0.0
    xyz, q = RN.refine_grid(*_mirror_pair(), r)
    assert xyz[0, 0] == 0.0 and xyz[0, 1] == 0.0 and q.views[0] == 2 and 29.0 < q.max_px[0] <= 30.0 and q.rms_px[0] == q.max_px[0]


# ---- depth --------------------------------------------------------------------------------------------------------------------------

def _plane_case():
    """Camera 0 at the origin looking along +z sees the pixel (0, 0): every point of the z axis, in front or behind.  Cameras 1 and 2
    at x = +2 and x = -2 look at the axis from the side and both see T = (0, 0, -0.5) exactly: F(T) = 0, and T is behind camera 0."""
    R1, R2 = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])
    C1, C2, T = np.array([2.0, 0, -0.2]), np.array([-2.0, 0, -0.2]), np.array([0.0, 0.0, -0.5])
    cams = [(np.eye(3), np.zeros(3)), (R1, -R1 @ C1), (R2, -R2 @ C2)]
    K, dist = np.array([[1000.0, 0, 0], [0, 1000.0, 0], [0, 0, 1]]), np.zeros(5)
    models = [(cm.project_pinhole, cm.rotation_to_rvec(R), t, K, dist, R, False) for R, t in cams]
    xy = np.array([[[0.0, 0.0]]] + [[m[0](T.reshape(1, 3), m[1], m[2], K, dist)[0][0]] for m in models[1:]])
    intr = np.tile([1000.0, 1000.0, 0.0, 0.0, 0, 0, 0, 0, 0], (3, 1))
    P = np.array([np.hstack([R, t.reshape(3, 1)]).ravel() for R, t in cams])
    return models, np.zeros(3, dtype=np.int32), intr, P, xy, T


def test_a_start_point_behind_a_camera_keeps_the_dlt_bits():
    models, model, intr, P, xy, T = _plane_case()
    start = T + [1e-3, -2e-3, 0.0]
    xyz, q = RN.refine_grid(model, intr, P, xy, start.reshape(1, 3), RefineOptions(loss="linear", reject_px=5.0))
    assert q.status[0] == 3 and N.bits(xyz[0]).tolist() == N.bits(start).tolist()
    assert q.views[0] == 3 and q.iterations[0] == 1 and np.isnan(q.rms_px[0]) and np.isnan(q.max_px[0]) and q.view_state[:, 0].tolist() == [1, 1, 1]


def test_a_trial_step_across_a_camera_plane_is_refused():
    """From (0, 0, 0.05) the Gauss-Newton step aims at T, 0.55 m away and behind camera 0: scipy, which knows no depth rule, goes
    there.  The routine refuses every trial with z <= 0 and ends in front of the camera, with a smaller error than it started with."""
    models, model, intr, P, xy, T = _plane_case()
    start = np.array([[0.0, 0.0, 0.05]])
    with np.errstate(all="ignore"):  # (its path crosses the plane z = 0 of camera 0)
        free, _, _, _, status, _ = RO.refine_slot(models, [0, 1, 2], list(xy[:, 0]), start[0], "linear", 1.0, 0.0, 0, 2)
    assert status == 1 and np.allclose(free, T, atol=1e-9)
    _, q0 = RN.refine_grid(model, intr, P, xy, start, RefineOptions(loss="linear", max_iter=1))
    xyz, q = RN.refine_grid(model, intr, P, xy, start, RefineOptions(loss="linear", max_iter=50))
    print(f"start rms {q0.rms_px[0]:.2f} px, end {xyz[0]} rms {q.rms_px[0]:.2f} px after {q.iterations[0]} evaluations, status {q.status[0]}")
    assert q0.iterations[0] == 1 and q0.status[0] == 2
    assert 0.0 < xyz[0, 2] < 0.05 and q.status[0] in (1, 2) and q.rms_px[0] < q0.rms_px[0] and q.views[0] == 3


# ---- the refinement inside the call ---------------------------------------------------------------------------------------------------

def test_the_fill_and_the_filter_run_on_the_refined_points():
    RN.check_placement(RN.HarnessRefinedSolver(), OPTIONS)


def test_a_dlt_point_behind_a_camera_goes_through_the_call_unchanged():
    RN.check_point_behind_a_camera(RN.HarnessRefinedSolver())


@pytest.mark.parametrize("n_slots", [256, 257])
def test_a_grid_of_one_workgroup_and_of_one_thread_more(n_slots):
    RN.check_slot_count(RN.HarnessRefinedSolver(), n_slots, _refined("huber"), OPTIONS)


def test_without_refine_the_call_is_the_one_it_was():
    sc = RS.scene()
    solver = RN.HarnessRefinedSolver()
    a = reconstruct_trajectories(sc.image_points, sc.cameras, xyz_gap_fill=3, smooth=(30.0, 6.0, 2), _solver=solver)
    b = reconstruct_trajectories(sc.image_points, sc.cameras, xyz_gap_fill=3, smooth=(30.0, 6.0, 2), refine=None, _solver=N.HarnessTrajectorySolver())
    assert list(a.df.columns) == N.WORLD_COLS and a.df.equals(b.df) and N.bits(a.df[N.WORLD_COLS[3:]].to_numpy()).tolist() == N.bits(b.df[N.WORLD_COLS[3:]].to_numpy()).tolist()
    with pytest.raises(ValueError, match="return_quality"):
        reconstruct_trajectories(sc.image_points, sc.cameras, return_quality=True, _solver=solver)
    import caliscope_amd

    assert caliscope_amd.RefineOptions is RefineOptions and RefineOptions() == RefineOptions("huber", 2.0, 20, 0.0, 2, 2)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field,bad", [("f_scale", dict(f_scale=float("nan"))), ("f_scale", dict(f_scale=float("inf"))), ("f_scale", dict(f_scale=0.0)),
                                       ("f_scale", dict(f_scale=-1.0)), ("max_iter", dict(max_iter=0)), ("reject_px", dict(reject_px=-1.0)),
                                       ("reject_px", dict(reject_px=float("inf"))), ("reject_px", dict(reject_px=float("nan"))),
                                       ("min_views", dict(min_views=1)), ("max_reject", dict(max_reject=-1)), ("loss", dict(loss="tukey"))])
def test_refused_options_name_the_field(field, bad):
    sc = RS.scene()
    solver = RN.HarnessRefinedSolver()
    with pytest.raises(ValueError, match=field):
        reconstruct_trajectories(sc.image_points, sc.cameras, refine=RefineOptions(**bad), _solver=solver)
    assert solver.calls == (0 if field == "loss" else 1)


def test_the_library_s_own_refusals():
    grid, lib = _grid(), RN.harness()
    err = lambda: lib.trh_last_error().decode()
    q, cq = RN.empty_quality(grid.n_cams, grid.n_slots)

    def call(refine, limit=0):
        ref = C.byref(refine) if refine is not None else None
        return run_trajectory_call(lambda d, o: lib.trh_reconstruct_trajectories_refined(d, ref, o, C.byref(cq)), grid, 0, 0, None, True, limit, False,
                                   "cba_reconstruct_trajectories_refined", err)

    good = TrajRefine(loss=1, max_iter=20, f_scale=2.0, reject_px=0.0, max_reject=2, min_views=2)
    with pytest.raises(ValueError, match="refine: null"):
        call(None)
    for loss in (-1, 5):
        with pytest.raises(ValueError, match=f"unknown loss {loss}"):
            call(TrajRefine(loss=loss, max_iter=20, f_scale=2.0, reject_px=0.0, max_reject=2, min_views=2))
    call(TrajRefine(loss=0, max_iter=1, f_scale=0.0, reject_px=0.0, max_reject=0, min_views=2))  # f_scale is not read for the linear loss
    # the memory check counts the refinement's buffers: n_cams n_slots + 25 n_slots bytes on top of the plain call's
    plain = grid.n_cams * grid.n_slots * 24 + grid.n_slots * 33 + grid.n_frames * 8 + len(grid.row_cam) * 36 + grid.n_cams * 200
    more = plain + grid.n_cams * grid.n_slots + 25 * grid.n_slots
    call(good, more)
    with pytest.raises(ValueError, match=f"needs {more} bytes of device memory, {more - 1} are available"):
        call(good, more - 1)
    N.HarnessTrajectorySolver(memory_limit=plain).reconstruct(grid)
    with pytest.raises(ValueError, match=f"needs {more} bytes"):
        RN.HarnessRefinedSolver(memory_limit=plain).reconstruct_refined(grid, RefineOptions())
    # no rows: nothing to do, and it is said in every output
    empty = dataclasses.replace(grid, row_cam=grid.row_cam[:0], row_slot=grid.row_slot[:0], row_xy=grid.row_xy[:0], row_time=grid.row_time[:0])
    res, q = RN.HarnessRefinedSolver().reconstruct_refined(empty, RefineOptions())
    assert not res.valid.any() and not q.views.any() and not q.status.any() and not q.view_state.any() and np.isnan(q.rms_px).all()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------

def test_the_header_the_table_and_the_build_agree():
    from caliscope_amd import build

    header = (ROOT / "include" / "caliscope" / "trajectory_refine.h").read_text()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    assert set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", text)) == set(REFINE_SIGNATURES) == {"cba_reconstruct_trajectories_refined"}
    assert list(TRAJECTORY_SIGNATURES) == ["cba_reconstruct_trajectories"] and "cba_reconstruct_trajectories_refined" not in _lib.SIGNATURES
    assert "cba_reconstruct_trajectories_refined" not in (ROOT / "include" / "caliscope_trajectory.h").read_text()
    assert ROOT / "include" / "caliscope" / "trajectory_refine.h" in build.DEPENDS and build.CSRC / "trajectory_refine_math.h" in build.DEPENDS
    # the structures are the header's: field for field, and the sizes a C compiler gives them
    fields = lambda name: re.findall(r"(\w+);", re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1))
    from caliscope_amd.trajectory_refinement import TrajQuality

    assert fields("cba_traj_refine") == [f[0] for f in TrajRefine._fields_] and C.sizeof(TrajRefine) == 32
    assert fields("cba_traj_quality") == [f[0] for f in TrajQuality._fields_] and C.sizeof(TrajQuality) == 48
    build.build(verbose=False)
    lib = _lib.bind(_lib.load(), REFINE_SIGNATURES)
    fn = lib.cba_reconstruct_trajectories_refined
    assert fn.restype == REFINE_SIGNATURES["cba_reconstruct_trajectories_refined"][0] and fn.argtypes == REFINE_SIGNATURES["cba_reconstruct_trajectories_refined"][1]
