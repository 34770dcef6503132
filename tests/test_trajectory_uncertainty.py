"""cba_reconstruct_trajectories_uncertain on the g++ build of its thread bodies and checks (tests/trajectory_cov_native.py): the
per-sample covariance against the numpy oracle of tests/trajectory_cov_oracle.py, what its two terms mean (the scatter of noisy
reconstructions; the response of the reconstruction to a change of the calibration), the refusals, and the C ABI.  The device runs
the same routines in tests/test_trajectory_uncertainty_gpu.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from caliscope_amd import _lib
from caliscope_amd.cameras import CameraArray, CameraData
from caliscope_amd.point_data import ImagePoints
from caliscope_amd.reconstruction import TRAJECTORY_SIGNATURES, reconstruct_trajectories, reconstruct_xyz, trajectory_grid, world_points_of
from caliscope_amd.trajectory_refinement import REFINE_SIGNATURES, RefineOptions
from caliscope_amd.trajectory_uncertainty import (COVARIANCE_COLUMNS, TRAJ_UNCERTAINTY_SIGNATURES, CovarianceOptions, TrajCovOut, TrajUncertainty,
                                                  covariance_frame, full_matrices, uncertainty_tables)
from oracle import camera_model as cm
from tests import refine_scenes as RS
from tests import trajectory_cov_native as CN

ROOT = Path(__file__).resolve().parent.parent
THREE = (0, 1, 3)  # the cameras of the two "meaning" tests: 9-, 9- and 6-wide in CN.WIDTHS


def _options(full: bool, widths=None) -> CovarianceOptions:
    return CovarianceOptions(CN.SIGMA_PX, CN.report(widths or CN.WIDTHS) if full else None)


# ---- 1. the formula ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [CN.REFINED, None], ids=["refined", "plain"])
@pytest.mark.parametrize("full", [True, False], ids=["full", "noise-only"])
def test_covariance_matches_the_oracle(refine, full):
    """Largest ||cov - oracle||_F / (1e-12 cond_2(V) ||cov||_F) observed on the g++ build: refined full 4.6e-4 (cov_calib 3.6e-4),
    plain full 4.4e-4 (3.8e-4), refined noise-only 3.7e-4, plain noise-only 3.1e-4; cond_2(V) up to 78 (the two-view trajectory)."""
    sc = RS.scene()
    grid = trajectory_grid(sc.image_points, sc.cameras)
    result, quality, cov, tables = CN.check_scene_against_oracle(CN.HarnessUncertainSolver(), grid, sc.cameras, _options(full), refine,
                                                                 f"{'refined' if refine else 'plain'} {'full' if full else 'noise-only'}")
    assert grid.n_slots == 300 and (cov.cov_status == 0).sum() == 6 and (cov.cov_status == 1).sum() == 294
    assert tables.cam_nparams.tolist() == ([9, 9, 6, 6, 9, 6, 0] if full else [6] * 6 + [0])
    assert tables.cam_offset.tolist() == ([0, 9, 18, 24, 30, 39, -1] if full else [-1] * 7)
    alone = CN.cov_grid(grid, tables, result, quality)  # (the thread body on the call's own points: what the GPU tests hold the device to)
    assert alone.cov.tobytes() == cov.cov.tobytes() and alone.cov_status.tobytes() == cov.cov_status.tobytes()
    if not full:  # sigma_px^2 V^-1 and nothing else: it scales with sigma_px^2 exactly
        twice = CN.HarnessUncertainSolver().reconstruct_uncertain(grid, CovarianceOptions(2 * CN.SIGMA_PX), RefineOptions(**refine) if refine else None,
                                                                  camera_array=sc.cameras)[2]
        assert np.array_equal(twice.cov, 4.0 * cov.cov, equal_nan=True)
    else:  # the calibration term is there, and it is PSD like cam_cov
        extra = full_matrices(cov.cov_calib[cov.cov_status == 1])
        assert np.linalg.eigvalsh(extra).min() > -1e-12 * np.abs(extra).max() and np.trace(extra, axis1=1, axis2=2).min() > 0


def test_a_rig_of_129_cameras_of_which_each_landmark_sees_a_fifth():
    """The recording of the GPU test at the size where k_traj_cov reads its camera tables from global memory: 6- and 9-wide blocks
    alternating along 903 rows of cam_cov, 26 views and 351 camera pairs per slot, four cameras in five skipped."""
    image_points, cameras, rep = CN.wide_rig(129)
    grid = trajectory_grid(image_points, cameras)
    _, quality, cov, tables = CN.check_scene_against_oracle(CN.HarnessUncertainSolver(), grid, cameras, CovarianceOptions(CN.SIGMA_PX, rep), CN.REFINED,
                                                            "129 cameras")
    assert grid.n_cams == 129 and tables.cam_cov.shape == (903, 903) and (cov.cov_status == 1).all()
    assert sorted(set((quality.view_state == 1).sum(axis=0).tolist())) == [25, 26]


def test_filled_cells_and_points_behind_a_camera_have_no_covariance():
    sc = RS.scene()
    grid = trajectory_grid(sc.image_points, sc.cameras)
    solver = CN.HarnessUncertainSolver()
    for refine in (CN.REFINED, None):
        result, _, cov, _ = CN.check_scene_against_oracle(solver, grid, sc.cameras, _options(True), refine, "with xyz_gap = 3", xyz_gap=3)
        filled = result.valid == 2
        assert filled.sum() == 6 and (cov.cov_status[filled] == 2).all() and np.isnan(cov.cov[filled]).all() and np.isnan(cov.cov_calib[filled]).all()
        frame = covariance_frame(grid, result, cov)
        world = world_points_of(grid, result).df
        assert list(frame.columns) == list(COVARIANCE_COLUMNS) and len(frame) == len(world) == 300
        assert np.array_equal(frame[["sync_index", "object_id", "keypoint_id"]].to_numpy(), world[["sync_index", "object_id", "keypoint_id"]].to_numpy())
        assert (frame["cov_status"] == 2).sum() == 6 and frame.loc[frame["cov_status"] == 2, "std_major"].isna().all()
    ip, cams, _ = RS.behind_camera_case()
    grid = trajectory_grid(ip, cams)
    options = CovarianceOptions(CN.SIGMA_PX, CN.report({0: 9, 1: 9, 3: 6}))
    for refine in (RefineOptions(reject_px=5.0), None):  # (refined: status 3, the DLT point is kept)
        result, quality, cov = solver.reconstruct_uncertain(grid, options, refine, camera_array=cams)
        assert result.valid.tolist() == [1] and cov.cov_status.tolist() == [2] and np.isnan(cov.cov).all() and np.isnan(cov.cov_calib).all()
        assert quality is None or quality.status.tolist() == [3]


def test_the_frame_and_the_public_call():
    sc = RS.scene()
    solver = CN.HarnessUncertainSolver()
    options = _options(True)
    world, quality, frame = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, refine=RefineOptions(**CN.REFINED), return_quality=True,
                                                     covariance=options, _solver=solver)
    base, base_q = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, refine=RefineOptions(**CN.REFINED), return_quality=True,
                                            _solver=solver)
    assert world.df.equals(base.df) and quality.equals(base_q)  # the covariance changes nothing else
    keys = ["sync_index", "object_id", "keypoint_id"]
    assert list(frame.columns) == list(COVARIANCE_COLUMNS) and np.array_equal(frame[keys].to_numpy(), world.df[keys].to_numpy())
    assert (frame["cov_status"] == 1).all() and ((frame["calib_share"] > 0) & (frame["calib_share"] < 1)).all()
    S = full_matrices(frame[list(COVARIANCE_COLUMNS[3:9])].to_numpy())
    assert np.allclose(frame["std_major"] ** 2, np.linalg.eigvalsh(S)[:, -1], rtol=1e-12)
    assert np.allclose(frame[["std_x", "std_y", "std_z"]].to_numpy() ** 2, np.einsum("njj->nj", S), rtol=1e-12)
    assert (frame["std_major"] >= frame[["std_x", "std_y", "std_z"]].max(axis=1) * (1 - 1e-12)).all()
    # two views determine less than six: the two-camera trajectory is the least certain, the six-camera one the most
    per_traj = frame.groupby(["object_id", "keypoint_id"])["std_major"].median()
    assert per_traj.idxmax() == RS.TRAJ[2] and per_traj.idxmin() == RS.TRAJ[0]
    plain, plain_frame = reconstruct_trajectories(sc.image_points, sc.cameras, xy_gap_fill=0, covariance=CovarianceOptions(CN.SIGMA_PX), _solver=solver)
    assert len(plain_frame) == len(plain) and plain_frame["calib_share"].isna().all() and (plain_frame["cov_status"] == 1).all()
    empty = reconstruct_trajectories(ImagePoints(sc.image_points.df.iloc[:0]), sc.cameras, covariance=options, _solver=solver)
    assert len(empty[0]) == 0 and list(empty[1].columns) == list(COVARIANCE_COLUMNS) and len(empty[1]) == 0


def test_reconstruct_xyz_writes_the_covariance_beside_the_table(tmp_path):
    sc = RS.scene()
    path = reconstruct_xyz(RS.restricted(sc, 2, (0, 4)), sc.cameras, "take", tmp_path, xy_gap_fill=0, covariance=_options(True),
                           _solver=CN.HarnessUncertainSolver())
    table, frame = pd.read_csv(path), pd.read_csv(tmp_path / "xyz_take_covariance.csv")
    assert path == tmp_path / "xyz_take.csv" and list(frame.columns) == list(COVARIANCE_COLUMNS) and len(frame) == len(table) == 95
    assert np.array_equal(frame["sync_index"], table["sync_index"]) and (frame["cov_status"] == 1).all()


# ---- 2. and 3. what the two terms mean ---------------------------------------------------------------------------------------------------------
POINT = np.array([0.15, -0.05, 0.55])


def _three_cameras(params=None):
    """CameraArray of cam_ids 0, 1, 3 of the rig at BA parameters `params` {cam_id: [rvec, tvec, s, k1, k2]} (None: the rig's own)."""
    cams = {}
    for cid, cam, _ in RS.rig():
        if cid not in THREE:
            continue
        if params is not None:
            p = params[cid]
            K = cam.matrix.copy()
            K[0, 0], K[1, 1] = p[6] * K[0, 0], p[6] * K[1, 1]
            dist = cam.distortions.copy()
            dist[0], dist[1] = p[7], p[8]
            cam = CameraData(cam_id=cid, size=cam.size, matrix=K, distortions=dist, fisheye=False, rotation=cm.rodrigues(p[0:3]), translation=p[3:6].copy())
        cams[cid] = cam
    return CameraArray(cams)


def _pixels_of(point, n_frames, noise, seed=0):
    rng = np.random.default_rng(seed)
    rows = []
    for cid, _, project in RS.rig():
        if cid in THREE:
            uv = project(point.reshape(1, 3))[0][0] + rng.normal(0.0, noise, (n_frames, 2)) * (noise > 0)
            rows.append(pd.DataFrame({"sync_index": np.arange(n_frames), "cam_id": cid, "object_id": 0, "keypoint_id": 0, "img_loc_x": uv[:, 0],
                                      "img_loc_y": uv[:, 1], "frame_time": np.arange(n_frames) / 30.0}))
    return ImagePoints(pd.concat(rows, ignore_index=True))


def test_noise_term_is_the_scatter_of_the_reconstruction():
    """4000 frames of one point under independent 0.3 px noise, refined under the linear loss: the mean of d^T cov^-1 d, d the error of a
    frame and cov its own returned covariance, is that of chi^2 with 3 degrees of freedom, 3 +- 5 sqrt(6 / 4000)."""
    n = 4000
    cams = _three_cameras()
    grid = trajectory_grid(_pixels_of(POINT, n, 0.3), cams)
    result, quality, cov = CN.HarnessUncertainSolver().reconstruct_uncertain(grid, CovarianceOptions(0.3), RefineOptions(loss="linear"), camera_array=cams)
    assert (cov.cov_status == 1).all() and (quality.status == 1).all() and cov.cov_calib is None
    d = result.xyz - POINT
    m2 = np.einsum("ni,nij,nj->n", d, np.linalg.inv(full_matrices(cov.cov)), d)
    print(f"mean d^T cov^-1 d over {n} frames = {m2.mean():.4f} (3 +- {5 * np.sqrt(6 / n):.4f}); rms error {np.sqrt((d ** 2).sum(axis=1).mean()) * 1e3:.3f} mm, "
          f"mean sqrt(tr cov) {np.sqrt(cov.cov[:, [0, 3, 5]].sum(axis=1)).mean() * 1e3:.3f} mm")
    assert abs(m2.mean() - 3.0) <= 5.0 * np.sqrt(6.0 / n)


def test_calibration_term_is_the_response_to_the_camera_parameters():
    """Noise-free pixels of three cameras (zero residual: Gauss-Newton is exact): F = d X / d theta by central differences (h = 1e-4) of
    the refined reconstruction itself, one BA parameter at a time with the CameraArray rebuilt; F cam_cov F^T is cov_calib to
    1e-4 ||cov_calib||_F."""
    from caliscope_amd.bundle_parameterization import BundleParameterization

    widths = {cid: CN.WIDTHS[cid] for cid in THREE}
    cams = _three_cameras()
    par = BundleParameterization.from_camera_array(cams, 0, refine_intrinsics=True)
    x = par.pack(cams, np.zeros((0, 3)))
    base = {blk.cam_id: x[off:off + 9].copy() for blk, off in zip(par.blocks, par.camera_param_offsets)}
    image_points = _pixels_of(POINT, 1, 0.0)
    solver = CN.HarnessUncertainSolver()
    refine = RefineOptions(loss="linear", max_iter=50)

    def reconstruct(params):
        array = _three_cameras(params)
        return solver.reconstruct_uncertain(trajectory_grid(image_points, array), CovarianceOptions(1.0), refine, camera_array=array)[0].xyz[0]

    assert np.allclose(reconstruct(base), POINT, atol=1e-8)  # (the rebuilt array is the rig)
    h, columns = 1e-4, []
    for cid in THREE:
        for k in range(widths[cid]):
            plus, minus = {c: p.copy() for c, p in base.items()}, {c: p.copy() for c, p in base.items()}
            plus[cid][k] += h
            minus[cid][k] -= h
            columns.append((reconstruct(plus) - reconstruct(minus)) / (2 * h))
    F = np.column_stack(columns)
    rep = CN.report(widths)
    grid = trajectory_grid(image_points, cams)
    _, quality, cov = solver.reconstruct_uncertain(grid, CovarianceOptions(1.0, rep), refine, camera_array=cams)
    assert cov.cov_status.tolist() == [1] and quality.rms_px[0] < 1e-6
    got, want = full_matrices(cov.cov_calib)[0], F @ rep.cam_cov_full @ F.T
    err = np.linalg.norm(got - want) / np.linalg.norm(got)
    print(f"||F cam_cov F^T - cov_calib||_F / ||cov_calib||_F = {err:.3e} (bar 1e-4), ||cov_calib||_F = {np.linalg.norm(got):.3e}")
    assert F.shape == (3, 24) and err <= 1e-4


# ---- 4. refusals and the C ABI -------------------------------------------------------------------------------------------------------------------
def _scene_tables(**change):
    sc = RS.scene()
    grid = trajectory_grid(sc.image_points, sc.cameras)
    tables = uncertainty_tables(grid, sc.cameras, _options(True))
    fields = {name: np.array(getattr(tables, name)) for name in ("cam_nparams", "cam_const", "cam_x", "cam_offset", "cam_cov")}
    fields["sigma_px"] = tables.sigma_px
    for name, value in change.items():
        if callable(value):
            value(fields[name])
        else:
            fields[name] = value
    return grid, type(tables)(**fields)


def _set(index, value):
    def apply(a):
        a[index] = value
    return apply


@pytest.mark.parametrize("change,words", [
    (dict(sigma_px=0.0), "sigma_px"), (dict(sigma_px=-1.0), "sigma_px"), (dict(sigma_px=float("nan")), "sigma_px"), (dict(sigma_px=float("inf")), "sigma_px"),
    (dict(cam_nparams=_set(3, 7)), "camera 3: cam_nparams must be 6 or 9, got 7"),
    (dict(cam_nparams=_set(2, 9)), "camera 2: cam_nparams: a fisheye camera"),
    (dict(cam_offset=_set(1, 5)), "camera 1: cam_offset 5 overlaps the rows of camera 0"),
    (dict(cam_offset=_set(5, 40)), "camera 5: cam_offset 40"),
    (dict(cam_offset=_set(0, -2)), "camera 0: cam_offset -2"),
    (dict(cam_cov=_set((3, 20), 1.0)), "cam_cov is not symmetric at [20][3]"),
    (dict(cam_cov=_set((7, 7), float("inf"))), "cam_cov[7][7] is not finite"),
    (dict(cam_cov=_set((2, 30), float("nan"))), "cam_cov[2][30] is not finite"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_host_checks_name_the_field(change, words):
    grid, tables = _scene_tables(**change)
    for refine in (RefineOptions(), None):
        with pytest.raises(ValueError, match=re.escape(words)):
            CN.HarnessUncertainSolver().reconstruct_uncertain(grid, tables, refine)
    # an unposed camera's row is not read, and a camera without a covariance is no overlap
    grid, tables = _scene_tables(cam_nparams=_set(6, 7), cam_offset=_set(1, -1))
    assert (CN.HarnessUncertainSolver().reconstruct_uncertain(grid, tables)[2].cov_status == 1).sum() == 294


def test_memory_limit_counts_the_buffers_of_the_covariance():
    grid, tables = _scene_tables()
    slots, cams, rows, ncp = grid.n_slots, grid.n_cams, len(grid.row_cam), tables.cam_cov.shape[0]
    plain = cams * slots * 24 + slots * 33 + grid.n_frames * 8 + rows * 36 + cams * 200  # caliscope_trajectory.h
    refined = cams * slots + slots * 25                                                    # trajectory_refine.h
    extra = slots * 49 + cams * 396 + 8 * ncp * ncp + slots * 48                           # trajectory_uncertainty.h
    for refine, total in ((RefineOptions(), plain + refined + extra), (None, plain + extra)):
        assert (CN.HarnessUncertainSolver(total).reconstruct_uncertain(grid, tables, refine)[2].cov_status == 1).any()
        with pytest.raises(ValueError, match=f"needs {total} bytes of device memory, {total - 1} are available"):
            CN.HarnessUncertainSolver(total - 1).reconstruct_uncertain(grid, tables, refine)
    noise_only = type(tables)(**{**tables.__dict__, "cam_cov": None})
    total = plain + slots * 49 + cams * 396
    CN.HarnessUncertainSolver(total).reconstruct_uncertain(grid, noise_only)
    with pytest.raises(ValueError, match=f"needs {total} bytes"):
        CN.HarnessUncertainSolver(total - 1).reconstruct_uncertain(grid, noise_only)


def test_the_report_must_fit_the_camera_array():
    sc = RS.scene()
    call = lambda rep: reconstruct_trajectories(sc.image_points, sc.cameras, covariance=CovarianceOptions(1.0, rep), _solver=CN.HarnessUncertainSolver())
    with pytest.raises(ValueError, match="has no camera 4"):
        call(CN.report({c: w for c, w in CN.WIDTHS.items() if c != 4}))
    with pytest.raises(ValueError, match="camera 2 9 parameters: a fisheye camera has no free intrinsics"):
        call(CN.report({**CN.WIDTHS, 2: 9}))
    with pytest.raises(ValueError, match="camera 3 7 parameters"):
        call(CN.report({**CN.WIDTHS, 3: 7}))
    rep = CN.report(CN.WIDTHS)
    rep.cam_cov_full = rep.cam_cov_full[:42, :42]
    with pytest.raises(ValueError, match="block of camera 5 .6 wide, from row 39. does not fit cam_cov_full of 42 rows"):
        call(rep)
    rep = CN.report({**CN.WIDTHS, 7: 6})  # a camera more in the report than in the recording: fine, its rows are skipped
    rep.cameras.pop(7)
    with pytest.raises(ValueError, match="add up to 45 after camera 5, cam_cov_full has 51 rows"):
        call(rep)
    more = call(CN.report({**CN.WIDTHS, 7: 6}))
    assert (more[1]["cov_status"] == 1).all()
    with pytest.raises(ValueError, match="sigma_px"):
        reconstruct_trajectories(sc.image_points, sc.cameras, covariance=CovarianceOptions(0.0), _solver=CN.HarnessUncertainSolver())


def test_the_header_the_table_and_the_build_agree():
    from caliscope_amd import build

    header = (ROOT / "include" / "caliscope" / "trajectory_uncertainty.h").read_text()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    name = "cba_reconstruct_trajectories_uncertain"
    assert set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", text)) == set(TRAJ_UNCERTAINTY_SIGNATURES) == {name}
    assert name not in TRAJECTORY_SIGNATURES and name not in REFINE_SIGNATURES and name not in _lib.SIGNATURES
    for other in ("caliscope_trajectory.h", "caliscope/trajectory_refine.h"):
        assert name not in (ROOT / "include" / other).read_text()
    assert ROOT / "include" / "caliscope" / "trajectory_uncertainty.h" in build.DEPENDS and build.CSRC / "trajectory_cov_math.h" in build.DEPENDS
    fields = lambda struct: re.findall(r"(\w+);", re.search(r"typedef struct \{([^}]*)\} " + struct + ";", text).group(1))
    assert fields("cba_traj_uncertainty") == [f[0] for f in TrajUncertainty._fields_] and C.sizeof(TrajUncertainty) == 56
    assert fields("cba_traj_cov_out") == [f[0] for f in TrajCovOut._fields_] and C.sizeof(TrajCovOut) == 24
    build.build(verbose=False)
    lib = _lib.bind(_lib.load(), TRAJ_UNCERTAINTY_SIGNATURES)
    fn = getattr(lib, name)
    assert fn.restype == TRAJ_UNCERTAINTY_SIGNATURES[name][0] and fn.argtypes == TRAJ_UNCERTAINTY_SIGNATURES[name][1]
    # the kernel is in the code object under its name, in both forms
    blob = build.OUT.read_bytes()
    assert blob.count(b"k_traj_covILb1") and blob.count(b"k_traj_covILb0") and blob.count(b"k_traj_cov_filled")
