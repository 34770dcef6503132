"""Frame selection on the MI355X: cba_pose_select_frames against the g++ build of the same header and against the reference's own
selector (fixtures of tests/golden/frame_selection), run-to-run identity, degenerate frames, and
calibrate_camera_array_intrinsics(frames="select") on a ring session.  Each device call runs once."""
import numpy as np
import pytest

from caliscope_amd import frame_selector as FS
from caliscope_amd.calibrate_intrinsics import calibrate_camera_array_intrinsics
from caliscope_amd.cameras import CameraArray, CameraData
from caliscope_amd.frame_selector import DeviceFrameSelection
from tests import frame_select_fixtures as F
from tests import intrinsic_scenes as S
from tests.frame_select_native import HarnessFrameSelection

pytestmark = pytest.mark.gpu

# Orientation features and the transfer RMSE of the device against the g++ build: BASE_ATOL * max(1, |value|), the bound
# cba_pose_pnp_batch holds against its CPU build (tests/test_pose_bootstrap_gpu.py).  Both builds run the same source without
# contraction, so the fit takes the same path to the last bit (+, -, *, / and sqrt only); they differ through atan2 alone, about an
# ulp of an angle below 2 pi (~1e-15).  DEVICE_FACTOR is the place for a factor MEASURED on a GPU run, with the observed value
# beside it.  Observed on an MI355X: 0.00022 of the base bound at worst over all cases: no widening needed.
BASE_ATOL = 1e-12
DEVICE_FACTOR = 1.0
DEV, CPU = DeviceFrameSelection(), HarnessFrameSelection()


def _same(dev, cpu, label):
    """Everything discrete and the pose features bit-equal; orientation and RMSE within the bound.  Returns the worst ratio."""
    for name in ("homography_status", "cell_mask", "selected", "n_selected", "n_anchors", "bin_mask", "eligible", "pose_features"):
        assert np.array_equal(getattr(dev, name), getattr(cpu, name)), (label, name)
    worst = 0.0
    for name in ("orientation", "homography_rmse"):
        d, c = getattr(dev, name), getattr(cpu, name)
        assert np.isfinite(d).all(), (label, name)
        if c.size:
            worst = max(worst, float((np.abs(d - c) / (BASE_ATOL * np.maximum(1.0, np.abs(c)))).max()))
    assert worst <= DEVICE_FACTOR, (label, worst)
    return worst


@pytest.fixture(scope="module")
def rig_runs():
    """The default-argument cases as one rig of eight cameras with 70, 300, 70, 24, 40, 0, 9 and 1 frames, once per float32_io value
    on each build."""
    ip, cams, fxs = F.default_rig()
    runs = {}
    for f32 in (True, False):
        runs[f32] = (FS.select_rig(ip, cams, by_object=False, float32_io=f32, _solver=DEV), FS.select_rig(ip, cams, by_object=False, float32_io=f32, _solver=CPU))
    return cams, fxs, runs


def test_rig_call_matches_the_cpu_build_and_the_reference(rig_runs, capsys):
    cams, fxs, runs = rig_runs
    bound = F.orientation_bound()
    for f32 in (True, False):
        (rep_d, gathered, dev), (rep_c, _, cpu) = runs[f32]
        ratio = _same(dev, cpu, f"rig float32_io={f32}")
        assert rep_d == rep_c
        assert np.diff(gathered.cam_frame_start).tolist() == [70, 300, 70, 24, 40, 0, 9, 1]
        worst = np.zeros(3)
        if f32:  # the reference's arithmetic
            for k, ((c, _), fx) in enumerate(zip(cams, fxs)):
                if fx is None:
                    continue
                a, b = gathered.cam_frame_start[k], gathered.cam_frame_start[k + 1]
                worst = np.maximum(worst, F.compare(fx, rep_d[c], gathered.frame_sync[a:b], dev.cell_mask[a:b], dev.pose_features[a:b],
                                                    dev.orientation[a:b], bound, label=f"rig camera {c}"))
        with capsys.disabled():
            print(f"device vs g++ build [rig, float32_io={f32}]: largest difference {ratio:.3g} x 1e-12 max(1, |value|)"
                  + (f"; device vs reference orientation {worst}, bound {bound}" if f32 else ""))


@pytest.mark.parametrize("case", [1, 2, 3, 5, 9, 10])
def test_other_arguments_match_the_cpu_build_and_the_reference(case, capsys):
    """target_frame_count 1, 3 and 200, min_corners_per_frame 3, grid_size 1 and 8 with corners outside the image."""
    fx = F.load(case)
    rep_d, gathered, dev = F.run_case(fx, DEV)
    rep_c, _, cpu = F.run_case(fx, CPU)
    ratio = _same(dev, cpu, f"sel_{case:02d}")
    assert rep_d == rep_c
    worst = F.compare(fx, rep_d, gathered.frame_sync, dev.cell_mask, dev.pose_features, dev.orientation, F.orientation_bound(), label=f"sel_{case:02d}")
    with capsys.disabled():
        print(f"device vs g++ build [sel_{case:02d}]: largest difference {ratio:.3g} x 1e-12 max(1, |value|); device vs reference orientation {worst}")


def test_two_calls_return_identical_bytes(rig_runs):
    ip, cams, _ = F.default_rig()
    (_, _, first), _ = rig_runs[2][True]
    _, _, again = FS.select_rig(ip, cams, by_object=False, float32_io=True, _solver=DEV)
    for name in ("cell_mask", "pose_features", "orientation", "homography_status", "homography_rmse", "selected", "n_selected", "n_anchors",
                 "bin_mask", "eligible"):
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name


def test_degenerate_frames_and_empty_calls():
    """A collinear frame, a frame with all corners at one pixel, a 3-corner frame and an empty frame next to good ones, in two
    cameras: statuses equal to the g++ build's, every output finite; a homography subrange; calls without frames or cameras."""
    fx = F.load(7)
    df = F.dataframe(fx)
    good = [g[["img_loc_x", "img_loc_y", "obj_loc_x", "obj_loc_y"]].to_numpy() for _, g in df.groupby("sync_index")][:6]
    line = np.column_stack([np.linspace(100, 900, 8), np.linspace(80, 600, 8), np.linspace(0, 0.2, 8), np.linspace(0, 0.1, 8)])
    spot = good[0].copy()
    spot[:, :2] = [640.25, 360.5]
    frames = [good[0], line, good[1], spot, good[2][:3], np.zeros((0, 4)), good[3], good[4], good[5]]
    rows = np.concatenate(frames)
    frame_start = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    args = ([0, 5, 9], [[1280.0, 720.0], [640.0, 480.0]], frame_start, rows[:, :2], rows[:, 2:])
    for kw in (dict(min_corners=0, target_count=7), dict(min_corners=6, target_count=2, float32_io=False),
               dict(min_corners=3, target_count=4, homog_start=frame_start[:-1] + np.array([1, 0, 2, 0, 0, 0, 0, 3, 0]),
                    homog_count=np.array([len(f) for f in frames]) - np.array([2, 0, 2, 0, 0, 0, 1, 3, 0]))):
        dev, cpu = DEV.select_frames(*args, **kw), CPU.select_frames(*args, **kw)
        _same(dev, cpu, str(kw))
        assert dev.homography_status[[1, 3, 4, 5]].tolist() == [FS.HOMOG_FAILED, FS.HOMOG_FAILED, FS.HOMOG_TOO_FEW, FS.HOMOG_TOO_FEW]
        assert not dev.orientation[[1, 3, 4, 5]].any() and not dev.homography_rmse[[1, 3, 4, 5]].any() and np.isfinite(dev.pose_features).all()
    none = DEV.select_frames([0, 0, 0], [[1280.0, 720.0], [640.0, 480.0]], [0], np.zeros((0, 2)), np.zeros((0, 2)), target_count=3)
    assert (none.selected == -1).all() and none.selected.shape == (2, 3) and not none.n_selected.any() and not none.eligible.any()
    assert DEV.select_frames([0], np.zeros((0, 2)), [0], np.zeros((0, 2)), np.zeros((0, 2))).selected.shape == (0, 30)


def test_library_refuses_bad_descriptors():
    """The C entry point's own checks (the Python layer makes the same ones first, so the library is called directly): a grid beyond
    8 x 8 is CBA_ERR_UNSUPPORTED, a decreasing CSR array and a subrange outside its frame are CBA_ERR_INVALID with the position."""
    import ctypes as C

    from caliscope_amd import _lib

    lib = FS._load()
    cfs, fs, size = np.array([0, 2], np.int64), np.array([0, 5, 9], np.int64), np.array([[1280.0, 720.0]])
    xy, obj = np.zeros((9, 2)), np.zeros((9, 2))
    hs, hc = np.array([0, 6], np.int64), np.array([5, 4], np.int32)

    def call(**kw):
        f = dict(n_cams=1, cam_frame_start=FS._ptr(cfs, C.c_int64), cam_size=FS._ptr(size), n_frames=2, frame_start=FS._ptr(fs, C.c_int64),
                 homog_start=None, homog_count=None, obs_xy=FS._ptr(xy), obs_obj=FS._ptr(obj), grid_size=5, min_corners=6, target_count=3, float32_io=1)
        f.update(kw)
        out = FS.FrameSelection.empty(1, 2, 3)
        rc = lib.cba_pose_select_frames(C.byref(FS.FrameSelectDesc(**f)), 0, FS._ptr(out.cell_mask, C.c_uint64), FS._ptr(out.pose_features),
                                        FS._ptr(out.orientation), FS._ptr(out.homography_status, C.c_int32), FS._ptr(out.homography_rmse),
                                        FS._ptr(out.selected, C.c_int32), FS._ptr(out.n_selected, C.c_int32), FS._ptr(out.n_anchors, C.c_int32),
                                        FS._ptr(out.bin_mask, C.c_int32), FS._ptr(out.eligible, C.c_int32))
        return rc, _lib.last_error(lib)

    assert call()[0] == 0
    for g in (0, 9):
        rc, msg = call(grid_size=g)
        assert rc == -4 and "grid_size" in msg
    assert call(target_count=0)[0] == -1
    bad = np.array([0, 5, 4], np.int64)
    rc, msg = call(frame_start=FS._ptr(bad, C.c_int64))
    assert rc == -1 and "frame 1" in msg
    rc, msg = call(homog_start=FS._ptr(hs, C.c_int64), homog_count=FS._ptr(hc, C.c_int32))
    assert rc == -1 and "frame 1" in msg
    assert call(homog_start=FS._ptr(hs, C.c_int64))[0] == -1  # the two go together


def test_ring_session_selects_then_calibrates(capsys):
    """The ring session of tests/test_intrinsic_calibration_gpu.py with intrinsics and poses removed:
    calibrate_camera_array_intrinsics(frames="select") solves every camera from at most 30 frames each, every focal length within
    the 1 % the all-frames test asserts; the RMSE is printed beside the all-frames figure."""
    ip, cams = S.ring_board_session()
    bare = CameraArray({c: CameraData(cam_id=c, size=cam.size, fisheye=cam.fisheye) for c, cam in cams.cameras.items()})
    out, reports = calibrate_camera_array_intrinsics(ip, bare, "select")
    every, all_reports = calibrate_camera_array_intrinsics(ip, bare)
    with capsys.disabled():
        for c, cam in sorted(out.cameras.items()):
            cov = reports[c].coverage
            print(f"  cam {c}: {cam.grid_count} of {every.cameras[c].grid_count} frames selected ({cov.orientation_count} tilt directions, coverage "
                  f"{cov.coverage_fraction:.2f}): f {cam.matrix[0, 0]:.2f} rmse {cam.error:.4f} px; all frames: f {every.cameras[c].matrix[0, 0]:.2f} "
                  f"rmse {every.cameras[c].error:.4f} px; truth {cams.cameras[c].matrix[0, 0]:.2f}")
    for c, cam in out.cameras.items():
        f_true = cams.cameras[c].matrix[0, 0]
        cov = reports[c].coverage
        assert reports[c].status == 0 and cov is not None and all_reports[c].coverage is None
        assert 0 < cam.grid_count <= 30 and cam.grid_count == len(cov.selected_frames) and sorted(cov.selected_frames) == reports[c].sync_index.tolist()
        assert abs(cam.matrix[0, 0] - f_true) <= 0.01 * f_true and abs(cam.matrix[1, 1] - f_true) <= 0.01 * f_true, (c, cam.matrix)
