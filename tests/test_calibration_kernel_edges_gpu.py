"""k_frame_features, k_frame_select and k_intrinsics on the MI355X at their launch and tie edges: the scenes of
tests/calibration_edge_scenes.py on DeviceFrameSelection / DeviceIntrinsics.

Against references that share nothing with the kernels (the purpose of this file): the NumPy selector of
tests/frame_select_reference.py fed the device's own per-frame outputs, the twin-tie properties (a twin in another wave or in a
later pass of a thread never wins), frame i of a twin camera equal to frame i % 64 bit for bit across the blocks and lanes of
k_frame_features, the NumPy too-few rule and the view statuses of cut and moved views, and the scipy yardstick on the two 129-view
cameras (bound: ten times the yardstick's own spread, tests/test_calibration_edge_scenes.py).  The check functions are those of
that file, which holds the g++ builds to them.

Against the g++ builds: `_same` of tests/test_frame_selection_gpu.py on every selection call and the comparison of
tests/test_intrinsic_calibration_gpu.py::test_device_matches_cpu_build on every intrinsic call, with their BASE_ATOL and
DEVICE_FACTOR.  Run-to-run identity of the twin call and of the 127 ... 257-view call.  Each device call is made once per module.

Observed on an MI355X: selection 0.00022 of the base bound at worst; intrinsics 0.088 (sizes), 0.078 (permuted), 0.071 (screened) and
0.076 (boundary) of it, iteration counts differing by one on some cameras as in the existing file: DEVICE_FACTOR stays 1.0.  Device
against the yardstick: 1.2e-7 (pinhole, 129 views) and 1.9e-8 (fisheye, 129 views) for a bound of 2.04e-6, cost within 1.2e-14
relative of scipy's (the yardstick is solved on the GPU host's CPU and moves by about its spread between machines; the g++ build
differs from the device by 1e-10 at most).
"""
import numpy as np
import pytest

from caliscope_amd.calibrate_intrinsics import DeviceIntrinsics
from caliscope_amd.frame_selector import DeviceFrameSelection
from tests import calibration_edge_scenes as E
from tests import test_calibration_edge_scenes as T
from tests.test_frame_selection_gpu import _same
from tests.test_intrinsic_calibration_gpu import BASE_ATOL, DEVICE_FACTOR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sel_runs():
    return T.selection_runs(DeviceFrameSelection())


@pytest.fixture(scope="module")
def intr_runs():
    return T.intrinsic_runs(DeviceIntrinsics())


# ---- against the independent references ------------------------------------------------------------------------------------------------

def test_selection_equals_the_numpy_selector(sel_runs, capsys):
    worst = T.check_selection_against_reference(sel_runs)
    with capsys.disabled():
        print(f"device selection equals the NumPy selector on every camera; smallest margin of a decision {worst:.3g}")


def test_twins_in_other_waves_and_passes_never_win(sel_runs):
    T.check_twin_ties(sel_runs)


def test_frame_outputs_do_not_depend_on_block_and_lane(sel_runs):
    T.check_frames_do_not_depend_on_position(sel_runs)


def test_late_winners_and_one_frame_repeated(sel_runs):
    T.check_late_winners(sel_runs)


def test_eligible_counts(sel_runs):
    T.check_eligibility(sel_runs)


def test_too_few_rule_and_view_statuses(intr_runs):
    T.check_too_few_rule_and_view_statuses(intr_runs)


def test_permuted_packing_means_the_same_call(intr_runs, capsys):
    worst = T.check_permuted_packing(intr_runs)
    with capsys.disabled():
        print(f"device, permuted against contiguous packing: largest difference {worst:.3g} x max(1, |value|), bound {T.PERMUTED_REL}")


def test_129_view_cameras_reach_the_yardstick_minimum(intr_runs, capsys):
    """The yardstick from the truth start alone (the cold start only measures its spread, which the CPU file asserts)."""
    got = T.check_against_yardstick(intr_runs["sizes"], T.yardstick_129(cold=False))
    with capsys.disabled():
        print("device vs yardstick: " + ", ".join(f"camera {c} |intrinsics - yardstick| {d:.3g} (bound {T.YARDSTICK_TOL:.3g}) cost / yardstick - 1 = {r:.2e}"
                                                  for c, (d, r) in got.items()))


# ---- against the g++ builds ------------------------------------------------------------------------------------------------------------

def test_selection_calls_match_the_cpu_build(sel_runs, capsys):
    cpu = T.harness_selection_runs()
    worst = max(_same(res, cpu[key][1], str(key)) for key, (_, res) in sel_runs.items())
    with capsys.disabled():
        print(f"device vs g++ build [selection edge scenes]: largest difference {worst:.3g} x 1e-12 max(1, |value|)")


def _intrinsics_same(dev, cpu, vstart, vcam, label):
    """The comparison of tests/test_intrinsic_calibration_gpu.py::test_device_matches_cpu_build.  Returns the worst ratio."""
    intr_d, rmse_d, st_d, it_d, pose_d, vr_d, vst_d = dev
    intr_c, rmse_c, st_c, it_c, pose_c, vr_c, vst_c = cpu
    assert np.array_equal(st_d, st_c) and np.array_equal(vst_d, vst_c), label
    assert all(np.isfinite(a).all() for a in (intr_d, rmse_d, pose_d, vr_d)), label
    bad = st_c != 0
    assert np.array_equal(intr_d[bad], intr_c[bad]) and (rmse_d[bad] == 0).all(), label  # start values, bit for bit
    ok = ~bad
    well = (vst_c == 0) & ok[vcam] & (np.diff(vstart) >= 8)
    worst = 0.0
    for d, c in ((intr_d[ok], intr_c[ok]), (rmse_d[ok], rmse_c[ok]), (pose_d[well], pose_c[well]), (vr_d[well], vr_c[well])):
        if c.size:
            worst = max(worst, float((np.abs(d - c) / (BASE_ATOL * np.maximum(1.0, np.abs(c)))).max()))
    left = vst_c != 0
    eye = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    assert np.array_equal(pose_d[left], np.tile(eye, (int(left.sum()), 1))) and (vr_d[left] == 0).all(), label
    return worst, it_d.tolist(), it_c.tolist()


def test_intrinsic_calls_match_the_cpu_build(intr_runs, capsys):
    cpu = T.harness_intrinsic_runs()
    calls = T.intrinsic_calls()
    assert BASE_ATOL * DEVICE_FACTOR * 2000.0 <= T.YARDSTICK_TOL  # never beyond the yardstick bound (values up to ~2e3)
    for name, dev in intr_runs.items():
        vstart, vcam = calls[name][1][2], calls[name][1][3]
        worst, it_d, it_c = _intrinsics_same(dev, cpu[name], vstart, vcam, name)
        with capsys.disabled():
            print(f"device vs g++ build [{name}]: largest difference {worst:.3g} x 1e-12 max(1, |value|); iterations {it_d} / {it_c}")
        assert worst <= DEVICE_FACTOR, (name, worst)


# ---- run to run ------------------------------------------------------------------------------------------------------------------------

def test_two_runs_return_identical_bytes(sel_runs, intr_runs):
    call = E.twin_call()
    first = sel_runs["twin", 200, 6][1]
    again = DeviceFrameSelection().select_frames(*call.args, min_corners=6, target_count=200)
    for name in T.PER_FRAME + T.PER_CAMERA:
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    model, size, vstart, vcam, xy, obj = T.intrinsic_calls()["sizes"][1]
    again = DeviceIntrinsics().intrinsics_batch(model, size, None, vstart, vcam, xy, obj, True, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(intr_runs["sizes"], again))
