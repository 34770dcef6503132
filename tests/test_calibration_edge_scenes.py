"""The scenes of tests/calibration_edge_scenes.py on the g++ builds of frame_select_math.h and intrinsic_math.h: the discrete
selection against the NumPy selector of tests/frame_select_reference.py, the twin-tie and position properties, the too-few rule
and the view statuses against NumPy, the permuted packing against the contiguous one, and the two 129-view cameras against the
scipy yardstick of tests/intrinsic_scenes.py.  The check functions take the results of a backend, and
tests/test_calibration_kernel_edges_gpu.py holds the device to the same ones.

The yardstick's own spread, measured here on the CPU: |yardstick(start = truth) - yardstick(cold start)| over the intrinsics of the
two 129-view cameras is 2.04e-7 (pinhole; 5.2e-8 fisheye; largest entry, the focal lengths and the principal point).  The bound on
|intrinsics - yardstick| is ten times that, the rule NOISY_TOL of tests/test_intrinsic_calibration.py was set by; it comes from
scipy alone, never from the harness or the device.  The g++ build lies within 2.9e-10 of the yardstick on these cameras and the device
within 1.2e-7 (MI355X).  The four
scipy solves take about 24 s together at 129 views (dense Jacobians of 5160 x 783); they stay at 129 views, because a prefix would
take the independent reference away from the one size at which a lane of k_intrinsics wraps to a second pass.
"""
import functools

import numpy as np

from caliscope_amd import frame_selector as FS
from tests import calibration_edge_scenes as E
from tests import frame_select_reference as R
from tests import intrinsic_scenes as S
from tests.frame_select_fixtures import MARGIN_FLOOR
from tests.frame_select_native import HarnessFrameSelection
from tests.intrinsic_native import HarnessIntrinsics
from tests.test_intrinsic_calibration import COST_REL, _f32

YARDSTICK_SPREAD = 2.04e-7           # measured, see above
YARDSTICK_TOL = 10 * YARDSTICK_SPREAD
PERMUTED_REL = 1e-12                 # permuted against contiguous packing: the sum order among views of equal corner count changes
FSEL_MIN_TILT = 0.1
PERM_SEED = 5
PER_FRAME = ("cell_mask", "pose_features", "orientation", "homography_status", "homography_rmse")
PER_CAMERA = ("selected", "n_selected", "n_anchors", "bin_mask", "eligible")


# ---- the calls, once per backend -------------------------------------------------------------------------------------------------------

def selection_runs(backend):
    """{(call name, target, min_corners): (SelCall, FrameSelection)} of every selection scene on ``backend``."""
    runs = {}
    for target in E.TWIN_TARGETS:
        runs["twin", target, 6] = (E.twin_call(), backend.select_frames(*E.twin_call().args, min_corners=6, target_count=target))
    runs["block", 30, 6] = (E.block_call(), backend.select_frames(*E.block_call().args, min_corners=6, target_count=30))
    runs["late", 30, 6] = (E.late_call(), backend.select_frames(*E.late_call().args, min_corners=6, target_count=30))
    for mc in (6, 0):
        runs["eligibility", 30, mc] = (E.eligibility_call(), backend.select_frames(*E.eligibility_call().args, min_corners=mc, target_count=30))
    return runs


def intrinsic_calls():
    """{name: (scenes, pack arguments)}; "permuted" is "sizes" in a seeded random view order."""
    sizes, screened, boundary = E.size_scenes(), E.screened_scenes()[1], E.boundary_scenes()[1]
    return {"sizes": (sizes, S.pack(sizes)), "permuted": (sizes, E.pack_permuted(sizes, PERM_SEED)[0]), "screened": (screened, S.pack(screened)),
            "boundary": (boundary, S.pack(boundary))}


def intrinsic_runs(backend):
    out = {}
    for name, (scenes, (model, size, vstart, vcam, xy, obj)) in intrinsic_calls().items():
        out[name] = backend.intrinsics_batch(model, size, None, vstart, vcam, xy, obj, True, 0)
    return out


@functools.cache
def harness_selection_runs():
    return selection_runs(HarnessFrameSelection())


@functools.cache
def harness_intrinsic_runs():
    return intrinsic_runs(HarnessIntrinsics())


# ---- checks of a backend's selection results -------------------------------------------------------------------------------------------

def check_selection_against_reference(runs):
    """The NumPy selector, fed the backend's own per-frame outputs, returns the backend's selected, n_selected, n_anchors, bin_mask
    and eligible for every camera of every call, and every decision of it has a margin of at least MARGIN_FLOOR (or is an exact
    tie of twins).  Returns the smallest margin."""
    worst = np.inf
    for (name, target, mc), (call, res) in runs.items():
        worst = min(worst, R.check_call(call, res, min_corners=mc, target=target, label=name))
    assert worst >= MARGIN_FLOOR, worst   # a condition on the scenes: re-seed them, never lower the floor
    return worst


def check_twin_ties(runs):
    """Twins in other waves and in later passes of a thread never win: every selected frame of the twin call is below 64, and the
    list of every camera with nf >= 64 equals the 64-frame camera's entry for entry, at every target."""
    call = E.twin_call()
    rows = {int(label[4:]): call.labels.index(label) for label in call.labels if label.startswith("twin")}
    for target in E.TWIN_TARGETS:
        res = runs["twin", target, 6][1]
        assert res.selected.max() < E.K_BASE, (target, res.selected.max())
        first = res.selected[rows[64]]
        for nf, c in rows.items():
            assert int(res.n_anchors[c]) == 8 and int(res.bin_mask[c]) == 255, (target, nf)
            if nf >= E.K_BASE:
                assert res.selected[c].tolist() == first.tolist(), (target, nf)
                assert int(res.n_selected[c]) == int(res.n_selected[rows[64]]), (target, nf)
        empty = call.labels.index("empty")
        assert (res.selected[empty] == -1).all() and res.n_selected[empty] == 0 and res.eligible[empty] == 0 and res.n_anchors[empty] == 0
        assert res.eligible[[rows[nf] for nf in E.TWIN_COUNTS]].tolist() == list(E.TWIN_COUNTS)
    eight = runs["twin", 8, 6][1]
    assert (eight.n_selected[list(rows.values())] == 8).all()                    # the na >= target return
    five = runs["twin", 5, 6][1]
    assert np.array_equal(five.selected[:, :5], eight.selected[:, :5]) and (five.n_selected[list(rows.values())] == 5).all()  # bins in order
    assert runs["twin", 1, 6][1].selected[:, 0].tolist() == eight.selected[:, 0].tolist()
    many = runs["twin", 200, 6][1]
    for nf, c in rows.items():
        k = int(many.n_selected[c])
        assert 30 < k < min(nf, E.K_BASE) + 1 and (many.selected[c, k:] == -1).all() and len(set(many.selected[c, :k].tolist())) == k, (nf, k)
    assert np.array_equal(many.selected[:, :30], runs["twin", 30, 6][1].selected)
    # what these scenes give (a CPU probe of the construction): at 30 every camera, the 63-frame one included, returns the same 30
    # frames; at 200 the greedy phase stops below FSEL_MIN_SCORE with one base frame left
    thirty = runs["twin", 30, 6][1]
    assert all(thirty.selected[c].tolist() == thirty.selected[rows[64]].tolist() and thirty.n_selected[c] == 30 for c in rows.values())
    assert [int(many.n_selected[rows[nf]]) for nf in E.TWIN_COUNTS] == [63, 62, 63, 63, 63, 63, 63]
    # the 64-frame camera alone (one block of k_frame_features) selects what it selects inside the rig
    alone = runs["block", 30, 6][1]
    inside = runs["twin", 30, 6][1]
    assert alone.selected[0].tolist() == inside.selected[rows[64]].tolist()
    a, b = call.camera("twin64")
    for name in PER_FRAME:
        assert getattr(alone, name).tobytes() == getattr(inside, name)[a:b].tobytes(), name


def check_frames_do_not_depend_on_position(runs):
    """Frames with the same rows return the same per-frame outputs bit for bit wherever they sit in a call (frame i of a twin camera
    equals frame i % 64), across the blocks and lanes of k_frame_features and across calls."""
    seen = {}
    for (name, target, mc), (call, res) in runs.items():
        for f, key in enumerate(call.content.tolist()):
            got = tuple(getattr(res, n)[f].tobytes() for n in PER_FRAME)
            assert seen.setdefault(key, got) == got, (name, target, f, key)
        assert np.isfinite(res.pose_features).all() and np.isfinite(res.orientation).all() and np.isfinite(res.homography_rmse).all()
    assert len(seen) == 2 * E.K_BASE + 1


def check_late_winners(runs):
    """late257: the single tilted frame at 256 (the second pass of thread 0) is the only anchor.  one257: one frame selected, frame
    0; every twin scores 0.  late513: the anchors are the 64-frame camera's, 449 frames later; nothing is selected among the 448
    later copies of the dull frame."""
    call, res = runs["late", 30, 6]
    c = call.labels.index("late257")
    a, b = call.camera("late257")
    assert (res.orientation[a:b - 1, 1] < FSEL_MIN_TILT).all() and res.orientation[b - 1, 1] >= FSEL_MIN_TILT
    assert int(res.n_anchors[c]) == 1 and int(res.selected[c, 0]) == 256 and bin(int(res.bin_mask[c])).count("1") == 1
    assert res.selected[c, :int(res.n_selected[c])].tolist() in ([256], [256, 0]) and (res.selected[c, int(res.n_selected[c]):] == -1).all()
    c = call.labels.index("one257")
    assert res.selected[c].tolist() == [0] + [-1] * 29 and int(res.n_selected[c]) == 1 and int(res.n_anchors[c]) == 1 and int(res.eligible[c]) == 257
    c = call.labels.index("late513")
    twin = runs["twin", 8, 6][1].selected[0]
    assert res.selected[c, :8].tolist() == (twin + 449).tolist() and int(res.n_anchors[c]) == 8 and int(res.n_selected[c]) == 30
    assert all(f == 0 or 449 <= f <= 512 for f in res.selected[c].tolist())
    for label in ("empty", "ineligible"):
        c = call.labels.index(label)
        assert (res.selected[c] == -1).all() and not res.n_selected[c] and not res.n_anchors[c] and not res.bin_mask[c] and not res.eligible[c]


def check_eligibility(runs):
    """eligible is the NumPy count of frames with at least min_corners corners; no cut frame is selected at min_corners = 6."""
    for mc in (6, 0):
        call, res = runs["eligibility", 30, mc]
        n = call.corners
        for c, label in enumerate(call.labels):
            a, b = call.camera(label)
            assert int(res.eligible[c]) == int((n[a:b] >= mc).sum()), (mc, label)
            chosen = res.selected[c, :int(res.n_selected[c])]
            assert (n[a:b][chosen] >= mc).all(), (mc, label)
        assert (res.homography_status == FS.HOMOG_OK).all()
    assert runs["eligibility", 30, 6][1].eligible.tolist() == [128, 0, 128, 0, 129] and runs["eligibility", 30, 0][1].eligible.tolist() == [255, 0, 256, 70, 257]


# ---- checks of a backend's intrinsic results -------------------------------------------------------------------------------------------

def _focal_within_one_percent(scenes, res, c):
    intr = res[0][c]
    assert np.isfinite(intr).all() and np.isfinite(res[1][c])
    assert abs(intr[0] - scenes[c].intr[0]) <= 0.01 * scenes[c].intr[0] and abs(intr[1] - scenes[c].intr[1]) <= 0.01 * scenes[c].intr[1], (c, intr)


def check_too_few_rule_and_view_statuses(runs):
    """Camera status INTR_TOO_FEW exactly where NumPy says so from the returned view statuses; the cut views PNP_TOO_FEW (1), the
    moved fisheye view PNP_FAILED (2), every other view 0; solved cameras finite and within 1 % of the true focal lengths."""
    calls = intrinsic_calls()
    for name, res in runs.items():
        scenes, (model, size, vstart, vcam, xy, obj) = calls[name]
        intr, rmse, status, iters, pose, vrmse, vstat = res
        assert np.array_equal(status == 1, E.too_few_rule(scenes, vcam, vstart, vstat)), (name, status)
        assert all(np.isfinite(a).all() for a in (intr, rmse, pose, vrmse)), name
        if name != "boundary":  # (a camera with as many residuals as unknowns solves, to whatever its noise says)
            for c in np.flatnonzero(status == 0):
                _focal_within_one_percent(scenes, res, c)
    assert (runs["sizes"][2] == 0).all() and (runs["sizes"][6] == 0).all()
    labels, scenes, expect = E.screened_scenes()
    vcam, status, vstat = calls["screened"][1][3], runs["screened"][2], runs["screened"][6]
    for c, label in enumerate(labels):
        got = vstat[vcam == c]
        assert {int(v): int(got[v]) for v in np.flatnonzero(got)} == expect.get(c, {}), label
        assert int(status[c]) == (1 if label in ("no views", "two views") else 0), label
    labels, scenes = E.boundary_scenes()
    vstart, status = calls["boundary"][1][2], runs["boundary"][2]
    assert np.diff(vstart).reshape(-1, 3).sum(axis=1).tolist()[:4] == [13, 14, 12, 13]
    assert status[[0, 2, 4]].tolist() == [1, 1, 1] and (status[[1, 3, 5]] != 1).all(), status
    assert runs["boundary"][6].tolist() == [0] * 13 + [1] + [0] * 4


def check_permuted_packing(runs):
    """An unsorted view_cam means the same call: statuses equal, values within PERMUTED_REL * max(1, |value|) of the contiguous
    packing (views permuted back).  Measured: 6.5e-14 on the g++ build, 7.1e-14 on an MI355X (largest over intrinsics,
    RMSE, poses and view RMSE).  Returns the worst ratio."""
    perm = E.pack_permuted(E.size_scenes(), PERM_SEED)[1]
    a, b = runs["sizes"], runs["permuted"]
    assert np.array_equal(b[2], a[2]) and np.array_equal(b[6], a[6][perm])
    worst = 0.0
    for k, back in ((0, None), (1, None), (4, perm), (5, perm)):
        ref = a[k] if back is None else a[k][back]
        worst = max(worst, float((np.abs(b[k] - ref) / np.maximum(1.0, np.abs(ref))).max()))
    assert worst <= PERMUTED_REL, worst
    return worst


@functools.cache
def yardstick_129(cold=True):
    """scipy's minimum on the two 129-view cameras (cameras 2 and 6 of the "sizes" call) from the truth and, with ``cold``, from the
    product's cold start: {camera: (intr9 from the truth, its sum of squares, intr9 from the cold start or None, its sum of squares
    or inf, corners)}."""
    scenes = E.size_scenes()
    out = {}
    for c in (2, 6):
        sc = scenes[c]
        assert len(sc.views) == 129
        views = [(_f32(X), _f32(uv)) for X, uv, _, _ in sc.views]
        ya, ssq_a, _, _ = S.yardstick(views, sc.fisheye, sc.truth9, S.truth_poses(sc))
        yb, ssq_b = None, np.inf
        if cold:
            start, pose0, st = S.cold_start_poses([sc], True)
            assert (st == 0).all()
            yb, ssq_b, _, _ = S.yardstick(views, sc.fisheye, start[0], pose0)
        out[c] = (ya, ssq_a, yb, ssq_b, sum(len(X) for X, _ in views))
    return out


def check_against_yardstick(run, yard):
    """The 129-view cameras of a "sizes" result: cost <= yardstick * (1 + COST_REL) and |intrinsics - yardstick| <= YARDSTICK_TOL.
    Returns {camera: (distance, cost / yardstick - 1)}."""
    out = {}
    for c, (ya, ssq_a, yb, ssq_b, n) in yard.items():
        assert run[2][c] == 0 and (run[6][E_VIEWS_OF[c]] == 0).all()
        ssq, ssq_y = run[1][c] ** 2 * n, min(ssq_a, ssq_b)
        d = float(np.abs(run[0][c] - ya).max())
        out[c] = (d, ssq / ssq_y - 1)
        assert ssq <= ssq_y * (1.0 + COST_REL), (c, ssq, ssq_y)
        assert d <= YARDSTICK_TOL, (c, d)
    return out


_counts = np.cumsum((0,) + E.PINHOLE_COUNTS + E.FISHEYE_COUNTS)
E_VIEWS_OF = {c: slice(int(_counts[c]), int(_counts[c + 1])) for c in range(len(_counts) - 1)}   # the views of camera c of "sizes"


# ---- the g++ builds --------------------------------------------------------------------------------------------------------------------

def test_selection_equals_the_numpy_selector_and_the_margins_hold(capsys):
    worst = check_selection_against_reference(harness_selection_runs())
    with capsys.disabled():
        print(f"smallest margin of a discrete decision over the edge scenes: {worst:.3g} (floor {MARGIN_FLOOR})")


def test_twins_in_other_waves_and_passes_never_win():
    check_twin_ties(harness_selection_runs())


def test_frame_outputs_do_not_depend_on_the_position_in_the_call():
    check_frames_do_not_depend_on_position(harness_selection_runs())


def test_late_winners_and_one_frame_repeated():
    check_late_winners(harness_selection_runs())


def test_eligible_counts():
    check_eligibility(harness_selection_runs())


def test_too_few_rule_and_view_statuses():
    check_too_few_rule_and_view_statuses(harness_intrinsic_runs())
    assert harness_intrinsic_runs()["boundary"][2].tolist() == [1, 0, 1, 0, 1, 0]


def test_permuted_packing_means_the_same_call(capsys):
    worst = check_permuted_packing(harness_intrinsic_runs())
    with capsys.disabled():
        print(f"permuted against contiguous packing: largest difference {worst:.3g} x max(1, |value|), bound {PERMUTED_REL}")


def test_129_view_cameras_reach_the_yardstick_minimum(capsys):
    yard = yardstick_129()
    spread = max(float(np.abs(ya - yb).max()) for ya, _, yb, _, _ in yard.values())
    got = check_against_yardstick(harness_intrinsic_runs()["sizes"], yard)
    with capsys.disabled():
        print(f"|yardstick(truth) - yardstick(cold)| {spread:.3g} (recorded {YARDSTICK_SPREAD}); g++ build: "
              + ", ".join(f"camera {c} |intrinsics - yardstick| {d:.3g} cost / yardstick - 1 = {r:.2e}" for c, (d, r) in got.items()))
    assert spread <= YARDSTICK_SPREAD * 1.0001, spread   # the yardstick is as good as when the bound was set
