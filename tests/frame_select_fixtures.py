"""The fixtures of tests/golden/frame_selection (the reference's own selector, tests/golden/make_frame_selection_fixtures.py) and the
comparison both the CPU and the GPU frame-selection tests hold a backend to.  TEST INFRASTRUCTURE."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pandas as pd

from caliscope_amd import frame_selector as FS
from caliscope_amd.point_data import ImagePoints

GOLDEN = Path(__file__).resolve().parent / "golden" / "frame_selection"
N_CASES = 13
POSE_REL = 1e-12      # pose features and pose_diversity: pandas and the header sum in different orders
MARGIN_FLOOR = 1e-6   # the generator's condition on every discrete decision
INT_COLS = ["sync_index", "cam_id", "object_id", "keypoint_id"]
FLOAT_COLS = ["img_loc_x", "img_loc_y", "obj_loc_x", "obj_loc_y", "obj_loc_z"]


def load(case: int) -> dict:
    with np.load(GOLDEN / f"sel_{case:02d}.npz") as z:
        return {k: z[k] for k in z.files}


def cases() -> list[dict]:
    return [load(i) for i in range(N_CASES)]


def dataframe(fx: dict, cam_id=None) -> pd.DataFrame:
    df = pd.DataFrame(fx["df_int"], columns=INT_COLS)
    for k, name in enumerate(FLOAT_COLS):
        df[name] = fx["df_float"][:, k]
    if cam_id is not None:  # the rows of the fixture's camera under another id
        df = df[df["cam_id"] == int(fx["cam_id"])].copy()
        df["cam_id"] = cam_id
    return df


def keywords(fx: dict) -> dict:
    return dict(target_frame_count=int(fx["target_frame_count"]), min_corners_per_frame=int(fx["min_corners_per_frame"]),
                min_orientations=int(fx["min_orientations"]), grid_size=int(fx["grid_size"]))


def orientation_bound() -> np.ndarray:
    """Ten times the largest difference, per orientation feature, between the generator's two solves of every homography (from
    the normalised and from the raw DLT start): the yardstick's own uncertainty, the rule of the tolerance table of
    INTEGRATION.md section 3d."""
    return 10.0 * np.max([load(i)["orient_tol"] for i in range(N_CASES)], axis=0)


def circular(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def compare(fx: dict, report, frame_sync, sel_cell_mask, sel_pose, sel_orientation, bound, label=""):
    """``report`` and the per-frame outputs of the fixture's camera (arrays over its frames, ``frame_sync`` ascending) against the
    fixture.  Returns the worst orientation distances [3] over the case."""
    grid = int(fx["grid_size"])
    assert report.selected_frames == fx["selected_frames"].tolist(), (label, report.selected_frames, fx["selected_frames"].tolist())
    assert report.eligible_frame_count == int(fx["eligible_frame_count"]) and report.total_frame_count == int(fx["total_frame_count"]), label
    assert report.orientation_count == int(fx["orientation_count"]) and report.orientation_sufficient == bool(fx["orientation_sufficient"]), label
    assert isinstance(report.orientation_sufficient, bool) and isinstance(report.orientation_count, int)
    cov, edge, corner, diversity = fx["fractions"]
    assert (report.coverage_fraction, report.edge_coverage_fraction, report.corner_coverage_fraction) == (cov, edge, corner), label
    assert abs(report.pose_diversity - diversity) <= POSE_REL * max(1.0, abs(diversity)), (label, report.pose_diversity, diversity)
    worst = np.zeros(3)
    if len(fx["frame_sync"]) == 0:
        return worst
    at = np.searchsorted(frame_sync, fx["frame_sync"])
    assert np.array_equal(frame_sync[at], fx["frame_sync"]), label
    for i, f in enumerate(at):
        cells = FS.covered_cells(sel_cell_mask[f], grid)
        assert cells == {(int(r), int(c)) for r, c in zip(*np.nonzero(fx["frame_cells"][i]))}, (label, int(frame_sync[f]))
    want = fx["frame_pose"]
    assert (np.abs(sel_pose[at] - want) <= POSE_REL * np.maximum(1.0, np.abs(want))).all(), (label, np.abs(sel_pose[at] - want).max())
    o, w = sel_orientation[at], fx["frame_orientation"]
    dist = np.column_stack([circular(o[:, 0], w[:, 0]), np.abs(o[:, 1] - w[:, 1]), circular(o[:, 2], w[:, 2])])
    worst = dist.max(axis=0)
    assert (worst <= bound).all(), (label, worst, bound)
    return worst


def run_case(fx: dict, solver, float32_io=True):
    """The fixture's own call through ``select_rig`` (one camera, the whole frame in the homography, as the reference)."""
    df = dataframe(fx)
    cam = int(fx["cam_id"])
    size = (int(fx["image_size"][0]), int(fx["image_size"][1]))
    reports, gathered, sel = FS.select_rig(ImagePoints(df), [(cam, size)], by_object=False, float32_io=float32_io, _solver=solver, **keywords(fx))
    return reports[cam], gathered, sel


DEFAULT_CASES = [0, 4, 6, 7, 8, 11, 12]   # the cases with default arguments: one rig call holds them all


def default_rig():
    """The default-argument cases as cameras 0.. of one table (70, 300, 70, 24, 40, 0 and 9 frames), plus a camera with a single
    frame.  Returns (ImagePoints, [(cam_id, size)], [fixture or None per camera])."""
    parts, cams, fxs = [], [], []
    for k, i in enumerate(DEFAULT_CASES):
        fx = load(i)
        if i == 11:  # the camera without rows: another id of the same table
            part = dataframe(fx).iloc[:0]
        else:
            part = dataframe(fx, cam_id=k)
        parts.append(part)
        cams.append((k, (int(fx["image_size"][0]), int(fx["image_size"][1]))))
        fxs.append(fx)
    one = dataframe(load(0), cam_id=len(cams))
    parts.append(one[one["sync_index"] == one["sync_index"].min()])
    cams.append((len(cams), (1280, 720)))
    fxs.append(None)
    return ImagePoints(pd.concat(parts, ignore_index=True)), cams, fxs
