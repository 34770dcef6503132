"""The fixtures of tests/golden/coverage (the reference's own coverage analysis, tests/golden/make_coverage_fixtures.py) and the
comparison both the CPU and the GPU coverage tests hold a backend to: every figure equal, integer for integer.  TEST INFRASTRUCTURE."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pandas as pd

from caliscope_amd import coverage_analysis as CA
from caliscope_amd.point_data import ImagePoints

GOLDEN = Path(__file__).resolve().parent / "golden" / "coverage"
N_CASES = 11
COLS = ["sync_index", "cam_id", "object_id", "keypoint_id"]


def load(case: int) -> dict:
    with np.load(GOLDEN / f"cov_{case:02d}.npz") as z:
        return {k: z[k] for k in z.files}


def image_points(table) -> ImagePoints:
    """An ImagePoints of the four id columns ([rows, 4]: sync_index, cam_id, object_id, keypoint_id); the pixels are zeros."""
    df = pd.DataFrame(np.asarray(table, dtype=np.int64).reshape(-1, 4), columns=COLS)
    df["img_loc_x"] = 0.0
    df["img_loc_y"] = 0.0
    return ImagePoints(df)


def check_case(fx: dict, solver, label=""):
    """The three public functions on the fixture's table with `solver` against what the reference returned."""
    ip = image_points(fx["table"])
    cam_map = {int(c): int(k) for c, k in zip(fx["map_ids"], fx["map_index"])}
    matrix = CA.compute_coverage_matrix(ip, cam_map, _solver=solver)
    assert matrix.dtype == np.int64 and matrix.shape == fx["matrix"].shape, label
    assert np.array_equal(matrix, fx["matrix"]), label
    report = CA.analyze_multi_camera_coverage(ip, _solver=solver)
    assert report.pairwise_observations.dtype == np.int64 and report.pairwise_observations.shape == fx["report_matrix"].shape, label
    assert np.array_equal(report.pairwise_observations, fx["report_matrix"]), label
    assert report.isolated_cameras == fx["isolated"].tolist(), label
    assert report.n_connected_components == int(fx["n_components"]), label
    assert report.leaf_cameras == [tuple(row) for row in fx["leaves"].tolist()], label
    assert report.n_cameras == len(fx["report_matrix"]), label
    assert report.has_critical_issues == (len(fx["isolated"]) > 0 or int(fx["n_components"]) > 1), label
    warnings = CA.detect_structural_warnings(report, report.n_cameras)
    assert [(w.severity.value, w.message) for w in warnings] == list(zip(fx["warn_severity"].tolist(), fx["warn_message"].tolist())), label
    return report
