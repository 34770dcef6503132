"""Answers of the REFERENCE's own coverage analysis on seeded observation tables, stored as fixtures.

    python tests/golden/make_coverage_fixtures.py REFERENCE_SRC     (build container only: imports the reference's src/)

What is run is the reference's ``compute_coverage_matrix``, ``analyze_multi_camera_coverage`` and ``detect_structural_warnings``
(core/coverage_analysis.py), unmodified.  The reference's package imports ``cv2`` and ``rtoml`` on the way; neither is installed
here and neither is reached by these functions, so empty stub modules stand in for them.  Nothing of the reference is copied: the
fixtures hold the tables this script made and what the reference answered.

Per case ``coverage/cov_NN.npz`` stores

* ``table`` [rows, 4] int64: sync_index, cam_id, object_id, keypoint_id (the pixel columns do not enter the analysis);
* ``map_ids`` / ``map_index``: a camera map, and ``matrix``: ``compute_coverage_matrix`` with it;
* ``report_matrix``, ``isolated``, ``n_components``, ``leaves`` [k, 3]: the report of ``analyze_multi_camera_coverage``;
* ``warn_severity`` / ``warn_message``: ``detect_structural_warnings(report, report.n_cameras)`` in its order.

Cases: 00 four cameras, all pairs linked; 01 a chain 0-1-2-3; 02 two islands; 03 one isolated camera; 04 a two-camera rig (leaf
warnings suppressed); 05 a leaf with at least 100 shared keys (INFO); 06 a leaf with fewer (WARNING); 07 every fifth row repeated
and a map over a subset of the cameras; 08 cam ids 3, 11 and 40 with ``sync_index = -1`` rows, two objects sharing keypoint ids and
a map in another order; 09 seventy cameras, random and sparse; 10 the empty table.  Consumer: tests/test_coverage.py,
tests/test_coverage_gpu.py (through tests/coverage_fixtures.py).
"""
import sys
import types
from pathlib import Path

import numpy as np
import pandas as pd

OUT = Path(__file__).parent / "coverage"
COLS = ["sync_index", "cam_id", "object_id", "keypoint_id"]


def linked(groups, seed, kp_per_frame=12):
    """Rows of a table in which, for every (cameras, n) of ``groups``, n keys of their own are seen by exactly those cameras; the
    k-th key is keypoint k % kp_per_frame of frame k // kp_per_frame.  Rows shuffled."""
    rng = np.random.default_rng(seed)
    rows, k = [], 0
    for cams, n in groups:
        for _ in range(n):
            rows += [(k // kp_per_frame, c, 0, k % kp_per_frame) for c in cams]
            k += 1
    rows = np.array(rows, dtype=np.int64).reshape(-1, 4)
    return rows[rng.permutation(len(rows))]


def mixed_ids(seed):
    """Cameras 3, 11 and 40; frames -1 (static objects), 5 and 6; objects 2 and 7 with the same keypoint ids 0..5."""
    rng = np.random.default_rng(seed)
    rows = [(s, c, o, k) for s in (-1, 5, 6) for c in (3, 11, 40) for o in (2, 7) for k in range(6) if rng.random() < 0.6]
    rows = np.array(rows, dtype=np.int64)
    return rows[rng.permutation(len(rows))]


def sparse_rig(seed, n_cams=70, n_keys=400):
    """Every key is seen by 1 to 4 cameras out of a window of 6 neighbouring ids, plus a block of cameras that sees nothing shared."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n_keys):
        first = int(rng.integers(0, n_cams - 9))
        for c in rng.choice(np.arange(first, first + 6), int(rng.integers(1, 5)), replace=False):
            rows.append((k // 9 - 1, int(c), k % 2, k % 9))
    for c in range(n_cams - 4, n_cams):  # cameras with keys of their own only
        rows += [(900 + c, c, 0, k) for k in range(3)]
    rows = np.array(rows, dtype=np.int64)
    return rows[rng.permutation(len(rows))]


def cases():
    """(name, table, camera map or None for the sorted cam ids)"""
    repeated = linked([((0, 1, 2, 3), 60), ((0, 4), 30), ((2, 4), 25), ((1,), 10)], 7)
    repeated = np.concatenate([repeated, repeated[::5]])
    return [
        ("all pairs linked", linked([((0, 1, 2, 3), 120), ((0, 1), 40), ((2, 3), 35), ((1, 2), 5)], 0), None),
        ("chain 0-1-2-3", linked([((0, 1), 210), ((1, 2), 130), ((2, 3), 205)], 1), None),
        ("two islands", linked([((0, 1), 150), ((2, 3), 160), ((2, 3, 4), 20)], 2), None),
        ("one isolated camera", linked([((0, 1, 2), 140), ((0, 1), 30), ((3,), 80)], 3), None),
        ("two cameras", linked([((0, 1), 70), ((0,), 9)], 4), None),
        ("leaf with 150 shared keys", linked([((0, 1, 2), 100), ((2, 3), 150)], 5), None),
        ("leaf with 40 shared keys", linked([((0, 1, 2), 100), ((2, 3), 40)], 6), None),
        ("repeated rows, subset map", repeated, {0: 0, 2: 1, 4: 2}),
        ("ids 3 11 40, static frame, two objects", mixed_ids(8), {40: 0, 3: 1, 11: 2}),
        ("70 cameras, sparse", sparse_rig(9), None),
        ("empty table", np.zeros((0, 4), dtype=np.int64), None),
    ]


def main(reference_src):
    sys.path.insert(0, reference_src)
    for name in ("cv2", "rtoml"):
        sys.modules.setdefault(name, types.ModuleType(name))
    from caliscope.core import coverage_analysis as ca
    from caliscope.core.point_data import ImagePoints

    OUT.mkdir(exist_ok=True)
    for i, (name, table, cam_map) in enumerate(cases()):
        df = pd.DataFrame(table, columns=COLS)
        df["img_loc_x"] = np.linspace(10.0, 600.0, len(df))
        df["img_loc_y"] = np.linspace(400.0, 20.0, len(df))
        ip = ImagePoints(df)
        if cam_map is None:
            cam_map = {int(c): k for k, c in enumerate(sorted(set(table[:, 1].tolist())))}
        matrix = ca.compute_coverage_matrix(ip, cam_map)
        report = ca.analyze_multi_camera_coverage(ip)
        warnings = ca.detect_structural_warnings(report, report.n_cameras)
        fixture = dict(
            table=table, map_ids=np.array(list(cam_map.keys()), dtype=np.int64), map_index=np.array(list(cam_map.values()), dtype=np.int64),
            matrix=np.asarray(matrix, dtype=np.int64).reshape(len(cam_map), len(cam_map)),
            report_matrix=np.asarray(report.pairwise_observations, dtype=np.int64).reshape(report.n_cameras, report.n_cameras),
            isolated=np.array(report.isolated_cameras, dtype=np.int64), n_components=np.int64(report.n_connected_components),
            leaves=np.array(report.leaf_cameras, dtype=np.int64).reshape(-1, 3),
            warn_severity=np.array([w.severity.value for w in warnings], dtype="U16"),
            warn_message=np.array([w.message for w in warnings], dtype="U96"),
        )
        np.savez_compressed(OUT / f"cov_{i:02d}.npz", **fixture)
        print(f"cov_{i:02d} {name}: {len(table)} rows, {report.n_cameras} cameras, {report.n_connected_components} components, "
              f"isolated {report.isolated_cameras}, {len(report.leaf_cameras)} leaves, warnings "
              f"{[w.severity.value for w in warnings]}, {(OUT / f'cov_{i:02d}.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
