"""Camera-pair coverage on the g++ build of csrc/coverage_math.h (tests/coverage_native.py): the public functions of
caliscope_amd.coverage_analysis against the reference's own answers (fixtures of tests/golden/coverage), the count against a dense
numpy brute force at the word, tile and slab edges, the two key paths, and the host-side pieces.  Every comparison is exact."""
import numpy as np
import pytest

from caliscope_amd import coverage_analysis as CA
from caliscope_amd.exceptions import BackendError
from caliscope_amd.point_data import STATIC_SYNC_INDEX
from tests import coverage_fixtures as F
from tests import coverage_native as N

CPU = N.HarnessCoverageCounts()


@pytest.mark.parametrize("case", range(F.N_CASES))
def test_public_functions_return_what_the_reference_returned(case):
    F.check_case(F.load(case), CPU, label=f"cov_{case:02d}")


def test_fixtures_cover_the_scenes():
    """What each fixture is there for, read off the reference's recorded answers."""
    fx = [F.load(i) for i in range(F.N_CASES)]
    assert (fx[0]["report_matrix"] > 0).all() and len(fx[0]["warn_message"]) == 0
    assert fx[1]["leaves"][:, 0].tolist() == [0, 3] and int(fx[1]["n_components"]) == 1
    assert int(fx[2]["n_components"]) == 2 and len(fx[2]["isolated"]) == 0
    assert fx[3]["isolated"].tolist() == [3]
    assert len(fx[4]["report_matrix"]) == 2 and len(fx[4]["leaves"]) == 2 and len(fx[4]["warn_message"]) == 0
    assert fx[5]["warn_severity"].tolist() == ["info"] and fx[5]["leaves"][0, 2] >= 100
    assert fx[6]["warn_severity"].tolist() == ["warning"] and fx[6]["leaves"][0, 2] < 100
    assert len(np.unique(fx[7]["table"], axis=0)) < len(fx[7]["table"]) and not set(fx[7]["table"][:, 1]) <= set(fx[7]["map_ids"].tolist())
    assert sorted(set(fx[8]["table"][:, 1].tolist())) == [3, 11, 40] and (fx[8]["table"][:, 0] == STATIC_SYNC_INDEX).any()
    assert len(fx[9]["report_matrix"]) == 70
    assert fx[10]["table"].shape == (0, 4) and fx[10]["report_matrix"].shape == (0, 0) and int(fx[10]["n_components"]) == 0


@pytest.mark.parametrize("n_keys", [1, 63, 64, 65, 4097])
def test_harness_equals_the_brute_force_at_word_and_tile_edges(n_keys):
    tile = N.constants()["tile"]
    for n_cams in (1, 2, tile - 1, tile, tile + 1, 65, 200):
        assert (n_keys, n_cams) in N.edge_grid()
        key, cam, M = N.random_rows(n_keys, n_cams, seed=1000 * n_keys + n_cams)
        assert (cam == -1).any() and len(key) > M.sum()
        assert np.array_equal(CPU.coverage_counts(key, cam, n_cams, n_keys), N.brute_force(M)), (n_keys, n_cams)


@pytest.mark.parametrize("slab_words", [1, 2, 3])
def test_slabs_with_a_partial_last_slab_equal_the_single_slab(slab_words):
    n_keys, n_cams = 64 * 6 + 13, 19  # 7 words: the last slab holds one word for slabs of 2 and of 3
    p = N.plan(n_cams, n_keys, slab_words)
    assert p["n_words"] == 7 and p["n_slabs"] == -(-7 // slab_words) and (slab_words == 1 or 7 % slab_words == 1)
    key, cam, M = N.random_rows(n_keys, n_cams, seed=5)
    one = CPU.coverage_counts(key, cam, n_cams, n_keys)
    assert N.plan(n_cams, n_keys)["n_slabs"] == 1
    assert np.array_equal(CPU.coverage_counts(key, cam, n_cams, n_keys, slab_words), one) and np.array_equal(one, N.brute_force(M))


def test_enumeration_of_tile_pairs_chunks_and_slabs():
    c = N.constants()
    assert c["block"] == c["tile"] ** 2 and c["lds_stride"] == c["stage_words"] + 1 and c["lds_stride"] % 2 == 1
    for n_tiles in (1, 2, 3, 7, 64, 2048):
        n_pairs = n_tiles * (n_tiles + 1) // 2
        probe = range(n_pairs) if n_tiles <= 64 else [0, 1, n_tiles - 1, n_tiles, n_pairs // 2, n_pairs - 2, n_pairs - 1]
        seen = [N.tile_pair(p, n_tiles) for p in probe]
        assert all(0 <= i <= j < n_tiles for i, j in seen)
        if n_tiles <= 64:
            assert seen == [(i, j) for i in range(n_tiles) for j in range(i, n_tiles)]
        else:
            assert seen[0] == (0, 0) and seen[2] == (0, n_tiles - 1) and seen[3] == (1, 1) and seen[-1] == (n_tiles - 1, n_tiles - 1)
    for n_cams, n_keys, slab in ((4, 10_000_000, 0), (1000, 3 * 10**9, 0), (70, 5000, 0), (5, 64 * 64 * 5 + 1, 0), (33, 4097, 3)):
        p = N.plan(n_cams, n_keys, slab)
        assert p["n_words"] == -(-n_keys // 64) and p["n_slabs"] * p["slab_words"] >= p["n_words"] > (p["n_slabs"] - 1) * p["slab_words"]
        assert p["stride"] % c["stage_words"] == 0 and p["slab_words"] <= p["stride"] < p["slab_words"] + c["stage_words"]
        assert p["chunk_words"] % c["stage_words"] == 0 and p["n_chunks"] * p["chunk_words"] >= p["stride"] > (p["n_chunks"] - 1) * p["chunk_words"]
        assert p["n_tiles"] == -(-n_cams // c["tile"]) and p["n_tile_pairs"] == p["n_tiles"] * (p["n_tiles"] + 1) // 2
        assert n_cams * p["stride"] * 8 <= 256 * 2**20  # the bit table of a slab
    assert N.plan(1000, 3 * 10**9)["n_slabs"] > 1
    small_rig = N.plan(4, 10_000_000)
    assert small_rig["n_tile_pairs"] == 1 and small_rig["n_chunks"] >= 256  # the word range alone fills the chip


def _table(seed, rows=600):
    rng = np.random.default_rng(seed)
    t = np.column_stack([rng.integers(-1, 14, rows), rng.integers(0, 5, rows) * 7 + 2, rng.integers(3, 5, rows), rng.integers(10, 16, rows)])
    return t.astype(np.int64)


def _brute_force_of_table(table, cam_ids):
    keys = {k: n for n, k in enumerate(sorted({(s, o, k) for s, _, o, k in table.tolist()}))}
    M = np.zeros((len(keys), len(cam_ids)), dtype=bool)
    for s, c, o, k in table.tolist():
        if c in cam_ids:
            M[keys[(s, o, k)], cam_ids.index(c)] = True
    return N.brute_force(M)


def test_dense_and_unique_key_paths_give_the_same_matrix(monkeypatch):
    table = _table(3)
    cam_ids = sorted(set(table[:, 1].tolist()))
    key_d, n_d, path_d = CA.coverage_keys(table[:, 0], table[:, 2], table[:, 3])
    key_u, n_u, path_u = CA.coverage_keys(table[:, 0], table[:, 2], table[:, 3], force_unique=True)
    assert (path_d, path_u) == ("dense", "unique") and n_d == 15 * 2 * 6 and n_u == len(np.unique(table[:, [0, 2, 3]], axis=0)) <= n_d
    assert key_d.min() == 0 and key_d.max() < n_d and key_u.min() == 0 and key_u.max() == n_u - 1
    cam = np.searchsorted(cam_ids, table[:, 1]).astype(np.int32)
    expected = _brute_force_of_table(table, cam_ids)
    assert np.array_equal(CPU.coverage_counts(key_d, cam, len(cam_ids), n_d), expected)
    assert np.array_equal(CPU.coverage_counts(key_u, cam, len(cam_ids), n_u), expected)
    # and through the public function: with no floor every table beyond 8 keys per row is compressed
    ip = F.image_points(table)
    dense = CA.analyze_multi_camera_coverage(ip, _solver=CPU).pairwise_observations
    monkeypatch.setattr(CA, "DENSE_KEYS_FLOOR", 0)
    monkeypatch.setattr(CA, "DENSE_KEYS_PER_ROW", 0)
    assert CA.coverage_keys(table[:, 0], table[:, 2], table[:, 3])[2] == "unique"
    assert np.array_equal(CA.analyze_multi_camera_coverage(ip, _solver=CPU).pairwise_observations, dense) and np.array_equal(dense, expected)


def test_a_sparse_key_range_takes_the_unique_path():
    """Ids far apart: the dense range would be 2e22 keys (its product does not fit 64 bits), the table has 9."""
    table = np.array([[s, c, o, k] for s in (-1, 2_000_000_000, 4_000_000_000_000) for c in (0, 1, 2) for o, k in ((0, 5), (7_000, 5), (7_000, 900_000))],
                     dtype=np.int64)
    table = table[[r for r in range(len(table)) if r % 4 != 1]]
    key, n_keys, path = CA.coverage_keys(table[:, 0], table[:, 2], table[:, 3])
    assert path == "unique" and n_keys == 9 and key.dtype == np.int64
    got = CA.compute_coverage_matrix(F.image_points(table), {0: 0, 1: 1, 2: 2}, _solver=CPU)
    assert np.array_equal(got, _brute_force_of_table(table, [0, 1, 2]))
    # the largest dense range, and one key more
    rows = 2**17 + 1
    assert CA.coverage_keys(np.array([0, rows * 8 - 1] + [0] * (rows - 2)), np.zeros(rows, int), np.zeros(rows, int))[2] == "dense"
    assert CA.coverage_keys(np.array([0, rows * 8] + [0] * (rows - 2)), np.zeros(rows, int), np.zeros(rows, int))[2] == "unique"
    assert CA.coverage_keys([0, 2**20 - 1], [0, 0], [0, 0])[1:] == (2**20, "dense") and CA.coverage_keys([0, 2**20], [0, 0], [0, 0])[1:] == (2, "unique")


def test_classify_link_quality_at_the_thresholds():
    assert [CA.classify_link_quality(n) for n in (49, 50, 199, 200)] == [CA.LinkQuality.INSUFFICIENT, CA.LinkQuality.MARGINAL, CA.LinkQuality.MARGINAL,
                                                                         CA.LinkQuality.GOOD]
    assert CA.classify_link_quality(0) is CA.LinkQuality.INSUFFICIENT
    assert (CA.GOOD_OBSERVATION_THRESHOLD, CA.MARGINAL_OBSERVATION_THRESHOLD) == (200, 50)
    assert [q.value for q in CA.LinkQuality] == ["good", "marginal", "insufficient"] and [s.value for s in CA.WarningSeverity] == ["critical", "warning", "info"]


def test_out_of_range_key_or_camera_raises_with_the_position():
    key, cam = np.array([0, 5, 9], dtype=np.int64), np.array([0, 1, -1], dtype=np.int32)
    assert CPU.coverage_counts(key, cam, 2, 10).tolist() == [[1, 0], [0, 1]]
    for bad_key, bad_cam, n_cams, n_keys, text in ((key, cam, 2, 9, "observation 2: key 9 out of range [0, 9)"),
                                                   ([0, -1, 3], cam, 2, 10, "observation 1: key -1 out of range [0, 10)"),
                                                   (key, [0, 2, 1], 2, 10, "observation 1: camera 2 out of range [-1, 2)"),
                                                   (key, [-2, 0, 1], 2, 10, "observation 0: camera -2 out of range [-1, 2)")):
        with pytest.raises(BackendError, match="cba_coverage_counts") as info:
            CPU.coverage_counts(bad_key, bad_cam, n_cams, n_keys)
        assert text in str(info.value)
    lib = N.harness()  # (called directly: the matrix of such a rig is not allocated)
    assert lib.ch_coverage_counts(N.constants()["max_cams"] + 1, 10, 0, None, None, 0, None) == -4 and b"at most 32768" in lib.ch_last_error()
    with pytest.raises(ValueError):
        CPU.coverage_counts(key, cam[:2], 2, 10)


def test_empty_inputs_make_no_device_call():
    solver = N.HarnessCoverageCounts()
    table = F.load(0)["table"]
    assert CA.compute_coverage_matrix(F.image_points(table[:0]), {4: 0, 9: 1}, _solver=solver).tolist() == [[0, 0], [0, 0]]
    assert CA.compute_coverage_matrix(F.image_points(table), {}, _solver=solver).shape == (0, 0)
    report = CA.analyze_multi_camera_coverage(F.image_points(table[:0]), _solver=solver)
    assert report.n_cameras == 0 and report.n_connected_components == 0 and not report.has_critical_issues and solver.calls == 0
    assert CA.detect_structural_warnings(report, 0) == []
    # a map none of whose cameras occurs: one call, all rows skipped
    assert not CA.compute_coverage_matrix(F.image_points(table), {77: 0, 78: 1}, _solver=solver).any() and solver.calls == 1
    for bad in ({0: 0, 1: 0}, {0: 1, 1: 2}, {0: -1, 1: 0}):
        with pytest.raises(ValueError, match="distinct indices"):
            CA.compute_coverage_matrix(F.image_points(table), bad, _solver=solver)


def test_components_leaves_and_warning_order_on_random_graphs():
    """connected_component_count against a plain depth-first search; a long path needs many label rounds."""
    rng = np.random.default_rng(11)
    for n, p in ((1, 0.0), (2, 0.0), (12, 0.08), (40, 0.03), (90, 0.02), (200, 0.004)):
        adj = np.triu(rng.random((n, n)) < p, 1)
        adj = adj | adj.T
        left, count = set(range(n)), 0
        while left:
            count += 1
            stack = [left.pop()]
            while stack:
                for m in np.flatnonzero(adj[stack.pop()]).tolist():
                    if m in left:
                        left.remove(m)
                        stack.append(m)
        assert CA.connected_component_count(adj) == count, n
    order = rng.permutation(300)
    path = np.zeros((300, 300), dtype=bool)
    path[order[:-1], order[1:]] = path[order[1:], order[:-1]] = True
    assert CA.connected_component_count(path) == 1 and CA.connected_component_count(np.zeros((0, 0), dtype=bool)) == 0
    report = CA.ExtrinsicCoverageReport(np.zeros((5, 5), dtype=np.int64), [9], 2, [(1, 2, 150), (3, 2, 99), (4, 2, 100)])
    assert [(w.severity.value, w.message) for w in CA.detect_structural_warnings(report, 5)] == [
        ("critical", "Camera C9 has no shared observations with any other camera"), ("critical", "Camera network has 2 disconnected groups"),
        ("warning", "Camera C3 only connected to C2 (99 obs)"), ("info", "Camera C1 connects only through C2"),
        ("info", "Camera C4 connects only through C2")]
    assert [w.severity.value for w in CA.detect_structural_warnings(report, 5, min_leaf_observations=151)] == ["critical"] * 2 + ["warning"] * 3
    assert len(CA.detect_structural_warnings(report, 2)) == 2


def test_descriptor_binding_follows_the_header():
    """The ctypes structure lists the fields of cba_coverage_desc in the header's order and widths; the entry is declared once, in
    include/caliscope_coverage.h, and bound by coverage_analysis.py, not by _lib.py."""
    import ctypes as C
    import re
    from pathlib import Path

    from caliscope_amd import _lib

    root = Path(CA.__file__).resolve().parent.parent
    header = (root / "include" / "caliscope_coverage.h").read_text()
    body = re.search(r"typedef struct \{(.*?)\} cba_coverage_desc;", header, re.S).group(1)
    fields = re.findall(r"^\s*(const\s+)?(int32_t|int64_t)(\*?)\s+(\w+);", body, re.M)
    ctype = {("int32_t", ""): C.c_int32, ("int64_t", ""): C.c_int64, ("int32_t", "*"): _lib.c_int32_p, ("int64_t", "*"): _lib.c_int64_p}
    assert [(name, ctype[(base, star)]) for _, base, star, name in fields] == list(CA.CoverageDesc._fields_)
    assert "int cba_coverage_counts(const cba_coverage_desc* d, int32_t device, int64_t* counts_out);" in header
    assert list(CA.COVERAGE_SIGNATURES) == ["cba_coverage_counts"] and "cba_coverage_counts" not in _lib.SIGNATURES
    assert "cba_coverage" not in (root / "include" / "caliscope_ba.h").read_text()


def test_library_entry_checks_the_table_before_it_looks_for_a_device():
    """cba_coverage_counts itself, on any machine: a bad table is refused with the words of the g++ build, and calls without rows or
    cameras return zeros — all before the device is selected, so none of it needs one."""
    from caliscope_amd import build

    build.build(verbose=False)
    dev = CA.DeviceCoverageCounts()
    key, cam = np.array([0, 5, 9], dtype=np.int64), np.array([0, 1, -1], dtype=np.int32)
    for bad_key, bad_cam, n_keys in ((key, cam, 9), ([0, -1, 3], cam, 10), (key, [0, 2, 1], 10), (key, [-2, 0, 1], 10)):
        with pytest.raises(BackendError) as cpu:
            CPU.coverage_counts(bad_key, bad_cam, 2, n_keys)
        with pytest.raises(BackendError, match=r"cba_coverage_counts failed \(code -1\)") as lib:
            dev.coverage_counts(bad_key, bad_cam, 2, n_keys)
        assert str(lib.value) == str(cpu.value)
    assert dev.coverage_counts(key[:0], cam[:0], 3, 0).tolist() == [[0] * 3] * 3 and dev.coverage_counts(key[:0], cam[:0], 0, 10).shape == (0, 0)
