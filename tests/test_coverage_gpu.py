"""Camera-pair coverage on the MI355X: cba_coverage_counts against the g++ build of the same header (tests/coverage_native.py) and
against a dense numpy brute force at the word, tile, chunk and slab edges, under contention, on the reference's own answers
(fixtures of tests/golden/coverage) through the public functions, and its refusal of a bad table.  Every comparison is exact."""
import numpy as np
import pytest

from caliscope_amd import coverage_analysis as CA
from caliscope_amd.coverage_analysis import DeviceCoverageCounts
from caliscope_amd.exceptions import BackendError
from tests import coverage_fixtures as F
from tests import coverage_native as N

pytestmark = pytest.mark.gpu

DEV, CPU = DeviceCoverageCounts(), N.HarnessCoverageCounts()


@pytest.mark.parametrize("n_keys", [1, 63, 64, 65, 4097])
def test_device_equals_the_cpu_build_and_the_brute_force_at_word_and_tile_edges(n_keys):
    for _, n_cams in [e for e in N.edge_grid() if e[0] == n_keys]:
        key, cam, M = N.random_rows(n_keys, n_cams, seed=1000 * n_keys + n_cams)
        dev = DEV.coverage_counts(key, cam, n_cams, n_keys)
        assert dev.dtype == np.int64 and dev.shape == (n_cams, n_cams)
        assert np.array_equal(dev, N.brute_force(M)), (n_keys, n_cams)
        assert np.array_equal(dev, CPU.coverage_counts(key, cam, n_cams, n_keys)), (n_keys, n_cams)


@pytest.mark.parametrize("slab_words", [1, 2, 3])
def test_slabs_with_a_partial_last_slab_equal_the_single_slab(slab_words):
    n_keys, n_cams = 64 * 6 + 13, 19  # 7 words: the last slab holds one word for slabs of 2 and of 3
    assert N.plan(n_cams, n_keys, slab_words)["n_slabs"] == -(-7 // slab_words)
    key, cam, M = N.random_rows(n_keys, n_cams, seed=5)
    dev = DEV.coverage_counts(key, cam, n_cams, n_keys, slab_words)
    assert np.array_equal(dev, DEV.coverage_counts(key, cam, n_cams, n_keys)) and np.array_equal(dev, N.brute_force(M))


@pytest.mark.parametrize("n_cams, stages", [(5, 3), (40, 5)])
def test_word_range_split_over_several_workgroups(n_cams, stages):
    """More words than one stage: with few tile pairs every stage of the row is a chunk of its own, taken by another workgroup; the
    last chunk ends in the padding of the row.  A slab shorter than the row on top of it."""
    c = N.constants()
    n_keys = 64 * c["stage_words"] * (stages - 1) + 70
    p = N.plan(n_cams, n_keys)
    assert p["n_slabs"] == 1 and p["n_chunks"] == stages and p["chunk_words"] == c["stage_words"] and p["n_tile_pairs"] == (1 if n_cams == 5 else 6)
    key, cam, M = N.random_rows(n_keys, n_cams, seed=77 + n_cams, density=0.2)
    expected = N.brute_force(M)
    assert np.array_equal(DEV.coverage_counts(key, cam, n_cams, n_keys), expected)
    slab = c["stage_words"] * 2 + 1
    assert N.plan(n_cams, n_keys, slab)["n_slabs"] > 1 and N.plan(n_cams, n_keys, slab)["n_chunks"] == 3
    assert np.array_equal(DEV.coverage_counts(key, cam, n_cams, n_keys, slab), expected)


def test_every_camera_on_every_key():
    """20 000 keys all seen by the same 8 cameras: every word of the bit table is hit 64 times per camera, every count is 20 000."""
    n_keys, n_cams = 20_000, 8
    rng = np.random.default_rng(3)
    order = rng.permutation(n_keys * n_cams)
    key, cam = (order // n_cams).astype(np.int64), (order % n_cams).astype(np.int32)
    first = DEV.coverage_counts(key, cam, n_cams, n_keys)
    assert (first == n_keys).all()
    assert first.tobytes() == DEV.coverage_counts(key, cam, n_cams, n_keys).tobytes()


@pytest.mark.parametrize("case", range(F.N_CASES))
def test_public_functions_return_what_the_reference_returned(case):
    F.check_case(F.load(case), None, label=f"cov_{case:02d}")  # no _solver: the device call


def test_session_of_8_cameras_5000_points_40000_rows():
    rng = np.random.default_rng(2)
    n_cams, n_points, rows = 8, 5000, 40_000
    point, cam_id = rng.integers(0, n_points, rows), rng.integers(0, n_cams, rows) * 3 + 1
    table = np.column_stack([point // 20 - 1, cam_id, np.zeros(rows, dtype=np.int64), point % 20])
    M = np.zeros((n_points, n_cams), dtype=bool)
    M[point, (cam_id - 1) // 3] = True
    report = CA.analyze_multi_camera_coverage(F.image_points(table))
    assert np.array_equal(report.pairwise_observations, N.brute_force(M))
    assert report.n_connected_components == 1 and not report.isolated_cameras and not report.leaf_cameras


def test_a_bad_table_is_refused_before_any_launch_and_the_next_call_succeeds():
    key, cam, M = N.random_rows(300, 6, seed=9)
    bad_key, bad_cam = key.copy(), cam.copy()
    bad_key[17] = 300
    bad_cam[40] = 6
    for k, c, text in ((bad_key, cam, "observation 17: key 300 out of range [0, 300)"), (key, bad_cam, "observation 40: camera 6 out of range [-1, 6)")):
        with pytest.raises(BackendError, match=r"cba_coverage_counts failed \(code -1\)") as info:
            DEV.coverage_counts(k, c, 6, 300)
        assert text in str(info.value)
        with pytest.raises(BackendError) as same:  # the CPU build refuses with the same words
            CPU.coverage_counts(k, c, 6, 300)
        assert text in str(same.value)
    assert np.array_equal(DEV.coverage_counts(key, cam, 6, 300), N.brute_force(M))
    assert DEV.coverage_counts(key[:0], cam[:0], 3, 0).tolist() == [[0] * 3] * 3 and DEV.coverage_counts(key[:0], cam[:0], 0, 0).shape == (0, 0)
