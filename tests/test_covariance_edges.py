"""The scenes of tests/covariance_edge_scenes.py on the CPU: that each is what its name says, that each is fit to test with (the two CPU
formulations agree to 1e-8, asserted by the tolerance rule itself), and the g++ harnesses of the covariance and the reliability call on
them under the rule of tests/test_uncertainty.py and tests/test_reliability.py (ten times the disagreement of the two CPU formulations,
floor 1e-12).  tests/test_covariance_edges_gpu.py runs the device on the same scenes and says which loop of which kernel each one is for.

Measured disagreements of the two CPU formulations (camera block, point blocks), the eighth eigenvalue relative to the largest, and the
harness's error against the pseudo-inverse (camera block, point blocks):

    MANY_VIEWS         65 fisheye x 60 (ncp = 390)                 6.1e-15  2.4e-15   1.6e-02   7.1e-15  4.0e-15
    MANY_VIEWS_RAGGED  64 / 65 / 2 views, a repeated row           3.1e-14  2.6e-13   9.6e-05   3.2e-14  2.6e-13
    MANY_VIEWS_MIXED   10 free pinhole + 56 fisheye x 60 (426)     4.7e-12  2.8e-12   8.9e-06   5.0e-12  2.8e-12
    LIMIT_SIX          192 locked x 40 (ncp = 1152)                2.4e-14  2.9e-15   6.0e-03   9.7e-15  1.1e-14
    LIMIT_NINE         128 free pinhole x 40 (ncp = 1152)          1.2e-11  1.4e-11   2.3e-06   1.2e-11  1.4e-11
    BELOW_LIMIT        190 fisheye + 1 free pinhole x 40 (1149)    1.7e-12  2.3e-13   2.3e-05   1.7e-12  2.4e-13
    OBS_256            4 locked x 64                               8.1e-15  3.1e-15   4.9e-03   1.1e-14  5.2e-15
    OBS_257            the same, one row twice                     1.7e-14  2.8e-15   4.9e-03   2.0e-14  5.5e-15
    POINTS_256         3 locked x 256                              1.5e-14  2.0e-14   9.3e-04   1.3e-14  2.3e-14
    POINTS_257         3 locked x 257                              7.1e-15  1.5e-14   9.2e-04   7.6e-15  1.7e-14

(The pseudo-inverse is the less exact of the two formulations on the larger scenes: the harness follows the bordered formula, so its
error and the disagreement move together, and both change by a small factor with the BLAS that numpy runs on.)  With locked pinhole
cameras beside a free one the parameterisation frees all of them, so BELOW_LIMIT takes its six-wide cameras as fisheye ones, as MIXED33 does.

Reliability (disagreement of the dense projector and the block formula, error of R_oo, error of w times r_j, smallest reference r):

    REL_VIEWS          65 fisheye x 30                             2.1e-15  1.9e-15  1.1e-15  0.34
    REL_VIEWS_RAGGED   64 / 65 / 2 views, a repeated row           8.4e-14  8.1e-14  4.0e-14  0.036
    OBS_256                                                        1.1e-15  1.3e-15  1.6e-15  0.17
    OBS_257                                                        1.0e-15  1.4e-15  1.7e-15  0.17

MANY_POINTS (3 locked cameras x 65 793 points) has no dense reference: the recorded blocks of tests/golden/covariance_many_points.npz
(a sparse LU of the bordered system) stand in for the pseudo-inverse, and the bordered formula restated block-sparsely
(covariance_edge_scenes.sparse_bordered_blocks) is the second formulation.  The restatement is first held to
covariance_native.bordered_blocks where both can be formed (1e-12 relative, block-wise max-norm: the same arithmetic in another order,
so the floor of the rule).  Measured (camera block, point blocks): restatement against bordered_blocks 9.7e-15 8.5e-15 (SMALL), 1.2e-13
7.3e-15 (MIXED33), 1.8e-15 6.4e-16 (ragged); on MANY_POINTS, restatement against the recorded blocks 4.1e-14 7.0e-15, harness against
the recorded blocks 4.0e-14 1.8e-14, against the restatement on all 65 793 points 1.4e-14; its cost 1.1e-14 off the oracle's.

The file takes about 20 s, half of it the three scenes at the size limit (an eigh of 1272 unknowns each).
"""
import re

import numpy as np
import pytest

from caliscope_amd.exceptions import BackendError
from tests import covariance_edge_scenes as es
from tests import covariance_native as cn
from tests import reliability_native as rn
from tests.test_uncertainty import MIXED33, SMALL

COVARIANCE_SCENES = {"many_views": es.MANY_VIEWS, "many_views_ragged": es.MANY_VIEWS_RAGGED, "many_views_mixed": es.MANY_VIEWS_MIXED,
                     "limit_six": es.LIMIT_SIX, "limit_nine": es.LIMIT_NINE, "below_limit": es.BELOW_LIMIT, "obs_256": es.OBS_256,
                     "obs_257": es.OBS_257, "points_256": es.POINTS_256, "points_257": es.POINTS_257}
RELIABILITY_SCENES = {"rel_views": es.REL_VIEWS, "rel_views_ragged": es.REL_VIEWS_RAGGED, "obs_256": es.OBS_256, "obs_257": es.OBS_257}
OVER_LIMIT_WORDS = "1158 camera parameters: the dense factorisation handles 1152"

# name -> (ncp, blocks of 32, rows of the last block, n_obs, n_points, the distinct view counts, repeated rows)
EXPECTED = {
    "many_views": (390, 13, 6, 3900, 60, {65}, 0),
    "many_views_ragged": (390, 13, 6, 3900 - 1 - 63 + 1, 60, {2, 64, 65, 66}, 1),
    "rel_views": (390, 13, 6, 1950, 30, {65}, 0),
    "rel_views_ragged": (390, 13, 6, 1950 - 1 - 63 + 1, 30, {2, 64, 65, 66}, 1),
    "many_views_mixed": (426, 14, 10, 3960, 60, {66}, 0),
    "limit_six": (1152, 36, 32, 7680, 40, {192}, 0),
    "limit_nine": (1152, 36, 32, 5120, 40, {128}, 0),
    "below_limit": (1149, 36, 29, 7640, 40, {191}, 0),
    "over_limit": (1158, 37, 6, 7720, 40, {193}, 0),
    "obs_256": (24, 1, 24, 256, 64, {4}, 0),
    "obs_257": (24, 1, 24, 257, 64, {4, 5}, 1),
    "points_256": (18, 1, 18, 768, 256, {3}, 0),
    "points_257": (18, 1, 18, 771, 257, {3}, 0),
    "many_points": (18, 1, 18, 197379, 65793, {3}, 0),
}
ALL_SCENES = dict(COVARIANCE_SCENES, rel_views=es.REL_VIEWS, rel_views_ragged=es.REL_VIEWS_RAGGED, over_limit=es.OVER_LIMIT, many_points=es.MANY_POINTS)


def harness_covariance(key):
    sc = cn.key_scene(key)
    return cn.HarnessUncertainty().parameter_covariance(*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]))


def harness_reliability(key):
    return rn.HarnessReliability().observation_reliability(*rn.scene_arguments(key))


# ---- the scenes are what their names say --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EXPECTED))
def test_scene_is_what_its_name_says(name):
    d = es.describe(ALL_SCENES[name])
    ncp, blocks, last_rows, n_obs, n_points, views, repeated = EXPECTED[name]
    assert (d["ncp"], d["blocks"], d["last_rows"], d["n_obs"], d["n_points"], d["repeated"]) == (ncp, blocks, last_rows, n_obs, n_points, repeated)
    assert set(d["views"]) == views and d["cam_obs"].min() >= 1
    sc = cn.key_scene(ALL_SCENES[name])
    widths = tuple(b.n_params for b in sc["par"].blocks)
    if name.endswith("ragged"):  # point 0: a whole wave of views, point 1: one more, point 2: the least, point 3: a row twice
        assert d["views"][:4].tolist() == [64, 65, 2, 66] and set(d["views"][4:]) == {65}
        pairs = np.stack([sc["cam"], sc["obj"]], axis=1)
        uniq, counts = np.unique(pairs, axis=0, return_counts=True)
        assert uniq[counts == 2][:, 1].tolist() == [3]
    if name == "many_views_mixed":
        assert [i for i, w in enumerate(widths) if w == 9] == list(range(0, 66, 7)) and set(widths) == {6, 9}
        offs = np.asarray(sc["par"].camera_param_offsets)
        assert any(o // 32 != (o + 8) // 32 for o, w in zip(offs, widths) if w == 9)  # a nine-wide camera lies across a block boundary
    if name == "below_limit":
        assert widths == (6,) * 190 + (9,)
    if name == "obs_257":
        assert d["n_obs"] == 256 + 1  # one past a whole workgroup of k_unc_obs: its last wave has one live lane
    if name == "many_points":
        assert d["n_points"] > 256 * 256 + 256  # k_unc_d: 256 blocks of 256 threads, then a second trip of more than one block
        assert all(0 <= p < d["n_points"] for p in es.MANY_POINTS_SAMPLE)


# ---- the harnesses against the dense references --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(COVARIANCE_SCENES))
def test_covariance_harness_matches_the_pseudo_inverse(name):
    key = COVARIANCE_SCENES[name]
    figures = cn.check_against_pinv(harness_covariance(key), key)
    assert figures["lam8"] > 1e-6


@pytest.mark.parametrize("name", list(RELIABILITY_SCENES))
def test_reliability_harness_matches_the_dense_projector(name):
    key = RELIABILITY_SCENES[name]
    figures = rn.check_against_dense(harness_reliability(key), key)
    assert figures["lam8"] > 1e-6


# ---- MANY_POINTS ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [SMALL, MIXED33, ("ragged",)], ids=["small", "mixed33", "ragged"])
def test_block_sparse_restatement_is_the_bordered_formula(key):
    sc = cn.key_scene(key)
    J, cost = cn.robust_jacobian(sc)
    ncp = sc["par"].n_camera_params
    bc, bp = cn.bordered_blocks(J, cn.gauge_matrix(sc["par"], sc["x"]), ncp)
    sp = es.sparse_bordered_blocks(sc)
    figures = dict(key=key, camera=cn._rel(sp["cc"], bc), points=cn._rel_blocks(sp["pp"], bp))
    print(figures)
    assert figures["camera"] <= 1e-12 and figures["points"] <= 1e-12, figures
    assert sp["dof"] == cn.reference(key)["dof"] and abs(sp["cost"] - cost) <= 1e-14 * cost


def test_many_points_harness_matches_the_recorded_reference():
    es.check_many_points(harness_covariance(es.MANY_POINTS))


def test_recorded_reference_refuses_another_scene(monkeypatch):
    sc = dict(cn.key_scene(es.MANY_POINTS))
    sc["uv"] = sc["uv"].copy()
    sc["uv"][12345, 0] = np.nextafter(sc["uv"][12345, 0], np.inf)  # one bit of one observation
    assert es.scene_hash(sc) != es.scene_hash(cn.key_scene(es.MANY_POINTS))
    monkeypatch.setitem(cn._SCENES, es.MANY_POINTS, sc)
    with pytest.raises(AssertionError, match="recorded on another scene"):
        es.many_points_reference.__wrapped__()


# ---- the size limit ---------------------------------------------------------------------------------------------------------------------------
def test_over_limit_is_refused_by_both_harnesses():
    for call in (harness_covariance, harness_reliability):
        with pytest.raises(BackendError, match=re.escape("(code -4)")) as info:
            call(es.OVER_LIMIT)
        assert OVER_LIMIT_WORDS in str(info.value)
