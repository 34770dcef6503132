"""cba_parameter_covariance and cba_observation_reliability on the device at the edges of their loops, on the scenes of
tests/covariance_edge_scenes.py (tests/test_covariance_edges.py shows on the CPU that each scene is what its name says and fit to test
with).  The rule is that of tests/test_uncertainty.py and tests/test_reliability.py, unchanged: the code under test within ten times the
disagreement of two CPU formulations of the reference, floor 1e-12; the disagreement itself at most 1e-8.  What each scene runs:

    MANY_VIEWS_RAGGED  64, 65 and 66 rows of a point: the second trip of k_unc_point_cov's `a += COV_POINT_THREADS` (the E term) and of
                       k_rel_point's finishing loop, 17 passes of its camera part with one live group in the last; two views; a repeated
                       (camera, point) pair (k_unc_rows under fixed order); ncp = 390, 13 blocks, the last of six rows
    MANY_VIEWS_MIXED   nine-wide cameras across block boundaries, ncp = 426, 14 blocks, the last of ten rows
    LIMIT_SIX / _NINE  ncp = 1152 = COV_MAX_NCP: k_unc_assemble, the blocked factorisation, k_unc_pivots and k_unc_ttt on 36 whole blocks
    BELOW_LIMIT        ncp = 1149: 36 blocks, the last of 29 rows
    OVER_LIMIT         ncp = 1158: refused by name, by both calls, before any launch
    OBS_256 / OBS_257  k_unc_obs on one whole workgroup, and on a second one whose only wave has one live lane in its cost sum
    POINTS_256 / _257  k_unc_d on one block and on two
    MANY_POINTS        65 793 points: the second trip of k_unc_d's grid-stride loop, k_unc_obs's cost over 771 workgroups; under fixed
                       order k_unc_fixed_sums over 1024 wave rows and k_unc_cam_sums over 65 793 observations of a camera.  Reference:
                       the recorded blocks of tests/golden/covariance_many_points.npz and the block-sparse bordered formula
    fixed order        (CBA_DETERMINISTIC=1) k_unc_cam_sums, k_unc_rows and k_unc_fixed_sums against the pseudo-inverse, not only against
                       bits the device produced once: the ragged scene, SIX (300 observations of a camera: five lane trips), MIXED33,
                       ncp = 99, MANY_VIEWS_RAGGED, LIMIT_SIX and MANY_POINTS; the same bytes from two calls; within both tolerances of
                       the atomics path

References are computed once per scene and shared (covariance_native.reference, reliability_native.reference,
covariance_edge_scenes.many_points_reference); a device result that two tests look at is computed once too.

Measured on an MI355X: error of the camera block and its tolerance, error of the point blocks and their tolerance (ten times the CPU
disagreement measured on the same machine, floor 1e-12), the larger of the two ratios.  On the scenes whose tolerance is above the floor
the pseudo-inverse is the less exact of the two CPU formulations and the device follows the bordered formula, so the error is a tenth of
the tolerance there whatever the device does in the last bits; a dropped term shows as 1e-4 and more (mutation runs of this file).

    atomics path
    MANY_VIEWS_RAGGED  5.6e-14  5.6e-13   9.1e-13  9.3e-12   0.10
    MANY_VIEWS_MIXED   7.0e-12  6.9e-11   2.6e-12  2.6e-11   0.10
    LIMIT_SIX          9.5e-15  1e-12     7.0e-15  1e-12     0.01
    LIMIT_NINE         2.0e-11  2.0e-10   8.2e-12  8.3e-11   0.10
    BELOW_LIMIT        3.3e-13  3.1e-12   1.7e-13  1.7e-12   0.10
    OBS_256            8.5e-15  1e-12     5.9e-15  1e-12     0.01
    OBS_257            1.5e-14  1e-12     5.9e-15  1e-12     0.02
    POINTS_256         1.2e-14  1e-12     2.7e-14  1e-12     0.03
    POINTS_257         4.3e-15  1e-12     6.0e-15  1e-12     0.01
    MANY_POINTS        3.8e-14  1e-12     6.3e-15  1e-12     0.04   (every other point against the restatement 7.5e-15; cost 4.5e-15)
    fixed order                                                      and its difference to the atomics path (camera, points)
    ragged             2.6e-14  1e-12     1.2e-14  1e-12     0.03    1.2e-15  3.3e-16
    SIX                2.7e-14  1e-12     5.1e-15  1e-12     0.03    2.3e-15  6.6e-16
    MIXED33            2.4e-12  2.3e-11   4.8e-13  4.8e-12   0.10    8.9e-14  2.9e-15
    ncp = 99           1.8e-11  1.8e-10   1.2e-12  1.2e-11   0.10    3.7e-14  6.9e-15
    MANY_VIEWS_RAGGED  5.6e-14  5.6e-13   9.3e-13  9.3e-12   0.10    1.0e-15  1.7e-14
    LIMIT_SIX          8.3e-15  1e-12     7.6e-15  1e-12     0.01    6.1e-15  3.3e-15
    MANY_POINTS        3.4e-14  1e-12     6.0e-15  1e-12     0.03    4.7e-14  1.2e-15   (every other point 6.6e-15; cost 3.6e-15)

    reliability: error of R_oo, error of w times r_j, tolerance
    REL_VIEWS          1.9e-15  9.7e-16  1e-12
    REL_VIEWS_RAGGED   3.0e-13  1.5e-13  3.0e-12      (permuted rows under fixed order: no bit differs)
    OBS_256            2.2e-15  1.6e-15  1e-12
    OBS_257            1.1e-15  1.6e-15  1e-12

No test of this file takes more than 1.2 s on the device (MANY_POINTS, most of it the block-sparse restatement); the file takes 5 s.
"""
import re

import numpy as np
import pytest

from caliscope_amd import reliability, uncertainty
from caliscope_amd.exceptions import BackendError
from tests import covariance_edge_scenes as es
from tests import covariance_native as cn
from tests import reliability_native as rn
from tests.dense_solve_cases import widths
from tests.test_covariance_edges import COVARIANCE_SCENES, OVER_LIMIT_WORDS, RELIABILITY_SCENES
from tests.test_reliability import check_permuted, permuted_call
from tests.test_uncertainty import LEAST, MIXED33, SIX

pytestmark = pytest.mark.gpu

ATOMICS_SCENES = {name: key for name, key in COVARIANCE_SCENES.items() if name != "many_views"}  # (its ragged variant runs every loop it runs)
FIXED_ORDER_SCENES = {"ragged": ("ragged",), "six": SIX, "mixed33": MIXED33, "free99": ("wide", widths(99), False),
                      "many_views_ragged": es.MANY_VIEWS_RAGGED, "limit_six": es.LIMIT_SIX}
_RESULTS = {}


def device_covariance(monkeypatch, key, fixed_order=False, fresh=False):
    """The device result of a scene on one of the two paths; computed once per (scene, path) unless ``fresh``."""
    monkeypatch.setenv("CBA_DETERMINISTIC", "1" if fixed_order else "0")
    if fresh or (key, fixed_order) not in _RESULTS:
        sc = cn.key_scene(key)
        res = uncertainty.DeviceUncertainty().parameter_covariance(*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]))
        if fresh:
            return res
        _RESULTS[(key, fixed_order)] = res
    return _RESULTS[(key, fixed_order)]


def device_reliability(key):
    return reliability.DeviceReliability().observation_reliability(*rn.scene_arguments(key))


def check_named_points(result, key, points):
    """The blocks of single points against the pseudo-inverse under the rule, each named in the message when it fails."""
    ref = cn.reference(key)
    tol = max(10.0 * ref["dis_p"], 1e-12)
    for p, what in points:
        want = ref["sigma0_sq"] * ref["pp"][p]
        err = float(np.max(np.abs(result.point_cov[p] - want)) / np.max(np.abs(want)))
        assert err <= tol, f"point {p} ({what}): its 3 x 3 block is {err:.3e} off the pseudo-inverse, tolerance {tol:.3e}"


def difference_of_the_paths(a, b, cc, pp):
    """The difference of two results in the norm of the rule: relative to the block-wise max-norm of the reference (cc, pp)."""
    return dict(camera=float(np.max(np.abs(a.cam_cov_full - b.cam_cov_full)) / np.max(np.abs(cc))),
                points=float(np.max(np.max(np.abs(a.point_cov - b.point_cov), axis=(1, 2)) / np.max(np.abs(pp), axis=(1, 2)))))


# ---- the atomics path ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ATOMICS_SCENES))
def test_atomics_path_matches_the_pseudo_inverse(monkeypatch, name):
    key = ATOMICS_SCENES[name]
    result = device_covariance(monkeypatch, key)
    if key == es.MANY_VIEWS_RAGGED:
        check_named_points(result, key, ((0, "64 views"), (1, "65 views"), (3, "66 rows, one (camera, point) pair twice"), (2, "two views")))
    figures = cn.check_against_pinv(result, key)
    assert figures["lam8"] > 1e-6


def test_many_points_match_the_recorded_reference(monkeypatch):
    ref = es.many_points_reference()
    result = device_covariance(monkeypatch, es.MANY_POINTS)
    es.check_many_points(result, path="atomics")
    assert result.dof == ref["dof"] and abs(result.cost - ref["cost"]) <= 1e-12 * ref["cost"]  # k_unc_obs's sum over 771 workgroups


# ---- the fixed-order path against a reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXED_ORDER_SCENES))
def test_fixed_order_path_matches_the_pseudo_inverse_and_the_atomics_path(monkeypatch, name):
    key = FIXED_ORDER_SCENES[name]
    fixed = device_covariance(monkeypatch, key, fixed_order=True)
    if key == es.MANY_VIEWS_RAGGED:
        check_named_points(fixed, key, ((0, "64 views"), (1, "65 views"), (3, "66 rows, one (camera, point) pair twice"), (2, "two views")))
    figures = cn.check_against_pinv(fixed, key)
    assert figures["lam8"] > 1e-6
    atomics = device_covariance(monkeypatch, key)
    ref = cn.reference(key)
    tol_c, tol_p = max(10.0 * ref["dis_c"], 1e-12), max(10.0 * ref["dis_p"], 1e-12)
    between = dict(name=name, **difference_of_the_paths(fixed, atomics, ref["sigma0_sq"] * ref["cc"], ref["sigma0_sq"] * ref["pp"]))
    print(between)
    assert between["camera"] <= 2.0 * tol_c and between["points"] <= 2.0 * tol_p, between  # each path is within its tolerance of one reference
    assert fixed.dof == atomics.dof and abs(fixed.cost - atomics.cost) <= 2e-12 * ref["cost"]


def test_fixed_order_many_points_match_the_recorded_reference(monkeypatch):
    """d_rows = 1024 for k_unc_fixed_sums; every camera has 65 793 observations for k_unc_cam_sums."""
    ref = es.many_points_reference()
    fixed = device_covariance(monkeypatch, es.MANY_POINTS, fixed_order=True)
    figures = es.check_many_points(fixed, path="fixed order")
    atomics = device_covariance(monkeypatch, es.MANY_POINTS)
    s2 = ref["sigma0_sq"]
    tol_c, tol_p = max(10.0 * figures["dis_c"], 1e-12), max(10.0 * figures["dis_p"], 1e-12)
    between = difference_of_the_paths(fixed, atomics, s2 * ref["bc"], s2 * ref["bp"])
    print(between)
    assert between["camera"] <= 2.0 * tol_c and between["points"] <= 2.0 * tol_p, between
    assert fixed.dof == atomics.dof and abs(fixed.cost - atomics.cost) <= 2e-12 * ref["cost"]


@pytest.mark.parametrize("name", ["ragged", "many_views_ragged", "many_points"])
def test_fixed_order_returns_the_same_bytes_twice(monkeypatch, name):
    key = dict(FIXED_ORDER_SCENES, many_points=es.MANY_POINTS)[name]
    first = device_covariance(monkeypatch, key, fixed_order=True)
    again = device_covariance(monkeypatch, key, fixed_order=True, fresh=True)
    for field in ("cam_cov_full", "point_cov"):
        assert getattr(first, field).tobytes() == getattr(again, field).tobytes(), field
    assert first.cost == again.cost and first.sigma0_sq == again.sigma0_sq and first.dof == again.dof


# ---- the reliability call -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RELIABILITY_SCENES))
def test_reliability_matches_the_dense_projector(monkeypatch, name):
    monkeypatch.setenv("CBA_DETERMINISTIC", "0")
    key = RELIABILITY_SCENES[name]
    figures = rn.check_against_dense(device_reliability(key), key)
    assert figures["lam8"] > 1e-6


def test_reliability_of_permuted_rows_is_permuted_bit_for_bit_under_fixed_order(monkeypatch):
    """As tests/test_reliability_gpu.py on the ragged scene, with 64, 65 and 66 rows of a point."""
    monkeypatch.setenv("CBA_DETERMINISTIC", "1")
    key = es.REL_VIEWS_RAGGED
    plain, moved, perm = permuted_call(reliability.DeviceReliability().observation_reliability, key)
    check_permuted(plain, moved, perm, key, bitwise=True)
    rn.check_against_dense(plain, key)


# ---- the size limit ---------------------------------------------------------------------------------------------------------------------------------
def test_over_limit_is_refused_by_both_device_calls(monkeypatch):
    monkeypatch.setenv("CBA_DETERMINISTIC", "0")
    sc = cn.key_scene(es.OVER_LIMIT)
    args = cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"])
    for call in (uncertainty.DeviceUncertainty().parameter_covariance, reliability.DeviceReliability().observation_reliability):
        with pytest.raises(BackendError, match=re.escape("(code -4)")) as info:
            call(*args)
        assert OVER_LIMIT_WORDS in str(info.value)
    assert np.isfinite(device_covariance(monkeypatch, LEAST, fresh=True).cam_cov_full).all()  # the device is fine afterwards
    assert np.isfinite(device_reliability(LEAST).redundancy).all()
