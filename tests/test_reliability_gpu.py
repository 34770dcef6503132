"""cba_observation_reliability on the device against the dense projector of the oracle's Jacobian, under the tolerance rule of
tests/test_reliability.py (ten times the disagreement of the two CPU formulations, floor 1e-12, absolute on R_oo; w relative within that
over r_j; reliability_native.check_against_dense).  The scenes: the fewest degrees of freedom the gauge allows, two, three, five, six,
nine and ten views per point (k_rel_point takes four observations per pass: one pass, and two and three passes with a partly filled
last one), six- and nine-wide cameras side by side, fisheye cameras, ncp = 33 (one past the Cholesky block), a repeated (camera, point)
pair, a robust loss with outliers.  References are computed once per scene and shared.  Measured on an MI355X (error of R_oo, error of
w times r_j, against the tolerance):

    LEAST    1.2e-14  4.7e-15  1e-12        FREE27   1.8e-13  9.1e-14  1.8e-12
    SMALL    4.0e-15  2.1e-15  1e-12        MIXED33  1.9e-13  9.6e-14  1.9e-12
    ragged   8.4e-15  4.2e-15  1e-12        WIDE9    1.4e-15  1.9e-15  1e-12
    ROBUST   9.9e-14  5.0e-14  1e-12        WIDE10   4.0e-14  2.0e-14  1e-12

On the 6 x 300 scene with 8 px added to u of row 10 / 777 / 1500 and solved by optimize(): |w| = 13.70 / 13.92 / 14.72 on the bumped row,
6.29 / 6.07 / 7.54 on the runner-up (same point); the clean volume loses 6 of 1800 observations to one pass at 0.1 %.

Also here: cba_parameter_covariance returns, with CBA_DETERMINISTIC=1, the bits it returned before its launches up to C were shared with
the new call (tests/golden/covariance_bits, written by tests/golden/make_covariance_bits_fixtures.py from the library of the commit before)."""
import re
from pathlib import Path

import numpy as np
import pytest

from caliscope_amd import reliability, uncertainty
from caliscope_amd.exceptions import BackendError
from tests import covariance_native as cn
from tests import reliability_native as rn
from tests.test_reliability import (BUMPED_ROWS, BUMP_PX, F_1PX, SCENE_IDS, SCENES, check_clean, check_detection, check_null_outputs, check_permuted,
                                    nulled, permuted_call)
from tests.test_uncertainty import LEAST, MIXED33, SMALL, _args, error_cases

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "covariance_bits"


def device_call(key, loss="linear", f_scale=1.0):
    return reliability.DeviceReliability().observation_reliability(*rn.scene_arguments(key), loss=loss, f_scale=f_scale)


@pytest.mark.parametrize("key,loss", SCENES, ids=SCENE_IDS)
def test_device_call_matches_the_dense_projector(key, loss):
    figures = rn.check_against_dense(device_call(key, loss, F_1PX), key, loss, F_1PX)
    assert figures["lam8"] > 1e-6


@pytest.mark.parametrize("deterministic", [True, False], ids=["fixed-order", "atomics"])
def test_permuted_rows_return_permuted_outputs(monkeypatch, deterministic):
    """The ragged scene (a repeated pair among its rows): bit-equal when the sums before C are formed in a fixed order, within the
    tolerance when they are formed with atomics."""
    monkeypatch.setenv("CBA_DETERMINISTIC", "1" if deterministic else "0")
    key = ("ragged",)
    plain, moved, perm = permuted_call(reliability.DeviceReliability().observation_reliability, key)
    check_permuted(plain, moved, perm, key, bitwise=deterministic)
    if deterministic:
        again = device_call(key)
        assert np.array_equal(again.redundancy, plain.redundancy) and np.array_equal(again.w, plain.w)


def test_null_outputs_in_every_combination(monkeypatch):
    from caliscope_amd import _lib

    monkeypatch.setenv("CBA_DETERMINISTIC", "1")  # (so that the outputs that are returned can be compared bit for bit)
    lib = _lib.bind(_lib.load(), reliability.RELIABILITY_SIGNATURES)
    args = reliability.check_covariance_arguments(*rn.scene_arguments(SMALL), "linear", 1.0)
    call = lambda d, o: lib.cba_observation_reliability(d, 0, o)  # noqa: E731
    full = check_null_outputs(lambda fields: reliability.run_reliability_call(nulled(call, fields), args, "device", lambda: _lib.last_error(lib)), exact=True)
    assert full.redundancy.any() and full.dof == rn.reference(SMALL)["dof"]


@pytest.mark.parametrize("case", error_cases(), ids=lambda c: c[0])
def test_host_checks_return_the_codes_of_the_covariance_call(case):
    _, args, code, words = case
    with pytest.raises(BackendError, match=re.escape(f"(code {code})")) as info:
        reliability.DeviceReliability().observation_reliability(*args)
    assert words in str(info.value)
    assert np.isfinite(device_call(LEAST).redundancy).all()  # the device is fine afterwards


def test_degenerate_scenes_return_the_numeric_error_not_nans():
    with pytest.raises(BackendError, match=r"code -6.*not positive definite beyond the gauge"):
        reliability.DeviceReliability().observation_reliability(*cn.planar_degenerate_scene())
    a = _args()
    rows = np.flatnonzero(a[6] == 3)
    a[5][rows] = a[5][rows[0]]  # every view of point 3 from one camera: one ray
    with pytest.raises(BackendError, match=r"code -6.*point 3"):
        reliability.DeviceReliability().observation_reliability(*a)
    with pytest.raises(BackendError, match="device 99"):
        reliability.DeviceReliability(99).observation_reliability(*_args())


def optimised_volume(bumped_row):
    from caliscope_amd.capture_volume import CaptureVolume
    from tests.helpers import small_problem

    sc, _, _ = small_problem(n_cams=6, n_points=300, k=6)
    uv = np.array(sc.image_coords, dtype=np.float64)
    if bumped_row is not None:
        uv[bumped_row, 0] += BUMP_PX
    return CaptureVolume.from_arrays(sc.cameras_init, sc.camera_indices, uv, sc.obj_indices, sc.points_init).optimize()


@pytest.mark.parametrize("row", BUMPED_ROWS)
def test_blunder_is_found_and_removed(row):
    vol = optimised_volume(row)
    rep = check_detection(vol, row)
    by_harness = vol.observation_reliability(_solver=rn.HarnessReliability())
    assert np.allclose(rep.w, by_harness.w, rtol=1e-6, atol=1e-9) and rep.dof == by_harness.dof
    assert rep.sigma0 == pytest.approx(np.sqrt(2.0 * vol.optimization_status.final_cost / rep.dof), rel=1e-9)


def test_clean_volume_keeps_its_points():
    check_clean(optimised_volume(None))


@pytest.mark.parametrize("name,key", [("small", SMALL), ("mixed33", MIXED33)])
def test_covariance_call_returns_the_bits_it_returned_before_the_refactor(monkeypatch, name, key):
    monkeypatch.setenv("CBA_DETERMINISTIC", "1")
    sc = cn.key_scene(key)
    res = uncertainty.DeviceUncertainty().parameter_covariance(*cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"]))
    with np.load(GOLDEN / f"{name}.npz") as gold:
        for field in ("cam_cov", "cam_cov_full", "point_cov"):
            assert np.array_equal(getattr(res, field), gold[field]), field
        assert res.sigma0_sq == float(gold["sigma0_sq"]) and res.dof == int(gold["dof"]) and res.cost == float(gold["cost"])
