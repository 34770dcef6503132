"""cba_parameter_covariance_constrained on the device against the float64 eigh pseudo-inverse of the oracle's J^T J (constraint rows in J, six
eigenvalues zeroed) under the tolerance rule of tests/test_uncertainty_constrained.py (ten times the disagreement of the two CPU formulations,
floor 1e-12; tests.covariance_constrained_native.check_against_pinv).  The scenes are those of the CPU tests and their references are shared:
four-point components with a zero centroid row, 12 points and 30 rows a component, 25 points and 73 rows, the mixed scene (points in no row, a
corner seen once, a camera blind to a component, a repeated observation), nine-wide cameras, a robust loss that scales constraint rows, and one
component of exactly COV_COMPONENT_CAP points."""
import re

import numpy as np
import pytest

from caliscope_amd import uncertainty
from caliscope_amd.exceptions import BackendError
from tests import covariance_constrained_native as ccn
from tests.test_uncertainty_constrained import SOFT_F_SCALE, check_seam, refusal_cases

pytestmark = pytest.mark.gpu

ATOMIC_SPREAD = 1e-9  # relative to the largest entry: what tests/test_uncertainty_gpu.py allows between two calls of the unconstrained call


def device_call(key, loss="linear", f_scale=1.0):
    return uncertainty.DeviceUncertainty().parameter_covariance_constrained(*ccn.call_arguments(ccn.key_scene(key)), loss=loss, f_scale=f_scale)


def _close(a, b, rel):
    ok = np.abs(a.cam_cov_full - b.cam_cov_full).max() <= rel * np.abs(b.cam_cov_full).max()
    return ok and (np.abs(a.point_cov - b.point_cov).max(axis=(1, 2)) <= rel * np.abs(b.point_cov).max(axis=(1, 2))).all()


@pytest.mark.parametrize("key,loss,f_scale", [
    (ccn.TWO_BY_TWO, "linear", 1.0), (ccn.DEFAULT, "linear", 1.0), (ccn.MANY_ROWS, "linear", 1.0), (ccn.MIXED, "linear", 1.0),
    (ccn.FREE_INTRINSICS, "linear", 1.0), (ccn.DEFAULT, "soft_l1", SOFT_F_SCALE), (ccn.CAP, "linear", 1.0),
], ids=["2x2 boards", "default boards", "5x5 boards 73 rows", "mixed", "free intrinsics", "soft_l1 on constraint rows", "one component at the cap"])
def test_device_call_matches_the_pseudo_inverse(key, loss, f_scale):
    res = device_call(key, loss, f_scale)
    ccn.check_against_pinv(res, key, loss, f_scale)
    assert np.isfinite(res.point_cov).all()


def test_device_agrees_with_the_host_build_on_the_mixed_scene():
    """Both meet the rule against the same reference, so they differ by at most twice its tolerance."""
    dev = device_call(ccn.MIXED)
    host = ccn.HarnessConstrainedUncertainty().parameter_covariance_constrained(*ccn.call_arguments(ccn.key_scene(ccn.MIXED)))
    ref = ccn.reference(ccn.MIXED)
    assert np.abs(dev.cam_cov_full - host.cam_cov_full).max() <= 2 * max(10 * ref["dis_c"], 1e-12) * np.abs(host.cam_cov_full).max()
    assert (np.abs(dev.point_cov - host.point_cov).max(axis=(1, 2)) <= 2 * max(10 * ref["dis_p"], 1e-12) * np.abs(host.point_cov).max(axis=(1, 2))).all()
    assert (dev.dof, dev.gauge_dim, dev.n_constraint_rows) == (host.dof, 6, host.n_constraint_rows)
    single = dev.point_cov[ccn.MIXED_SINGLE]
    assert np.isfinite(single).all() and np.linalg.eigvalsh(single).min() > 0  # the corner with one observation


def test_two_device_calls_agree_within_the_spread_of_their_atomics():
    assert _close(device_call(ccn.DEFAULT), device_call(ccn.DEFAULT), 10 * ATOMIC_SPREAD)


def test_without_rows_the_device_call_is_the_unconstrained_call():
    twelve = ccn.call_arguments(ccn.key_scene(ccn.DEFAULT))
    dev = uncertainty.DeviceUncertainty()
    plain = dev.parameter_covariance(*twelve[:8])
    empty = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4), dtype=np.int32), np.zeros(0), np.zeros(0))
    for res in (dev.parameter_covariance_constrained(*twelve[:8], *empty), dev.parameter_covariance_constrained(*twelve[:8], None, None, None, None),
                dev.parameter_covariance_constrained(*twelve[:11], np.zeros(len(twelve[11])))):
        assert (res.gauge_dim, res.n_constraint_rows, res.dof) == (7, 0, plain.dof)
        assert _close(res, plain, ATOMIC_SPREAD) and res.sigma0_sq == pytest.approx(plain.sigma0_sq, rel=1e-12)


@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0])
def test_host_checks_return_their_code_before_any_launch(case):
    _, args, code, words = case
    with pytest.raises(BackendError, match=re.escape(f"(code {code})")) as info:
        uncertainty.DeviceUncertainty().parameter_covariance_constrained(*args)
    assert words in str(info.value)


def test_deterministic_mode_is_refused_and_the_device_is_fine_afterwards(monkeypatch):
    monkeypatch.setenv("CBA_DETERMINISTIC", "1")
    with pytest.raises(BackendError, match=r"code -4.*CBA_DETERMINISTIC=1 with constraint rows"):
        device_call(ccn.TWO_BY_TWO)
    monkeypatch.delenv("CBA_DETERMINISTIC")
    assert np.isfinite(device_call(ccn.TWO_BY_TWO).cam_cov_full).all()


def test_seam_on_an_optimised_board_volume():
    from tests.constrained_scene import board_volume

    vol, _ = board_volume()
    vol = vol.optimize()
    assert vol.optimization_status.converged
    check_seam(vol, None, None)
