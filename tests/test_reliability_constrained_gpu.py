"""cba_observation_reliability_constrained on the device against the dense projector of the oracle's J (constraint rows in J, six eigenvalues
zeroed) under the tolerance rule of tests/test_reliability_constrained.py (ten times the disagreement of the two CPU formulations, floor 1e-12, on
every R_oo and every constraint r_j; tests.reliability_constrained_native.check_against_dense).  The scenes are those of the CPU tests and their
references are shared: four-point components with zero-Jacobian centroid rows, five cameras (more than one trip of four entry groups), 25 points
and 73 rows, the mixed scene, nine-wide cameras, a robust loss on the constraint rows, one component at the cap, and 70 observations of one
(camera, point) pair."""
import re

import numpy as np
import pytest

from caliscope_amd import reliability
from caliscope_amd.exceptions import BackendError
from tests import covariance_constrained_native as ccn
from tests import reliability_constrained_native as rcn
from tests.test_reliability_constrained import (LINK_BUMP_M, SCENE_IDS, SCENES, check_image_blunder, check_link_blunder, check_mixed_scene, check_permutation,
                                                check_seam, check_zero_jacobian_row)
from tests.test_uncertainty_constrained import refusal_cases
from tests.test_uncertainty_constrained_gpu import ATOMIC_SPREAD

pytestmark = pytest.mark.gpu


def device_call(key, loss="linear", f_scale=1.0):
    return reliability.DeviceReliability().observation_reliability_constrained(*rcn.call_arguments(key), loss=loss, f_scale=f_scale)


@pytest.mark.parametrize("key,loss,f_scale", SCENES, ids=SCENE_IDS)
def test_device_call_matches_the_dense_projector(key, loss, f_scale):
    res = device_call(key, loss, f_scale)
    rcn.check_against_dense(res, key, loss, f_scale)
    if key == ccn.TWO_BY_TWO:
        check_zero_jacobian_row(res)
    if key == ccn.MIXED:
        check_mixed_scene(res)


def test_device_agrees_with_the_host_build_on_the_mixed_scene():
    """Both meet the rule against the same reference, so they differ by at most twice its tolerance."""
    dev = device_call(ccn.MIXED)
    host = rcn.HarnessConstrainedReliability().observation_reliability_constrained(*rcn.call_arguments(ccn.MIXED))
    tol = 2 * max(10 * rcn.reference(ccn.MIXED)["dis"], 1e-12)
    assert np.abs(dev.redundancy - host.redundancy).max() <= tol and np.abs(dev.constraint_redundancy - host.constraint_redundancy).max() <= tol
    assert (dev.dof, dev.gauge_dim, dev.n_uncontrolled, dev.n_constraints_uncontrolled) == (host.dof, 6, 0, 0)
    ref = rcn.reference(ccn.MIXED)  # (both match the oracle's residuals to rounding)
    assert (np.abs(dev.constraint_residual - host.constraint_residual) <= 2 * rcn.constraint_residual_tolerance(rcn.key_scene(ccn.MIXED), ref)).all()


def test_two_device_calls_agree_within_the_spread_of_their_atomics():
    """Behind C nothing is added across points or rows; C itself carries the spread of the atomics of the covariance call.  r is of order one."""
    a, b = device_call(ccn.DEFAULT), device_call(ccn.DEFAULT)
    assert np.abs(a.redundancy - b.redundancy).max() <= 10 * ATOMIC_SPREAD and np.abs(a.constraint_redundancy - b.constraint_redundancy).max() <= 10 * ATOMIC_SPREAD
    assert np.array_equal(a.residual, b.residual) and np.array_equal(a.constraint_residual, b.constraint_residual)


def test_permuting_the_rows_permutes_the_outputs():
    check_permutation(reliability.DeviceReliability().observation_reliability_constrained, max(10 * rcn.reference(ccn.MIXED)["dis"], 1e-12))


def test_without_rows_the_device_call_is_the_unconstrained_call():
    twelve = rcn.call_arguments(ccn.DEFAULT)
    dev = reliability.DeviceReliability()
    plain = dev.observation_reliability(*twelve[:8])
    empty = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4), dtype=np.int32), np.zeros(0), np.zeros(0))
    for res, n_con in ((dev.observation_reliability_constrained(*twelve[:8], *empty), 0), (dev.observation_reliability_constrained(*twelve[:8], None, None, None, None), 0),
                       (dev.observation_reliability_constrained(*twelve[:11], np.zeros(len(twelve[11]))), len(twelve[10]))):
        assert (res.gauge_dim, res.dof, res.n_uncontrolled, res.n_constraints_uncontrolled) == (7, plain.dof, plain.n_uncontrolled, 0)
        assert np.abs(res.redundancy - plain.redundancy).max() <= ATOMIC_SPREAD and res.sigma0_sq == pytest.approx(plain.sigma0_sq, rel=1e-12)
        assert np.array_equal(res.residual, plain.residual)
        for arr in (res.constraint_redundancy, res.constraint_w, res.constraint_residual):
            assert arr.shape == (n_con,) and np.isnan(arr).all()


def test_null_outputs_in_every_combination():
    """Every pointer of both structures may be NULL, and so may either structure: what is asked for is what a full call returns."""
    import ctypes as C

    from caliscope_amd import _lib
    from caliscope_amd.reliability import RELIABILITY_CONSTRAINED_SIGNATURES, RelConOut, RelOut
    from caliscope_amd.uncertainty import check_constraint_arguments, check_covariance_arguments, constraint_struct

    twelve = rcn.call_arguments(ccn.TWO_BY_TWO)
    full = device_call(ccn.TWO_BY_TWO)
    args = check_covariance_arguments(*twelve[:8], "linear", 1.0)
    con = check_constraint_arguments(*twelve[8:])
    struct = constraint_struct(con)
    desc = ccn._desc(args)
    lib = _lib.bind(_lib.load(), RELIABILITY_CONSTRAINED_SIGNATURES)
    n_obs, n_con = len(twelve[5]), len(twelve[10])
    names = ["redundancy", "w", "residual", "sigma0_sq", "dof", "cost", "n_uncontrolled"]
    con_names = ["redundancy", "w", "residual", "n_uncontrolled"]

    def run(asked, con_asked, null_out=False, null_con=False):
        arrays = dict(redundancy=np.full((n_obs, 3), 7.0), w=np.full((n_obs, 2), 7.0), residual=np.full((n_obs, 2), 7.0), sigma0_sq=np.full(1, 7.0),
                      dof=np.full(1, 7, dtype=np.int64), cost=np.full(1, 7.0), n_uncontrolled=np.full(1, 7, dtype=np.int64))
        con_arrays = dict(redundancy=np.full(n_con, 7.0), w=np.full(n_con, 7.0), residual=np.full(n_con, 7.0), n_uncontrolled=np.full(1, 7, dtype=np.int64))
        out = RelOut(**{n: _lib.ptr(arrays[n]) for n in asked})
        con_out = RelConOut(**{n: _lib.ptr(con_arrays[n]) for n in con_asked})
        rc = lib.cba_observation_reliability_constrained(C.byref(desc), C.byref(struct), 0, None if null_out else C.byref(out), None if null_con else C.byref(con_out))
        assert rc == 0, _lib.last_error(lib)
        got, con_got = (set() if null_out else set(asked)), (set() if null_con else set(con_asked))
        for n in names:  # what was not asked for is not touched
            assert n in got or (arrays[n] == 7).all(), (asked, n)
        for n in con_names:
            assert n in con_got or (con_arrays[n] == 7).all(), (con_asked, n)
        if "redundancy" in got:
            assert np.abs(arrays["redundancy"][:, 0] - full.redundancy[:, 0, 0]).max() <= 10 * ATOMIC_SPREAD
        if "w" in got:
            assert np.isfinite(arrays["w"]).all() and not (arrays["w"] == 7).all()
        if "residual" in got:
            assert np.array_equal(arrays["residual"], full.residual)
        if "dof" in got:
            assert arrays["dof"][0] == full.dof
        if "n_uncontrolled" in got:
            assert arrays["n_uncontrolled"][0] == 0
        if "redundancy" in con_got:
            assert np.abs(con_arrays["redundancy"] - full.constraint_redundancy).max() <= 10 * ATOMIC_SPREAD
        if "residual" in con_got:
            assert np.array_equal(con_arrays["residual"], full.constraint_residual)
        if "n_uncontrolled" in con_got:
            assert con_arrays["n_uncontrolled"][0] == 0

    for bits in range(1 << len(names)):  # every subset of cba_rel_out beside a full cba_rel_con_out
        run([n for i, n in enumerate(names) if bits >> i & 1], con_names)
    for bits in range(1 << len(con_names)):  # every subset of cba_rel_con_out beside a full cba_rel_out
        run(names, [n for i, n in enumerate(con_names) if bits >> i & 1])
    run(names, con_names, null_out=True)
    run(names, con_names, null_con=True)
    run(names, con_names, null_out=True, null_con=True)


@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0])
def test_host_checks_return_their_code_before_any_launch(case):
    _, args, code, words = case
    with pytest.raises(BackendError, match=re.escape(f"(code {code})")) as info:
        reliability.DeviceReliability().observation_reliability_constrained(*args)
    assert "cba_observation_reliability_constrained: " + words in str(info.value)


def test_deterministic_mode_is_refused_and_the_device_is_fine_afterwards(monkeypatch):
    monkeypatch.setenv("CBA_DETERMINISTIC", "1")
    with pytest.raises(BackendError, match=r"code -4.*CBA_DETERMINISTIC=1 with constraint rows"):
        device_call(ccn.TWO_BY_TWO)
    monkeypatch.delenv("CBA_DETERMINISTIC")
    assert np.isfinite(device_call(ccn.TWO_BY_TWO).redundancy).all()


def test_seam_on_an_optimised_board_volume():
    from tests.constrained_scene import board_volume

    vol, _ = board_volume()
    vol = vol.optimize()
    assert vol.optimization_status.converged
    check_seam(vol, None)


def test_image_blunder_is_found_and_removed_with_the_constraints_in_the_adjustment():
    check_image_blunder(lambda v: v.optimize(), None)


def test_wrong_link_distance_is_the_flagged_constraint():
    check_link_blunder(lambda v: v.optimize(), None, LINK_BUMP_M)
