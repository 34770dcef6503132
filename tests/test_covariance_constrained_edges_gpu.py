"""cba_parameter_covariance_constrained and cba_observation_reliability_constrained on the device at the edges of the loops of their five
kernels, on the scenes of tests/covariance_constrained_edge_scenes.py (tests/test_covariance_constrained_edges.py shows on the CPU that
each scene is what its name says and fit to test with).  The rule is that of tests/test_uncertainty_constrained.py and
tests/test_reliability_constrained.py, unchanged: the code under test within ten times the disagreement of two CPU formulations of the
reference, floor 1e-12; the disagreement itself at most 1e-8; no row left out.  What each scene runs that the scenes of the feature tests
(three to five cameras of one width a component, components of one size and at least four points, at most 219 rows, contiguous labels) do not:

    NINE_MIXED             nine cameras on three components and eight on one: the second trip of k_rel_con_rows (17 and 8 live lanes), entry
                           trips of 4 + 4 + 1 and 4 + 4 in k_rel_con_point, 81 pairs (and 64: one whole trip) in k_unc_point_cov on entries;
                           widths 9 6 6 9 6 6 9 6 6 inside every component: np != np_b in step 4 of k_unc_component (the skip test, the
                           np x G update of B, the Yc store), the binary search and rel_row_times_y of k_rel_con_point and the r >= np skip of
                           k_rel_con_rows at offsets 0 9 15 21 30 ...; camera 4 sees one point of a four-point component; vstride from the
                           widest component beside a narrower one
    NINE_MIXED_RELABELLED  the components among each other and among the free points: pts[], row_loc, obs_loc, entry_start[pts[i / 3]],
                           free_list and con_list
    SIXTY_FIVE             65 entries of a point: the second trip of k_unc_point_cov's `a` loop with one live lane, 4225 pairs; 17 entry trips
                           of k_rel_con_point, one group in the last, and 16 whole ones on the component camera 64 is blind to; ten trips of
                           k_rel_con_rows; 65 cameras in step 4 of k_unc_component (ncp = 390)
    STICKS_257             257 components of two points (n = 6) and one row: a second workgroup of k_unc_con_rows with one live lane in its
                           cost sum, more workgroups of k_unc_component than compute units, no free point
    STICKS_256             the caller's last row has weight zero: one whole workgroup of rows, two free points through the list, NaN in the
                           caller's row 256 and nowhere else
    SIZES                  components of 54 (the cap), 4, 2 and 2 points in one launch: the dynamic LDS sized for max_m = 54, laid out by
                           each workgroup from its own m
    SIZES_OVER_CAP         55 points in a component: refused by name, by both calls, before any launch

References and host results are computed once per scene and shared; so is every device result.

Measured on an MI355X.  Covariance: error of the camera block and its tolerance, error of the point blocks and their tolerance (ten times
the CPU disagreement measured on the same machine, floor 1e-12), the larger of the two ratios.  Where the tolerance is above the floor the
pseudo-inverse is the less exact of the two CPU formulations and the device follows the bordered formula, so the error is a tenth of the
tolerance whatever the device does in the last bits; against the host build, which follows the same formula, the device is within 4e-14.

    NINE_MIXED             5.0e-12  5.0e-11   1.7e-12  1.7e-11   0.10
    NINE_MIXED_RELABELLED  6.5e-12  6.5e-11   6.7e-13  6.7e-12   0.10
    SIXTY_FIVE             1.9e-14  1e-12     3.6e-14  1e-12     0.04
    STICKS_257             3.5e-14  1e-12     5.2e-14  1e-12     0.05
    STICKS_256             6.5e-15  1e-12     4.8e-14  1e-12     0.05
    SIZES                  4.6e-15  1e-12     6.4e-15  1e-12     0.01

    reliability: error of R_oo, of the constraint r_j, of w times r_j (observations, rows), tolerance
    NINE_MIXED             1.0e-12  4.7e-15   5.0e-13  2.3e-15   1.0e-11
    NINE_MIXED_RELABELLED  1.2e-12  6.4e-15   6.0e-13  3.1e-15   1.2e-11
    SIXTY_FIVE             2.6e-15  1.5e-14   9.1e-16  7.7e-15   1e-12
    STICKS_257             3.5e-14  2.2e-15   1.7e-14  1.4e-15   1e-12
    STICKS_256             4.0e-14  3.2e-15   2.0e-14  1.9e-15   1e-12
    SIZES                  1.1e-15  1.0e-15   1.8e-15  1.3e-15   1e-12

    device against the host build: camera block, point blocks, R_oo, constraint r_j (tolerance: twice the above)
    NINE_MIXED             6.8e-15  2.6e-15   1.6e-14  4.4e-16
    NINE_MIXED_RELABELLED  4.0e-14  6.0e-15   1.5e-14  6.7e-16
    SIXTY_FIVE             3.9e-15  8.8e-15   1.0e-15  6.7e-16
    STICKS_257             1.7e-15  2.1e-15   1.4e-15  5.6e-16
    STICKS_256             1.3e-15  2.1e-15   1.4e-15  5.6e-16
    SIZES                  9.3e-16  2.3e-15   5.6e-16  8.9e-16
    relabelled against plain, renamed: 3.4e-14 (tolerance 1.1e-10), 5.5e-15 (2.4e-11), 1.1e-14 and 3.3e-16 (2.2e-11); the residuals bit-equal

No test of this file takes more than 2.6 s on the device (the first one to ask for NINE_MIXED's host results compiles a harness); the file takes 5.4 s.

Mutation runs of this file (scratch builds, one arithmetic term changed each, never an index, a bound, a barrier or a launch size; the library
rebuilt, this file run once, then tests/test_uncertainty_constrained_gpu.py and tests/test_reliability_constrained_gpu.py once: 45 tests).
"Fails" lists the scenes whose tests of this file fail; the first message names the point or row given here.

    1. k_rel_con_rows adds 0 to acc where it >= 64                 fails reliability and host agreement on NINE_MIXED, _RELABELLED, SIXTY_FIVE
                                                                   (constraint row 0: r_j 4.7e-3 off; 0.17 on SIXTY_FIVE); the earlier files pass
    2. k_unc_point_cov skips the pair term where it >= 64          fails covariance and host agreement on NINE_MIXED, _RELABELLED, SIXTY_FIVE
                                                                   (point 0: 8.4e-3 off; 0.23 on SIXTY_FIVE); the earlier files pass
    3. k_unc_component step 4 adds 0 to the Schur block where      fails covariance, reliability and host agreement on NINE_MIXED and _RELABELLED
       c >= np (np where np_b belongs)                             (point 0: 1.8e-3 off, its R_oo 1.5e-4); the earlier files pass
       ... where c >= 6                                            both calls refuse NINE_MIXED and _RELABELLED (code -6, a pivot not safely positive): the
                                                                   same six tests and the relabelling test fail; so do the two FREE_INTRINSICS
                                                                   tests of the earlier files (nine-wide cameras lose columns there too)
    4. k_unc_con_rows forces rho to 0 in workgroup 1               fails covariance, reliability and host agreement on STICKS_257 (point 0: 2.3e-5
                                                                   off through sigma0^2; the cost of the reliability call); the earlier files pass
    5. k_unc_component stores Yc as 0 for the last camera of a     fails covariance, reliability and host agreement on NINE_MIXED, _RELABELLED and
       component where nc > 5                                      SIXTY_FIVE (point 0: 2.8e-3 off, its R_oo 4.3e-4); the earlier files pass
    6. k_rel_con_point drops the Q terms of entries e >= 8         fails reliability and host agreement on NINE_MIXED, _RELABELLED, SIXTY_FIVE
                                                                   (observation 0 of point 0: R_oo 5.5e-4 off); the earlier files pass
    7. k_unc_component step 4 adds 0 to B where r >= 6             fails covariance and host agreement on NINE_MIXED and _RELABELLED (point 0: 2.4e-3
                                                                   off); the FREE_INTRINSICS covariance test of the earlier files fails too
"""
import functools
import re

import numpy as np
import pytest

from caliscope_amd import reliability, uncertainty
from caliscope_amd.exceptions import BackendError
from tests import covariance_constrained_edge_scenes as es
from tests import covariance_constrained_native as ccn
from tests import reliability_constrained_native as rcn
from tests.test_covariance_constrained_edges import (OVER_CAP_WORDS, REFERENCE_OF, SCENES, check_covariance, check_named, check_relabelling, check_reliability,
                                                     harness_covariance, harness_reliability, kept_rows)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def atomics_path(monkeypatch):
    """Fixed order is refused with constraint rows: these tests run without it whatever the environment says."""
    monkeypatch.delenv("CBA_DETERMINISTIC", raising=False)


@functools.cache
def device_covariance(key):
    return uncertainty.DeviceUncertainty().parameter_covariance_constrained(*ccn.call_arguments(ccn.key_scene(key)))


@functools.cache
def device_reliability(key):
    return reliability.DeviceReliability().observation_reliability_constrained(*rcn.call_arguments(key))


host_covariance = functools.cache(harness_covariance)
host_reliability = functools.cache(harness_reliability)


# ---- both calls against the dense references ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_covariance_matches_the_pseudo_inverse(name):
    key = SCENES[name]
    result = device_covariance(key)
    check_named(name, cov=result)
    figures = check_covariance(result, key)
    assert figures["lam7"] > 1e-7
    assert np.isfinite(result.point_cov).all() and np.isfinite(result.cam_cov_full).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_reliability_matches_the_dense_projector(name):
    key = SCENES[name]
    result = device_reliability(key)
    check_named(name, rel=result)
    figures = check_reliability(result, key)  # (no row is left out)
    assert figures["lam7"] > 1e-7


# ---- against the host build ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_device_agrees_with_the_host_build(name):
    """Both meet the rule against the same reference, so they differ by at most twice its tolerance."""
    key = SCENES[name]
    ref_key = REFERENCE_OF.get(key, key)
    dev, host, ref = device_covariance(key), host_covariance(key), ccn.reference(ref_key)
    tol_c, tol_p = 2 * max(10 * ref["dis_c"], 1e-12), 2 * max(10 * ref["dis_p"], 1e-12)
    err_c = float(np.abs(dev.cam_cov_full - host.cam_cov_full).max() / np.abs(host.cam_cov_full).max())
    err_p = np.abs(dev.point_cov - host.point_cov).max(axis=(1, 2)) / np.abs(host.point_cov).max(axis=(1, 2))
    assert err_c <= tol_c, f"{name}: the camera block is {err_c:.3e} off the host build, tolerance {tol_c:.3e}"
    worst = int(np.argmax(err_p))
    assert err_p[worst] <= tol_p, f"{name}: point {worst}: its block is {err_p[worst]:.3e} off the host build, tolerance {tol_p:.3e}"
    assert (dev.dof, dev.gauge_dim, dev.n_constraint_rows) == (host.dof, 6, host.n_constraint_rows)
    dev, host, ref = device_reliability(key), host_reliability(key), rcn.reference(ref_key)
    if key in REFERENCE_OF:
        dev, host = kept_rows(dev, key), kept_rows(host, key)
    tol = 2 * max(10 * ref["dis"], 1e-12)
    err_R, err_rc = np.abs(dev.redundancy - host.redundancy).max(axis=(1, 2)), np.abs(dev.constraint_redundancy - host.constraint_redundancy)
    worst = int(np.argmax(err_R))
    assert err_R[worst] <= tol, f"{name}: observation {worst}: its R_oo is {err_R[worst]:.3e} off the host build, tolerance {tol:.3e}"
    worst = int(np.argmax(err_rc))
    assert err_rc[worst] <= tol, f"{name}: constraint row {worst}: its redundancy number is {err_rc[worst]:.3e} off the host build, tolerance {tol:.3e}"
    assert (dev.dof, dev.gauge_dim, dev.n_uncontrolled, dev.n_constraints_uncontrolled) == (host.dof, 6, 0, 0)
    assert (np.abs(dev.constraint_residual - host.constraint_residual) <= 2 * rcn.constraint_residual_tolerance(rcn.key_scene(ref_key), ref)).all()
    print(dict(name=name, err_c=err_c, tol_c=tol_c, err_p=float(err_p.max()), tol_p=tol_p, err_R=float(err_R.max()), err_rc=float(err_rc.max()), tol=tol))


# ---- what single scenes are for --------------------------------------------------------------------------------------------------------------------
def test_relabelling_the_points_renames_the_outputs():
    check_relabelling(device_covariance(es.NINE_MIXED), device_covariance(es.NINE_MIXED_RELABELLED), device_reliability(es.NINE_MIXED),
                      device_reliability(es.NINE_MIXED_RELABELLED))


def test_sticks_256_leaves_the_callers_last_row_nan():
    res = device_reliability(es.STICKS_256)
    for name in ("constraint_redundancy", "constraint_w", "constraint_residual"):
        arr = getattr(res, name)
        assert arr.shape == (257,) and np.isnan(arr[256]), name
        assert np.isfinite(arr[:256]).all(), f"{name}: rows {np.flatnonzero(~np.isfinite(arr[:256])).tolist()} of the 256 that take part are not finite"
    assert res.n_constraints_uncontrolled == 0 and res.dof == device_reliability(es.STICKS_257).dof - 1
    cov = device_covariance(es.STICKS_256)
    assert cov.n_constraint_rows == 256 and cov.dof == device_covariance(es.STICKS_257).dof - 1


def test_a_component_over_the_cap_is_refused_by_both_device_calls_and_the_next_call_succeeds():
    cov = uncertainty.DeviceUncertainty().parameter_covariance_constrained
    rel = reliability.DeviceReliability().observation_reliability_constrained
    for call in (cov, rel):
        with pytest.raises(BackendError, match=re.escape("(code -4)")) as info:
            call(*rcn.call_arguments(es.SIZES_OVER_CAP))
        assert OVER_CAP_WORDS in str(info.value)
    again = cov(*rcn.call_arguments(es.SIZES))
    first = device_covariance(es.SIZES)
    assert np.isfinite(again.cam_cov_full).all() and np.isfinite(again.point_cov).all() and (again.dof, again.n_constraint_rows) == (first.dof, 165)
    assert np.isfinite(rel(*rcn.call_arguments(es.SIZES)).redundancy).all()
