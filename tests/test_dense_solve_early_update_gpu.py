"""The early panel update of the blocked dense solve (k_chol_step<true>, csrc/chol_schedule.h) against the parent's schedule (CBA_CHOL_EARLY=0,
k_chol_step<false>): the same sums in the same order, so everything is compared TO THE BIT — the flag of the factorisation, the reduced system and
the camera part of the step.

Every ncp of tests/dense_solve_cases.SWEEP takes the blocked route (CBA_SMALL_SOLVE=0 up to 96), at lam = 1e-3 and 1e-10.  What the shapes reach:
12 and 27 are one block (no early update); 33, 36 and 63 update only the rhs row early; 66 and 96 are the first to hand a former trailing block
to a panel workgroup; 99 and above are the first with the double update P_k-1, P_k; 351 is 11 blocks with a 31-row tail.  Handles are
deterministic (fixed-order sums), without which two handles do not even form the same system.

Further: one deterministic handle repeated to the bit; the rig with an unobserved camera at lam = 0 (ncp 66), whose exactly-zero pivot must raise
the same flag on both schedules; and cba_parameter_covariance (what parameter_uncertainty() calls, which factors through the same
enqueue_chol_factor) on a wide-field scene of four blocks: bit-equal camera covariances, with the call's sums in fixed order too
(CBA_DETERMINISTIC=1), which are themselves held to the pseudo-inverse.
"""
from __future__ import annotations

import numpy as np
import pytest

from caliscope_amd.engine import BAProblem
from tests import dense_solve_cases as D

pytestmark = pytest.mark.gpu

SMALL_SOLVE = 64  # cba_info.build_camg bit 6: the dense camera system is solved by k_small_solve
SCHEDULES = {"early": None, "parent": "0"}  # value of CBA_CHOL_EARLY (None: unset, the default)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension


def _handle(sc, monkeypatch, schedule):
    """A deterministic handle on the rig ``sc`` on the blocked route with ``schedule``, linearised at the rig's initial point."""
    from caliscope_amd.hip_engine import HipEngine

    with monkeypatch.context() as m:
        m.delenv("CBA_CHOL_EARLY", raising=False)
        if SCHEDULES[schedule] is not None:
            m.setenv("CBA_CHOL_EARLY", SCHEDULES[schedule])
        if sc["par"].n_camera_params <= D.SMALL_N:
            m.setenv("CBA_SMALL_SOLVE", "0")
        hip = HipEngine(BAProblem(sc["par"], sc["cam"], sc["uv"], sc["obj"]), deterministic=True)
    assert not hip.info()["build_camg"] & SMALL_SOLVE
    hip.begin(sc["x0"])
    hip.linearize()
    return hip


def _step(hip, lam):
    ok = hip.newton_step(lam).ok
    S, rhs = hip.reduced_system()
    return ok, S.tobytes(), rhs.tobytes(), hip.get_vector(3)[: len(rhs)].copy()


@pytest.mark.parametrize("ncp", sorted(D.SWEEP))
def test_both_schedules_agree_to_the_bit(ncp, monkeypatch):
    got = {}
    for schedule in SCHEDULES:
        hip = _handle(D.rig(ncp), monkeypatch, schedule)
        got[schedule] = [_step(hip, lam) for lam in (1e-3, 1e-10)]
        hip.close()
    for lam, e, p in zip((1e-3, 1e-10), got["early"], got["parent"]):
        assert e[0] and p[0], (ncp, lam, e[0], p[0])
        assert e[1] == p[1] and e[2] == p[2], (ncp, lam, "the reduced systems differ")
        assert np.all(np.isfinite(e[3]))
        differ = np.flatnonzero(e[3] != p[3])
        print(f"ncp {ncp} lam {lam:g}: {len(differ)} of {ncp} step entries differ, max |s| {np.abs(p[3]).max():.3e}")
        assert e[3].tobytes() == p[3].tobytes(), (ncp, lam, differ[:8], float(np.abs(e[3] - p[3]).max()))


def test_one_handle_repeats_to_the_bit(monkeypatch):
    hip = _handle(D.rig(129), monkeypatch, "early")
    first = _step(hip, 1e-3)
    for _ in range(2):
        again = _step(hip, 1e-3)
        assert again[0] and again[1:3] == first[1:3] and again[3].tobytes() == first[3].tobytes()
    hip.close()


def test_failed_pivot_is_flagged_on_both_schedules(monkeypatch):
    n_cams, stripped = 11, 5  # ncp 66: the sixth camera without observations, its first pivot exactly zero at lam = 0
    sc = D.unobserved_rig(n_cams, stripped)
    got = {}
    for schedule in SCHEDULES:
        hip = _handle(sc, monkeypatch, schedule)
        ok0, _, _, s0 = _step(hip, 0.0)
        ok1, _, _, s1 = _step(hip, 1e-3)  # and the handle recovers
        got[schedule] = (ok0, ok1, s1.tobytes())
        assert np.all(np.isfinite(s0)) and np.all(np.isfinite(s1))
        hip.close()
    assert not got["early"][0]  # (the oracle's step fails too: tests/test_dense_solve_gpu.py)
    assert got["early"] == got["parent"], (got["early"][:2], got["parent"][:2])


F_1PX = 1.0 / 1394.6  # tests/test_uncertainty_gpu.py


def _covariance(key, monkeypatch, schedule, loss="linear", f_scale=1.0):
    """cba_parameter_covariance with fixed-order sums (CBA_DETERMINISTIC=1) on ``schedule``."""
    from caliscope_amd import uncertainty
    from tests import covariance_native as cn

    sc = cn.key_scene(key)
    args = cn.call_arguments(sc["par"], sc["x"], sc["cam"], sc["obj"], sc["uv"])
    with monkeypatch.context() as m:
        m.setenv("CBA_DETERMINISTIC", "1")
        m.delenv("CBA_CHOL_EARLY", raising=False)
        if SCHEDULES[schedule] is not None:
            m.setenv("CBA_CHOL_EARLY", SCHEDULES[schedule])
        return uncertainty.DeviceUncertainty().parameter_covariance(*args, loss=loss, f_scale=f_scale)


def test_covariance_call_agrees_to_the_bit(monkeypatch):
    """cba_parameter_covariance (what parameter_uncertainty() calls; it factors through the same enqueue_chol_factor with its own buffers) on a
    wide-field scene of four blocks, camera covariances compared to the bit between the schedules.  The call runs with CBA_DETERMINISTIC=1, as
    the handles above do: with its default FP64 atomics no two calls even factor the same matrix (measured on this scene: six distinct results
    in six calls on either schedule, 1.2e-13 of max |C| apart).  Two calls on one schedule come first, so that a difference between the
    schedules can only be the schedule's."""
    key = ("wide", D.widths(99), False)  # eleven free cameras: four blocks, the double update
    e, again, p = (_covariance(key, monkeypatch, s) for s in ("early", "early", "parent"))
    assert np.all(np.isfinite(e.cam_cov_full)) and e.cam_cov_full.any()
    assert e.cam_cov_full.tobytes() == again.cam_cov_full.tobytes() and e.point_cov.tobytes() == again.point_cov.tobytes() and e.cost == again.cost
    print(f"early against parent: largest difference {np.abs(e.cam_cov_full - p.cam_cov_full).max() / np.abs(p.cam_cov_full).max():.3e} of max |C|")
    assert e.cam_cov.tobytes() == p.cam_cov.tobytes() and e.cam_cov_full.tobytes() == p.cam_cov_full.tobytes()


@pytest.mark.parametrize("key, loss", [(("wide", D.widths(99), False), "linear"), (("ragged",), "linear"), (("wide", D.widths(33), True), "linear"),
                                       (("small", 6, 300, 6, False, "soft_l1", 0.05), "soft_l1")],
                         ids=["wide99", "ragged", "mixed33", "robust"])
def test_fixed_order_covariance_matches_the_pseudo_inverse(key, loss, monkeypatch):
    """The fixed-order sums of the covariance call (k_unc_cam_sums, k_unc_rows, k_unc_fixed_sums) against the dense pseudo-inverse, by the rule of
    tests/test_uncertainty_gpu.py: free and mixed rigs, a robust loss, and the scene with two views, all views and a repeated (camera, point) pair."""
    from tests import covariance_native as cn

    figures = cn.check_against_pinv(_covariance(key, monkeypatch, "early", loss, F_1PX), key, loss, F_1PX)
    assert figures["lam8"] > 1e-6
