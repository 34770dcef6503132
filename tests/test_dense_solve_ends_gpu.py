"""The end of the dense solve's launch sequence folded into one launch (k_chol_last_apply: the last k_chol_step launch and k_chol_apply; csrc/
chol_schedule.h) against the old sequence (``CBA_CHOL_ENDS=0``): the same instructions on the same operands in the same order, so everything a
handle lets out is compared TO THE BIT — the flag of the factorisation, the reduced system S and rhs, and the camera part of the step.  (L, Xinv and
T have no readback; the folded launch keeps T(:, last) and y_last private and stores neither, since nothing reads them after the solve, so those
buffers are not the old sequence's to the bit and are not meant to be.  The fold of launch -1 into launch 0 is not built.)

Sizes, all on the blocked route (CBA_SMALL_SOLVE=0 up to 96): 30 is one block, which keeps the old sequence; 33 has a last block of one row; 63 of 31;
66 and 96 are three blocks (the last one full at 96); 99 is the first size beyond the one-workgroup solve, four blocks; 129 and 351 (11 blocks, a
31-row tail).  The plan of this change named 64 and 97 as well: no rig has them, a handle's cameras have six or nine parameters and ncp is a multiple of
three, so their neighbours 63 and 99 stand in.  Six-parameter rigs (30, 66, 96), nine-parameter ones (63, 99, 351) and mixed ones (33, 129); both schedules of
the factorisation (CBA_CHOL_EARLY unset and 0: the folded launch carries the parent schedule's pending update of the rhs block); lam = 1e-3 and
1e-10.  Two rigs with an unobserved camera at lam = 0 put an exactly zero pivot into D_0 (camera 5: parameters 30 .. 35) and into D_1 (camera 6:
36 .. 41): the flag is raised, the block becomes the identity, and flag and step are the old sequence's.  Handles are deterministic (fixed-order
sums), without which two handles do not form the same system.
"""
from __future__ import annotations

import numpy as np
import pytest

from caliscope_amd.engine import BAProblem
from tests import dense_solve_cases as D

pytestmark = pytest.mark.gpu

SMALL_SOLVE = 64  # cba_info.build_camg bit 6: the dense camera system is solved by k_small_solve
SIZES = (30, 33, 63, 66, 96, 99, 129, 351)
LAMS = (1e-3, 1e-10)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension


def _rig(ncp):
    return D._scene((6,) * 5) if ncp == 30 else D.rig(ncp)


def _handle(sc, monkeypatch, ends, early):
    """A deterministic handle on the rig ``sc`` on the blocked route, linearised at the rig's initial point."""
    from caliscope_amd.hip_engine import HipEngine

    with monkeypatch.context() as m:
        for name, value in (("CBA_CHOL_ENDS", ends), ("CBA_CHOL_EARLY", early)):
            m.delenv(name, raising=False)
            if value is not None:
                m.setenv(name, value)
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


def _both(sc, monkeypatch, early, lams):
    got = {}
    for ends in (None, "0"):
        hip = _handle(sc, monkeypatch, ends, early)
        try:
            got[ends] = [_step(hip, lam) for lam in lams]
        finally:
            hip.close()
    return got[None], got["0"]


@pytest.mark.parametrize("early", [None, "0"], ids=["early", "parent"])
@pytest.mark.parametrize("ncp", SIZES)
def test_folded_end_agrees_to_the_bit(ncp, early, monkeypatch):
    sc = _rig(ncp)
    assert sc["par"].n_camera_params == ncp
    new, old = _both(sc, monkeypatch, early, LAMS)
    for lam, a, b in zip(LAMS, new, old):
        assert a[0] and b[0], (ncp, lam, a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2], (ncp, lam, "the reduced systems differ")
        assert np.all(np.isfinite(a[3]))
        differ = np.flatnonzero(a[3] != b[3])
        print(f"ncp {ncp} lam {lam:g}: {len(differ)} of {ncp} step entries differ, max |s| {np.abs(b[3]).max():.3e}")
        assert a[3].tobytes() == b[3].tobytes(), (ncp, lam, differ[:8], float(np.abs(a[3] - b[3]).max()))


@pytest.mark.parametrize("early", [None, "0"], ids=["early", "parent"])
@pytest.mark.parametrize("stripped", [5, 6], ids=["pivot_in_D0", "pivot_in_D1"])
def test_failed_pivot_is_the_old_sequences(stripped, early, monkeypatch):
    """ncp 66, three blocks: the stripped camera's first pivot is exactly zero at lam = 0; lam = 1e-3 behind it: the handle recovers."""
    sc = D.unobserved_rig(11, stripped)
    new, old = _both(sc, monkeypatch, early, (0.0, 1e-3))
    assert not old[0][0] and old[1][0], "the case is meant to fail at lam = 0 and to recover"
    for a, b in zip(new, old):
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        assert np.all(np.isfinite(a[3])) and a[3].tobytes() == b[3].tobytes()
