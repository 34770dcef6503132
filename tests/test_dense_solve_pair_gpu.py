"""The paired first launch of the dense solve (launches -1 and 0 of k_chol_step as ONE launch, every workgroup factoring D_0 privately; csrc/
chol_schedule.h) against the unpaired sequence (``CBA_CHOL_PAIR=0``): the same instructions on the same operands in the same order, so everything a
handle lets out is compared TO THE BIT — the flag of the factorisation, the reduced system S and rhs, and the camera part of the step.

Sizes, all on the blocked route (CBA_SMALL_SOLVE=0 up to 96): 30 is one block, which keeps the unpaired sequence; 33 and 63 are two blocks (a last
block of one row and of 31): the paired launch and the folded end, nothing between them; 66 and 96 three blocks, the paired launch and one single
launch; 99 four, 129 five, 351 eleven blocks with a tail of 31 rows, 384 twelve full blocks (64 six-parameter cameras, the block count of the
benchmark's headline workload).  Six-parameter rigs (30, 66, 96, 384), nine-parameter ones (63, 99, 351) and mixed ones (33, 129); lam = 1e-3 and
1e-10.  Rigs with an unobserved camera at lam = 0 put an exactly zero pivot into D_0 (camera 5 of 11: parameters 30 .. 35), which every workgroup of
the paired launch factors for itself, into D_1 (camera 6 of 11: 36 .. 41), the block the paired launch factors second, and into D_2 (camera 11 of
18: 66 .. 71), behind the paired launch: the flag is raised, the block becomes the identity, and flag and step are the unpaired sequence's; lam = 1e-3
behind it, the handle recovers.  Handles are deterministic (fixed-order sums), without which two handles do not form the same system.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from caliscope_amd.engine import BAProblem
from tests import dense_solve_cases as D

pytestmark = pytest.mark.gpu

SMALL_SOLVE = 64  # cba_info.build_camg bit 6: the dense camera system is solved by k_small_solve
SIZES = (30, 33, 63, 66, 96, 99, 129, 351, 384)
LAMS = (1e-3, 1e-10)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension


@functools.lru_cache(maxsize=None)
def _rig(ncp):
    if ncp == 30:
        return D._scene((6,) * 5)
    if ncp == 384:
        return D._scene((6,) * 64)  # twelve full blocks
    return D.rig(ncp)


def _handle(sc, monkeypatch, pair):
    """A deterministic handle on the rig ``sc`` on the blocked route, linearised at the rig's initial point."""
    from caliscope_amd.hip_engine import HipEngine

    with monkeypatch.context() as m:
        for name in ("CBA_CHOL_PAIR", "CBA_CHOL_ENDS", "CBA_CHOL_EARLY"):
            m.delenv(name, raising=False)
        if pair is not None:
            m.setenv("CBA_CHOL_PAIR", pair)
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


def _both(sc, monkeypatch, lams):
    got = {}
    for pair in (None, "0"):
        hip = _handle(sc, monkeypatch, pair)
        try:
            got[pair] = [_step(hip, lam) for lam in lams]
        finally:
            hip.close()
    return got[None], got["0"]


@pytest.mark.parametrize("ncp", SIZES)
def test_paired_launch_agrees_to_the_bit(ncp, monkeypatch):
    sc = _rig(ncp)
    assert sc["par"].n_camera_params == ncp
    new, old = _both(sc, monkeypatch, LAMS)
    for lam, a, b in zip(LAMS, new, old):
        assert a[0] and b[0], (ncp, lam, a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2], (ncp, lam, "the reduced systems differ")
        assert np.all(np.isfinite(a[3]))
        differ = np.flatnonzero(a[3] != b[3])
        print(f"ncp {ncp} lam {lam:g}: {len(differ)} of {ncp} step entries differ, max |s| {np.abs(b[3]).max():.3e}")
        assert a[3].tobytes() == b[3].tobytes(), (ncp, lam, differ[:8], float(np.abs(a[3] - b[3]).max()))


@pytest.mark.parametrize("n_cams,stripped", [(11, 5), (11, 6), (18, 11)], ids=["pivot_in_D0", "pivot_in_D1", "pivot_in_D2"])
def test_failed_pivot_is_the_unpaired_sequences(n_cams, stripped, monkeypatch):
    """The stripped camera's first pivot is exactly zero at lam = 0; lam = 1e-3 behind it: the handle recovers."""
    sc = D.unobserved_rig(n_cams, stripped)
    new, old = _both(sc, monkeypatch, (0.0, 1e-3))
    assert not old[0][0] and old[1][0], "the case is meant to fail at lam = 0 and to recover"
    for a, b in zip(new, old):
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        assert np.all(np.isfinite(a[3])) and a[3].tobytes() == b[3].tobytes()
