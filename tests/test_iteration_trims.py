"""The J.g pass nobody reads, against the route that still runs it (run with ``-m gpu``).

``CBA_SPEC_SKIP`` (default on): the J.g pass of the speculative linearisation behind a trial point at which the solve ends is skipped on the device
(cba_set_tolerances), not enqueued behind the last trial ``max_nfev`` allows (cba_hint_last_trial), and cba_solve reads max |g| of the last point
through cba_gradient_norm.  No number that reaches ``x`` changes: nfev, njev, status, cost, optimality and x must be BIT-equal with the switch on and
off (``CBA_SPEC_SKIP=0``: the speculative pass always runs and the driver's last call is the whole linearisation, as before).

Everything goes through the C ABI with ``CBA_DETERMINISTIC=1`` (fixed summation orders), so that two runs are bit-comparable at all; the switch is
read by cba_create.  Each comparison prints its figures before it asserts (``-s`` shows them).
"""
import numpy as np
import pytest

from caliscope_amd.engine import BAProblem
from tests.helpers import small_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension


@pytest.fixture(scope="module")
def rigs():
    """The shapes, built once: 300 points with 4 - 6 observations each."""
    out = {}
    for name, n_cams, k in (("six_C8", 8, 6), ("six_C17", 17, 4)):  # 48 camera parameters: the one-workgroup dense solve; 102: the blocked one
        out[name] = small_problem(n_cams=n_cams, n_points=300, k=k)
    return out


def _engine(monkeypatch, prob, **env):
    from caliscope_amd.hip_engine import HipEngine

    with monkeypatch.context() as m:
        m.setenv("CBA_DETERMINISTIC", "1")
        for k, v in env.items():
            m.setenv(k, v)
        return HipEngine(prob)


# ---- the unused J.g pass ---------------------------------------------------------------------------------------------------------------------------

def _solve(monkeypatch, prob, x0, skip, timers=False, twice=False, **kw):
    eng = _engine(monkeypatch, prob, CBA_SPEC_SKIP=skip)
    try:
        if timers:
            eng.enable_timers(True); eng.reset_timers()
        res = [eng.solve(x0, **kw)]
        if twice:
            res.append(eng.solve(None, **kw))  # restart from the x0 on the device
        return res, eng.info()["spec_jv_skipped"], (eng.timers()["jv"][1] if timers else None)
    finally:
        eng.close()


def _same(a, b):
    return (a.nfev, a.njev, a.status, a.n_iterations) == (b.nfev, b.njev, b.status, b.n_iterations) and a.cost == b.cost and a.optimality == b.optimality \
        and np.array_equal(a.x, b.x)


# gtol far below what double precision reaches: the solve ends at a trial point (ftol or xtol), which is the case the device decides
TOL = dict(ftol=1e-8, xtol=1e-8, gtol=1e-300)


@pytest.mark.parametrize("name", ["six_C8", "six_C17"])  # the one-workgroup solve and the blocked one
def test_skipped_pass_changes_nothing(monkeypatch, rigs, name):
    sc, par, x0 = rigs[name]
    prob = BAProblem(par, sc.camera_indices, sc.image_coords, sc.obj_indices)
    (on,), n_on, _ = _solve(monkeypatch, prob, x0, "1", **TOL)
    (off,), n_off, _ = _solve(monkeypatch, prob, x0, "0", **TOL)
    print(f"{name}: on  nfev {on.nfev} njev {on.njev} status {on.status} cost {on.cost!r} optimality {on.optimality!r} skipped {n_on}\n"
          f"{name}: off nfev {off.nfev} njev {off.njev} status {off.status} cost {off.cost!r} optimality {off.optimality!r} skipped {n_off}")
    assert on.status in (2, 3, 4)
    assert _same(on, off)
    assert n_on == 1 and n_off == 0


@pytest.mark.parametrize("name", ["six_C8", "six_C17"])
def test_last_allowed_trial_gets_no_speculative_pass(monkeypatch, rigs, name):
    """max_nfev = 3: x0 and two fused steps.  J.g passes with the switch off: the first linearisation, and one behind each of the two steps' packets (the
    final cba_linearize finds the second one done); with the switch on the second step is announced as the last and gets none, and the gradient norm of
    the last point comes from its scale pass: one launch fewer, the device skipped nothing."""
    sc, par, x0 = rigs[name]
    prob = BAProblem(par, sc.camera_indices, sc.image_coords, sc.obj_indices)
    (on,), n_on, jv_on = _solve(monkeypatch, prob, x0, "1", timers=True, max_nfev=3, **TOL)
    (off,), n_off, jv_off = _solve(monkeypatch, prob, x0, "0", timers=True, max_nfev=3, **TOL)
    print(f"{name}: max_nfev 3: status {on.status} nfev {on.nfev} njev {on.njev}, k_jv launches on {jv_on} off {jv_off}, skipped {n_on} / {n_off}")
    assert on.status == 0 and on.nfev == 3
    assert _same(on, off)
    assert n_on == 0 and n_off == 0
    assert jv_on == jv_off - 1


def test_rejected_trials_of_a_robust_solve(monkeypatch):
    sc, par, x0 = small_problem(n_cams=8, n_points=400, k=8, loss="huber", outliers=0.05)
    fs = sc.f_scale_1px() * 2.0
    prob = BAProblem(par, sc.camera_indices, sc.image_coords, sc.obj_indices, loss="huber", f_scale=fs)
    (on,), n_on, _ = _solve(monkeypatch, prob, x0, "1", **TOL)
    (off,), n_off, _ = _solve(monkeypatch, prob, x0, "0", **TOL)
    print(f"huber: nfev {on.nfev} njev {on.njev} status {on.status} cost {on.cost!r} skipped {n_on} / {n_off}")
    assert on.nfev > on.njev, "the case is meant to reject trials"
    assert _same(on, off)
    assert n_off == 0 and n_on <= 1


def test_two_solves_on_one_handle(monkeypatch, rigs):
    """The word the skipped pass reads is written by every packet: the second solve's passes run (same evaluations, same bits as the first) and its
    own last one is skipped again."""
    sc, par, x0 = rigs["six_C17"]
    prob = BAProblem(par, sc.camera_indices, sc.image_coords, sc.obj_indices)
    (a, b), n_on, _ = _solve(monkeypatch, prob, x0, "1", twice=True, **TOL)
    (c, d), n_off, _ = _solve(monkeypatch, prob, x0, "0", twice=True, **TOL)
    print(f"two solves: nfev {a.nfev} / {b.nfev}, status {a.status} / {b.status}, skipped {n_on} / {n_off}")
    assert (a.nfev, a.njev, a.status, a.cost, a.optimality) == (b.nfev, b.njev, b.status, b.cost, b.optimality)
    assert _same(a, c) and (b.nfev, b.njev, b.status, b.cost, b.optimality) == (d.nfev, d.njev, d.status, d.cost, d.optimality)
    assert n_on == 2 and n_off == 0
