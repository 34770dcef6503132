"""The linear-loss forms of ``k_tprep`` and ``k_jv`` (``CBA_LINEAR_PASS``, on by default) on a real MI355X (run with ``-m gpu``).

Under a linear loss the two kernels that linearise every observation a second time use only the factors G, Y = R X, A_intr and B of it: the
residual would reach them through a row scale that is exactly 1.0.  Their LIN instantiations therefore load no pixels and read no principal point.
Nothing behind them may change: a handle with ``CBA_LINEAR_PASS=0`` runs the generic kernels and has to give the same reduced system, the same
step and the same ``jg_sq`` — within the bounds tests/test_gpu_parity.py uses between two assembly routes for default handles (whose LDS atomics
add in an order that varies from launch to launch), and bit for bit for ``deterministic=True`` handles, whose sums are all in fixed order.  The
fixed-order ``DETM`` variants of ``k_tprep`` are specialised too, so the bit comparison runs the LIN kernels against the generic ones.  The LIN
forms are launched for six-parameter kernels; a rig with free intrinsics (``refine``: the nine-parameter kernels, whose ``k_tprep`` measured slower
without the pixels) keeps the generic ones under either switch value, and has to give the same bits for that reason."""
import functools

import numpy as np
import pytest

from caliscope_amd.engine import BAProblem
from tests.helpers import small_problem

pytestmark = pytest.mark.gpu

LAM = 1e-4

# The smallest shapes at which the changed code can go wrong.  The two kernels walk the observations in 256-thread workgroups: k_jv in trips of
# jv_grid x 256 (jv_grid = min(ceil(N / 256), what the device holds at once)) with the records of trips i + 2 and i + 4 in flight, k_tprep in
# chunks with the record of chunk n + 2 in flight.
SHAPES = {
    "C40_k7": dict(n_cams=40, n_points=1500, k=7),                      # three camera groups, a ragged last chunk
    "C40_k7_refine": dict(n_cams=40, n_points=1500, k=7, refine=True),  # the nine-parameter kernels (generic under both switch values)
    "C4_90obs": dict(n_cams=4, n_points=30, k=3),                       # fewer observations than one workgroup: every prefetch is a clamped one
    "N_256m_plus_1": dict(n_cams=4, n_points=171, k=3),                 # 513 = 2 x 256 + 1: one thread of the last workgroup is live
    "N_jv_grid_x_256": dict(n_cams=6, n_points=128, k=6),               # 768 = 3 x 256, jv_grid = 3: exactly one full trip, none ragged
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()


@functools.lru_cache(maxsize=None)
def _problem(shape, loss="linear"):
    cfg = dict(SHAPES[shape]) if shape in SHAPES else dict(n_cams=8, n_points=400, k=8)
    sc, par, x0 = small_problem(loss=loss, outliers=0.05 if loss != "linear" else 0.0, **cfg)
    fs = sc.f_scale_1px() * 2.0 if loss != "linear" else 1.0
    n_obs = cfg["n_points"] * cfg["k"]
    assert len(sc.camera_indices) == n_obs
    return BAProblem(par, sc.camera_indices, sc.image_coords, sc.obj_indices, loss=loss, f_scale=fs), x0, fs


def _one_step(eng, x0):
    """begin, linearize, newton_step at LAM: (S, rhs, step, jg_sq, gh_sq, cost)."""
    eng.begin(x0)
    lin = eng.linearize()
    assert eng.newton_step(LAM).ok
    S, rhs = eng.reduced_system()
    return S, rhs, eng.get_vector(3).copy(), lin.jg_sq, lin.gh_sq, eng.last_cost


@functools.lru_cache(maxsize=None)
def _result(shape, switch, deterministic, loss="linear"):
    """One handle created with CBA_LINEAR_PASS = switch (the library reads it where the handle is created), one step.  Computed once per argument
    set and shared: the tests only read it."""
    import os

    from caliscope_amd.hip_engine import HipEngine

    prob, x0, _ = _problem(shape, loss)
    old = os.environ.get("CBA_LINEAR_PASS")
    os.environ["CBA_LINEAR_PASS"] = switch
    try:
        with HipEngine(prob, deterministic=deterministic) as eng:
            out = _one_step(eng, x0)
    finally:
        if old is None:
            del os.environ["CBA_LINEAR_PASS"]
        else:
            os.environ["CBA_LINEAR_PASS"] = old
    for a in out[:3]:
        a.setflags(write=False)
    return out


def test_shapes_are_what_they_claim():
    assert SHAPES["C4_90obs"]["n_points"] * SHAPES["C4_90obs"]["k"] == 90 < 256
    assert SHAPES["N_256m_plus_1"]["n_points"] * SHAPES["N_256m_plus_1"]["k"] == 2 * 256 + 1
    assert SHAPES["N_jv_grid_x_256"]["n_points"] * SHAPES["N_jv_grid_x_256"]["k"] == 3 * 256


@pytest.mark.parametrize("shape", list(SHAPES))
def test_same_system_same_step(shape):
    """Default handles: S and rhs within 1e-12 max|.|, the step within 1e-8 max|.|, jg_sq and gh_sq within 1e-12 relative
    (tests/test_gpu_parity.py, between two assembly routes)."""
    S1, r1, s1, jg1, gh1, _ = _result(shape, "1", False)
    S0, r0, s0, jg0, gh0, _ = _result(shape, "0", False)
    print(f"{shape}: S {np.abs(S1 - S0).max() / np.abs(S0).max():.3g}  rhs {np.abs(r1 - r0).max() / np.abs(r0).max():.3g}  "
          f"step {np.abs(s1 - s0).max() / np.abs(s0).max():.3g}  jg_sq {abs(jg1 - jg0) / abs(jg0):.3g}  gh_sq {abs(gh1 - gh0) / abs(gh0):.3g}")
    assert np.abs(S1 - S0).max() <= 1e-12 * np.abs(S0).max()
    assert np.abs(r1 - r0).max() <= 1e-12 * np.abs(r0).max()
    assert np.abs(s1 - s0).max() <= 1e-8 * np.abs(s0).max()
    assert abs(jg1 - jg0) <= 1e-12 * abs(jg0) and abs(gh1 - gh0) <= 1e-12 * abs(gh0)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_deterministic_handles_are_bit_equal(shape):
    """Every sum in fixed order: the LIN kernels (k_tprep<NC, DETM, .., LIN>, k_jv<.., LIN>) leave the bits the generic ones leave."""
    a = _result(shape, "1", True)
    b = _result(shape, "0", True)
    for name, u, v in zip(("S", "rhs", "step"), a[:3], b[:3]):
        assert np.array_equal(u, v), name
    assert a[3] == b[3] and a[4] == b[4] and a[5] == b[5], (a[3:], b[3:])


def test_robust_handles_keep_the_generic_kernels():
    """A Huber handle never takes the LIN forms: with fixed-order sums the switch changes no bit."""
    a = _result("huber", "1", True, "huber")
    b = _result("huber", "0", True, "huber")
    for name, u, v in zip(("S", "rhs", "step"), a[:3], b[:3]):
        assert np.array_equal(u, v), name
    assert a[3:] == b[3:]


def test_set_loss_on_one_handle():
    """cba_set_loss changes the loss of a live handle, and with it the form of the two kernels at the next launch: after each call the step is
    that of a fresh handle of that loss (1e-8 max|.|)."""
    from caliscope_amd.hip_engine import HipEngine

    prob, x0, fs = _problem("huber", "huber")
    cam, uv, obj = prob.camera_indices, prob.image_coords, prob.obj_indices
    with HipEngine(BAProblem(prob.parameterization, cam, uv, obj)) as eng:
        _one_step(eng, x0)  # (linear first: the handle has launched its LIN forms)
        for loss, f in (("huber", fs), ("linear", 1.0)):
            eng.set_loss(loss, f)
            step = _one_step(eng, x0)[2]
            with HipEngine(BAProblem(prob.parameterization, cam, uv, obj, loss=loss, f_scale=f)) as fresh:
                ref = _one_step(fresh, x0)[2]
            print(f"after set_loss({loss}): step difference {np.abs(step - ref).max() / np.abs(ref).max():.3g}")
            assert np.abs(step - ref).max() <= 1e-8 * np.abs(ref).max(), loss
