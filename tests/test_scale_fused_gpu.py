"""The Jacobi scale pass inside the launch that reduces a build's camera blocks (k_reduce_scale_pub) against the two launches it replaces
(``CBA_SCALE_FUSED=0``: k_reduce_rows[_pub], then k_scale_lin).  Run with ``-m gpu``.

Per entry the arithmetic is one function (scale_lin_entry of csrc/cba_kernels.h) on both routes, so the new scale ``sinv``, the vector of the J.g
pass ``v1 = g / sinv^2`` and max |g| must be the same BITS; only the order of the three sums ||g_h||^2, ||x_h||^2, ||x||^2 changes, and each route's
sum is held to ``math.fsum`` of its own terms.

Fused routes (cba_lib.hip: scale_fusable): single rank, camera-sorted build, no bounds, no constraint rows, no fixed-order sums.  The handles here
are therefore the default ones (no CBA_DETERMINISTIC), whose builds add with FP64 atomics: two handles do not form the same gradient to the bit
(measured: the 17-camera rigs differ in the last bits from handle to handle on either route), so "the same bits" cannot be read off two handles'
outputs alone.  Each route is therefore held, on its own handle, to the pass as a function of what that handle's build left: with
``own = sqrt(diag(J^T J))``, zeros -> 1, read back through k_scale_update's first-call rule (CBA_VEC_SCALE_OWN), the pass must give
    sinv = own (first linearisation),  sinv = max(own, sinv before) (later),  v1 = (g / sinv) / sinv,  max |g| = max_i |g_i|
TO THE BIT (sqrt, divide and max are correctly rounded on the device and on the host).  Two routes that are the same function of their inputs give the
same bits on the same inputs; where the two handles' inputs do agree to the bit, the outputs are compared directly as well.

Stages: A, the first linearisation of a solve (cba_linearize behind cba_begin: first_scale, the pass rides in run_build's reducing launch, no packet);
B, the speculative pass of an accepted trial point (cba_step: beside the packet workgroup; the monotone maximum against A's scale), whose rows are then
summed by k_lin_finish; and whole solves, one ending by ``max_nfev`` (max |g| of the last point is read from the pass's rows by k_gnorm_pub).

Error bound of a sum of n non-negative terms added in any order: (number of additions a term passes through) x 2^-53 relative.  The depth allowed is
rows + terms per thread + 8, from the launch geometry below (ScaleFuse of cba_kernels.h; vec_grid of cba_lib.hip); the two norms come back as square
roots, whose rounding and the squaring here add 2 x 2^-53 to the bound of those two.  Every figure is printed before it is asserted (``-s``).
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from caliscope_amd.engine import BAProblem
from tests.helpers import small_problem

pytestmark = pytest.mark.gpu

VEC_X, VEC_GRAD, VEC_SCALE_INV, VEC_JG_INPUT, VEC_SCALE_OWN = 0, 2, 4, 5, 6
ROUTES = {"fused": None, "two_launches": "0"}  # value of CBA_SCALE_FUSED (None: unset, the default)
U = 2.0 ** -53

# (cameras, nine-parameter cameras, points): 300 points are one point workgroup with idle threads and one entry per thread (about 990 entries of
# 1024), 1500 are two whose threads take two or three (about 4540 of 2 x 1024: the last ones have no third); a reducing workgroup per camera: 27 or
# 54 of its 64 columns live.  (A thread takes at most four entries and the grid grows with the points: there is no other path at any size.)
RIGS = {"six_C2": (2, False, 300), "six_C3": (3, False, 300), "six_C17": (17, False, 1500),
        "nine_C2": (2, True, 300), "nine_C3": (3, True, 300), "nine_C17": (17, True, 1500)}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension


@pytest.fixture(scope="module")
def rigs():
    out = {}
    for name, (n_cams, nine, n_points) in RIGS.items():
        sc, par, x0 = small_problem(n_cams=n_cams, n_points=n_points, k=min(n_cams, 4), refine=nine)
        assert par.n_camera_params == n_cams * (9 if nine else 6) and par.n_camera_params % 32 != 0
        out[name] = (sc, par, x0)
    return out


def _engine(monkeypatch, prob, route):
    from caliscope_amd.hip_engine import HipEngine

    with monkeypatch.context() as m:
        m.delenv("CBA_DETERMINISTIC", raising=False)
        m.delenv("CBA_SCALE_FUSED", raising=False)
        if ROUTES[route] is not None:
            m.setenv("CBA_SCALE_FUSED", ROUTES[route])
        return HipEngine(prob)


def _pad32(n):
    return (n + 31) // 32 * 32


def depth(route, n_cams, nine, ncp, n_points):
    """rows + terms per thread + 8 of the launch that left the sums."""
    total = _pad32(ncp) + 3 * _pad32(n_points)
    if route == "fused":
        cams_per_wg = 1
        entries = total - ncp
        pt_wgs = -(-entries // 4096)
        rows, per_thread = -(-n_cams // cams_per_wg) + pt_wgs, -(-entries // (pt_wgs * 1024))
    else:
        rows = min(-(-total // 256), 1024)
        per_thread = -(-total // (rows * 256))
    return rows + per_thread + 8


def _stage(eng, lin):
    return dict(x=eng.get_vector(VEC_X), g=eng.get_vector(VEC_GRAD), sinv=eng.get_vector(VEC_SCALE_INV), v1=eng.get_vector(VEC_JG_INPUT),
                own=eng.get_vector(VEC_SCALE_OWN),
                gh_sq=lin.gh_sq, xs=lin.x_scaled_norm, xn=lin.x_norm, gmax=lin.g_norm_inf)


def _two_stages(monkeypatch, prob, x0, route):
    from caliscope_amd import _lib

    eng = _engine(monkeypatch, prob, route)
    try:
        assert eng.lib.cba_step_supported(eng._h)
        eng.begin(x0)
        a = _stage(eng, eng.linearize())  # stage A: first_scale
        si = _lib.StepInfo()
        eng._check(eng.lib.cba_step(eng._h, -1.0, C.byref(si)), "cba_step")
        assert si.need_host == 0 and si.newton.ok and si.trial.finite
        eng.accept()
        b = _stage(eng, eng.linearize())  # stage B: the speculative pass of the accepted point, its rows summed by k_lin_finish
        return a, b
    finally:
        eng.close()


def _check_own_arithmetic(tag, st, prev_sinv, d):
    """One route against IEEE arithmetic on its own vectors, and its three sums against math.fsum of their terms."""
    g, x, s = st["g"], st["x"], st["sinv"]
    assert np.all(np.isfinite(s)) and np.all(s > 0.0)
    assert np.array_equal(st["v1"], (g / s) / s), f"{tag}: v1 is not g / sinv / sinv to the bit"
    assert st["gmax"] == np.abs(g).max(), f"{tag}: max |g| {st['gmax']!r} against {np.abs(g).max()!r}"
    want = st["own"] if prev_sinv is None else np.maximum(st["own"], prev_sinv)
    assert np.array_equal(s, want), f"{tag}: sinv differs from the rule in {np.count_nonzero(s != want)} entries"
    gh = g / s
    xh = x * s
    ref = [math.fsum((gh * gh).tolist()), math.fsum((xh * xh).tolist()), math.fsum((x * x).tolist())]
    got = [Fraction(st["gh_sq"]), Fraction(st["xs"]) ** 2, Fraction(st["xn"]) ** 2]
    for name, r, v, extra in zip(("||g_h||^2", "||x_h||^2", "||x||^2"), ref, got, (0, 2, 2)):
        err = float(abs(v - Fraction(r)) / Fraction(r))
        print(f"{tag}: {name} relative error {err / U:.2f} x 2^-53, bound {d + extra}")
        assert err <= (d + extra) * U, (tag, name, err / U, d + extra)


@pytest.mark.parametrize("name", sorted(RIGS))
def test_scale_pass_is_the_same_bits_on_both_routes(monkeypatch, rigs, name):
    n_cams, nine, n_points = RIGS[name]
    sc, par, x0 = rigs[name]
    prob = BAProblem(par, sc.camera_indices, sc.image_coords, sc.obj_indices)
    got = {route: _two_stages(monkeypatch, prob, x0, route) for route in ROUTES}
    for route, (a, b) in got.items():
        d = depth(route, n_cams, nine, par.n_camera_params, n_points)
        _check_own_arithmetic(f"{name} {route} first", a, None, d)
        _check_own_arithmetic(f"{name} {route} later", b, a["sinv"], d)
        print(f"{name} {route}: the later pass raised {np.count_nonzero(b['sinv'] > a['sinv'])} of {len(x0)} scales")
        assert np.any(b["x"] != a["x"]), "the later stage is meant to be another point"
    for stage, (f, t) in zip(("first", "later"), zip(got["fused"], got["two_launches"])):
        same_inputs = all(np.array_equal(f[k], t[k]) for k in ("g", "x", "own")) and (stage == "first" or np.array_equal(got["fused"][0]["sinv"], got["two_launches"][0]["sinv"]))
        print(f"{name} {stage}: inputs of the two handles bit-identical: {same_inputs}; max |g| {f['gmax']!r} / {t['gmax']!r}")
        if same_inputs:
            assert np.array_equal(f["sinv"], t["sinv"]), f"{name} {stage}: sinv differs in {np.count_nonzero(f['sinv'] != t['sinv'])} entries"
            assert np.array_equal(f["v1"], t["v1"]), f"{name} {stage}: v1 differs in {np.count_nonzero(f['v1'] != t['v1'])} entries"
            assert f["gmax"] == t["gmax"]


TOL = dict(ftol=1e-8, xtol=1e-8, gtol=1e-300)  # (ends at a trial point: ftol or xtol)


@pytest.mark.parametrize("name", ["six_C3", "six_C17", "nine_C17"])
@pytest.mark.parametrize("max_nfev", [None, 3])
def test_whole_solves_agree(monkeypatch, rigs, name, max_nfev):
    """max_nfev = 3: the second fused step is announced as the last, no J.g pass is enqueued behind it and k_gnorm_pub mails max |g| of the last point
    from the rows the pass left."""
    sc, par, x0 = rigs[name]
    prob = BAProblem(par, sc.camera_indices, sc.image_coords, sc.obj_indices)
    res = {}
    for route in ROUTES:
        eng = _engine(monkeypatch, prob, route)
        try:
            r = eng.solve(x0, max_nfev=max_nfev, **TOL)
            res[route] = (r, np.abs(eng.get_vector(VEC_GRAD)).max())
        finally:
            eng.close()
    (f, gf), (t, gt) = res["fused"], res["two_launches"]
    print(f"{name} max_nfev {max_nfev}: fused nfev {f.nfev} njev {f.njev} status {f.status} optimality {f.optimality!r}; "
          f"two launches nfev {t.nfev} njev {t.njev} status {t.status} optimality {t.optimality!r}")
    assert f.status == (0 if max_nfev else f.status) and f.status in (0, 2, 3, 4)
    assert (f.nfev, f.njev, f.status) == (t.nfev, t.njev, t.status)
    assert f.optimality == gf and t.optimality == gt, "the reported optimality is max |g| of the handle's own gradient, to the bit"
