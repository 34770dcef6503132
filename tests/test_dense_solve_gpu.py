"""The dense solve of the reduced camera system S s_c = rhs on the device, on its own and against LAPACK (run with ``-m gpu``).

Both routes — k_small_solve (one workgroup, ncp <= 96) and the blocked k_chol_step + k_chol_apply (beyond, and for small rigs under
CBA_SMALL_SOLVE=0; ``cba_info.build_camg`` bit 6 says which ran) — over the sweep of tests/dense_solve_cases.py: last blocks of 1 to 32 live
rows, 1 to 11 blocks, mixed six- / nine-wide rigs with cameras across the block boundaries, at lam = 1e-3, 1e-7 and 1e-10
(cond(S) 1.6e4 .. 3e11).  Every case reads the device's OWN system (``reduced_system()``: S and rhs are kept apart from the work matrix) and
takes from it, in longdouble,

    eta(s) = ||rhs - S s||_inf / (||S||_inf ||s||_inf + ||rhs||_inf)      phi(s) = ||s - x_ref||_inf / ||x_ref||_inf

for the device's step and for LAPACK's (scipy cho_factor / cho_solve) on the same S and rhs; x_ref is the longdouble reference.  Asserted:
the step is reported ok where LAPACK factors S; S is finite, symmetric to the bit and within 1e-9 max|S| of the oracle's reduced system;
eta <= R_ETA max(eta_L, 2^-53) and phi <= R_PHI max(phi_L, n 2^-53).  A full run rewrites profiles/dense_solve_accuracy.json with every
case's figures.

The tolerances.  The rule: R = four times the largest ratio measured over all cases on the MI355X, rounded up to a power of two (S changes in
its last bits from run to run with the FP64 atomics of the linearisation), and a largest ratio above 64 (eta) or 16 (phi) is not adopted.
Two measuring runs gave eta ratios of at most 25.0 and 34.7 (ncp 96, blocked route, lam 1e-10, cond 2.4e11; the float64 emulation of the
same algorithm on the same systems: at most 31.1 and 38.8), so R_ETA = 256: the step is backward stable, eta <= 3.9e-15 in every case.  The phi
ratios reached 36.4 (ncp 192, lam 1e-7, cond 2.4e8) and 47.4 (ncp 66, blocked, lam 1e-7, cond 2.2e8), above 16 in 12 and 9 of 75 sweep
cases — other cases in the second run than in the first: between the runs a case's ratio moved by up to 36 times, mostly because LAPACK's
OWN forward error on one matrix does (6.5e-13 against 2.4e-14 at ncp 129, lam 1e-3).  The part that is the device's: both routes solve
their panels by a product with the explicit X_k = L_kk^-1, whose rounding error is u |U| |X_k^T| where a substitution's is
u |L_bk| |L_kk^T|; emulated in float64 on the oracle's systems that product costs a factor 2.9 in phi in the geometric mean and up to 31
on one system, with eta unchanged, while T = L^-T in the place of the backward substitution costs nothing.  The
loss is inherent in the explicit inverse, so no ratio above 16 is adopted: R_PHI = 4 x 16 = 64, and a case beyond it is asserted by the
suite's existing bounds (test_gpu_parity.py / test_kernel_edges_gpu.py::_check_step: ||S s - rhs||_2 < 1e-7 ||rhs||_2, and the step within
1e-8 of the reference at lam >= 1e-3, 1e-7 at lam = 1e-7) with its measured ratio printed and recorded beside it.

Further: the two-launch assembly of S (CBA_REG_FINALIZE=0, which fills the work matrix from another kernel), bit-identical results of
deterministic handles, and a camera without observations — exactly zero step entries at lam > 0, and at lam = 0 a pivot that is exactly 0:
chol_factor_block's own failure branch (flags[2], the block replaced by the identity, a finite step), after which the SAME handle (Xinv, Tinv
and the work matrix persist on it) takes the step of a fresh one to the bit.  Each case prints its figures before it asserts (``-s``).
"""
import json
from pathlib import Path

import numpy as np
import pytest

from caliscope_amd.engine import BAProblem
from tests import dense_solve_cases as D

pytestmark = pytest.mark.gpu

SMALL_SOLVE = 64  # cba_info.build_camg bit 6: the dense camera system is solved by k_small_solve
# The largest eta / max(eta_L, 2^-53) and phi / max(phi_L, n 2^-53) over all cases of the two measuring runs on the MI355X (the docstring has
# the cases); R = 4 x the largest adopted ratio, rounded up to a power of two.
MEASURED_ETA, MEASURED_PHI = (25.0, 34.7), (36.4, 47.4)
LIMIT_ETA, LIMIT_PHI = 64.0, 16.0  # largest ratios that may be adopted as a tolerance at all
R_ETA = 256.0  # 4 x 34.7 = 139
R_PHI = 64.0   # 4 x 16: the measured 47.4 is above the limit and not adopted
SUITE_STEP_BOUND = {1e-3: 1e-8, 1e-7: 1e-7}  # _check_step's bounds on a step against the LU solve; the suite has none at lam = 1e-10

ROOT = Path(__file__).resolve().parents[1]
ASSEMBLY_ENV = {"one_launch": {}, "two_launches": {"CBA_REG_FINALIZE": "0"}}
SWEEP_CASES = [(ncp, route, "one_launch") for ncp in sorted(D.SWEEP) for route in (("small", "blocked") if D.SWEEP[ncp][4] else ("blocked",))]
SWEEP_CASES += [(ncp, "blocked", "two_launches") for ncp in (126, 129, 225)]
RECORDS = {}


def _write_report():
    sweep = [f"ncp{n}-{r}-{a}-lam{lam:g}" for n, r, a in SWEEP_CASES for lam in D.LAMS]
    if not all(k in RECORDS for k in sweep):
        return  # a partial run (-k) leaves the committed figures alone
    cases = [RECORDS[k] for k in sweep] + [v for k, v in RECORDS.items() if k not in sweep]
    worst_eta, worst_phi = max(cases, key=lambda c: c["ratio_eta"]), max(cases, key=lambda c: c["ratio_phi"])
    out = {
        "what": "normwise backward error eta and forward error phi (against a longdouble reference) of the device's dense camera-system solve and of "
                "LAPACK's Cholesky on the device's own S and rhs; ratio_eta = eta / max(eta_L, 2^-53), ratio_phi = phi / max(phi_L, n 2^-53); "
                "emulation_*: the float64 emulation of the blocked route (tests/dense_solve_cases.py::blocked_inverse_solve) in the same units",
        "largest_ratio_eta": {k: worst_eta[k] for k in ("case", "ratio_eta", "cond")},
        "largest_ratio_phi": {k: worst_phi[k] for k in ("case", "ratio_phi", "cond")},
        "limit_for_adoption": {"eta": LIMIT_ETA, "phi": LIMIT_PHI},
        "R_eta": R_ETA, "R_phi": R_PHI,
        "rule": "R = 4 x the largest adopted ratio of the measuring runs, rounded up to a power of two; a phi ratio above 16 is not adopted (the loss of the "
                "explicit X_k = L_kk^-1 in the panel solves, DESIGN.md section 7): R_phi = 4 x 16, and a case beyond it is held to the suite's existing bounds",
        "measuring_runs": {"largest_ratio_eta": list(MEASURED_ETA), "largest_ratio_phi": list(MEASURED_PHI)},
        "cases_above_the_phi_limit": [{k: c[k] for k in ("case", "ncp", "lam", "cond", "ratio_phi")} for c in cases if c["ratio_phi"] > LIMIT_PHI],
        "cases": cases,
    }
    (ROOT / "profiles" / "dense_solve_accuracy.json").write_text(json.dumps(out, indent=1) + "\n")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension
    yield
    _write_report()


def _handle(sc, monkeypatch, route, assembly="one_launch", deterministic=False):
    """A handle on the rig ``sc`` whose dense solve takes ``route``, linearised at the rig's initial point."""
    from caliscope_amd.hip_engine import HipEngine

    ncp = sc["par"].n_camera_params
    env = dict(ASSEMBLY_ENV[assembly])
    if route == "blocked" and ncp <= D.SMALL_N:
        env["CBA_SMALL_SOLVE"] = "0"
    assert route == "blocked" or ncp <= D.SMALL_N
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        hip = HipEngine(BAProblem(sc["par"], sc["cam"], sc["uv"], sc["obj"]), deterministic=deterministic)
    bits = hip.info()["build_camg"]
    assert bool(bits & SMALL_SOLVE) == (route == "small"), (route, bits)
    hip.begin(sc["x0"])
    hip.linearize()
    return hip


def _step(hip, lam):
    """(ok, S, rhs, s[:ncp]) of one damped step."""
    ok = hip.newton_step(lam).ok
    S, rhs = hip.reduced_system()
    return ok, S, rhs, hip.get_vector(3)[: len(rhs)].copy()


def _check_system_and_accuracy(ok, S, rhs, s, key, lam, case):
    """Assertions a (ok where LAPACK factors), b (the device's S) and c (eta and phi against LAPACK on the same system)."""
    n = len(rhs)
    s_l = D.lapack_solve(S, rhs) if np.all(np.isfinite(S)) else None
    assert s_l is not None, case  # every system of these tests is one LAPACK factors
    assert ok, (case, "the device reports a failed factorisation where LAPACK succeeds")
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(rhs)) and np.all(np.isfinite(s)), case
    assert np.array_equal(S, S.T), (case, "S is not symmetric to the bit")
    S_ref, _ = D.oracle_system(key, lam)
    d_S = float(np.abs(S - S_ref).max() / np.abs(S_ref).max())
    x_ref = D.reference_solve(S, rhs)
    s_b = D.blocked_inverse_solve(S, rhs)
    eta, eta_l, eta_b = D.eta(S, rhs, s), D.eta(S, rhs, s_l), D.eta(S, rhs, s_b)
    phi, phi_l, phi_b = D.phi(s, x_ref), D.phi(s_l, x_ref), D.phi(s_b, x_ref)
    den_eta, den_phi = max(eta_l, D.U53), max(phi_l, n * D.U53)
    rec = dict(case=case, ncp=n, lam=lam, cond=float(np.linalg.cond(S)), eta=eta, eta_L=eta_l, phi=phi, phi_L=phi_l, ratio_eta=eta / den_eta,
               ratio_phi=phi / den_phi, emulation_ratio_eta=eta_b / den_eta, emulation_ratio_phi=phi_b / den_phi, S_against_oracle=d_S)
    RECORDS[case] = rec
    print(f"{case}: cond {rec['cond']:.1e} | eta {eta:.2e} LAPACK {eta_l:.2e} ratio {rec['ratio_eta']:.2f} (emulation {rec['emulation_ratio_eta']:.2f}) | "
          f"phi {phi:.2e} LAPACK {phi_l:.2e} ratio {rec['ratio_phi']:.2f} (emulation {rec['emulation_ratio_phi']:.2f}) | S - oracle {d_S:.1e}")
    assert d_S < 1e-9, (case, d_S)
    assert eta <= R_ETA * den_eta, (case, eta, eta_l, rec["ratio_eta"])
    if phi > R_PHI * den_phi:  # beyond what is adopted as a tolerance: the suite's existing bounds, the measured ratio beside them
        print(f"{case}: phi ratio {rec['ratio_phi']:.1f} is beyond R_PHI = {R_PHI:g}; held to the suite's bounds")
        rec["beyond_R_phi"] = True
        assert np.linalg.norm(S @ s - rhs) < 1e-7 * np.linalg.norm(rhs), (case, rec["ratio_phi"])
        assert lam not in SUITE_STEP_BOUND or phi < SUITE_STEP_BOUND[lam], (case, phi, rec["ratio_phi"])
    return rec


@pytest.mark.parametrize("lam", D.LAMS)
@pytest.mark.parametrize("ncp, route, assembly", SWEEP_CASES, ids=[f"ncp{n}-{r}-{a}" for n, r, a in SWEEP_CASES])
def test_sweep(ncp, route, assembly, lam, monkeypatch):
    hip = _handle(D.rig(ncp), monkeypatch, route, assembly)
    _check_system_and_accuracy(*_step(hip, lam), ("rig", ncp), lam, f"ncp{ncp}-{route}-{assembly}-lam{lam:g}")
    hip.close()


@pytest.mark.parametrize("ncp, route", [(33, "small"), (33, "blocked"), (129, "blocked")])
def test_deterministic_handles_repeat_to_the_bit(ncp, route, monkeypatch):
    got = []
    for _ in range(2):
        hip = _handle(D.rig(ncp), monkeypatch, route, deterministic=True)
        for _ in range(2):
            ok, S, rhs, s = _step(hip, 1e-3)
            assert ok
            got.append((S.tobytes(), rhs.tobytes(), s.tobytes()))
        hip.close()
    assert all(g == got[0] for g in got[1:]), [tuple(a == b for a, b in zip(g, got[0])) for g in got[1:]]


UNOBSERVED_CASES = [(n_cams, route, which) for ncp, n_cams in D.UNOBSERVED for route in (("small", "blocked") if ncp <= D.SMALL_N else ("blocked",))
                    for which in ("first", "sixth", "last")]


@pytest.mark.parametrize("n_cams, route, which", UNOBSERVED_CASES, ids=[f"ncp{6 * n}-{r}-{w}" for n, r, w in UNOBSERVED_CASES])
def test_camera_without_observations(n_cams, route, which, monkeypatch):
    stripped = {"first": 0, "sixth": 5, "last": n_cams - 1}[which]
    key, own = ("unobserved", n_cams, stripped), slice(6 * stripped, 6 * stripped + 6)
    sc = D.unobserved_rig(n_cams, stripped)
    case = f"ncp{6 * n_cams}-{route}-camera{stripped}-unobserved"
    # lam = 1e-3 on fresh handles, with atomic and with fixed-order sums: rows lam I and a zero right-hand side, step entries exactly zero
    fresh = {}
    for det in (False, True):
        hip = _handle(sc, monkeypatch, route, deterministic=det)
        ok, S, rhs, s = _step(hip, 1e-3)
        assert np.array_equal(S[own], 1e-3 * np.eye(6 * n_cams)[own]) and np.all(rhs[own] == 0.0), case
        assert ok and np.all(s[own] == 0.0), (case, s[own])
        _check_system_and_accuracy(ok, S, rhs, s, key, 1e-3, f"{case}-{'deterministic' if det else 'atomic'}")
        fresh[det] = s
        hip.close()
    # lam = 0: the pivot of the camera's first parameter is exactly 0 — a failed step (so says the oracle) that leaves nothing non-finite ...
    hip = _handle(sc, monkeypatch, route, deterministic=True)
    ok, S, rhs, s = _step(hip, 0.0)
    assert not np.any(S[own]) and not D.oracle_engine(key).newton_step(0.0).ok
    print(f"{case}: lam = 0 reported {'ok' if ok else 'failed'}, max |s| {np.abs(s).max():.2e}")
    assert not ok, case
    assert np.all(np.isfinite(s)), case
    # ... and the next step on the SAME handle is a fresh handle's, to the bit
    ok, S, rhs, s = _step(hip, 1e-3)
    _check_system_and_accuracy(ok, S, rhs, s, key, 1e-3, f"{case}-after-failed-pivot")
    assert s.tobytes() == fresh[True].tobytes(), (case, float(np.abs(s - fresh[True]).max()))
    hip.close()
