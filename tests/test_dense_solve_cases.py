"""The cases, the reference and the yardstick of tests/test_dense_solve_gpu.py, checked without a device: the sweep's residues and block counts,
mixed rigs with a camera across a block boundary, the longdouble reference against a 40-digit LU, and LAPACK's Cholesky on the oracle's
reduced systems within the bound the device is then measured against (eta_L <= n 2^-53), with a float64 emulation of substitution by an
explicit T = L^-T beside it.  Figures are printed before they are asserted (``-s``)."""
import numpy as np
import pytest

from tests import dense_solve_cases as D


def test_sweep_residues_blocks_and_routes():
    table = {  # ncp: (composition, ncp % 32, blocks) as the sweep was chosen
        12: ((0, 2), 12, 1), 27: ((3, 0), 27, 1), 33: ((1, 4), 1, 2), 36: ((0, 6), 4, 2), 63: ((7, 0), 31, 2), 66: ((0, 11), 2, 3),
        96: ((0, 16), 0, 3), 99: ((11, 0), 3, 4), 126: ((14, 0), 30, 4), 129: ((1, 20), 1, 5), 159: ((1, 25), 31, 5), 192: ((0, 32), 0, 6),
        225: ((25, 0), 1, 8), 288: ((32, 0), 0, 9), 351: ((39, 0), 31, 11),
    }
    assert set(table) == set(D.SWEEP)
    for ncp, ((n9, n6), residue, blocks) in table.items():
        assert D.SWEEP[ncp][:4] == (n9, n6, residue, blocks)
        assert 9 * n9 + 6 * n6 == ncp == sum(D.widths(ncp)) and ncp % D.NB == residue and -(-ncp // D.NB) == blocks
        assert D.SWEEP[ncp][4] == (ncp <= D.SMALL_N)  # both routes up to SMALL_N, the blocked one alone beyond
    assert {D.SWEEP[n][2] for n in D.SWEEP if n > D.SMALL_N} >= {0, 1, 3, 30, 31}
    assert {D.SWEEP[n][3] for n in D.SWEEP if n <= D.SMALL_N} == {1, 2, 3}
    assert ((225 + 3) & ~3) == 228 and ((99 + 3) & ~3) == 100  # row strides of the work matrix that are not ncp
    for ncp, n_cams in D.UNOBSERVED:
        assert ncp == 6 * n_cams and (ncp <= D.SMALL_N) == (ncp == 66)
        assert 6 * 5 < D.NB < 6 * 6 and ncp % D.NB not in (0, D.NB - 1)  # camera 5 lies across 32; the last camera ends a ragged last block


@pytest.mark.parametrize("ncp", sorted(D.PINHOLE_AT))
def test_mixed_rigs_interleave_and_straddle(ncp):
    w, par = D.widths(ncp), D.rig(ncp)["par"]
    assert set(w) == {6, 9} and w[0] == 6 and w[-1] == 6  # the pinhole camera stands among the fisheye cameras
    assert tuple(b.n_params for b in par.blocks) == w and tuple(par.camera_param_offsets) == D.offsets(ncp)
    assert any(o % 9 for o in D.offsets(ncp)) and any(o % 6 for o in D.offsets(ncp))
    across = D.straddlers(ncp)
    print(ncp, across)
    assert across and all(o < b < o + wd for c, wd, b in across for o in [D.offsets(ncp)[c]])
    assert {wd for _, wd, _ in across} == ({6} if ncp == 33 else {6, 9})
    # the fisheye observations are those of the fisheye model: the residuals at the initial point are pixel noise and pose error, not a model gap
    from oracle.residuals import joint_residuals

    sc = D.rig(ncp)
    r = joint_residuals(sc["x0"], par, sc["cam"], sc["uv"], sc["obj"]).reshape(-1, 2)
    fish = np.isin(sc["cam"], [c for c, wd in enumerate(w) if wd == 6])
    assert fish.any() and (~fish).any() and np.abs(r[fish]).max() < 4 * np.abs(r[~fish]).max()


def test_reference_agrees_with_a_40_digit_lu():
    import mpmath

    S, rhs = D.oracle_system(("rig", 33), 1e-10)  # cond 2.7e11: the hardest of the three
    assert np.array_equal(S, S.T)
    x = D.reference_solve(S, rhs)
    with mpmath.workdps(40):
        xm = mpmath.lu_solve(mpmath.matrix(S.tolist()), mpmath.matrix(rhs.tolist()))
        xm = np.array([np.longdouble(mpmath.nstr(v, 25)) for v in xm])
    err = float(np.max(np.abs(x - xm)) / np.max(np.abs(xm)))
    unrefined = float(np.max(np.abs(D.reference_solve(S, rhs, refinements=0) - xm)) / np.max(np.abs(xm)))
    print(f"reference against mpmath: {err:.2e} (without refinement {unrefined:.2e})")
    assert err <= 1e-17
    assert unrefined > 1e-14  # (the refinement is what gets it there: cond u_longdouble ~ 1e-8 is all the plain solve promises)
    assert D.eta(S, rhs, x) < 1e-19 and D.phi(x, xm) == err


def test_metrics_on_a_known_system():
    S = np.array([[4.0, 2.0], [2.0, 3.0]])
    x = np.array([1.0, -2.0])
    rhs = S @ x
    assert D.eta(S, rhs, x) == 0.0 and D.phi(x, x.astype(np.longdouble)) == 0.0
    off = x + np.array([0.0, 1e-3])
    assert abs(D.eta(S, rhs, off) - 3e-3 / (6.0 * 1.999 + 4.0)) < 1e-15 and abs(D.phi(off, x.astype(np.longdouble)) - 5e-4) < 1e-15
    assert D.lapack_solve(-S, rhs) is None
    with pytest.raises(np.linalg.LinAlgError):
        D.reference_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), rhs)


@pytest.mark.parametrize("ncp", sorted(D.SWEEP))
def test_lapack_and_the_explicit_inverse_on_the_oracle_systems(ncp):
    for lam in D.LAMS:
        S, rhs = D.oracle_system(("rig", ncp), lam)
        assert S.shape == (ncp, ncp) and np.all(np.isfinite(S)) and np.all(np.isfinite(rhs))
        x_ref = D.reference_solve(S, rhs)
        s_l, s_t, s_b = D.lapack_solve(S, rhs), D.explicit_inverse_solve(S, rhs), D.blocked_inverse_solve(S, rhs)
        assert s_l is not None
        eta_l, eta_t, eta_b = (D.eta(S, rhs, s) for s in (s_l, s_t, s_b))
        phi_l, phi_t, phi_b = (D.phi(s, x_ref) for s in (s_l, s_t, s_b))
        print(f"ncp={ncp} lam={lam:g} cond={np.linalg.cond(S):.1e}: eta LAPACK {eta_l:.1e} explicit T {eta_t:.1e} blocked {eta_b:.1e} | "
              f"phi LAPACK {phi_l:.1e} explicit T {phi_t:.1e} blocked {phi_b:.1e}")
        assert D.eta(S, rhs, x_ref) < 1e-19
        assert eta_l <= ncp * D.U53, (ncp, lam, eta_l)
        assert eta_t <= 16 * max(eta_l, D.U53), (ncp, lam, eta_t, eta_l)


@pytest.mark.parametrize("n_cams, stripped", [(11, 0), (11, 5), (11, 10), (18, 0), (18, 5), (18, 17)])
def test_unobserved_camera_in_the_oracle(n_cams, stripped):
    """Rows lam I and a zero right-hand side at lam > 0; at lam = 0 a pivot that is exactly 0, which the oracle reports as a failed step."""
    key = ("unobserved", n_cams, stripped)
    S, rhs = D.oracle_system(key, 1e-3)
    own = slice(6 * stripped, 6 * stripped + 6)
    assert np.array_equal(S[own], 1e-3 * np.eye(6 * n_cams)[own]) and np.all(rhs[own] == 0.0)
    s = D.lapack_solve(S, rhs)
    assert s is not None and np.all(s[own] == 0.0)
    ora = D.oracle_engine(key)
    assert ora.newton_step(1e-3).ok and np.all(ora.s[own] == 0.0)
    assert not ora.newton_step(0.0).ok


def test_device_tolerances_follow_the_measuring_rule():
    """R = 4 x the largest adopted ratio, rounded up to a power of two; nothing above 64 (eta) or 16 (phi) is adopted; the committed figures
    (profiles/dense_solve_accuracy.json, rewritten by a full run of tests/test_dense_solve_gpu.py) were taken with these tolerances."""
    import json

    from tests import test_dense_solve_gpu as G

    def rounded_up(ratio):
        return 2.0 ** np.ceil(np.log2(4 * ratio))

    assert max(G.MEASURED_ETA) <= G.LIMIT_ETA and G.R_ETA == rounded_up(max(G.MEASURED_ETA))
    assert max(G.MEASURED_PHI) > G.LIMIT_PHI and G.R_PHI == rounded_up(G.LIMIT_PHI)
    report = json.loads((G.ROOT / "profiles" / "dense_solve_accuracy.json").read_text())
    assert (report["R_eta"], report["R_phi"]) == (G.R_ETA, G.R_PHI)
    sweep = {f"ncp{n}-{r}-{a}-lam{lam:g}" for n, r, a in G.SWEEP_CASES for lam in D.LAMS}
    assert sweep <= {c["case"] for c in report["cases"]} and len(sweep) == 75
    assert report["largest_ratio_eta"]["ratio_eta"] <= G.LIMIT_ETA
    for c in report["cases"]:
        assert c["eta"] <= G.R_ETA * max(c["eta_L"], D.U53) and (c["phi"] <= G.R_PHI * max(c["phi_L"], c["ncp"] * D.U53) or c.get("beyond_R_phi")), c
