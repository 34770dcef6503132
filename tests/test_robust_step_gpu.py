"""One damped step under a robust loss on the device, at the linear-loss bars and on ALL parameters (run with ``-m gpu``).

The scenes of tests/robust_scenes.py are evaluated near a minimum, where a few per cent of the rows sit at scipy's sqrt(EPS) floor and no
column is starved (tests/test_robust_scenes.py shows that on the CPU), so nothing is masked: every comparison of
tests/test_gpu_parity.py::_check_step's linear branch is made with its bar unchanged, against two references that share their inputs and
not their solves (the oracle's numpy Schur step, and the damped normal equations of scipy's own row scaling solved as one system by splu,
with S_ref formed from its blocks).  scale_inv has no project bar under a robust loss: the device is held, column by column, to ten times
the distance of the oracle's column norms from the same norms formed in np.longdouble, floor 1e-12 (the measured distance is 1e-15 on every
scene, so the floor decides).

Every test asserts the route it means to run (``cba_info``: plan_state, schur_groups, the build_camg bits, n_heavy_points) and prints its
figures before it asserts (``-s`` shows them).

Measured on an MI355X (largest difference over all parameters, relative to the largest entry).  Columns: share of the scalar observation
rows at the floor; disagreement of the two references in the step at lam = 1e-3 and 1e-7; the device's step against the oracle and
against splu at lam = 1e-3; the same at lam = 1e-7; the device's S against S_ref (the larger of the two lam); scale_inv against the
np.longdouble column norms (bound 1e-12); the largest ratio of a step or S figure to its bar (1e-8 | 1e-8, 2e-8 | 1e-7, 1e-9).

                                                 floor  references        lam = 1e-3        lam = 1e-7        S        scale_inv ratio
    L6 huber                                     0.099  1.5e-13 1.3e-09   4.8e-13 4.0e-13   2.2e-09 2.4e-09   1.8e-15  5.7e-16   0.11
    L6 soft_l1                                   0.000  1.4e-13 1.7e-09   6.5e-13 6.4e-13   3.4e-09 4.5e-09   2.6e-14  1.4e-13   0.17
    L6 cauchy                                    0.026  8.5e-14 2.0e-09   5.9e-13 6.7e-13   3.1e-09 4.5e-09   2.4e-14  1.5e-13   0.15
    L6 arctan                                    0.094  8.2e-14 7.1e-10   2.6e-13 2.6e-13   7.6e-10 1.3e-09   2.4e-14  3.4e-13   0.04
    R6 huber                                     0.095  4.5e-12 4.1e-11   2.5e-12 2.1e-12   4.1e-11 1.9e-11   1.5e-15  1.2e-15   0.00
    R6 soft_l1                                   0.000  3.1e-12 1.3e-11   2.2e-12 1.9e-12   1.6e-11 2.9e-11   3.1e-14  1.2e-13   0.00
    R6 cauchy                                    0.028  5.9e-13 1.9e-11   8.5e-13 5.0e-13   1.9e-11 5.4e-12   3.3e-14  1.1e-13   0.00
    R6 arctan                                    0.091  1.6e-12 1.3e-11   9.7e-13 1.9e-12   3.4e-11 4.4e-11   4.2e-14  2.6e-13   0.00
    L24 huber                                    0.114  1.3e-13 9.9e-10   8.0e-13 8.3e-13   1.1e-09 2.1e-09   2.4e-15  6.2e-16   0.05
    L24 soft_l1                                  0.000  9.9e-14 1.8e-09   7.7e-13 7.3e-13   1.7e-09 2.3e-09   2.1e-14  1.2e-13   0.08
    L24 cauchy                                   0.036  1.2e-13 6.2e-10   6.8e-13 6.6e-13   6.1e-10 9.8e-10   1.9e-14  1.7e-13   0.03
    L24 arctan                                   0.108  5.4e-14 3.4e-10   3.9e-13 4.2e-13   4.9e-10 5.5e-10   1.9e-14  1.2e-13   0.02
    R20 huber                                    0.104  2.6e-12 1.2e-11   1.4e-12 2.4e-12   1.4e-11 3.8e-12   1.5e-15  1.8e-15   0.00
    R20 soft_l1                                  0.000  3.3e-12 8.4e-12   1.9e-12 2.6e-12   1.2e-11 3.6e-12   2.9e-14  1.5e-13   0.00
    R20 cauchy                                   0.031  2.2e-12 8.1e-12   1.4e-12 2.1e-12   1.7e-11 1.1e-11   2.3e-14  1.6e-13   0.00
    R20 arctan                                   0.100  3.2e-12 3.3e-12   1.1e-12 3.0e-12   4.0e-12 3.6e-12   2.9e-14  2.3e-13   0.00
    L6 soft_l1 point_ordered_build               0.000  1.4e-13 1.7e-09   6.3e-13 6.3e-13   9.9e-10 1.9e-09   2.6e-14  1.4e-13   0.05
    L6 huber point_ordered_build                 0.099  1.5e-13 1.3e-09   3.7e-13 3.7e-13   9.2e-10 1.2e-09   1.8e-15  5.7e-16   0.05
    R6 soft_l1 point_ordered_build               0.000  3.1e-12 1.3e-11   2.2e-12 2.0e-12   1.2e-11 2.5e-11   3.0e-14  1.2e-13   0.00
    R6 huber point_ordered_build                 0.095  4.5e-12 4.1e-11   2.8e-12 2.2e-12   4.3e-11 2.4e-11   1.5e-15  1.2e-15   0.00
    L6 soft_l1 camera_table_global               0.000  1.4e-13 1.7e-09   6.3e-13 6.3e-13   3.9e-09 5.0e-09   2.6e-14  1.4e-13   0.20
    L6 huber camera_table_global                 0.099  1.5e-13 1.3e-09   4.6e-13 3.8e-13   1.4e-09 1.6e-09   1.8e-15  5.7e-16   0.07
    R6 soft_l1 camera_table_global               0.000  3.1e-12 1.3e-11   2.2e-12 2.0e-12   1.5e-11 2.7e-11   3.1e-14  1.2e-13   0.00
    R6 huber camera_table_global                 0.095  4.5e-12 4.1e-11   2.5e-12 2.3e-12   4.2e-11 1.9e-11   1.8e-15  1.2e-15   0.00
    L6 soft_l1 deterministic                     0.000  1.4e-13 1.7e-09   6.7e-13 6.6e-13   8.3e-10 1.6e-09   2.6e-14  1.4e-13   0.04
    L6 huber deterministic                       0.099  1.5e-13 1.3e-09   4.6e-13 3.8e-13   1.5e-09 1.9e-09   1.8e-15  5.7e-16   0.07
    R6 soft_l1 deterministic                     0.000  3.1e-12 1.3e-11   2.2e-12 1.9e-12   1.5e-11 2.7e-11   3.1e-14  1.2e-13   0.00
    R6 huber deterministic                       0.095  4.5e-12 4.1e-11   2.7e-12 2.3e-12   3.7e-11 2.2e-11   1.8e-15  1.2e-15   0.00
    board huber                                  0.040  1.8e-14 2.4e-10   1.2e-13 1.1e-13   2.0e-10 2.2e-10   8.4e-16  6.0e-16   0.01
    board soft_l1                                0.000  6.2e-14 1.7e-09   7.9e-13 8.0e-13   8.4e-10 1.4e-09   1.8e-14  4.3e-14   0.04
    component_small soft_l1                      0.000  1.0e-13 1.6e-09   8.6e-13 8.4e-13   1.9e-09 1.0e-09   2.3e-14  1.9e-13   0.10
    component_large soft_l1                      0.000  1.1e-13 8.3e-10   1.2e-12 1.2e-12   8.1e-10 1.6e-09   1.5e-14  2.7e-13   0.04
    sparse_ids soft_l1 six                       0.000  3.1e-12 8.9e-10   1.0e-12 3.2e-12   5.2e-10 6.6e-10   8.3e-15  2.8e-13   0.03
    sparse_ids_refine soft_l1 nine               0.000  1.1e-12 1.2e-11   5.7e-13 6.5e-13   2.7e-11 3.1e-11   4.7e-15  1.9e-13   0.00
    sparse_ids_refine soft_l1 nine_backsub_rec_on 0.000  1.1e-12 1.2e-11   4.8e-13 6.7e-13   3.9e-11 4.3e-11   5.0e-15  1.9e-13   0.00
    fisheye_pinhole soft_l1                      0.000  5.7e-14 3.2e-10   5.2e-13 5.4e-13   1.6e-10 3.2e-10   6.8e-15  4.8e-14   0.01
    L6 linear (as created)                       0.000  2.6e-13 7.5e-09   1.6e-12 1.7e-12   4.5e-09 8.2e-09   1.2e-15  4.8e-16   0.22
    L6 after set_loss(cauchy)                    0.026  8.5e-14 2.0e-09   5.6e-13 6.4e-13   2.0e-09 3.4e-09   2.3e-14  1.5e-13   0.10
    L6 after set_loss(soft_l1)                   0.000  1.4e-13 1.7e-09   5.9e-13 5.9e-13   1.9e-09 2.8e-09   2.6e-14  1.4e-13   0.10

Nothing exceeds a quarter of a bar, so no allowance for the summation order of the atomics path is made: it is held to the same bars as the
fixed-order path.  The figures at lam = 1e-7 are those of the references among themselves (the gauge directions are held by the damping
alone there: cond(H) eps).  scale_inv is at 1e-13 wherever the row scale is not exactly 1 or the floor (soft_l1, cauchy, arctan: the
device forms rho' + 2 rho'' z in another order than scipy), a third of its bound at most.

Mutation runs of this file (one line of csrc/cba_kernels.h changed at a time, library rebuilt, file run once on the MI355X; each test
stops at its first failing figure, so the figures are those of the linearisation, bar 1e-10):

    1. obs_factors: row scale dropped from Aint[r][2]      17 of 37 fail: every nine-parameter case (default route R6 and R20 under all
       four losses, the six R6 variants, both nine-parameter sparse-id cases, fisheye + pinhole).  soft_l1: gh_sq off by 7e-2 (R6),
       6e-2 (R20), jg_sq by 5e-2 (k_build variants), 2e-2 (sparse ids); huber / cauchy / arctan: g_norm_inf 30 .. 150 against 0.005 .. 0.012
       (a floor row's residual is scaled by 1 / sqrt(EPS)); huber on the k_build variants: jg_sq off by 1.4e-3.  The six-parameter cases pass.
    2. obs_linearize: sqrt(rho') in place of sqrt(js) on B  11 of 37 fail: the cases whose linearisation runs k_build (point-ordered and
       fixed-order variants on L6 and R6, all three sparse-id cases, where the heavy point keeps the camera-sorted build off).  soft_l1:
       gh_sq off by 6e-2 (L6), 1.1e-1 (R6), 1.3e-1 (sparse ids); huber: g_norm_inf 2.5e4 / 3.3e4 against 0.013 / 0.012.
    3. k_con_eval: rs left out of w                         4 of 37 fail: both boards and both component scenes.  soft_l1: gh_sq off by
       3e-2 (board), 2.3e-2 / 2.4e-2 (components); huber: g_norm_inf 1.3e4 against 0.0033 (the rows moved to the floor).

No test of this file takes more than 0.6 s on the device (the sparse-id scenes, most of it their references); the file takes 4.4 s.
"""
import numpy as np
import pytest

from tests import robust_scenes as rs

pytestmark = pytest.mark.gpu

BUILD_CS, BACKSUB_REC, CON_SMALL = 4, 16, 32  # cba_info.build_camg bits
STEP_ORACLE = {1e-3: 1e-8, 1e-7: 2e-8}
STEP_LU = {1e-3: 1e-8, 1e-7: 1e-7}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension


def _handle(sc, monkeypatch, env=None, deterministic=False, loss=None, f_scale=None):
    """A HIP handle of a scene created under ``env`` (the switches are read by cba_create / cba_set_constraints)."""
    from caliscope_amd.hip_engine import HipEngine

    with monkeypatch.context() as m:
        for k, v in (env or {}).items():
            m.setenv(k, v)
        return HipEngine(rs.problem(sc, loss, f_scale), deterministic=deterministic)


def _close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


def check_step(hip, name, loss, label=None, second=True):
    """begin, linearize, the step at both lam with everything that hangs on it, accept and the second linearisation, against the shared
    references of (name, loss).  Returns the device's steps and reduced systems per lam."""
    sc, ref = rs.scene(name, loss), rs.reference(name, loss)
    label = label or f"{name} {loss}"
    ncp = sc["par"].n_camera_params
    cost = hip.begin(sc["x"])
    assert _close(cost, ref.cost, 1e-13), (label, cost, ref.cost)
    lin = hip.linearize()
    for fld in ("g_norm_inf", "gh_sq", "jg_sq", "x_scaled_norm", "x_norm"):
        assert _close(getattr(lin, fld), getattr(ref.lin, fld), 1e-10), (label, fld, getattr(lin, fld), getattr(ref.lin, fld))
    d_g = rs.rel(hip.get_vector(2), ref.g)
    assert d_g < 1e-11, (label, d_g)
    cols = ref.has_rows
    d_scale = float(np.max(np.abs(hip.get_vector(4) - ref.scale_inv_longdouble)[cols] / ref.scale_inv_longdouble[cols]))
    tol_scale = max(10.0 * ref.scale_inv_disagreement, 1e-12)
    print(f"{label}: floor share {ref.floor[:ref.n_obs_rows].mean():.3f}, gradient {d_g:.1e}, scale_inv {d_scale:.1e} (bound {tol_scale:.1e})")
    assert d_scale <= tol_scale, (label, d_scale, tol_scale)
    assert np.array_equal(hip.get_vector(4)[~cols], np.ones((~cols).sum()))  # (columns without rows: scale 1)
    out = {}
    for lam in rs.LAMS:
        st = ref.steps[lam]
        sh = hip.newton_step(lam)
        assert sh.ok, (label, lam)
        s = hip.get_vector(3)
        S, rhs = hip.reduced_system()
        th = hip.trial(*rs.TRIAL)
        gram = hip.subspace_gram(*rs.GRAM)
        d_ora, d_lu, d_S = rs.rel(s, st.s_oracle), rs.rel(s, st.s_lu), rs.rel(S, st.S_ref)
        print(f"{label} lam={lam:g}: references {rs.rel(st.s_oracle, st.s_lu):.1e} | step vs oracle {d_ora:.1e} ({d_ora / STEP_ORACLE[lam]:.2f} of the bar)"
              f", vs splu {d_lu:.1e} ({d_lu / STEP_LU[lam]:.2f}) | S {d_S:.1e} ({d_S / 1e-9:.3f})")
        assert d_ora < STEP_ORACLE[lam], (label, lam, d_ora)
        assert d_lu < STEP_LU[lam], (label, lam, d_lu)
        assert np.all(s[~cols] == 0.0), label  # (nothing moves a parameter without rows)
        assert d_S < 1e-9, (label, lam, d_S)
        assert np.abs(S - S.T).max() <= 1e-14 * np.abs(S).max(), (label, lam)
        assert np.linalg.norm(S @ s[:ncp] - rhs) < 1e-7 * np.linalg.norm(rhs), (label, lam)
        for fld in ("p_sq", "gh_dot_p", "w_sq"):
            assert _close(getattr(sh, fld), getattr(st, fld), 1e-7), (label, lam, fld, getattr(sh, fld), getattr(st, fld))
        assert np.allclose(gram, st.gram, rtol=1e-7, atol=0.0), (label, lam, gram, st.gram)
        assert th.finite and _close(th.cost, st.trial_cost, 1e-9), (label, lam, th.cost, st.trial_cost)
        assert _close(th.step_norm, st.trial_step_norm, 1e-7), (label, lam)
        out[lam] = (s, S)
    if second:  # the second linearisation exercises the monotone-max scale rule; the accepted points differ by the step tolerance
        hip.accept()
        lin2 = hip.linearize()
        assert _close(lin2.gh_sq, ref.lin2.gh_sq, 1e-7) and _close(lin2.jg_sq, ref.lin2.jg_sq, 1e-7), label
        assert rs.rel(hip.get_vector(4), ref.scale_inv2) < 1e-6, label
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", rs.LOSSES)
@pytest.mark.parametrize("shape", list(rs.SHAPES))
def test_default_route(shape, loss, monkeypatch):
    """The kernels a robust handle picks when left alone: the generic k_tprep / k_jv, obs_linearize / obs_factors with the row scale, the
    six-parameter compact record built from scaled G rows (L6, L24), the nine-parameter records (R6, R20), several camera groups (L24, R20)."""
    with _handle(rs.scene(shape, loss), monkeypatch) as hip:
        info = hip.info()
        assert info["plan_state"] == 0 and info["plan_error"] == 0, info
        assert (info["schur_groups"] > 1) == (shape in ("L24", "R20")), info
        assert info["build_camg"] & BUILD_CS and not info["build_camg"] & 2, info  # (camera-sorted build, camera table in LDS)
        check_step(hip, shape, loss)


VARIANTS = {
    "point_ordered_build": ({"CBA_BUILD_CS": "0"}, False),       # k_build
    "camera_table_global": ({"CBA_CAMTAB_GLOBAL": "1"}, False),  # the CAMG forms of k_cost, k_jv, k_tprep, k_backsub, k_build
    "deterministic": ({}, True),                                 # the DETM forms: sums in a fixed order
}


@pytest.mark.parametrize("loss", ["soft_l1", "huber"])
@pytest.mark.parametrize("shape", ["L6", "R6"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_variants(variant, shape, loss, monkeypatch):
    env, det = VARIANTS[variant]
    sc = rs.scene(shape, loss)
    with _handle(sc, monkeypatch, env=env, deterministic=det) as hip:
        bits = hip.info()["build_camg"]
        # bits 0 / 1: camera table through the vector cache (linearisation / every kernel); bit 2: camera-sorted build (off for
        # CBA_BUILD_CS=0 and for fixed-order sums), as tests/test_gpu_parity.py::_expect_build_variant reads them
        assert bool(bits & BUILD_CS) == (variant == "camera_table_global"), (variant, bits)
        assert (bits & 3) == (3 if variant == "camera_table_global" else 0), (variant, bits)
        out = check_step(hip, shape, loss, label=f"{shape} {loss} {variant}")
    if det:  # a second handle gives the same bytes
        with _handle(sc, monkeypatch, deterministic=True) as again:
            again.begin(sc["x"]); again.linearize()
            for lam in rs.LAMS:
                assert again.newton_step(lam).ok
                assert np.array_equal(again.get_vector(3), out[lam][0]), lam
                assert np.array_equal(again.reduced_system()[0], out[lam][1]), lam


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["huber", "soft_l1"])
def test_board_constraints(loss, monkeypatch):
    """k_con_eval<true> (under huber with rows at the floor: three moved distances, one of them a centroid row), k_con_jv, k_con_schur."""
    sc = rs.scene("board", loss)
    with _handle(sc, monkeypatch) as hip:
        assert hip.n_constraints == len(sc["constraints"][2]) == 180
        check_step(hip, "board", loss)


@pytest.mark.parametrize("name, small", [("component_small", True), ("component_large", False)])
def test_constraint_components(name, small, monkeypatch):
    """Two components of 55 rows (k_con_schur_small / k_con_backsub_small) and of 56 rows (the general kernels) over 12 points each, ncp = 24:
    the two sides of the small-component kernels' LDS limit (tests/test_kernel_edges_gpu.py COMPONENTS), under soft_l1."""
    sc = rs.scene(name, "soft_l1")
    assert sc["par"].n_camera_params == 24
    with _handle(sc, monkeypatch) as hip:
        bits = hip.info()["build_camg"]
        assert bool(bits & CON_SMALL) == small, bits
        check_step(hip, name, "soft_l1")


SPARSE = {  # scene, environment, k_backsub_rec expected
    "six": ("sparse_ids", {}, True),
    "nine": ("sparse_ids_refine", {}, False),
    "nine_backsub_rec_on": ("sparse_ids_refine", {"CBA_BACKSUB_REC": "1"}, True),
}


@pytest.mark.parametrize("mode", list(SPARSE))
def test_heavy_point_and_sparse_ids(mode, monkeypatch):
    """Chunk ranges of more than 512 point ids and a static marker of 256 observations (k_heavy_schur, the beyond-256-ids loops of k_build,
    k_backsub and k_backsub_rec) under soft_l1; unobserved points stand still."""
    name, env, rec = SPARSE[mode]
    sc = rs.scene(name, "soft_l1")
    with _handle(sc, monkeypatch, env=env) as hip:
        info = hip.info()
        assert bool(info["build_camg"] & BACKSUB_REC) == rec, info
        assert not info["build_camg"] & BUILD_CS and info["n_heavy_points"] == 1, info
        out = check_step(hip, name, "soft_l1", label=f"{name} soft_l1 {mode}")
    ncp = sc["par"].n_camera_params
    still = np.flatnonzero(~sc["observed"])
    assert len(still) > 4000 and np.all(out[1e-3][0][ncp:].reshape(-1, 3)[still] == 0.0)


def test_fisheye_and_pinhole(monkeypatch):
    """A six-parameter fisheye camera next to a nine-parameter pinhole camera under soft_l1."""
    sc = rs.scene("fisheye_pinhole", "soft_l1")
    assert [b.n_params for b in sc["par"].blocks] == [6, 9] and sc["par"].blocks[0].fisheye
    with _handle(sc, monkeypatch) as hip:
        check_step(hip, "fisheye_pinhole", "soft_l1")


def test_set_loss_on_a_live_handle(monkeypatch):
    """cba_set_loss: linear -> cauchy -> soft_l1 on one handle.  After each the step stands at the bar against the references of THAT loss
    (tests/test_linear_pass_gpu.py compares handle with handle at 1e-8)."""
    sc = rs.scene("L6", "linear")
    with _handle(sc, monkeypatch) as hip:
        check_step(hip, "L6", "linear", label="L6 linear (as created)")
        for loss in ("cauchy", "soft_l1"):
            hip.set_loss(loss, rs.scene("L6", loss)["f_scale"])
            check_step(hip, "L6", loss, label=f"L6 after set_loss({loss})")
