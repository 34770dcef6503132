"""The scenes of tests/robust_scenes.py are fit to test a robust-loss step with (no GPU): enough rows at the sqrt(EPS) floor to exercise the
clamp and not so many that a column is starved, a loss that is far from the identity, and two references that agree ten times better than
the bar the device is held to in tests/test_robust_step_gpu.py.  These are conditions on the inputs: a scene that misses one is changed (loss
scale, seed, FRACTION), not the condition."""
import numpy as np
import pytest

from tests import robust_scenes as rs

IDS = [f"{name}-{loss}" for name, loss in rs.ALL_SCENES]
STEP_BAR = {1e-3: 1e-8, 1e-7: 1e-7}  # device vs. splu in tests/test_robust_step_gpu.py; the references agree to a tenth of it


def _obs_rows(sc, ref):
    """Per scalar observation row: its point, its camera, whether it is off the floor."""
    return np.repeat(sc["obj"], 2), np.repeat(sc["cam"], 2), ~ref.floor[: ref.n_obs_rows]


def test_near_minimum_returns_the_four_shapes():
    for shape in rs.SHAPES:
        sc, par, x, f_scale = rs.near_minimum(shape, "huber")
        assert x.shape == (par.n_params,) and f_scale == 0.75 * sc.f_scale_1px()
        assert rs.near_minimum(shape, "cauchy")[2] is x  # (the oracle solve is shared among the losses)
    assert [len(rs.base_scene(s)["par"].blocks) for s in rs.SHAPES] == [6, 6, 24, 20]
    assert [rs.base_scene(s)["par"].blocks[0].n_params for s in rs.SHAPES] == [6, 9, 6, 9]


@pytest.mark.parametrize("name, loss", rs.ALL_SCENES, ids=IDS)
def test_floor_share_and_curved_rows(name, loss):
    ref = rs.reference(name, loss)
    share = float(ref.floor[: ref.n_obs_rows].mean())
    print(f"{name} {loss}: floor share {share:.3f}, rows with z > 0.05: {(ref.z > 0.05).mean():.2f}")
    if loss == "soft_l1":
        assert share == 0.0 and not ref.floor.any()
    else:
        assert 0.02 <= share <= 0.30
    assert (ref.z > 0.05).mean() >= 0.30


@pytest.mark.parametrize("name, loss", rs.ALL_SCENES, ids=IDS)
def test_every_point_keeps_rows_off_the_floor(name, loss):
    sc, ref = rs.scene(name, loss), rs.reference(name, loss)
    obj, cam, live = _obs_rows(sc, ref)
    P = sc["par"].n_points
    observed = np.unique(sc["obj"])
    rows = np.bincount(obj[live], minlength=P)[observed]
    pairs = np.unique(np.stack([obj[live], cam[live]], axis=1), axis=0)
    cams = np.bincount(pairs[:, 0], minlength=P)[observed]
    assert rows.min() >= 4 and cams.min() >= 2, (rows.min(), cams.min())


@pytest.mark.parametrize("name, loss", rs.ALL_SCENES, ids=IDS)
def test_column_scale(name, loss):
    ref = rs.reference(name, loss)
    d = ref.scale_inv[ref.has_rows]
    assert d.min() / np.median(d) >= 1e-3
    # the oracle's column norms against the same norms formed in np.longdouble: the device is held to ten times this figure
    print(f"{name} {loss}: min/median {d.min() / np.median(d):.1e}, scale_inv vs longdouble {ref.scale_inv_disagreement:.1e}")
    assert ref.scale_inv_disagreement <= 1e-9


def test_board_constraint_rows_under_huber():
    sc, ref = rs.scene("board", "huber"), rs.reference("board", "huber")
    ga, gb, dist, w = sc["constraints"]
    floor, z = ref.floor[ref.n_obs_rows:], ref.z[ref.n_obs_rows:]
    assert len(floor) == len(dist)
    assert len(set(ga[29])) == 4 and 29 in rs.BOARD_MOVED_ROWS  # (a centroid row among the moved ones)
    assert floor[list(rs.BOARD_MOVED_ROWS)].all() and floor.sum() >= 2
    assert (z > 0.05).mean() >= 0.25
    live_rows = np.zeros(sc["par"].n_points, dtype=int)
    for side in (ga, gb):
        for k in np.flatnonzero(~floor):
            live_rows[np.unique(side[k])] += 1
    constrained = np.unique(np.concatenate([ga.ravel(), gb.ravel()]))
    assert live_rows[constrained].min() >= 1
    # the soft_l1 board keeps the recorded distances
    assert np.array_equal(rs.scene("board", "soft_l1")["constraints"][2] != dist, np.isin(np.arange(len(dist)), rs.BOARD_MOVED_ROWS))


@pytest.mark.parametrize("name, loss", rs.ALL_SCENES, ids=IDS)
def test_references_agree(name, loss):
    ref = rs.reference(name, loss)
    for lam in rs.LAMS:
        st = ref.steps[lam]
        ds, dS = rs.rel(st.s_oracle, st.s_lu), rs.rel(st.S_oracle, st.S_ref)
        print(f"{name} {loss} lam={lam:g}: step {ds:.1e}, S {dS:.1e}")
        assert ds <= 0.1 * STEP_BAR[lam], lam
        assert dS <= 1e-10, lam


@pytest.mark.parametrize("name, loss", rs.ALL_SCENES, ids=IDS)
def test_the_loss_matters(name, loss):
    """The oracle's step under the loss against its linear-loss step at the same x: a kernel that ignored the loss could not pass."""
    ref = rs.reference(name, loss)
    for lam in rs.LAMS:
        assert rs.rel(ref.steps[lam].s_oracle, ref.s_linear[lam]) > 1e-3, lam


def test_longdouble_row_scale_is_scipys():
    """row_scale_longdouble restates scipy's loss functions: its double rounding is scipy's scale, its floor rows are scipy's."""
    from scipy.optimize._lsq.least_squares import construct_loss_function

    f = np.random.default_rng(0).normal(0, 1.5, 4000)
    for loss in rs.LOSSES:
        rho = construct_loss_function(len(f), loss, 0.8)(f)
        js = rho[1] + 2 * rho[2] * f ** 2
        mine, z, floor = rs.row_scale_longdouble(f, loss, 0.8)
        live = js >= 1e-12
        assert np.array_equal(floor[live], np.zeros(live.sum(), dtype=bool)) and floor[js < -1e-12].all()
        assert np.abs(mine[live].astype(np.float64) - js[live]).max() <= 1e-14
