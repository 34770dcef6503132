"""The scenes of tests/covariance_constrained_edge_scenes.py on the CPU: that each is what its name says (read from the host plan of its call
and from its arrays), that each is fit to test with (six null eigenvalues, the seventh above 1e-7 of the largest, the two CPU formulations
agreeing to 1e-8: the tolerance rule asserts the first and the last itself), and the g++ harnesses of both constrained calls on them under
the rule of tests/test_uncertainty_constrained.py and tests/test_reliability_constrained.py, unchanged (ten times the disagreement of the
two CPU formulations, floor 1e-12).  tests/test_covariance_constrained_edges_gpu.py runs the device on the same scenes and says which loop
of which kernel each one is for.

Measured: J, kept rows, ncp; the disagreement of the two CPU formulations of the covariance (camera block, point blocks); the seventh
eigenvalue relative to the largest; the harness's error against the pseudo-inverse (camera block, point blocks).

    NINE_MIXED             2187 x 423    57   63    4.3e-13  6.9e-13   2.0e-05   4.9e-13  6.9e-13
    NINE_MIXED_RELABELLED  2187 x 423    57   63    5.1e-12  2.6e-12   2.0e-05   5.2e-12  2.6e-12
    SIXTY_FIVE             3902 x 480    10  390    6.9e-15  2.4e-14   1.4e-03   5.8e-15  2.2e-14
    STICKS_257             3341 x 1560  257   18    3.1e-14  1.4e-14   4.8e-04   3.0e-14  1.7e-14
    STICKS_256             3340 x 1560  256   18    7.7e-15  2.6e-14   4.8e-04   7.9e-15  2.8e-14
    SIZES                   965 x 324   165   24    2.9e-15  5.3e-15   5.7e-03   5.0e-15  7.6e-15

(On the two scenes with nine-wide cameras the pseudo-inverse is the less exact of the two formulations and the harness follows the
bordered formula, so its error and the disagreement move together; both change by up to a factor of ten with the BLAS numpy runs on and
with the order of the unknowns, which is all that differs between NINE_MIXED and its relabelling.)  |J N6| is at most 1e-15 on every scene.
SIZES has 38 points in no row (100 less 54, 4, 2 and 2).

Reliability: the disagreement of the dense projector and the block formula, the error of R_oo, of the constraint r_j, of w times r_j
(observations, rows), the smallest reference r of an observation and of a row.

    NINE_MIXED             2.3e-13   2.4e-13  3.3e-15   1.2e-13  1.6e-15   0.25   0.39
    NINE_MIXED_RELABELLED  8.5e-13   8.6e-13  7.3e-15   4.3e-13  3.9e-15   0.25   0.39
    SIXTY_FIVE             3.1e-15   1.4e-15  2.2e-15   1.2e-15  1.5e-15   0.34   0.64
    STICKS_257             1.1e-14   1.2e-14  2.3e-15   5.7e-15  1.1e-15   0.086  0.073
    STICKS_256             3.3e-14   3.3e-14  2.3e-15   1.6e-14  1.4e-15   0.086  0.073
    SIZES                  1.4e-15   1.7e-15  1.6e-15   1.4e-15  1.2e-15   0.20   0.21

STICKS_256 gives its last row the weight zero.  Such a row leaves the adjustment (tests/test_reliability_constrained.py): it is no row
of J, it does not count in dof, and the call leaves NaN in its three outputs.  The references of STICKS_256 are therefore formed on
STICKS_256_KEPT, the same call stated without that row, and the rule is applied to the 256 rows that take part; that the 257th is NaN,
and nothing else, is asserted beside it.

The file takes about 15 s, five of them the compilation of the two harnesses.
"""
import dataclasses
import re

import numpy as np
import pytest

from caliscope_amd.exceptions import BackendError
from tests import covariance_constrained_edge_scenes as es
from tests import covariance_constrained_native as ccn
from tests import reliability_constrained_native as rcn

SCENES = {"nine_mixed": es.NINE_MIXED, "nine_mixed_relabelled": es.NINE_MIXED_RELABELLED, "sixty_five": es.SIXTY_FIVE, "sticks_257": es.STICKS_257,
          "sticks_256": es.STICKS_256, "sizes": es.SIZES}
REFERENCE_OF = {es.STICKS_256: es.STICKS_256_KEPT}  # the scene whose references a scene is held to, where it is not the scene itself
OVER_CAP_WORDS = "the constraint component of point 0 has 55 points: a component holds at most 54"

# name -> (J rows, J columns, kept rows, ncp, components, max_m, free points, observations)
EXPECTED = {
    "nine_mixed": (2187, 423, 57, 63, 4, 12, 94, 1065),
    "nine_mixed_relabelled": (2187, 423, 57, 63, 4, 12, 94, 1065),
    "sixty_five": (3902, 480, 10, 390, 3, 4, 21, 1946),
    "sticks_257": (3341, 1560, 257, 18, 257, 2, 0, 1542),
    "sticks_256": (3340, 1560, 256, 18, 256, 2, 2, 1542),
    "sizes": (965, 324, 165, 24, 4, 54, 38, 400),
}


def harness_covariance(key):
    return ccn.HarnessConstrainedUncertainty().parameter_covariance_constrained(*ccn.call_arguments(ccn.key_scene(key)))


def harness_reliability(key):
    return rcn.HarnessConstrainedReliability().observation_reliability_constrained(*rcn.call_arguments(key))


def kept_rows(result, key):
    """``result`` of a scene with rows of weight zero, after the assertion that its three constraint outputs are NaN on exactly those rows,
    with the rows that take part alone: what the dense reference of the adjustment has rows for."""
    keep = ccn.key_scene(key)["con"][3] > 0
    for name in ("constraint_redundancy", "constraint_w", "constraint_residual"):
        nan = np.isnan(getattr(result, name))
        assert np.array_equal(nan, ~keep), f"{name}: NaN on the caller's rows {np.flatnonzero(nan).tolist()}, weight zero on {np.flatnonzero(~keep).tolist()}"
    return dataclasses.replace(result, constraint_redundancy=result.constraint_redundancy[keep], constraint_w=result.constraint_w[keep],
                               constraint_residual=result.constraint_residual[keep])


def check_covariance(result, key, report=print):
    """covariance_constrained_native.check_against_pinv, on the references of the scene's adjustment."""
    return ccn.check_against_pinv(result, REFERENCE_OF.get(key, key), report=report)


def check_reliability(result, key, report=print):
    """reliability_constrained_native.check_against_dense, on the references of the scene's adjustment and the rows that take part in it."""
    if key in REFERENCE_OF:
        return rcn.check_against_dense(kept_rows(result, key), REFERENCE_OF[key], report=report)
    return rcn.check_against_dense(result, key, report=report)


def named(name):
    """The points and constraint rows a scene exists for: ([(point, what)], [(caller's row, what)])."""
    if name.startswith("nine_mixed"):
        perm = ccn.key_scene(SCENES[name]).get("perm", np.arange(120))
        points = [(0, "of the four-point component, the one camera 4 still sees"), (1, "of the four-point component, not seen by camera 4"),
                  (10, "of the twelve-point component that camera 7 is blind to: eight cameras"), (30, "of the two-point component"),
                  (40, "of the eight-point component"), (50, "in no row")]
        return [(int(perm[p]), f"point {p} of NINE_MIXED, {what}") for p, what in points], [(0, "first row of the four-point component"), (36, "centroid row of the twelve-point component"), (56, "centroid row of the eight-point component")]
    return {
        "sixty_five": ([(0, "65 cameras: one live lane in the second trip over its entries"), (5, "64 cameras: camera 64 is blind to its component"), (12, "of the three-point component"), (20, "in no row")],
                       [(0, "the stick of points 0 and 1"), (1, "first row of the component with 64 cameras"), (9, "last row")]),
        "sticks_257": ([(0, "of the first stick"), (511, "of stick 255"), (513, "of the last stick: workgroup 256 of k_unc_component")],
                       [(0, "first row"), (255, "last row of the first workgroup of k_unc_con_rows"), (256, "last row: the one live lane of the second workgroup")]),
        "sticks_256": ([(0, "of the first stick"), (511, "of the last stick"), (512, "free: its row has weight zero"), (513, "free: its row has weight zero")],
                       [(0, "first row"), (255, "last row of the one workgroup of k_unc_con_rows")]),
        "sizes": ([(0, "first of the component of 54"), (53, "last of the component of 54"), (60, "of the component of four"), (70, "of a component of two"), (81, "of the last component of two"), (90, "in no row")],
                  [(0, "first row of the component of 54"), (156, "centroid row of the component of 54"), (157, "first row of the component of four"), (164, "last row: a component of two")]),
    }[name]


def check_named(name, cov=None, rel=None):
    """The blocks of the named points and rows of a scene against the dense references under the rule, each named in the message when it fails:
    the 3 x 3 covariance block of a point (relative to its largest entry), the R_oo of each of its observations and the r_j of a row (absolute)."""
    key = SCENES[name]
    ref_key = REFERENCE_OF.get(key, key)
    sc = ccn.key_scene(key)
    points, rows = named(name)
    if cov is not None:
        ref = ccn.reference(ref_key)
        tol = max(10.0 * ref["dis_p"], 1e-12)
        for p, what in points:
            want = ref["sigma0_sq"] * ref["pp"][p]
            err = float(np.max(np.abs(cov.point_cov[p] - want)) / np.max(np.abs(want)))
            assert err <= tol, f"{name}: point {p} ({what}): its 3 x 3 block is {err:.3e} off the pseudo-inverse, tolerance {tol:.3e}"
    if rel is not None:
        ref = rcn.reference(ref_key)
        tol = max(10.0 * ref["dis"], 1e-12)
        for p, what in points:
            for o in np.flatnonzero(sc["obj"] == p):
                err = float(np.max(np.abs(rel.redundancy[o] - ref["R"][o])))
                assert err <= tol, f"{name}: observation {o} (camera {sc['cam'][o]}) of point {p} ({what}): its R_oo is {err:.3e} off the dense projector, tolerance {tol:.3e}"
        for j, what in rows:
            err = float(abs(rel.constraint_redundancy[j] - ref["rc"][j]))  # (a row of weight zero is the caller's last: the rows before it keep their numbers)
            assert err <= tol, f"{name}: constraint row {j} ({what}): its redundancy number is {err:.3e} off the dense projector, tolerance {tol:.3e}"
            want = rel.constraint_residual[j] / np.sqrt(ref["sigma0_sq"] * ref["rc"][j])  # the rule on w: relative within tol / r_j
            err = float(abs(rel.constraint_w[j] - want) * ref["rc"][j] / abs(want))
            assert err <= tol, f"{name}: constraint row {j} ({what}): its w is {err:.3e} / r_j off f~ / (sigma0 sqrt(r_j)) of the dense reference, tolerance {tol:.3e} / r_j"


def check_relabelling(cov, cov_moved, rel, rel_moved):
    """The outputs of NINE_MIXED_RELABELLED are those of NINE_MIXED with the points renamed; no observation or constraint row changed its place.
    Each result is within its scene's tolerance of its scene's reference, and the references are one quantity under two names: the two differ by at
    most the sum of the two tolerances.  No sum of a residual crosses a point or a row: those are equal to the bit."""
    perm = ccn.key_scene(es.NINE_MIXED_RELABELLED)["perm"]
    a, b = ccn.reference(es.NINE_MIXED), ccn.reference(es.NINE_MIXED_RELABELLED)
    tol_c = max(10.0 * a["dis_c"], 1e-12) + max(10.0 * b["dis_c"], 1e-12)
    tol_p = max(10.0 * a["dis_p"], 1e-12) + max(10.0 * b["dis_p"], 1e-12)
    err_c = float(np.abs(cov_moved.cam_cov_full - cov.cam_cov_full).max() / np.abs(cov.cam_cov_full).max())
    err_p = np.abs(cov_moved.point_cov[perm] - cov.point_cov).max(axis=(1, 2)) / np.abs(cov.point_cov).max(axis=(1, 2))
    ra, rb = rcn.reference(es.NINE_MIXED), rcn.reference(es.NINE_MIXED_RELABELLED)
    tol = max(10.0 * ra["dis"], 1e-12) + max(10.0 * rb["dis"], 1e-12)
    err_R = float(np.abs(rel_moved.redundancy - rel.redundancy).max())
    err_rc = float(np.abs(rel_moved.constraint_redundancy - rel.constraint_redundancy).max())
    print(dict(err_c=err_c, tol_c=tol_c, err_p=float(err_p.max()), tol_p=tol_p, err_R=err_R, err_rc=err_rc, tol=tol))
    assert err_c <= tol_c, (err_c, tol_c)
    worst = int(np.argmax(err_p))
    assert err_p[worst] <= tol_p, f"point {worst} (renamed {perm[worst]}): its block moved by {err_p[worst]:.3e} under the relabelling, tolerance {tol_p:.3e}"
    assert (cov_moved.dof, cov_moved.n_constraint_rows) == (cov.dof, cov.n_constraint_rows) and abs(cov_moved.cost - cov.cost) <= 2e-12 * cov.cost
    assert err_R <= tol and err_rc <= tol, (err_R, err_rc, tol)
    assert np.array_equal(rel_moved.residual, rel.residual) and np.array_equal(rel_moved.constraint_residual, rel.constraint_residual)
    relative = lambda w1, w0, r: np.abs(w1 - w0) * np.abs(r) / np.maximum(np.abs(w0), 1e-300)  # the rule on w: relative within tol / r_j
    assert relative(rel_moved.w, rel.w, np.stack([rel.redundancy[:, 0, 0], rel.redundancy[:, 1, 1]], axis=1)).max() <= tol
    assert relative(rel_moved.constraint_w, rel.constraint_w, rel.constraint_redundancy).max() <= tol
    assert rel_moved.dof == rel.dof


# ---- the scenes are what their names say --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EXPECTED))
def test_scene_has_the_sizes_its_name_says(name):
    d = es.describe(SCENES[name])
    j_rows, j_cols, n_rows, ncp, n_comp, max_m, n_free, n_obs = EXPECTED[name]
    assert (d["n_rows"], d["ncp"], d["n_comp"], d["max_m"], d["n_free"], d["n_obs"]) == (n_rows, ncp, n_comp, max_m, n_free, n_obs)
    n_points = len(d["entries"])
    assert (2 * n_obs + n_rows, ncp + 3 * n_points) == (j_rows, j_cols)
    assert n_free + sum(len(m) for m in d["members"]) == n_points
    for k, (members, cams) in enumerate(zip(d["members"], d["cams"])):  # a constrained point has one entry per camera of its component, a free one none
        assert (d["entries"][members] == len(cams)).all(), k
    assert not d["entries"][d["plan"]["free_pts"]].any()


def test_nine_mixed_cameras_widths_and_views():
    d = es.describe(es.NINE_MIXED)
    assert d["widths"] == es.NINE_WIDTHS and d["offsets"] == (0, 9, 15, 21, 30, 36, 42, 51, 57)
    assert any(o % 6 and o % 9 for o in d["offsets"])  # offsets that are multiples of neither width
    assert d["members"] == [list(g) for g in es.NINE_GROUPS] and [len(m) for m in d["members"]] == [4, 12, 2, 8]
    blind_cam, blind_comp = es.NINE_BLIND
    assert d["cams"] == [[c for c in range(9) if (c, k) != (blind_cam, blind_comp)] for k in range(4)]  # nine cameras on three components, eight on one
    for k in range(4):
        assert {d["widths"][c] for c in d["cams"][k]} == {6, 9}  # mixed widths inside every component
    assert [9 * len(c) - 64 for c in d["cams"]] == [17, 8, 17, 17]  # the live lanes of k_rel_con_rows's second trip
    assert [len(c) ** 2 - 64 for c in d["cams"]] == [17, 0, 17, 17]  # k_unc_point_cov's pair loop: 81 pairs, and one whole trip on eight cameras
    one_cam, one_point = es.NINE_ONE_POINT
    seen = d["cc_obs"][0][d["cams"][0].index(one_cam)]
    assert seen == [es.NINE_GROUPS[0].index(one_point)]  # camera 4 sees one point of the four-point component
    assert all(sorted(loc) == list(range(len(d["members"][k]))) for k in range(4) for c, loc in zip(d["cams"][k], d["cc_obs"][k]) if (c, k) != (one_cam, 0))
    assert sorted(set(d["entries"].tolist())) == [0, 8, 9]  # k_rel_con_point: entry trips of 4 + 4 + 1 and of 4 + 4
    assert max(len(c) for c in d["cams"]) == 9 > min(len(c) for c in d["cams"])  # vstride comes from the widest component, and one is narrower


def test_relabelled_components_lie_among_each_other_and_the_free_points():
    sc, plain = ccn.key_scene(es.NINE_MIXED_RELABELLED), ccn.key_scene(es.NINE_MIXED)
    perm = sc["perm"]
    assert sorted(perm.tolist()) == list(range(120)) and np.array_equal(sc["obj"], perm[plain["obj"]]) and np.array_equal(sc["cam"], plain["cam"])
    ncp = sc["par"].n_camera_params
    assert np.array_equal(sc["x"][ncp:].reshape(-1, 3)[perm], plain["x"][ncp:].reshape(-1, 3)) and np.array_equal(sc["x"][:ncp], plain["x"][:ncp])
    d, d0 = es.describe(es.NINE_MIXED_RELABELLED), es.describe(es.NINE_MIXED)
    assert sorted(d["members"]) == sorted(sorted(perm[m].tolist()) for m in d0["members"])  # the same bodies under their new names
    assert [m[0] for m in d["members"]] == sorted(m[0] for m in d["members"])  # components in the order of their smallest point
    free = set(d["plan"]["free_pts"].tolist())
    for k, members in enumerate(d["members"]):
        span = set(range(members[0], members[-1] + 1))
        assert len(members) < len(span), k  # not contiguous
        assert span & free, k  # free points between its points
        assert any(span & set(other) for j, other in enumerate(d["members"]) if j != k), k  # and points of another component
    for members in d["members"]:  # the indirection the kernels follow: a row's local indices name the points of its component
        assert members == sorted(members)
    p = d["plan"]
    ga, gb = sc["con"][0], sc["con"][1]
    for k in range(d["n_comp"]):
        pts = np.asarray(d["members"][k])
        for r in range(p["comp_row"][k], p["comp_row"][k + 1]):
            src = p["row_src"][r]
            assert np.array_equal(pts[p["row_loc"][8 * r: 8 * r + 8]], np.concatenate([ga[src], gb[src]]))
    one_cam, one_point = es.NINE_ONE_POINT
    k = next(k for k, m in enumerate(d["members"]) if perm[one_point] in m)
    assert d["cc_obs"][k][d["cams"][k].index(one_cam)] == [d["members"][k].index(perm[one_point])]
    blind_cam, blind_comp = es.NINE_BLIND
    k = next(k for k, m in enumerate(d["members"]) if perm[es.NINE_GROUPS[blind_comp][0]] in m)
    assert blind_cam not in d["cams"][k] and len(d["cams"][k]) == 8


def test_sixty_five_cameras_a_component():
    d = es.describe(es.SIXTY_FIVE)
    assert d["widths"] == (6,) * 65 and d["members"] == [list(g) for g in es.SIXTY_FIVE_GROUPS]
    assert [len(c) for c in d["cams"]] == [65, 64, 65] and es.SIXTY_FIVE_BLIND[0] not in d["cams"][es.SIXTY_FIVE_BLIND[1]]
    wave, groups = 64, 4  # COV_POINT_THREADS; the entry groups of a trip of k_rel_con_point
    k = int(d["entries"][0])
    assert (k - wave, k * k, -(-k // groups), k % groups) == (1, 4225, 17, 1)  # k_unc_point_cov: one live lane in the second trip over the entries; 17 entry trips, one group in the last
    assert d["entries"][5] == 64 == 16 * groups  # sixteen whole trips on the component camera 64 is blind to
    assert -(-9 * k // wave) == 10  # the trips of k_rel_con_rows
    assert d["n_rows"] == 1 + 6 + 3


@pytest.mark.parametrize("name,rows,free", [("sticks_257", 257, []), ("sticks_256", 256, [512, 513])])
def test_sticks_are_components_of_two_points_and_one_row(name, rows, free):
    d = es.describe(SCENES[name])
    assert d["widths"] == (6, 6, 6)
    assert d["members"] == [[2 * i, 2 * i + 1] for i in range(rows)] and d["cams"] == [[0, 1, 2]] * rows
    p = d["plan"]
    assert p["comp_row"].tolist() == list(range(rows + 1)) and p["row_src"].tolist() == list(range(rows))
    assert p["free_pts"].tolist() == free
    block, compute_units = 256, 256  # COV_BLOCK of k_unc_con_rows; the compute units of an MI355X
    assert (d["n_rows"] - block, d["n_comp"] - compute_units) == ((1, 1) if name == "sticks_257" else (0, 0))  # one live lane in a second workgroup; one whole workgroup
    w = ccn.key_scene(SCENES[name])["con"][3]
    assert len(w) == 257 and np.count_nonzero(w > 0) == rows and (w[:256] == 1.0).all()


def test_sticks_256_kept_is_the_adjustment_of_sticks_256():
    a, b = ccn.key_scene(es.STICKS_256), ccn.key_scene(es.STICKS_256_KEPT)
    for name in ("x", "cam", "obj", "uv"):
        assert a[name] is b[name]
    keep = a["con"][3] > 0
    assert keep.tolist() == [True] * 256 + [False]
    for whole, part in zip(a["con"], b["con"]):
        assert np.array_equal(whole[keep], part)


def test_sizes_holds_three_component_sizes_in_one_call():
    d = es.describe(es.SIZES)
    assert d["widths"] == (6, 6, 6, 6) and d["members"] == [list(g) for g in es.SIZES_GROUPS]
    assert [len(m) for m in d["members"]] == [ccn.constants()["cap"], 4, 2, 2] and d["max_m"] == 54 > 4 > 2
    assert np.diff(d["plan"]["comp_row"]).tolist() == [53 + 52 + 51 + 1, 6, 1, 1]
    assert d["cams"] == [[0, 1, 2, 3]] * 4


def test_weights_and_distances_of_the_rows():
    for key in SCENES.values():
        sc = ccn.key_scene(key)
        ga, gb, dist, w = sc["con"]
        pts = sc["x"][sc["par"].n_camera_params:].reshape(-1, 3)
        length = np.linalg.norm(pts[ga].mean(axis=1) - pts[gb].mean(axis=1), axis=1)
        assert set(w.tolist()) <= {0.0, 1.0} and (dist > 0.02).all()
        assert 0.0 < np.abs(length - dist).max() < 5 * 0.002  # the distance the points have plus N(0, 2 mm)
        corner = (ga[:, :1] == ga).all(axis=1)
        assert ((gb[:, :1] == gb).all(axis=1) == corner).all()
        centroid = np.flatnonzero(~corner)
        assert all(len(set(ga[j]) | set(gb[j])) == 8 for j in centroid)
    assert len(np.flatnonzero(~(ccn.key_scene(es.NINE_MIXED)["con"][0][:, :1] == ccn.key_scene(es.NINE_MIXED)["con"][0]).all(axis=1))) == 2
    assert len(np.flatnonzero(~(ccn.key_scene(es.SIZES)["con"][0][:, :1] == ccn.key_scene(es.SIZES)["con"][0]).all(axis=1))) == 1


# ---- the harnesses against the dense references --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_covariance_harness_matches_the_pseudo_inverse(name):
    key = SCENES[name]
    res = harness_covariance(key)
    figures = check_covariance(res, key)
    assert figures["lam7"] > 1e-7 and ccn.reference(REFERENCE_OF.get(key, key))["jn"] < 1e-12  # the seventh eigenvalue is far from the six; J N6 = 0
    assert np.isfinite(res.point_cov).all()
    assert res.n_constraint_rows == EXPECTED[name][2]


@pytest.mark.parametrize("name", list(SCENES))
def test_reliability_harness_matches_the_dense_projector(name):
    key = SCENES[name]
    figures = check_reliability(harness_reliability(key), key)
    assert figures["lam7"] > 1e-7


@pytest.mark.parametrize("name", list(SCENES))
def test_named_points_and_rows_of_the_harnesses(name):
    key = SCENES[name]
    points, rows = named(name)
    d = es.describe(key)
    constrained = {p for m in d["members"] for p in m}
    assert any(p in constrained for p, _ in points) and all(0 <= j < len(ccn.key_scene(key)["con"][2]) for j, _ in rows)
    check_named(name, cov=harness_covariance(key), rel=harness_reliability(key))


def test_relabelling_renames_the_outputs_of_the_harnesses():
    check_relabelling(harness_covariance(es.NINE_MIXED), harness_covariance(es.NINE_MIXED_RELABELLED), harness_reliability(es.NINE_MIXED),
                      harness_reliability(es.NINE_MIXED_RELABELLED))


def test_sticks_256_leaves_the_callers_last_row_nan():
    res = harness_reliability(es.STICKS_256)
    for arr in (res.constraint_redundancy, res.constraint_w, res.constraint_residual):
        assert arr.shape == (257,) and np.isnan(arr[256]) and np.isfinite(arr[:256]).all()
    assert res.n_constraints_uncontrolled == 0 and res.dof == harness_reliability(es.STICKS_257).dof - 1


# ---- the cap ---------------------------------------------------------------------------------------------------------------------------------
def test_a_component_over_the_cap_is_refused_by_both_harnesses():
    sc = ccn.key_scene(es.SIZES_OVER_CAP)
    assert len(sc["con"][2]) == len(ccn.key_scene(es.SIZES)["con"][2]) + 1
    with pytest.raises(RuntimeError, match=re.escape(OVER_CAP_WORDS)):
        es.describe(es.SIZES_OVER_CAP)
    for call in (harness_covariance, harness_reliability):
        with pytest.raises(BackendError, match=re.escape("(code -4)")) as info:
            call(es.SIZES_OVER_CAP)
        assert OVER_CAP_WORDS in str(info.value)
        assert call(es.SIZES).gauge_dim == 6
