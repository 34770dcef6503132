"""cba_observation_reliability_constrained (include/caliscope/reliability_constrained.h) without a GPU: the whole call on the g++ build of the
shared headers (tests/native/reliability_constrained_harness.cpp: covariance_replay.h as it is, the new steps in
reliability_constrained_replay.h) against the dense projector of the oracle's J with the constraint rows in it and six eigenvalues zeroed,
under the rule of tests.reliability_native.check_against_dense with six for seven and the constraint rows included
(tests.reliability_constrained_native.check_against_dense); the refusals under the call's name; and the seam on CaptureVolume with a blunder in
an image observation and one in a constraint row.  Disagreement of the two CPU formulations and the error of the g++ build on R_oo / constraint
r_j, measured here: 2 x 2 boards 1.7e-11 (4.1e-12 / 5.4e-12), default boards 1.4e-14 (1.3e-14 / 1.5e-14), mixed 4.2e-14 (4.1e-14 / 2.5e-14),
70 repeats 1.6e-14 (9.4e-15 / 1.7e-14); the other scenes print theirs."""
import dataclasses
import re

import numpy as np
import pytest

from caliscope_amd import _lib, build, reliability
from caliscope_amd.exceptions import BackendError, CalibrationError
from tests import covariance_constrained_native as ccn
from tests import reliability_constrained_native as rcn
from tests import reliability_native as rn
from tests.native_build import CSRC, ROOT
from tests.test_uncertainty_constrained import SOFT_F_SCALE, refusal_cases

SCENES = [(ccn.TWO_BY_TWO, "linear", 1.0), (ccn.DEFAULT, "linear", 1.0), (ccn.MANY_ROWS, "linear", 1.0), (ccn.MIXED, "linear", 1.0),
          (ccn.FREE_INTRINSICS, "linear", 1.0), (ccn.DEFAULT, "soft_l1", SOFT_F_SCALE), (ccn.CAP, "linear", 1.0), (rcn.REPEAT, "linear", 1.0)]
SCENE_IDS = ["2x2 boards", "default boards", "5x5 boards 73 rows", "mixed", "free intrinsics", "soft_l1 on constraint rows", "one component at the cap",
             "70 observations of one pair"]

# The wrong distance given to the static link 10 -> 11 of tests.constrained_scene.marker_volume: ten of the row's sigmas (2 mm) and four times
# its smallest detectable error (4.9 mm with delta0 = 4.13 at the row's r = 0.52, measured on the clean volume).  In the dense reference the row
# then has |w| = 16.3, the runner-up among the constraint rows 2.7; the critical value at 0.1 % is 3.29.
LINK_BUMP_M = 0.02
# The shift of one image observation of tests.constrained_scene.board_volume, in pixels: twenty of the scene's noise sigmas (0.4 px).  |w| = 16.5
# in the dense reference, the runner-up 3.0.
IMAGE_BUMP_PX = 8.0
IMAGE_BUMP_AT = dict(cam_id=2, sync_index=3, keypoint_id=6)
# A significance at which a clean volume must keep EVERY row: board_volume has 720 reprojection rows, so 1e-6 predicts 7e-4 false alarms
# (critical value 4.89); at the default 0.1 % it predicts 0.7, and the scene's noise draw has one row at |w| = 3.52.
ALPHA_NO_FALSE_ALARM = 1e-6


def harness_call(key, loss="linear", f_scale=1.0, **kw):
    return rcn.HarnessConstrainedReliability().observation_reliability_constrained(*rcn.call_arguments(key), loss=loss, f_scale=f_scale, **kw)


# ---- the call against the dense projector -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,loss,f_scale", SCENES, ids=SCENE_IDS)
def test_harness_call_matches_the_dense_projector(key, loss, f_scale):
    rcn.check_against_dense(harness_call(key, loss, f_scale), key, loss, f_scale)


def check_zero_jacobian_row(res):
    """TWO_BY_TWO: the centroid rows with coincident endpoints have a zero Jacobian row: r == 1 exactly and w = f~ / sigma0."""
    sc = rcn.key_scene(ccn.TWO_BY_TWO)
    ga, gb, dist, w = sc["con"]
    pts = sc["x"][sc["par"].n_camera_params:].reshape(-1, 3)
    zero = [j for j in range(len(dist)) if not ccn.constraint_row(pts, np.concatenate([ga[j], gb[j]]), dist[j], w[j])[1].any()]
    assert zero and len(zero) < len(dist)
    assert (res.constraint_redundancy[zero] == 1.0).all() and (np.delete(res.constraint_redundancy, zero) < 1.0).all()
    assert np.array_equal(res.constraint_w[zero], res.constraint_residual[zero] / np.sqrt(res.sigma0_sq))
    assert np.array_equal(res.constraint_residual[zero], -w[zero] * dist[zero])  # coincident endpoints: length 0


def check_mixed_scene(res):
    """MIXED: the repeated observation has two output rows with equal R_oo; the corner with one observation and the rows of the camera that is
    blind to a component are finite and controlled."""
    sc = rcn.key_scene(ccn.MIXED)
    twice = np.flatnonzero((sc["cam"] == ccn.MIXED_TWICE[0]) & (sc["obj"] == ccn.MIXED_TWICE[1]))
    assert len(twice) == 2 and np.array_equal(res.redundancy[twice[0]], res.redundancy[twice[1]]) and np.array_equal(res.w[twice[0]], res.w[twice[1]])
    single = np.flatnonzero(sc["obj"] == ccn.MIXED_SINGLE)
    assert len(single) == 1 and (np.diag(res.redundancy[single[0]]) > reliability.REL_R_TINY).all()  # one view, controlled through its board
    assert np.isfinite(res.redundancy).all() and np.isfinite(res.constraint_redundancy).all()


def test_zero_jacobian_rows_are_fully_redundant():
    check_zero_jacobian_row(harness_call(ccn.TWO_BY_TWO))


def test_mixed_scene_rows():
    check_mixed_scene(harness_call(ccn.MIXED))


def test_a_row_of_weight_zero_is_nan_and_leaves_the_adjustment():
    a = [np.array(v) for v in rcn.call_arguments(ccn.DEFAULT)]
    full = rcn.HarnessConstrainedReliability().observation_reliability_constrained(*a)
    a[11][[3, 40]] = 0.0
    res = rcn.HarnessConstrainedReliability().observation_reliability_constrained(*a)
    for arr in (res.constraint_redundancy, res.constraint_w, res.constraint_residual):
        assert np.isnan(arr[[3, 40]]).all() and np.isfinite(np.delete(arr, [3, 40])).all()
    assert res.dof == full.dof - 2 and res.gauge_dim == 6
    r = np.concatenate([res.redundancy[:, 0, 0], res.redundancy[:, 1, 1], np.delete(res.constraint_redundancy, [3, 40])])
    assert abs(r.sum() - res.dof) <= 1e-9 * res.dof
    keep = np.ones(len(a[10]), dtype=bool); keep[[3, 40]] = False  # the same as the call without the two rows
    less = rcn.HarnessConstrainedReliability().observation_reliability_constrained(*a[:8], *(v[keep] for v in a[8:]))
    assert np.array_equal(less.redundancy, res.redundancy) and np.array_equal(less.constraint_redundancy, res.constraint_redundancy[keep])


def check_permutation(call, tol):
    """Permuting the caller's observation rows and constraint rows permutes the outputs."""
    a = rcn.call_arguments(ccn.MIXED)
    rng = np.random.default_rng(5)
    po, pc = rng.permutation(len(a[5])), rng.permutation(len(a[10]))
    first = call(*a)
    again = call(*a[:5], a[5][po], a[6][po], a[7][po], a[8][pc], a[9][pc], a[10][pc], a[11][pc])
    assert np.abs(again.redundancy - first.redundancy[po]).max() <= tol and np.abs(again.constraint_redundancy - first.constraint_redundancy[pc]).max() <= tol
    assert np.array_equal(again.residual, first.residual[po]) and np.array_equal(again.constraint_residual, first.constraint_residual[pc])
    rel = lambda w1, w0, r: np.abs(w1 - w0) * np.abs(r) / np.maximum(np.abs(w0), 1e-300)  # the rule on w: relative within tol / r_j
    assert rel(again.w, first.w[po], np.stack([first.redundancy[po, 0, 0], first.redundancy[po, 1, 1]], axis=1)).max() <= tol
    assert rel(again.constraint_w, first.constraint_w[pc], first.constraint_redundancy[pc]).max() <= tol
    assert again.dof == first.dof


def test_permuting_the_rows_permutes_the_outputs():
    ref = rcn.reference(ccn.MIXED)
    check_permutation(rcn.HarnessConstrainedReliability().observation_reliability_constrained, max(10 * ref["dis"], 1e-12))


def test_without_rows_the_call_is_the_unconstrained_call():
    twelve = rcn.call_arguments(ccn.DEFAULT)
    plain = rn.HarnessReliability().observation_reliability(*twelve[:8])
    hook = rcn.HarnessConstrainedReliability()
    empty = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4), dtype=np.int32), np.zeros(0), np.zeros(0))
    for res, n_con in ((hook.observation_reliability_constrained(*twelve[:8], *empty), 0), (hook.observation_reliability(*twelve[:8]), 0),
                       (hook.observation_reliability_constrained(*twelve, null_struct=True), 0),
                       (hook.observation_reliability_constrained(*twelve[:11], np.zeros(len(twelve[11]))), len(twelve[10]))):
        assert (res.gauge_dim, res.dof, res.n_uncontrolled) == (7, plain.dof, plain.n_uncontrolled)
        assert res.redundancy.tobytes() == plain.redundancy.tobytes() and res.w.tobytes() == plain.w.tobytes() and res.residual.tobytes() == plain.residual.tobytes()
        assert res.sigma0_sq == plain.sigma0_sq and res.cost == plain.cost
        for arr in (res.constraint_redundancy, res.constraint_w, res.constraint_residual):
            assert arr.shape == (n_con,) and np.isnan(arr).all()
        assert res.n_constraints_uncontrolled == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0])
def test_host_checks_name_the_offender_under_the_calls_name(case):
    _, args, code, words = case
    with pytest.raises(BackendError, match=re.escape(f"(code {code})")) as info:
        rcn.HarnessConstrainedReliability().observation_reliability_constrained(*args)
    assert "cba_observation_reliability_constrained: " + words in str(info.value)


def test_argument_checks_of_the_binding():
    a = list(rcn.call_arguments(ccn.TWO_BY_TWO))
    with pytest.raises(ValueError, match=r"groups_a and groups_b must be \(14, 4\)"):
        rcn.HarnessConstrainedReliability().observation_reliability_constrained(*a[:8], a[8][:, :3], *a[9:])
    with pytest.raises(ValueError, match="go together"):
        rcn.HarnessConstrainedReliability().observation_reliability_constrained(*a[:8], a[8], None, a[10], a[11])


def test_deterministic_mode_is_refused_with_rows_only(monkeypatch):
    monkeypatch.setenv("CBA_DETERMINISTIC", "1")
    with pytest.raises(BackendError, match=r"code -4.*cba_observation_reliability_constrained: CBA_DETERMINISTIC=1 with constraint rows"):
        harness_call(ccn.TWO_BY_TWO)
    a = rcn.call_arguments(ccn.TWO_BY_TWO)
    assert rcn.HarnessConstrainedReliability().observation_reliability_constrained(*a[:11], np.zeros(len(a[11]))).gauge_dim == 7  # no rows left: not refused
    monkeypatch.setenv("CBA_DETERMINISTIC", "0")
    assert harness_call(ccn.TWO_BY_TWO).gauge_dim == 6


# ---- the seam ----------------------------------------------------------------------------------------------------------------------------------
def oracle_factory():
    from oracle.engine import OracleEngine

    return lambda prob: OracleEngine(prob.parameterization, prob.camera_indices, prob.image_coords, prob.obj_indices, loss=prob.loss, f_scale=prob.f_scale,
                                     constraints=prob.constraint_args())


def check_seam(vol, hook):
    """An optimised board volume with `hook` as the device call (None: the device): array alignment, NaN rows, sum r == dof, the refusal without
    the flag."""
    ga, gb, dist, sig = vol._build_constraint_arrays()
    rep = vol.observation_reliability(include_constraints=True, _solver=hook)
    n_img = len(vol.image_points._df)
    assert rep.gauge_dim == 6 and rep.redundancy.shape == rep.w.shape == rep.residual_px.shape == rep.mdb_px.shape == (n_img, 2)
    for arr in (rep.constraint_redundancy, rep.constraint_w, rep.constraint_residual_m, rep.constraint_mdb_m):
        assert arr.shape == (len(dist),) and np.isfinite(arr).all()
    instances = list(vol._constraint_instances())
    assert len(rep.constraint_instances) == len(dist) and all(a[0] is b[0] and a[1] == b[1] for a, b in zip(rep.constraint_instances, instances))
    mask = vol._matched_arrays()[0]
    assert np.isnan(rep.redundancy[~mask]).all() and np.isfinite(rep.redundancy[mask]).all()  # every board corner is in a row: every matched row takes part
    total = np.nansum(rep.redundancy) + rep.constraint_redundancy.sum()
    assert abs(total - rep.dof) <= 1e-9 * rep.dof
    n_cams, n_pts = len(vol.camera_array.posed_cameras), len(vol.world_points)
    assert rep.dof == 2 * int(mask.sum()) + len(dist) - (6 * n_cams + 3 * n_pts) + 6
    assert rep.sigma0 == pytest.approx(np.sqrt(2.0 * vol.optimization_status.final_cost / rep.dof), rel=1e-6)
    # world units: the residual is measured minus nominal distance, the smallest detectable error follows delta0 sigma0 / (weight sqrt(r))
    xyz = vol.world_points.points
    measured = np.linalg.norm(xyz[ga].mean(axis=1) - xyz[gb].mean(axis=1), axis=1)
    assert np.allclose(rep.constraint_residual_m, measured - dist, rtol=0, atol=1e-12)
    f_median = float(np.median([cam.matrix[0, 0] for cam in vol.camera_array.posed_cameras.values()]))
    assert np.allclose(rep.constraint_mdb_m, rep.delta0 * rep.sigma0 / ((1.0 / f_median) / sig * np.sqrt(rep.constraint_redundancy)), rtol=1e-12)
    assert rep.worst_constraints(3)[0][1] == np.abs(rep.constraint_w).max() and len(rep.worst_constraints(3)) == 3
    for method in (vol.observation_reliability, vol.filter_by_w_test):  # the default stays: refused, and the hint names the flag
        with pytest.raises(CalibrationError, match=r"without constraints.*include_constraints=True"):
            method(_solver=hook)
    return rep


def test_seam_on_an_optimised_board_volume():
    from caliscope_amd.capture_volume import CaptureVolume
    from tests.constrained_scene import board_volume

    vol, _ = board_volume()
    vol = vol.optimize(_engine_factory=oracle_factory())
    assert vol.optimization_status.converged
    hook = rcn.HarnessConstrainedReliability()
    check_seam(vol, hook)
    assert hook.constrained_calls == 1
    # without a ConstraintSet include_constraints=True is the unconstrained report, with empty constraint arrays
    bare = CaptureVolume(vol.camera_array, vol.image_points, vol.world_points)
    plain = bare.observation_reliability(_solver=rn.HarnessReliability())
    same = bare.observation_reliability(include_constraints=True, _solver=hook)
    assert (same.gauge_dim, same.dof) == (7, plain.dof) and same.redundancy.tobytes() == plain.redundancy.tobytes()
    assert same.constraint_redundancy.shape == (0,) and same.constraint_instances == () and len(same.flagged_constraints()) == 0


def test_report_defaults_keep_existing_constructions_working():
    rep = reliability.ReliabilityReport(sigma0=1.0, dof=1, redundancy=np.zeros((0, 2)), redundancy_uv=np.zeros(0), w=np.zeros((0, 2)), residual_px=np.zeros((0, 2)),
                                        mdb_px=np.zeros((0, 2)), camera_redundancy={}, point_redundancy=np.zeros(0), n_uncontrolled=0)
    assert rep.gauge_dim == 7 and rep.constraint_w.shape == (0,) and rep.constraint_instances == () and rep.worst_constraints() == []
    res = reliability.ReliabilityResult(redundancy=np.zeros((0, 2, 2)), w=np.zeros((0, 2)), residual=np.zeros((0, 2)), sigma0_sq=1.0, dof=1, cost=0.5, n_uncontrolled=0)
    assert res.gauge_dim == 7 and res.constraint_redundancy is None


# ---- blunders through the seam -----------------------------------------------------------------------------------------------------------------
def bumped_board_volume(bump_px):
    """tests.constrained_scene.board_volume with one image observation shifted by `bump_px` in x (0: the clean volume), not optimised; and
    the row of that observation in its image points."""
    from caliscope_amd.capture_volume import CaptureVolume
    from caliscope_amd.point_data import ImagePoints
    from tests.constrained_scene import board_volume

    vol, _ = board_volume()
    img = vol.image_points._df.copy()
    row = int(np.flatnonzero(np.logical_and.reduce([img[k].to_numpy() == v for k, v in IMAGE_BUMP_AT.items()]))[0])
    img.loc[img.index[row], "img_loc_x"] += bump_px
    return CaptureVolume(vol.camera_array, ImagePoints(img), vol.world_points, vol.constraints), row


def check_image_blunder(optimise, hook):
    """The bumped observation has the worst |w|, is flagged, and filter_by_w_test(include_constraints=True) removes it; no constraint row is
    flagged.  A clean volume keeps its rows (ALPHA_NO_FALSE_ALARM), and loses at the default significance no more than are flagged."""
    how = dict(include_constraints=True, _solver=hook)
    vol, row = bumped_board_volume(IMAGE_BUMP_PX)
    vol = optimise(vol)
    rep = vol.observation_reliability(**how)
    print(dict(row=row, worst=rep.worst_observations(2), flagged=rep.flagged().tolist(), constraints=rep.worst_constraints(1)))
    assert rep.worst_observations(1)[0][0] == row and row in rep.flagged() and row in rep.flagged(ALPHA_NO_FALSE_ALARM)
    assert len(rep.flagged_constraints()) == 0
    key = lambda df: set(zip(df["cam_id"].tolist(), df["sync_index"].tolist(), df["keypoint_id"].tolist()))  # noqa: E731
    before = vol.image_points._df
    gone = key(before) - key(vol.filter_by_w_test(ALPHA_NO_FALSE_ALARM, **how).image_points._df)
    assert gone == {tuple(int(before[k].iloc[row]) for k in ("cam_id", "sync_index", "keypoint_id"))}
    after = vol.filter_by_w_test(**how)
    assert after.constraints is vol.constraints and gone <= key(before) - key(after.image_points._df)  # (constraint rows are never removed)
    clean, _ = bumped_board_volume(0.0)
    clean = optimise(clean)
    assert len(clean.filter_by_w_test(ALPHA_NO_FALSE_ALARM, **how).image_points._df) == len(clean.image_points._df)
    lost = len(clean.image_points._df) - len(clean.filter_by_w_test(**how).image_points._df)
    assert lost <= len(clean.observation_reliability(**how).flagged())


def bumped_marker_volume(bump_m):
    """tests.constrained_scene.marker_volume with the nominal distance of its static link 10 -> 11 changed by `bump_m`, not optimised."""
    from caliscope_amd.capture_volume import CaptureVolume
    from caliscope_amd.constraints import ConstraintSet
    from tests.constrained_scene import marker_volume

    vol, _ = marker_volume()
    cs = vol.constraints
    rows = list(cs.distances)
    at = [i for i, c in enumerate(rows) if (c.object_id_a, c.object_id_b) == (10, 11)]
    assert len(at) == 1
    rows[at[0]] = dataclasses.replace(rows[at[0]], distance=rows[at[0]].distance + bump_m)
    return CaptureVolume(vol.camera_array, vol.image_points, vol.world_points, ConstraintSet(tuple(rows), cs.static_object_ids, cs.centroid_distances))


def check_link_blunder(optimise, hook, bump_m):
    """flagged_constraints() names exactly the link's one instance, it is the worst constraint row, and its residual (measured minus nominal
    distance) has the sign of the bump as the data see it: a nominal distance that is too long leaves the measured one short of it."""
    vol = optimise(bumped_marker_volume(bump_m))
    rep = vol.observation_reliability(include_constraints=True, _solver=hook)
    link = [i for i, (c, _) in enumerate(rep.constraint_instances) if (c.object_id_a, c.object_id_b) == (10, 11)]
    print(dict(bump=bump_m, link=link, flagged=rep.flagged_constraints().tolist(), worst=rep.worst_constraints(2), mdb=rep.constraint_mdb_m[link].tolist()))
    assert len(link) == 1 and rep.flagged_constraints().tolist() == link and rep.worst_constraints(1)[0][0] == link[0]
    assert np.sign(rep.constraint_residual_m[link[0]]) == -np.sign(bump_m) and abs(rep.constraint_residual_m[link[0]]) > 0.25 * abs(bump_m)
    assert abs(bump_m) > rep.constraint_mdb_m[link[0]]  # above the smallest error the adjustment detects in this row
    return vol, rep


def test_image_blunder_is_found_and_removed_with_the_constraints_in_the_adjustment():
    check_image_blunder(lambda v: v.optimize(_engine_factory=oracle_factory()), rcn.HarnessConstrainedReliability())


@pytest.mark.parametrize("bump_m", [LINK_BUMP_M, -LINK_BUMP_M], ids=["too long", "too short"])
def test_wrong_link_distance_is_the_flagged_constraint(bump_m):
    vol, rep = check_link_blunder(lambda v: v.optimize(_engine_factory=oracle_factory()), rcn.HarnessConstrainedReliability(), bump_m)
    if bump_m < 0:
        return
    # "chosen on the CPU": in the DENSE reference at these parameters the link has the largest |w| of the constraint rows, above the critical value
    ga, gb, dist, sig = vol._build_constraint_arrays()
    par, args, used, _, _ = vol._free_network_arguments("observation_reliability", "reliability report", False, constraint_groups=(ga, gb), allow_constraints=True)
    assert used.all()
    f_median = float(np.median([cam.matrix[0, 0] for cam in vol.camera_array.posed_cameras.values()]))
    key = ("repeat-free marker volume with a wrong link",)
    rcn._SCENES[key] = dict(par=par, x=par.pack(vol.camera_array, vol.world_points.points), cam=args[5], obj=args[6], uv=args[7], con=(ga, gb, dist, (1.0 / f_median) / sig))
    ref = rcn.reference(key)
    w_dense = np.abs(ref["fc"]) / np.sqrt(ref["sigma0_sq"] * ref["rc"])
    link = rep.flagged_constraints()[0]
    assert int(np.argmax(w_dense)) == link and w_dense[link] > reliability.critical_value(0.001) and np.sum(w_dense > reliability.critical_value(0.001)) == 1
    assert abs(abs(rep.constraint_w[link]) - w_dense[link]) * ref["rc"][link] / w_dense[link] <= max(10 * ref["dis"], 1e-12)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_is_declared_exported_bound_and_typed():
    build.build(verbose=False)
    lib = _lib.load()
    header = (ROOT / "include" / "caliscope" / "reliability_constrained.h").read_text()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", text))
    assert declared == {"cba_observation_reliability_constrained"} == set(reliability.RELIABILITY_CONSTRAINED_SIGNATURES)
    assert not declared & set(_lib.SIGNATURES) and not declared & set(reliability.RELIABILITY_SIGNATURES)
    assert hasattr(lib, "cba_observation_reliability_constrained")
    typed = _lib.bind(lib, reliability.RELIABILITY_CONSTRAINED_SIGNATURES)
    for name, (res, args) in reliability.RELIABILITY_CONSTRAINED_SIGNATURES.items():
        assert getattr(typed, name).argtypes == args and getattr(typed, name).restype == res
    body = re.search(r"typedef struct \{([^{}]*)\}\s*cba_rel_con_out", text).group(1)
    assert [f for f, _ in reliability.RelConOut._fields_] == re.findall(r"(\w+)\s*;", body)
    assert (CSRC / "reliability_constraint_math.h") in build.DEPENDS and (ROOT / "include" / "caliscope" / "reliability_constrained.h") in build.DEPENDS
    math_header = (CSRC / "reliability_constraint_math.h").read_text()
    assert "#include <hip" not in math_header and "__global__" not in math_header  # hipcc and g++ compile the same code


def test_harness_call_under_sanitizers():
    """tests/native/reliability_constrained_check.cpp (the harness call on one scene with components, free points, a constrained point seen once,
    a repeated observation, a zero Jacobian row, a row of weight 0 and null outputs, then refused calls) as a program of its own under
    AddressSanitizer and UndefinedBehaviorSanitizer: exit status 0 and no report.  No Python in the process under the sanitizers."""
    import subprocess

    from tests.native_build import NATIVE, compile_native

    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas")
    exe = compile_native(NATIVE / "reliability_constrained_check.cpp", flags=flags, include=(CSRC, NATIVE), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "Sanitizer" not in proc.stderr and "runtime error" not in proc.stderr
    assert "all checks passed" in proc.stdout


def test_device_call_fails_loudly_without_a_device():
    build.build(verbose=False)
    if _lib.load().cba_device_count() > 0:
        return  # (with a device the call runs: tests/test_reliability_constrained_gpu.py)
    a = rcn.call_arguments(ccn.TWO_BY_TWO)
    with pytest.raises(BackendError, match="no HIP device"):
        reliability.DeviceReliability().observation_reliability_constrained(*a)
    with pytest.raises(BackendError, match=r"code -1.*cba_observation_reliability_constrained: constraint row 0: weight -1"):  # the plan's refusals come first
        reliability.DeviceReliability().observation_reliability_constrained(*a[:11], -np.ones(len(a[11])))
