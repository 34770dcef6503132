"""Gravity fits from perspective fields on the MI355X: cba_vertical_fit against the reference's recorded answers
(tests/golden/vertical: roll and pitch within 1e-12 rad, uncertainties and costs within 1e-10 relative, stop_step equal), against the
g++ build of the same header (tests/vertical_native.py) at the chunk edges and in a mixed-shape batch within the same tolerance,
bit-identical from run to run and from a single fit to its entry in a batch, with more fits than compute units, the two error
statuses, and the public fit_gravity.  The largest differences seen against the fixtures go to profiles/vertical_parity.json."""
import json

import numpy as np
import pytest

from caliscope_amd import vertical as V
from tests import vertical_native as N

pytestmark = pytest.mark.gpu

DEV, CPU = V.DeviceVerticalFit(), N.HarnessVerticalFit()


def _close(dev: V.GravityFit, cpu: V.GravityFit, label):
    """Device against the g++ build: the tolerance of the fixtures (both stand within it of the reference)."""
    N.assert_matches(dev, [getattr(cpu, f) for f in N.FIT_FIELDS], cpu.stop_step, label)


def test_device_within_the_tolerance_of_every_fixture():
    names = N.fixture_names()
    sets, expected = [], []
    for name in names:
        fx = N.load(name)
        assert int(fx["num_steps"]) in (0, 1, 3, 30)
        for variant in N.VARIANTS:
            sets.append((name, variant, int(fx["num_steps"]), N.field_set(fx, variant)))
            expected.append((fx[f"expected_{variant}"], fx[f"stop_step_{variant}"]))
    fits = {}
    for steps in (0, 1, 3, 30):  # one device call per step budget
        group = [k for k, s in enumerate(sets) if s[2] == steps]
        for k, fit in zip(group, V.fit_gravity_batch([sets[k][3] for k in group], steps)):
            fits[k] = fit
    worst = {"angle_rad": 0.0, "relative": 0.0, "stop_step_mismatches": 0, "fits": len(sets)}
    diffs = [N.differences(fits[k], *expected[k]) for k in range(len(sets))]
    for (name, variant, _, _), d in zip(sets, diffs):
        print(f"{name}/{variant}: angle {d['angle']:.3e} rad, relative {d['rel']:.3e}, stop_step equal {d['stop_equal']}")
        worst["angle_rad"], worst["relative"] = max(worst["angle_rad"], d["angle"]), max(worst["relative"], d["rel"])
        worst["stop_step_mismatches"] += not d["stop_equal"]
    out = N.ROOT / "profiles" / "vertical_parity.json"
    out.write_text(json.dumps({"what": "largest differences of cba_vertical_fit on the device from the reference's fit_gravity over tests/golden/vertical",
                               "tolerance": {"angle_rad": N.ANGLE_ATOL, "relative": N.REL_TOL}, **worst}, indent=1) + "\n")
    for k, (name, variant, _, _) in enumerate(sets):
        N.assert_matches(fits[k], *expected[k], f"{name}/{variant}")


def test_device_equals_the_cpu_build_at_the_chunk_edges_and_in_a_mixed_batch():
    edge = N.chunk_edge_shapes()
    shapes = edge + [(2, 2), (7, 9), (33, 31), edge[2]]
    sets = [N.noisy_fields(0.15 * k - 0.4, 0.1 * k - 0.2, 70 + 9 * k, 72 + 8 * k, h, w, seed=40 + k, uniform_confidence=k % 2 == 1) for k, (h, w) in enumerate(shapes)]
    dev, cpu = V.fit_gravity_batch(sets), V.fit_gravity_batch(sets, _solver=CPU)
    for k, (d, c) in enumerate(zip(dev, cpu)):
        _close(d, c, f"shape {shapes[k]}")
    # float64 planes take the other template of the kernels: same numbers, the widening of float32 is exact
    assert V.fit_gravity_batch([tuple(np.asarray(a, dtype=np.float64) for a in s[:4]) + s[4:] for s in sets]) == dev


def test_two_runs_and_single_against_batch_are_bit_identical():
    shapes = [(2, 2), (7, 9), (33, 31), N.chunk_edge_shapes()[2], (70, 130)]
    sets = [N.noisy_fields(0.1 * k - 0.2, 0.05 * k, 80 + k, 81 + k, h, w, seed=k) for k, (h, w) in enumerate(shapes)]
    first = V.fit_gravity_batch(sets)
    assert V.fit_gravity_batch(sets) == first
    for k, s in enumerate(sets):
        assert V.fit_gravity(*s) == first[k], shapes[k]
    assert V.fit_gravity_batch(sets[::-1]) == first[::-1]


def test_300_small_fits_more_than_compute_units():
    rng = np.random.default_rng(8)
    base = [N.noisy_fields(r, p, 40, 42, 9, 11, seed=100 + k) for k, (r, p) in enumerate(rng.uniform(-0.5, 0.5, (6, 2)))]
    sets = [base[k % 6] for k in range(300)]
    dev = V.fit_gravity_batch(sets)
    cpu = V.fit_gravity_batch(base, _solver=CPU)
    assert len(dev) == 300
    for k in range(6):
        _close(dev[k], cpu[k], f"fit {k}")
    assert all(dev[k] == dev[k % 6] for k in range(300))


def test_error_statuses_and_the_fit_next_to_them():
    up, uc, lat, lc, fx, fy = N.noisy_fields(0.1, 0.1, 60, 60, 8, 8, seed=1)
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        V.fit_gravity(up, np.zeros_like(uc), lat, np.zeros_like(lc), fx, fy)
    bad = lat.copy()
    bad[0, 3, 3] = np.nan
    with pytest.raises(ValueError, match="field set 0: the cost at the start vector is not finite"):
        V.fit_gravity(up, uc, bad, lc, fx, fy)
    zero = np.zeros(64, dtype=np.float32)
    planes = [np.concatenate(p) for p in ((up[0].reshape(-1),) * 3, (up[1].reshape(-1),) * 3, (uc.reshape(-1), uc.reshape(-1), zero),
                                          (lat.reshape(-1), bad.reshape(-1), lat.reshape(-1)), (lc.reshape(-1), lc.reshape(-1), zero))]
    fits, stop, status = DEV.vertical_fit(planes, [8] * 3, [8] * 3, [fx] * 3, [fy] * 3, [0, 64, 128])
    assert status.tolist() == [V.STATUS_OK, V.STATUS_NONFINITE, V.STATUS_SINGULAR]
    assert V.GravityFit(*fits[0, :7].tolist(), stop_step=int(stop[0])) == V.fit_gravity(up, uc, lat, lc, fx, fy)
    assert status.tolist() == CPU.vertical_fit(planes, [8] * 3, [8] * 3, [fx] * 3, [fy] * 3, [0, 64, 128])[2].tolist()


def test_public_fit_gravity_on_an_analytic_case():
    roll, pitch = 0.35, -0.25
    fit = V.fit_gravity(*N.analytic_fields(roll, pitch, 300.0, 300.0, 96, 128), 300.0, 300.0)
    cosine = np.dot(V.gravity_vec_from_roll_pitch(fit.roll_rad, fit.pitch_rad), V.gravity_vec_from_roll_pitch(roll, pitch))
    assert np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0))) < 0.1
    assert fit.final_cost < fit.initial_cost and 1 <= fit.stop_step <= 30 and fit.gravity_uncertainty_rad > 0.0
