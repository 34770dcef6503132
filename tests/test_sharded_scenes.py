"""The scenes of tests/sharded_scenes.py on the CPU: each scene's defining property read from the product's ``shard_problem`` (not assumed),
the conditioning cap of the references, and the lock-step driver of tests/sharded_native.py on the CPU test build of the library.

Conditioning cap: tests/test_sharded_step_gpu.py holds the device's sharded step to 1e-8 (2e-8 at lam = 1e-7) of the oracle's step and, as
tests/test_gpu_parity.py::_check_step does, to the sparse LU of the full damped system.  For that to say something about the device, the
two references must agree among themselves well inside the bar: a tenth of it, at every linear-loss scene and every lam used.
"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from caliscope_amd.sharding import shard_problem
from tests import sharded_scenes as ss
from tests.native_build import CSRC, INCLUDE, NATIVE, ROOT, compile_native
from tests.sharded_native import _relmax, first_step_shape, oracle_for, sparse_reference, step_tolerance


def _shards(name, world):
    sc = ss.scene(name)
    return sc, [shard_problem(sc["problem"], r, world) for r in range(world)]


def _views(problem):
    return np.bincount(problem.obj_indices, minlength=problem.parameterization.n_points)


@pytest.mark.parametrize("name,world", ss.CASES)
def test_every_rank_owns_points_and_the_shards_cover_the_scene(name, world):
    sc, shards = _shards(name, world)
    par = sc["par"]
    assert len(par.blocks) <= 50 and par.n_points <= 600  # the smallest scene that shows its edge
    owned = np.concatenate([s.owned_points for s in shards])
    assert np.array_equal(owned, np.arange(par.n_points))
    assert sum(s.problem.n_obs for s in shards) == sc["problem"].n_obs
    assert all(_views(s.problem).min() >= 2 for s in shards)  # no unobserved or one-view point hides in a shard
    assert set(np.unique(sc["problem"].camera_indices)) == set(range(len(par.blocks)))  # every camera is observed somewhere


def test_even_is_the_plain_case():
    for world in (2, 3):
        sc, shards = _shards("EVEN", world)
        assert len(sc["par"].blocks) == 8 and sc["par"].n_camera_params == 48 and sc["loss"] == "linear"
        assert len({s.problem.n_obs for s in shards}) == 1
        assert all(np.unique(s.problem.camera_indices).size == 8 for s in shards)


def test_tiny_rig_is_below_one_cholesky_block():
    sc, shards = _shards("TINY_RIG", 2)
    assert len(sc["par"].blocks) == 2 and sc["par"].n_camera_params == 12 < ss.NB


def test_global_rigs_span_several_camera_groups():
    sc, _ = _shards("GLOBAL", 3)
    assert len(sc["par"].blocks) == 24 and all(b.n_params == 6 for b in sc["par"].blocks)
    sc, _ = _shards("GLOBAL_REFINE", 2)
    assert len(sc["par"].blocks) == 20 and all(b.n_params == 9 for b in sc["par"].blocks)
    # (more than the 16 cameras of one Schur group: the device test asserts info()["schur_groups"] > 1 on every rank)


def test_subset_leaves_a_camera_unseen_on_rank_0_only():
    sc, (first, second) = _shards("SUBSET", 2)
    n_cams = len(sc["par"].blocks)
    seen0, seen1 = set(np.unique(first.problem.camera_indices)), set(np.unique(second.problem.camera_indices))
    assert seen0 < set(range(n_cams)) and 7 not in seen0  # a strict subset: camera 7 has no record in that shard, its local U_c is zero
    assert seen1 == set(range(n_cams))


def test_one_point_gives_rank_0_the_heavy_point_alone():
    sc, shards = _shards("ONE_POINT", 8)
    views = _views(sc["problem"])
    assert views[0] > ss.HEAVY_OBS and 8 * views[0] >= views.sum()
    assert np.array_equal(shards[0].owned_points, [0]) and shards[0].problem.n_obs == views[0]
    assert all(_views(s.problem).max() <= ss.HEAVY_OBS for s in shards[1:])  # k_heavy_schur on rank 0 only


def test_constrained_keeps_every_component_on_rank_0():
    sc, (first, second) = _shards("CONSTRAINED", 2)
    total = sc["problem"].n_constraints
    assert total > 0 and first.problem.n_constraints == total and second.problem.n_constraints == 0  # mine.any() is false on rank 1
    assert first.owned_points.size == second.owned_points.size  # the cut is the balanced one, not one pushed by a component


def test_robust_has_outlier_rows_on_both_ranks():
    sc, shards = _shards("ROBUST", 2)
    from oracle.residuals import joint_residuals

    assert sc["loss"] == "huber"
    for s in shards:
        f = joint_residuals(s.local_x(sc["x0"]), s.problem.parameterization, s.problem.camera_indices, s.problem.image_coords, s.problem.obj_indices)
        beyond = float(((f / sc["f_scale"]) ** 2 > 1.0).mean())
        print(f"ROBUST: {beyond:.3f} of the rows beyond huber's quadratic region")
        assert 0.05 < beyond < 0.95  # both branches of the loss on every rank


def test_mixed_is_the_fisheye_and_pinhole_rig():
    sc, shards = _shards("MIXED", 2)
    assert [b.n_params for b in sc["par"].blocks] == [6, 9]
    assert all(np.unique(s.problem.camera_indices).size == 2 for s in shards)


def test_world16_fills_the_group():
    sc, shards = _shards("WORLD16", ss.GROUP_MAX)
    assert len(shards) == 16 and all(s.problem.n_obs > 0 for s in shards)


@pytest.mark.parametrize("name", [n for n in ss.SCENES if n != "ROBUST"])
def test_the_references_agree_within_a_tenth_of_the_step_bar(name):
    sc = ss.scene(name)
    assert sc["loss"] == "linear"
    ora = oracle_for(sc)
    ora.begin(sc["x0"])
    ora.linearize()
    for lam in ss.LAMBDAS:
        assert ora.newton_step(lam).ok
        s_full, S_ref = sparse_reference(ora, lam, sc["par"].n_camera_params)
        d_step, d_S = _relmax(ora.s, s_full), _relmax(ora.S, S_ref)
        print(f"{name} lam {lam:g}: oracle step against splu {d_step:.2e} (cap {0.1 * step_tolerance(lam):.0e}), S against S_ref {d_S:.2e} (cap 1e-10)")
        assert d_step <= 0.1 * step_tolerance(lam)
        assert d_S <= 1e-10  # a tenth of the bar on S


@pytest.mark.parametrize("name", sorted({n for n, _ in ss.FUSED_CASES}))
def test_the_fused_step_has_a_trial_point_to_compare(name):
    """``cba_step`` makes its trial point only while ||w||^2 > 1e-3 ||p||^2 (the damped step not collinear with the gradient); the scenes of
    the fused comparison start a hundred times clear of that.  ROBUST at x0 would not: that is why it starts near a minimum."""
    sc = ss.scene(name)
    lam, ratio = first_step_shape(sc, ss.fused_start(name))
    print(f"{name}: first iteration lam {lam:.3e}, ||w||^2 / ||p||^2 {ratio:.3f}")
    assert ratio > 0.1
    if name == "ROBUST":
        assert first_step_shape(sc, sc["x0"])[1] < 1e-3 and not np.array_equal(ss.fused_start(name), sc["x0"])
    else:
        assert ss.fused_start(name) is sc["x0"]


# ---- the driver and the comparisons on the CPU test build (tests/test_cpu_abi.py: a child interpreter bound to it) ---------------------------
@pytest.fixture(scope="module")
def cpu_lib():
    return compile_native(NATIVE / "cpu_library.cpp", CSRC / "cba_solve.cpp", flags=("-pthread",), include=(INCLUDE,))


def test_the_lock_step_driver_on_the_cpu_build(cpu_lib):
    """tests/sharded_native.py's driver, records and comparisons on EVEN (two and three ranks), SUBSET, ROBUST and the ``refine=True`` rig, with
    the CPU test build's host group under them: the bars are those of the device test, and the replicated state must be the same bits on
    every rank.  S is left out: the CPU build's ``cba_reduced_system`` rebuilds S from the rank's own J (it is half the whole S and differs
    from rank to rank), whereas the device returns the exchanged ``p->S`` — that comparison is made on the device only."""
    body = f"""
        import json
        from tests import sharded_scenes as ss
        from tests.sharded_native import compare_step, replicated_differences, run_ranks, step_body
        out = {{}}
        for name, world in {ss.CPU_BUILD_CASES!r}:
            sc = ss.scene(name)
            recs = run_ranks(sc["problem"], sc["x0"], world, step_body(sc["x0"], ss.LAMBDAS, with_system=False))
            fig = compare_step(sc, recs, ss.LAMBDAS, f"{{name}} world {{world}} (CPU build)", with_system=False)
            out[f"{{name}}-{{world}}"] = dict(differ=replicated_differences(recs), worst=fig.worst)
        print(json.dumps(out))
    """
    env = dict(os.environ, CALISCOPE_BA_LIB=str(cpu_lib), PYTHONPATH=str(ROOT))
    proc = subprocess.run([sys.executable, "-c", textwrap.dedent(body)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    print(proc.stdout[-6000:])
    assert proc.returncode == 0, proc.stderr[-3000:]
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert set(out) == {f"{n}-{w}" for n, w in ss.CPU_BUILD_CASES}
    for case, row in out.items():
        assert row["differ"] == [], (case, row["differ"])
