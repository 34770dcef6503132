"""A point-sharded step on the device, rank by rank, against the oracle on the WHOLE problem (run with ``-m gpu``).

tests/test_multi_device.py compares converged sharded solves with the single-rank solve; a trust-region loop corrects itself, so a sharded
step that is wrong in a way that is the same on every rank (camera entries of a norm counted once per rank, lam D^2 added ``world`` times
to S, a dropped slice of b, a wrong max |g|) still converges and passes there.  Here the step itself is held, entry by entry, to what
tests/test_gpu_parity.py::test_step_parity (``_check_step``) holds the single-rank step to, with that test's bars for the same loss and
nothing added: a sharded step differs from the single-rank one only in the order of its sums.

Several ranks are several handles on ONE device joined by the library's in-process group (``cba_group_*``), driven in lock step by
tests/sharded_native.py::run_ranks.  That is the code that runs only when ``p->sharded()``: k_tri_pack around the one large exchange,
k_group_sum / group_allreduce and its two staging parities, k_xpack / k_xunpack with their world-sized max tail, the all-reduce of the
packed camera blocks and k_unpack_camera_grad (fused route), the ``rank == 0`` / ``first = ncp_pad`` arguments that count replicated
camera entries once, the unfused k_reg_reduce + k_reg_fold + k_schur_finalize route, run_cholesky on rigs a single rank sends to
k_small_solve, and the negotiation of the fused route at the join.

Scenes (tests/sharded_scenes.py; their defining properties and the agreement of the two references within a tenth of the step bar are
asserted on the CPU in tests/test_sharded_scenes.py): EVEN, TINY_RIG, GLOBAL and GLOBAL_REFINE, SUBSET, ONE_POINT, CONSTRAINED, ROBUST,
MIXED, WORLD16.

After every primitive the replicated state — the scalars, the camera blocks of g, scale_inv and s, S and rhs, the trial cost — must be
the same BITS on every rank (``solve_multi_device`` promises identical bits; a rank that differs in one bit can take another branch and
leave its peers in a collective).  The bodies only record and the comparison runs afterwards: an assertion inside one rank's thread would
do exactly that.

``CBA_GROUP_TIMEOUT_S`` is set to a few seconds before any group is created, so that a mistake in the driver ends in the library's own
"device group aborted" error and not after the default 120 s.

Every figure is printed before it is asserted (``-s``).  Bars: linearisation scalars 1e-10 (``stol`` 5e-2 for gh_sq / jg_sq under the
robust loss), scale_inv 1e-12 (1e-7 robust), gradient 1e-11 of max |g|, step 1e-8 at lam = 1e-3 and 2e-8 at lam = 1e-7 against the oracle,
1e-8 / 1e-7 against the sparse LU, p_sq / gh_dot_p / w_sq 1e-7, S symmetric to 1e-14 and within 1e-9 of S_ref, |S s_c - rhs| 1e-7 |rhs|,
trial cost 1e-9, step norm 1e-7; the robust scene takes _check_step's floor-column exclusion and its looser bars (step 1e-5, trial 1e-6).

Measured on an MI355X (one run; relative figures, the largest of the kind and over both lam where no lam is named).  Columns and bars:
lin = cost, g_norm_inf, x_scaled_norm, x_norm (1e-10); gh/jg = gh_sq, jg_sq (1e-10, robust 5e-2); sinv = scale_inv (1e-12, robust 1e-7);
grad (1e-11); s = step against the oracle at lam = 1e-3 (1e-8, robust 1e-5) and 1e-7 (2e-8, robust 1e-5); lu = step against the sparse LU
(1e-8, 1e-7); sums = p_sq, gh_dot_p, w_sq (1e-7); sym = S - S^T (1e-14); S against S_ref (1e-9); res = |S s_c - rhs| / |rhs| (1e-7);
gram (1e-7, robust 5e-2); cost = trial cost (1e-9, robust 1e-6); norm = step norm (1e-7); 2nd = gh_sq, jg_sq of the second linearisation
(1e-7, robust 5e-2); sinv2 = its scale_inv (1e-6, robust 1e-4).

                      lin     gh/jg   sinv    grad    s 1e-3  s 1e-7  lu 1e-3 lu 1e-7 sums    sym  S       res     gram    cost    norm    2nd     sinv2
    EVEN 2            2.0e-15 1.9e-15 3.8e-16 3.7e-15 4.3e-13 2.6e-09 3.7e-13 3.5e-09 4.0e-15 0    1.4e-15 1.9e-15 2.4e-15 2.2e-11 9.7e-10 1.4e-11 1.1e-11
    EVEN 3            2.0e-15 2.1e-15 3.8e-16 3.7e-15 4.3e-13 1.6e-09 3.7e-13 2.5e-09 4.0e-15 0    1.5e-15 1.9e-15 2.4e-15 7.7e-12 1.1e-09 8.0e-12 1.3e-11
    TINY_RIG 2        2.8e-16 1.2e-15 3.3e-16 2.0e-15 4.1e-14 5.1e-10 9.7e-13 1.1e-09 1.0e-14 0    3.3e-15 1.5e-16 1.1e-15 1.3e-11 4.8e-10 6.8e-12 9.7e-12
    GLOBAL 3          2.3e-15 6.1e-16 8.0e-16 5.1e-15 1.4e-13 2.4e-09 2.0e-13 2.2e-09 3.3e-15 0    2.1e-15 1.1e-15 8.6e-16 7.6e-12 1.6e-10 1.8e-11 1.6e-11
    GLOBAL_REFINE 2   1.5e-15 5.2e-16 7.7e-16 4.9e-15 4.7e-11 1.3e-10 6.3e-11 1.1e-10 1.9e-13 0    1.6e-15 4.6e-16 8.6e-16 4.5e-11 1.3e-11 6.3e-11 6.5e-14
    SUBSET 2          1.9e-15 3.8e-15 4.6e-16 2.7e-15 1.2e-13 1.7e-09 1.7e-13 1.9e-09 5.7e-15 0    1.2e-15 5.0e-16 4.1e-15 1.7e-11 7.1e-10 4.4e-11 1.7e-11
    ONE_POINT 8       1.9e-15 1.3e-15 2.1e-16 5.5e-15 1.5e-13 1.1e-09 3.2e-13 1.4e-09 1.1e-15 0    6.3e-16 7.2e-16 1.1e-15 1.1e-11 2.9e-10 6.3e-12 4.8e-12
    CONSTRAINED 2     2.3e-15 9.9e-16 4.5e-16 2.3e-15 7.2e-14 6.8e-10 9.8e-14 6.8e-10 1.4e-14 0    1.0e-15 1.7e-15 1.1e-15 1.1e-12 9.8e-11 2.9e-11 1.9e-12
    ROBUST 2          3.8e-16 1.1e-03 1.2e-10 4.5e-15 9.1e-09 3.8e-07    -       -       -    0       -    1.9e-11 1.1e-03 7.7e-12    -    2.0e-06 7.0e-12
    MIXED 2           1.2e-14 4.1e-14 2.6e-16 7.3e-14 1.1e-13 2.9e-10 2.1e-13 1.8e-09 3.4e-13 0    1.4e-15 4.3e-15 4.8e-14 3.5e-11 7.4e-11 7.4e-11 7.9e-12
    WORLD16 16        2.2e-15 8.7e-16 3.9e-16 4.7e-15 1.2e-13 2.4e-09 1.9e-13 1.7e-09 4.7e-15 0    1.5e-15 3.7e-16 8.5e-16 3.0e-11 5.3e-10 1.3e-11 1.3e-11

The step at lam = 1e-7 is the only figure within a factor of ten of its bar (2.6e-9 of 2e-8; over four runs EVEN read between 1.5e-9 and 2.9e-9: the
order of the FP64 atomics changes from run to run), and it is the distance of the two references among themselves there (5e-11 .. 1.7e-9 on these scenes, tests/test_sharded_scenes.py).
The replicated state was the same bits on every rank in every case.

Fused route (``cba_step``; lam as the step reports it; point = the accepted trial point, relative to the largest entry of the step, bar 1e-7,
robust 1e-5 on the columns above the floor):

                        lam      lin     gh/jg   sinv    grad    step    sums    cost    norm    point
    EVEN 2              1.58e-4  1.9e-16 2.1e-15 3.8e-16 3.7e-15 3.4e-12 2.4e-15 4.8e-13 1.3e-12 3.4e-12
    EVEN 3              1.58e-4  2.2e-16 2.1e-15 3.8e-16 3.6e-15 3.1e-12 2.6e-15 4.6e-13 1.2e-12 3.1e-12
    GLOBAL 3            1.62e-4  2.3e-15 6.1e-16 8.0e-16 5.1e-15 1.2e-12 1.5e-15 2.3e-14 5.5e-14 1.2e-12
    GLOBAL_REFINE 2     2.16e-4  1.5e-15 5.2e-16 7.7e-16 4.9e-15 3.9e-11 2.2e-13 2.5e-13 6.3e-15 3.9e-11
    ROBUST 2 (near min) 2.24e-1  2.3e-15 1.7e-13 7.1e-16 8.4e-14 3.5e-13    -    3.7e-12    -    4.4e-14

Whole solves against the single-rank solve (bars of tests/test_multi_device.py: cost 1e-9, nfev +-5, aligned poses 1e-7, scale 1e-4):
SUBSET on 2 ranks status 2 / 2, nfev 5 / 5, cost 4e-15, poses 7e-15, scale 2e-7; ONE_POINT on 8 ranks status 1 / 1, nfev 5 / 5, cost 4e-13,
poses 1.4e-9, scale 2e-9.

Seeded fault (a scratch build, never committed: ``first = 0`` on every rank in run_step_scalars, so the camera entries of ||p||^2, <g_h, p>
and ||w||^2 are counted once per rank; the same on every rank, so no branch changes).  This file run once on it: 15 of 19 fail, every
linear-loss step test and every linear-loss fused test on p_sq (off by 0.19 .. 8.1 relative, bar 1e-7) and the ONE_POINT whole solve;
only the robust cases pass, which hold no step scalar (as _check_step), with SUBSET's solve and the refused group.
tests/test_multi_device.py run once on it: 4 of 11 fail (nfev 19 against 5 and 106 / 105 against 121, one status 1 against 2) — the
converged comparison notices this fault by its route on four of its six parametrised cases and not at all on the others.

No test of this file takes more than 0.5 s on the device; the file takes 2.3 s.
"""
from __future__ import annotations

import pytest

from tests import sharded_scenes as ss
from tests.helpers import aligned_difference
from tests.sharded_native import compare_fused, compare_step, fused_body, gather, replicated_differences, run_ranks, solve_body, step_body

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    from caliscope_amd import build
    from caliscope_amd.hip_engine import require_device

    build.build(verbose=False)
    require_device()  # fail loudly: these tests must never pass without the HIP extension


@pytest.fixture(autouse=True)
def _short_group_timeout(monkeypatch):
    monkeypatch.setenv("CBA_GROUP_TIMEOUT_S", "20")  # read by cba_group_create


def _ids(cases):
    return [f"{name}-{world}" for name, world in cases]


def _check_routes(name, recs):
    """The route every rank took, from ``cba_info`` and ``cba_step_supported`` after the join."""
    for rec in recs:
        assert rec["info"]["plan_state"] == 0 and rec["info"]["plan_error"] == 0
    heavy = [rec["info"]["n_heavy_points"] for rec in recs]
    supported = [rec["step_supported"] for rec in recs]
    print(f"{name}: schur_groups {[rec['info']['schur_groups'] for rec in recs]} heavy points {heavy} cba_step_supported {supported}")
    if name in ("GLOBAL", "GLOBAL_REFINE"):
        assert all(rec["info"]["schur_groups"] > 1 for rec in recs)
    if name == "ONE_POINT":  # k_heavy_schur on rank 0 only; the fused route is off for every rank, the seven that could run it included
        assert heavy == [1] + [0] * (len(recs) - 1) and supported == [0] * len(recs)
    elif name == "CONSTRAINED":  # rank 1 has no constraint rows and follows rank 0 to the primitives
        assert heavy == [0, 0] and supported == [0, 0]
    else:
        assert not any(heavy) and supported == [1] * len(recs)


@pytest.mark.parametrize("name,world", ss.CASES, ids=_ids(ss.CASES))
def test_sharded_step_matches_the_whole_problem_oracle(name, world):
    sc = ss.scene(name)
    recs = run_ranks(sc["problem"], sc["x0"], world, step_body(sc["x0"], ss.LAMBDAS))
    _check_routes(name, recs)
    differ = replicated_differences(recs)
    assert differ == [], f"{name} world {world}: not the same bits on every rank: {differ}"
    compare_step(sc, recs, ss.LAMBDAS, f"{name} world {world}")


@pytest.mark.parametrize("name,world", ss.FUSED_CASES, ids=_ids(ss.FUSED_CASES))
def test_fused_sharded_step_matches_the_whole_problem_oracle(name, world):
    """One ``cba_step(-1.0)`` per rank: the trial's camera blocks, its cost, the step norm and the flags in one collective, then
    k_unpack_camera_grad.  The step is compared at the damping it reports; the trial point is read back after ``accept``.  ROBUST starts near a
    minimum (``sharded_scenes.fused_start``): at x0 the library hands the iteration back to the primitives and there is no trial to compare."""
    sc, x = ss.scene(name), ss.fused_start(name)
    recs = run_ranks(sc["problem"], x, world, fused_body(x))
    assert [rec["step_supported"] for rec in recs] == [1] * world
    differ = replicated_differences(recs)
    assert differ == [], f"{name} world {world}: not the same bits on every rank: {differ}"
    compare_fused(sc, x, recs, f"{name} world {world} fused")


@pytest.mark.parametrize("name,world", ss.SOLVE_CASES, ids=_ids(ss.SOLVE_CASES))
def test_whole_sharded_solve_is_the_same_bits_on_every_rank(name, world):
    """``eng.solve`` on every rank: x (camera block), cost, nfev and status the same bits everywhere, and the result held to the single-rank
    solve under tests/test_multi_device.py's bars."""
    from caliscope_amd.hip_engine import HipEngine

    sc = ss.scene(name)
    tol = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12, max_nfev=200)
    with HipEngine(sc["problem"]) as eng:
        one = eng.solve(sc["x0"], **tol)
    recs = run_ranks(sc["problem"], sc["x0"], world, solve_body(sc["x0"], **tol))
    differ = replicated_differences(recs)
    assert differ == [], f"{name} world {world}: not the same bits on every rank: {differ}"
    cost, nfev, status = recs[0]["result"]
    pos, ang, scale = aligned_difference(sc["par"], gather(recs, "x"), one.x)
    print(f"{name} world {world} solve: status {status} / {one.status}, nfev {nfev} / {one.nfev}, cost {abs(cost - one.cost) / one.cost:.2e} (bar 1e-9), "
          f"position {pos:.2e} angle {ang:.2e} (bar 1e-7), scale - 1 {abs(scale - 1):.2e} (bar 1e-4)")
    assert status == one.status
    assert abs(cost - one.cost) <= 1e-9 * one.cost
    assert abs(nfev - one.nfev) <= 5
    assert pos < 1e-7 and ang < 1e-7 and abs(scale - 1) < 1e-4


def test_a_group_of_seventeen_is_refused():
    from caliscope_amd.exceptions import BackendError
    from caliscope_amd.hip_engine import DeviceGroup

    with pytest.raises(BackendError, match=r"cba_group_create: world 17 \(1\.\.16\)"):
        DeviceGroup(ss.GROUP_MAX + 1)
