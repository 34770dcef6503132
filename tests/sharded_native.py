"""Lock-step driver of a point-sharded step and its comparison with the whole-problem oracle.

``run_ranks`` runs one host thread per rank on the library's in-process group (``cba_group_*``: several handles of one process, on one device
or on the CPU test build), ``step_body`` / ``fused_body`` / ``solve_body`` record what every rank returned, ``gather`` puts the ranks' vectors
back into the reference layout, and ``compare_step`` / ``compare_fused`` hold the records to ``oracle.engine.OracleEngine`` on the WHOLE,
unsharded problem and to the sparse checks of tests/test_gpu_parity.py::_check_step (``splu`` of J^T J + lam D^2 for the full step, S formed
from its blocks) under that function's bars.

Nothing is asserted inside a rank's thread: a rank that stops early would leave its peers in a collective.  The bodies only record; the
comparisons run afterwards in the caller's thread.
"""
from __future__ import annotations

import ctypes as C
import threading
import time

import numpy as np

from caliscope_amd.sharding import shard_problem

VEC_GRAD, VEC_STEP, VEC_SCALE_INV = 2, 3, 4
LIN_FIELDS = ("g_norm_inf", "gh_sq", "jg_sq", "x_scaled_norm", "x_norm")
STEP_FIELDS = ("p_sq", "gh_dot_p", "w_sq")
GRAM_ARGS = (0.3, -1.2, 1.1, 0.4)
TRIAL_ARGS = (-1e-3, 0.5)


def run_ranks(problem, x0, world, body):
    """``body(rank, engine, shard)`` on every rank of a ``world``-rank device group; returns the list of what the bodies returned.

    One ``DeviceGroup(world)`` and one thread per rank; each rank shards ``problem`` with the product's ``shard_problem``, creates its
    ``HipEngine``, joins the group, runs ``body`` and closes its handle.  A rank that raises aborts the group, so that its peers come back with
    the library's "group aborted" error instead of waiting, and the exception of the rank that failed first is re-raised here — the pattern of
    ``caliscope_amd.distributed.solve_multi_device``.

    EVERY RANK MUST RUN THE SAME SEQUENCE OF COLLECTIVE CALLS: ``begin``, ``linearize``, ``newton_step``, ``subspace_gram``, ``trial``,
    ``cba_step``, ``residuals`` and ``solve`` exchange between the ranks, so a body must not branch on anything that differs between ranks
    (``get_vector``, ``reduced_system``, ``info``, ``accept`` are local).  ``x0`` is the whole vector; a body takes its part with
    ``shard.local_x(x0)``."""
    from caliscope_amd.hip_engine import DeviceGroup, HipEngine

    group = DeviceGroup(world)
    results: list = [None] * world
    errors: list = [None] * world

    def member(rank):
        engine = None
        try:
            shard = shard_problem(problem, rank, world)
            engine = HipEngine(shard.problem)
            engine.group_join(group, rank)
            results[rank] = body(rank, engine, shard)
        except BaseException as exc:  # noqa: BLE001 - re-raised in the caller's thread
            errors[rank] = (time.monotonic(), exc)
            group.abort()
        finally:
            if engine is not None:
                engine.close()

    threads = [threading.Thread(target=member, args=(r,), name=f"cba-rank{r}", daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    group.close()
    failed = sorted((e for e in errors if e is not None), key=lambda te: te[0])
    if failed:
        raise failed[0][1]
    return results


def gather(shard_results, name):
    """The whole vector ``name`` in the reference layout from the ranks' records (dicts with their ``shard``): the camera block from rank 0,
    the points scattered back through ``shard.owned_points``."""
    first = shard_results[0]
    ncp = first["shard"].problem.parameterization.n_camera_params
    pts = np.full((first["shard"].n_points_global, 3), np.nan)
    for rec in shard_results:
        pts[rec["shard"].owned_points] = rec[name][ncp:].reshape(-1, 3)
    assert not np.isnan(pts).any(), "the shards do not cover every point"
    return np.concatenate([first[name][:ncp], pts.reshape(-1)])


# ---- bodies: what one rank does and records ---------------------------------------------------------------------------------------------
def _lin(o):
    return tuple(float(getattr(o, f)) for f in LIN_FIELDS)


def _newton(o):
    return (bool(o.ok),) + tuple(float(getattr(o, f)) for f in STEP_FIELDS)


def step_body(x0, lambdas, with_system=True):
    """tests/test_gpu_parity.py::_check_step's sequence.  ``with_system=False`` leaves ``reduced_system`` out (the CPU build)."""

    def body(rank, eng, shard):
        rec = dict(shard=shard, info=eng.info(), step_supported=int(eng.lib.cba_step_supported(eng._h)))
        rec["cost0"] = eng.begin(shard.local_x(x0))
        rec["lin"] = _lin(eng.linearize())
        rec["g"], rec["sinv"] = eng.get_vector(VEC_GRAD), eng.get_vector(VEC_SCALE_INV)
        for i, lam in enumerate(lambdas):
            rec[f"newton{i}"] = _newton(eng.newton_step(lam))
            rec[f"s{i}"] = eng.get_vector(VEC_STEP)
            if with_system:
                rec[f"S{i}"], rec[f"rhs{i}"] = eng.reduced_system()
            rec[f"gram{i}"] = eng.subspace_gram(*GRAM_ARGS)
            t = eng.trial(*TRIAL_ARGS)
            rec[f"trial{i}"] = (float(t.cost), float(t.step_norm), bool(t.finite))
        eng.accept()
        rec["lin2"] = _lin(eng.linearize())
        rec["sinv2"] = eng.get_vector(VEC_SCALE_INV)
        return rec

    return body


def fused_body(x0):
    """One ``cba_step(-1.0)`` (called as tests/test_scale_fused_gpu.py calls it), the accepted trial point read back through ``current_x``."""
    from caliscope_amd import _lib

    def body(rank, eng, shard):
        rec = dict(shard=shard, step_supported=int(eng.lib.cba_step_supported(eng._h)))
        rec["cost0"] = eng.begin(shard.local_x(x0))
        si = _lib.StepInfo()
        eng._check(eng.lib.cba_step(eng._h, -1.0, C.byref(si)), "cba_step")
        rec["need_host"] = int(si.need_host)
        rec["lin"], rec["newton"] = _lin(si.lin), _newton(si.newton)
        rec["trial"] = (float(si.trial.cost), float(si.trial.step_norm), bool(si.trial.finite))
        rec["step"] = (float(si.lam), float(si.radius), float(si.alpha), float(si.beta))
        rec["g"], rec["sinv"], rec["s"] = eng.get_vector(VEC_GRAD), eng.get_vector(VEC_SCALE_INV), eng.get_vector(VEC_STEP)
        if rec["need_host"] == 0:  # (the same on every rank: it came out of the exchange; need_host != 0 means there is no trial point to accept)
            eng.accept()
        rec["x_new"] = eng.current_x()
        return rec

    return body


def solve_body(x0, **tol):
    def body(rank, eng, shard):
        res = eng.solve(shard.local_x(x0), **tol)
        return dict(shard=shard, x=res.x, result=(float(res.cost), int(res.nfev), int(res.status)))

    return body


# ---- replicated state: the same bits on every rank -----------------------------------------------------------------------------------------
def _bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def replicated_differences(recs):
    """Names of the replicated quantities that are not the same bits on every rank (scalars, S and rhs as they are; of the vectors the
    camera block).  Empty when the ranks agree."""
    ncp = recs[0]["shard"].problem.parameterization.n_camera_params
    vectors = ("g", "sinv", "sinv2", "s", "x_new", "x")
    local = ("shard", "info", "step_supported")
    bad = []
    for name, v0 in recs[0].items():
        if name in local:
            continue
        is_vec = name in vectors or (name[0] == "s" and name[1:].isdigit())
        for q, rec in enumerate(recs[1:], 1):
            a, b = (v0[:ncp], rec[name][:ncp]) if is_vec else (v0, rec[name])
            if _bits(a) != _bits(b):
                bad.append(f"{name}@rank{q}")
    return bad


# ---- the reference and the comparisons --------------------------------------------------------------------------------------------------------
def oracle_for(scene):
    from oracle.engine import OracleEngine

    prob = scene["problem"]
    return OracleEngine(scene["par"], prob.camera_indices, prob.image_coords, prob.obj_indices, loss=scene["loss"], f_scale=scene["f_scale"],
                        constraints=scene["constraints"])


def sparse_reference(ora, lam, ncp):
    """(s_full, S_ref) of tests/test_gpu_parity.py::_check_step: the damped normal equations of the oracle's sparse J solved as ONE system by
    splu, and the reduced camera system formed from its blocks — independent of any Schur code."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu

    H = (ora.J.T @ ora.J + lam * sp.diags(ora.scale_inv ** 2)).tocsc()
    s_full = splu(H).solve(-ora.g)
    Hcc, Hcp, Hpp = H[:ncp, :ncp].toarray(), H[:ncp, ncp:], H[ncp:, ncp:].tocsc()
    return s_full, Hcc - Hcp @ splu(Hpp).solve(Hcp.T.toarray())


def first_step_shape(scene, x):
    """(lam, ||w||^2 / ||p||^2) of the first trust-region iteration at ``x`` on the oracle: the damping trf's rule gives for the initial radius
    ||x scale_inv|| and how far the damped step is from collinear with the gradient.  ``cba_step`` makes a trial point only while the ratio is
    above 1e-3 (fused_subspace in csrc/cba_kernels.h); below, it returns need_host = 1."""
    import math

    from oracle.trf_driver import DAMPING_FLOOR, _min_quadratic_on_segment

    ora = oracle_for(scene)
    ora.begin(x)
    lin = ora.linearize()
    radius = lin.x_scaled_norm if lin.x_scaled_norm > 0 else 1.0
    lam = max(-_min_quadratic_on_segment(0.5 * lin.jg_sq, -lin.gh_sq, radius / math.sqrt(lin.gh_sq)) / (radius * radius), DAMPING_FLOOR)
    st = ora.newton_step(lam)
    assert st.ok
    return lam, st.w_sq / st.p_sq


def _relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def _relscalar(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


class Figures:
    """Every figure is printed before it is asserted; ``worst`` keeps the largest ratio figure / bar per name."""

    def __init__(self, tag):
        self.tag, self.worst = tag, {}

    def hold(self, name, value, bar):
        print(f"{self.tag}: {name} {value:.3e} (bar {bar:.0e})")
        self.worst[name] = max(self.worst.get(name, 0.0), value)
        assert value <= bar, f"{self.tag}: {name} {value:.3e} exceeds {bar:.0e}"

    def summary(self):
        print(f"FIGURES {self.tag}: " + " ".join(f"{k}={v:.1e}" for k, v in self.worst.items()))


def step_tolerance(lam):
    """Step against the oracle: 1e-8, 2e-8 at lam = 1e-7 (test_gpu_parity.py::_check_step: the summation order of the FP64 atomics is amplified by
    the nearly singular gauge directions)."""
    return 1e-8 if lam >= 1e-4 else 2e-8


def full_tolerance(lam):
    """Step against the sparse LU of the full system (the same function; these rigs have fewer than 300 cameras)."""
    return 1e-8 if lam >= 1e-3 else 1e-7


def compare_step(scene, recs, lambdas, tag, with_system=True):
    """The records of ``step_body`` on every rank against the whole-problem oracle, under the bars test_gpu_parity.py::test_step_parity holds
    the single-rank step to for the same loss (``_check_step``; nothing is added for the sharded order of the sums)."""
    ora = oracle_for(scene)
    loss, ncp, x0 = scene["loss"], scene["par"].n_camera_params, scene["x0"]
    linear = loss == "linear"
    fig = Figures(tag)
    r0 = recs[0]
    fig.hold("cost0", _relscalar(r0["cost0"], ora.begin(x0)), 1e-13)
    lo = ora.linearize()
    stol = 1e-10 if linear else 5e-2
    for k, fld in enumerate(LIN_FIELDS):
        fig.hold(fld, _relscalar(r0["lin"][k], getattr(lo, fld)), stol if fld in ("gh_sq", "jg_sq") else 1e-10)
    fig.hold("scale_inv", _relmax(gather(recs, "sinv"), ora.scale_inv), 1e-12 if linear else 1e-7)
    fig.hold("gradient", _relmax(gather(recs, "g"), ora.g), 1e-11)
    for i, lam in enumerate(lambdas):
        so = ora.newton_step(lam)
        nh = r0[f"newton{i}"]
        assert nh[0] and so.ok, (tag, lam)
        s_h = gather(recs, f"s{i}")
        if linear:
            fig.hold(f"step[{lam:g}]", _relmax(s_h, ora.s), step_tolerance(lam))
            for k, fld in enumerate(STEP_FIELDS):
                fig.hold(f"{fld}[{lam:g}]", _relscalar(nh[1 + k], getattr(so, fld)), 1e-7)
        else:  # leave out the parameters whose columns live at the sqrt(EPS) floor (_check_step)
            ok = ora.scale_inv > 1e-4 * np.median(ora.scale_inv)
            assert ok.mean() > 0.9
            fig.hold(f"step[{lam:g}]", float(np.abs(s_h - ora.s)[ok].max() / np.abs(ora.s[ok]).max()), 1e-5)
        if linear:
            s_full, S_ref = sparse_reference(ora, lam, ncp)
            fig.hold(f"step_vs_splu[{lam:g}]", _relmax(s_h, s_full), full_tolerance(lam))
        if with_system:
            S, rhs = r0[f"S{i}"], r0[f"rhs{i}"]
            fig.hold(f"S_symmetry[{lam:g}]", float(np.abs(S - S.T).max() / np.abs(S).max()), 1e-14)
            if linear:
                fig.hold(f"S[{lam:g}]", _relmax(S, S_ref), 1e-9)
            fig.hold(f"S_residual[{lam:g}]", float(np.linalg.norm(S @ s_h[:ncp] - rhs) / np.linalg.norm(rhs)), 1e-7)
        go = ora.subspace_gram(*GRAM_ARGS)
        fig.hold(f"gram[{lam:g}]", max(_relscalar(a, b) for a, b in zip(r0[f"gram{i}"], go)), max(1e-7, stol))
        cost_h, norm_h, finite_h = r0[f"trial{i}"]
        if linear:
            to = ora.trial(*TRIAL_ARGS)
            assert finite_h
            fig.hold(f"trial_cost[{lam:g}]", _relscalar(cost_h, to.cost), 1e-9)
            fig.hold(f"step_norm[{lam:g}]", _relscalar(norm_h, to.step_norm), 1e-7)
        else:  # the same trial on both engines from the device's step, so that floor-column noise does not enter (_check_step)
            ora.s = s_h
            to = ora.trial(*TRIAL_ARGS)
            assert finite_h == to.finite
            if to.finite:
                fig.hold(f"trial_cost[{lam:g}]", _relscalar(cost_h, to.cost), 1e-6 if to.step_norm < 1e6 else 1e-4)
    ora.accept()
    lo = ora.linearize()  # the second linearisation: the monotone-max scale rule across the exchange
    fig.hold("gh_sq_2nd", _relscalar(r0["lin2"][1], lo.gh_sq), max(1e-7, stol))
    fig.hold("jg_sq_2nd", _relscalar(r0["lin2"][2], lo.jg_sq), max(1e-7, stol))
    fig.hold("scale_inv_2nd", _relmax(gather(recs, "sinv2"), ora.scale_inv), 1e-6 if linear else 1e-4)
    fig.summary()
    return fig


def compare_fused(scene, x0, recs, tag):
    """``fused_body(x0)``'s records against the oracle at the damping and the trial coefficients the step reports, under compare_step's bars."""
    ora = oracle_for(scene)
    loss = scene["loss"]
    linear = loss == "linear"
    fig = Figures(tag)
    r0 = recs[0]
    lam, _, alpha, beta = r0["step"]
    assert r0["need_host"] == 0 and r0["newton"][0] and r0["trial"][2], (tag, r0["need_host"], r0["newton"], r0["trial"])
    ora.begin(x0)
    lo = ora.linearize()
    stol = 1e-10 if linear else 5e-2
    for k, fld in enumerate(LIN_FIELDS):
        fig.hold(fld, _relscalar(r0["lin"][k], getattr(lo, fld)), stol if fld in ("gh_sq", "jg_sq") else 1e-10)
    fig.hold("scale_inv", _relmax(gather(recs, "sinv"), ora.scale_inv), 1e-12 if linear else 1e-7)
    fig.hold("gradient", _relmax(gather(recs, "g"), ora.g), 1e-11)
    so = ora.newton_step(lam)
    assert so.ok
    s_h = gather(recs, "s")
    print(f"{tag}: lam {lam:.6e} alpha {alpha:.6e} beta {beta:.6e}")
    if linear:
        fig.hold("step", _relmax(s_h, ora.s), step_tolerance(lam))
        for k, fld in enumerate(STEP_FIELDS):
            fig.hold(fld, _relscalar(r0["newton"][1 + k], getattr(so, fld)), 1e-7)
    else:
        ok = ora.scale_inv > 1e-4 * np.median(ora.scale_inv)
        assert ok.mean() > 0.9
        fig.hold("step", float(np.abs(s_h - ora.s)[ok].max() / np.abs(ora.s[ok]).max()), 1e-5)
        ora.s = s_h
    to = ora.trial(alpha, beta)
    assert to.finite
    ctol = 1e-9 if linear else (1e-6 if to.step_norm < 1e6 else 1e-4)
    fig.hold("trial_cost", _relscalar(r0["trial"][0], to.cost), ctol)
    # the accepted trial point against x + alpha g / scale_inv^2 + beta s on the oracle's own vectors, relative to the largest entry of the step
    # that was taken: the step-norm bar (linear), the step bar on the columns above the floor (robust)
    x_h, taken = gather(recs, "x_new"), ora.x_new - ora.x
    if linear:
        fig.hold("step_norm", _relscalar(r0["trial"][1], to.step_norm), 1e-7)
        fig.hold("trial_point", float(np.abs(x_h - ora.x_new).max() / np.abs(taken).max()), 1e-7)
    else:
        fig.hold("trial_point", float(np.abs(x_h - ora.x_new)[ok].max() / np.abs(taken[ok]).max()), 1e-5)
    fig.summary()
    return fig
