"""The host planning of a handle's set-up (csrc/host_plan.h: what cba_create and cba_set_constraints decide between their device calls) on the
CPU: compiled by g++ behind tests/native/setup_harness.cpp and checked against numpy / scipy restatements and invariants.  The problem
description's checks are driven through the CPU build of the C ABI (tests/native/cpu_library.cpp), which shares them with the device library."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests.native_build import CSRC, INCLUDE, NATIVE, ROOT, compile_native, load_native

I32P, I64P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_long), C.POINTER(C.c_double)
U8P, U16P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
ERR_INVALID, ERR_UNSUPPORTED = -1, -4

_KERNELS = (ROOT / "caliscope_amd" / "csrc" / "cba_kernels.h").read_text()


def _const(name):
    return int(re.search(rf"constexpr int {name} = (\d+);", _KERNELS).group(1))


CHUNK, BLOCK, HEAVY_OBS, CS_MAX_PTS, DET_ROUND, CON_LDS_POINTS = (_const(n) for n in ("CHUNK", "BLOCK", "HEAVY_OBS", "CS_MAX_PTS", "DET_ROUND", "CON_LDS_POINTS"))


def _p(a, t):
    return a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def lib():
    lib = load_native(NATIVE / "setup_harness.cpp", flags=("-pthread",))
    lib.sp_last_error.restype = C.c_char_p
    lib.sp_point_tables.restype = C.c_int
    lib.sp_point_tables.argtypes = [C.c_int, C.c_long, I32P, I32P, C.c_int, C.c_int, C.c_int] + [I32P] * 7 + [I64P]
    lib.sp_det_plan.restype = C.c_int
    lib.sp_det_plan.argtypes = [C.c_int, C.c_int, C.c_long, I32P, I32P, C.c_int, C.c_int, C.c_int, U8P, U16P, I32P]
    lib.sp_cs_plan.restype = None
    lib.sp_cs_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, I32P, I32P, I32P, C.c_long, C.c_long, C.c_int, C.c_int] + [I32P] * 4 + [I64P]
    lib.sp_constraint_plan.restype = C.c_int
    lib.sp_constraint_plan.argtypes = [C.c_int, C.c_int, C.c_int, I32P, I32P, F64P, F64P, C.c_int, I32P] + [I32P] * 6 + [I64P, F64P, F64P, I32P, I64P]
    lib.sp_mail_layout.restype = None
    lib.sp_mail_layout.argtypes = [C.c_int, I64P]
    return lib


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _observations(counts, n_cams, rng):
    """Observations point by point: `counts[q]` of point q, cameras drawn at random (repeats allowed), in (point, camera) order."""
    counts = np.asarray(counts, dtype=np.int64)
    obs_pt = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    obs_cam = rng.integers(0, n_cams, size=len(obs_pt)).astype(np.int32)
    order = np.lexsort((obs_cam, obs_pt))
    return obs_pt[order], obs_cam[order]


def _tables(lib, counts, n_cams, rng, shuffle=False):
    obs_pt, obs_cam = _observations(counts, n_cams, rng)
    if shuffle:
        perm = rng.permutation(len(obs_pt))
        obs_pt, obs_cam = np.ascontiguousarray(obs_pt[perm]), np.ascontiguousarray(obs_cam[perm])
    P, N = len(counts), len(obs_pt)
    i32 = lambda n: np.zeros(n, dtype=np.int32)  # noqa: E731
    out = dict(cam=i32(N), pt=i32(N), pt_start=i32(P + 1), chunk_start=i32(N + 2), chunk_pts=i32(2 * (N + 1)), heavy=i32(P), heavy_frag=i32(P))
    scal = np.zeros(4, dtype=np.int64)
    rc = lib.sp_point_tables(P, N, _p(obs_pt, I32P), _p(obs_cam, I32P), n_cams, CHUNK, HEAVY_OBS, *(_p(out[k], I32P) for k in ("cam", "pt", "pt_start", "chunk_start", "chunk_pts", "heavy", "heavy_frag")),
                             _p(scal, I64P))
    if rc:
        return rc, lib.sp_last_error().decode()
    nch, n_heavy = int(scal[0]), int(scal[2])
    out.update(P=P, N=N, C=n_cams, n_chunks=nch, max_obs=int(scal[1]), has_fragments=bool(scal[3]), counts=np.asarray(counts))
    out["chunk_start"] = out["chunk_start"][: nch + 1]
    out["chunk_pts"] = out["chunk_pts"][: 2 * nch].reshape(nch, 2)
    out["heavy"], out["heavy_frag"] = out["heavy"][:n_heavy], out["heavy_frag"][:n_heavy]
    return out


def _cs(lib, t, workgroups, cap, enabled=True, deterministic=False, chunk_pts=None):
    nch = t["n_chunks"]
    cp = np.ascontiguousarray(t["chunk_pts"] if chunk_pts is None else chunk_pts, dtype=np.int32)
    sc_obs, sc_p0, sc_np, cperm = (np.zeros(n, dtype=np.int32) for n in (nch + 1, nch, nch, t["N"]))
    scal = np.zeros(4, dtype=np.int64)
    lib.sp_cs_plan(int(enabled), int(deterministic), t["C"], t["N"], nch, _p(t["chunk_start"], I32P), _p(cp, I32P), _p(t["cam"], I32P), workgroups, cap, CHUNK, CS_MAX_PTS,
                   _p(sc_obs, I32P), _p(sc_p0, I32P), _p(sc_np, I32P), _p(cperm, I32P), _p(scal, I64P))
    n_sc = int(scal[0])
    return dict(n_sc=n_sc, pmax=int(scal[1]), rounds=int(scal[2]), greedy=bool(scal[3]), sc_obs=sc_obs[: n_sc + 1], sc_p0=sc_p0[:n_sc], sc_np=sc_np[:n_sc], cperm=cperm)


# ---- point tables ----------------------------------------------------------------------------------------------------------------------
def test_point_tables_follow_the_sorted_observations(lib):
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 30, size=3000)  # (zeros: unobserved points inside the chunks' ranges)
    counts[[17, 900, 2999]] = (HEAVY_OBS + 1, HEAVY_OBS, CHUNK + 44)
    t = _tables(lib, counts, 12, rng, shuffle=True)
    starts = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(t["pt_start"], starts) and t["max_obs"] == counts.max()
    assert np.array_equal(t["pt"], np.repeat(np.arange(len(counts)), counts))
    assert np.all((np.diff(t["pt"]) > 0) | (np.diff(t["cam"]) >= 0))  # cameras ascend inside a point
    cs = t["chunk_start"]
    assert cs[0] == 0 and cs[-1] == t["N"] and np.all(np.diff(cs) > 0) and np.all(np.diff(cs) <= CHUNK)
    # per chunk: first point and number of points in its range, observed or not; a fragment of a point larger than a chunk is marked -1
    first, last = t["pt"][cs[:-1]], t["pt"][cs[1:] - 1]
    fragment = counts[first] > CHUNK
    assert np.array_equal(t["chunk_pts"][:, 0], first)
    assert np.array_equal(t["chunk_pts"][:, 1], np.where(fragment, -1, last - first + 1))
    assert fragment.sum() == 2 and np.all(first[fragment] == 2999) and t["has_fragments"]
    whole = ~fragment
    assert np.all(first[whole][1:] > last[whole][:-1])  # whole points only: no point in two chunks
    unobserved_inside = sum(int((counts[a : b + 1] == 0).sum()) for a, b in zip(first[whole], last[whole]))
    assert (counts == 0).sum() // 2 < unobserved_inside <= (counts == 0).sum()  # the ranges do count points nobody saw (all but those between two chunks)
    # heavy points: exactly those above HEAVY_OBS, flagged when they do not fit a chunk
    assert np.array_equal(t["heavy"], np.flatnonzero(counts > HEAVY_OBS)) and list(t["heavy"]) == [17, 2999]
    assert list(t["heavy_frag"]) == [0, 1]
    assert not _tables(lib, np.full(500, 7), 12, rng)["has_fragments"]


@pytest.mark.parametrize("n_points", [100, 6400])
def test_too_many_heavy_points_keep_the_pair_plan_or_are_refused(lib, n_points):
    rng = np.random.default_rng(1)
    limit = max(64, n_points // 64)
    counts = np.full(n_points, 4)
    counts[:limit] = HEAVY_OBS + 1
    t = _tables(lib, counts, 16, rng)
    assert np.array_equal(t["heavy"], np.arange(limit))  # at the limit: kept
    counts[limit] = HEAVY_OBS + 1
    t = _tables(lib, counts, 16, rng)
    assert len(t["heavy"]) == 0 and t["max_obs"] == HEAVY_OBS + 1  # one more, none beyond a chunk: the list is cleared
    counts[limit + 1] = CHUNK  # (a full chunk is not beyond one)
    assert len(_tables(lib, counts, 16, rng)["heavy"]) == 0
    counts[limit + 1] = CHUNK + 1
    rc, msg = _tables(lib, counts, 16, rng)
    assert rc == ERR_UNSUPPORTED
    assert msg == f"{limit + 2} world points have more than {HEAVY_OBS} observations (one has {CHUNK + 1}); at most {limit} such points are supported"


# ---- fixed-order sums ------------------------------------------------------------------------------------------------------------------
def _det(lib, t, nct):
    nch, n_cams = t["n_chunks"], t["C"]
    perm, cst, det_m = np.zeros(nch * CHUNK, dtype=np.uint8), np.zeros(nch * (n_cams + 1), dtype=np.uint16), np.zeros(1, dtype=np.int32)
    rc = lib.sp_det_plan(n_cams, nct, nch, _p(t["chunk_start"], I32P), _p(t["cam"], I32P), CHUNK, DET_ROUND, BLOCK, _p(perm, U8P), _p(cst, U16P), _p(det_m, I32P))
    return rc, int(det_m[0]), perm.reshape(nch, CHUNK), cst.reshape(nch, n_cams + 1)


@pytest.mark.parametrize("nct,steps", [(6, (3, 5, 8, 16)), (9, (3, 5, 8))])
def test_tasks_per_thread_of_the_fixed_order_sums_at_every_step(lib, nct, steps):
    rng = np.random.default_rng(2)
    for m in steps:
        edge = m * BLOCK // DET_ROUND  # the last camera count with ceil(C DET_ROUND / BLOCK) <= m
        for n_cams in (edge, edge + 1):
            need = -(-n_cams * DET_ROUND // BLOCK)
            assert (need <= m) == (n_cams == edge)
            expect = next((s for s in steps if need <= s), None)
            rc, det_m, _, _ = _det(lib, _tables(lib, np.full(300, 5), n_cams, rng), nct)
            if expect is None:
                assert rc == ERR_UNSUPPORTED
                assert lib.sp_last_error().decode() == (f"deterministic sums support up to {steps[-1] * BLOCK // DET_ROUND} {'six' if nct == 6 else 'nine'}-parameter cameras, "
                                                        f"the problem has {n_cams}")
            else:
                assert rc == 0 and det_m == expect, (n_cams, det_m)


def test_fixed_order_plan_is_a_stable_order_by_camera_per_chunk(lib):
    rng = np.random.default_rng(3)
    t = _tables(lib, rng.integers(1, 40, size=2000), 9, rng)
    rc, det_m, perm, cst = _det(lib, t, 6)
    assert rc == 0 and det_m == 3 and t["n_chunks"] > 100
    for c in range(t["n_chunks"]):
        o0, o1 = t["chunk_start"][c : c + 2]
        cams = t["cam"][o0:o1]
        assert np.array_equal(perm[c, : o1 - o0], np.argsort(cams, kind="stable"))
        assert np.array_equal(cst[c], np.concatenate([[0], np.cumsum(np.bincount(cams, minlength=9))]))


# ---- camera-sorted super-chunks --------------------------------------------------------------------------------------------------------
def _check_super_chunks(t, cs, cap):
    """(a) tiling, (b) caps, (c) the permutation — whatever way the cut was made."""
    sc_obs, hcs, hcp = cs["sc_obs"], t["chunk_start"], t["chunk_pts"]
    assert cs["n_sc"] > 0 and sc_obs[0] == 0 and sc_obs[-1] == t["N"] and np.all(np.diff(sc_obs) > 0)
    at = np.searchsorted(hcs, sc_obs)  # the chunk every super-chunk begins with
    assert np.array_equal(hcs[at], sc_obs)  # cut at chunk boundaries only: with the line above, every chunk is in exactly one, in order
    assert np.all(np.diff(sc_obs) <= cap + CHUNK)
    last = at[1:] - 1
    assert np.array_equal(cs["sc_p0"], hcp[at[:-1], 0])
    assert np.array_equal(cs["sc_np"], hcp[last, 0] + hcp[last, 1] - hcp[at[:-1], 0])
    assert np.all(cs["sc_np"] <= CS_MAX_PTS) and cs["pmax"] == -(-cs["sc_np"].max() // 32) * 32
    # positions of a super-chunk hold its own observations, by camera, point order kept inside a camera: one stable sort by (super-chunk, camera)
    sc_of = np.searchsorted(sc_obs, np.arange(t["N"]), side="right") - 1
    assert np.array_equal(cs["cperm"], np.argsort(sc_of.astype(np.int64) * t["C"] + t["cam"], kind="stable"))


def _nearest_cuts(hcs, N, n):
    """Cut k at the chunk boundary nearest to ceil(k N / n): at least one chunk past the previous cut, a tie to the earlier one, the last at the end."""
    cuts, q = [0], 0
    for k in range(1, n):
        goal = -(-N * k // n)
        cand = np.arange(q + 1, len(hcs))
        q = int(cand[np.argmin(np.abs(hcs[cand].astype(np.int64) - goal))])  # (argmin: the first of equals)
        cuts.append(q)
    return hcs[np.array(cuts + [len(hcs) - 1])]


@pytest.mark.parametrize("name,workgroups,cap,n_expected", [("20k x 10", 52, 2048, 104), ("200k x 10", 512, 2048, 1024), ("20k x 2..18", 52, 2048, 104), ("100k x 10", 256, 4096, 256)])
def test_regular_inputs_get_exactly_rounds_times_workgroups_super_chunks(lib, name, workgroups, cap, n_expected):
    rng = np.random.default_rng(0)
    counts = rng.integers(2, 19, size=20000) if ".." in name else np.full(int(name.split("k")[0]) * 1000, 10)
    t = _tables(lib, counts, 16, rng)
    cs = _cs(lib, t, workgroups, cap)
    _check_super_chunks(t, cs, cap)
    assert not cs["greedy"] and cs["rounds"] == max(1, -(-t["N"] // (workgroups * cap)))  # the first cut fitted
    n = min(cs["rounds"] * workgroups, t["n_chunks"])
    assert cs["n_sc"] == n == n_expected
    assert np.array_equal(cs["sc_obs"], _nearest_cuts(t["chunk_start"], t["N"], n))
    sizes = np.diff(cs["sc_obs"])
    assert sizes.max() <= cap and sizes.min() >= t["N"] // n - CHUNK  # (a nearest boundary is at most half a chunk from its goal)
    if name == "20k x 10":
        assert sizes.min() >= 1750 and sizes.max() <= 2000


def test_a_small_problem_gets_one_super_chunk_per_chunk(lib):
    rng = np.random.default_rng(4)
    t = _tables(lib, np.full(300, 6), 4, rng)
    cs = _cs(lib, t, 512, 2048)
    _check_super_chunks(t, cs, 2048)
    assert cs["n_sc"] == t["n_chunks"] == 8 and not cs["greedy"]


def test_the_point_cap_sends_sparse_points_to_the_greedy_fill(lib):
    rng = np.random.default_rng(5)
    t = _tables(lib, np.full(20000, 2), 4, rng)
    cs = _cs(lib, t, 2, 2048)
    # 2 observations per point: a cut of N / (2 rounds) observations holds N / (4 rounds) points, below CS_MAX_PTS only from round 20 on; the
    # eight attempts are rounds 10 .. 17
    assert cs["greedy"] and cs["rounds"] == 17
    _check_super_chunks(t, cs, 2048)
    assert cs["n_sc"] > 2 * 17 and np.all(np.diff(cs["sc_obs"]) <= max(CHUNK, -(-t["N"] // 34)))


def test_no_super_chunks_where_k_build_cs_cannot_run(lib):
    rng = np.random.default_rng(6)
    regular = _tables(lib, np.full(2000, 10), 8, rng)
    assert _cs(lib, regular, 52, 2048)["n_sc"] > 0
    assert _cs(lib, regular, 52, 2048, enabled=False)["n_sc"] == 0
    assert _cs(lib, regular, 52, 2048, deterministic=True)["n_sc"] == 0
    counts = np.full(2000, 10)
    counts[1000] = CHUNK + 1  # a fragment
    t = _tables(lib, counts, 8, rng)
    assert t["has_fragments"] and _cs(lib, t, 52, 2048)["n_sc"] == 0
    counts = np.zeros(3000, dtype=np.int64)
    counts[:: CS_MAX_PTS + 100] = 50  # five observed points per chunk, CS_MAX_PTS + 100 unobserved ones between two of them
    t = _tables(lib, counts, 8, rng)
    assert not t["has_fragments"] and t["chunk_pts"][:, 1].max() > CS_MAX_PTS and _cs(lib, t, 52, 2048)["n_sc"] == 0
    counts[:: CS_MAX_PTS + 100] = CHUNK  # one point per chunk: every range is a single point again
    t = _tables(lib, counts, 8, rng)
    assert t["chunk_pts"][:, 1].max() == 1 and _cs(lib, t, 52, 2048)["n_sc"] > 0


# ---- constraint rows -------------------------------------------------------------------------------------------------------------------
def _con(lib, P, ncp, ga, gb, dist, wgt, pt_start=None, lds_points=CON_LDS_POINTS):
    n = len(dist)
    ga, gb = np.ascontiguousarray(ga, dtype=np.int32), np.ascontiguousarray(gb, dtype=np.int32)
    if pt_start is None:
        pt_start = np.arange(P + 1)
    pt_start = np.ascontiguousarray(pt_start, dtype=np.int32)
    i32 = lambda k: np.zeros(k, dtype=np.int32)  # noqa: E731
    o = dict(pt=i32(8 * n), lp=i32(8 * n), order=i32(n), comp_con=i32(n + 1), comp_pt=i32(n + 1), comp_pts=i32(8 * n), comp_m=np.zeros(n + 1, dtype=np.int64),
             dist=np.zeros(n), wgt=np.zeros(n), orphan=i32(8 * n))
    scal = np.zeros(6, dtype=np.int64)
    rc = lib.sp_constraint_plan(P, ncp, n, _p(ga, I32P), _p(gb, I32P), _p(np.ascontiguousarray(dist, dtype=np.float64), F64P), _p(np.ascontiguousarray(wgt, dtype=np.float64), F64P),
                                lds_points, _p(pt_start, I32P), *(_p(o[k], I32P) for k in ("pt", "lp", "order", "comp_con", "comp_pt", "comp_pts")), _p(o["comp_m"], I64P),
                                _p(o["dist"], F64P), _p(o["wgt"], F64P), _p(o["orphan"], I32P), _p(scal, I64P))
    if rc:
        return rc, lib.sp_last_error().decode()
    K, n_pts, n_orphan = int(scal[0]), int(scal[4]), int(scal[5])
    o.update(K=K, max_m=int(scal[1]), max_pts=int(scal[2]), big=bool(scal[3]), pt=o["pt"].reshape(n, 8), lp=o["lp"].reshape(n, 8), comp_con=o["comp_con"][: K + 1],
             comp_pt=o["comp_pt"][: K + 1], comp_m=o["comp_m"][: K + 1], comp_pts=o["comp_pts"][:n_pts], orphan=o["orphan"][:n_orphan])
    return o


@pytest.mark.parametrize("seed,P,n_con,spread", [(0, 400, 120, 12), (1, 5000, 800, 40), (2, 60, 200, 60), (3, 3000, 40, 3000)])
def test_constraint_rows_are_grouped_by_connected_component(lib, seed, P, n_con, spread):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, P - spread + 1, size=n_con)  # rows of points near `base`: components of several rows, several components
    slots = (base[:, None] + rng.integers(0, spread, size=(n_con, 8))).astype(np.int32)
    slots[::5, 3] = slots[::5, 0]  # a point twice in a group ...
    slots[::7, 6] = slots[::7, 1]  # ... and in both groups of a row
    ga, gb = slots[:, :4], slots[:, 4:]
    dist, wgt = rng.random(n_con) + 0.5, rng.random(n_con) + 1.0
    counts = rng.integers(0, 3, size=P)  # a third of the points unobserved
    pt_start = np.concatenate([[0], np.cumsum(counts)])
    o = _con(lib, P, 24, ga, gb, dist, wgt, pt_start, lds_points=20)
    # the partition: components of the graph "points of a row are connected"
    rows = np.repeat(np.arange(n_con), 8)
    graph = coo_matrix((np.ones(8 * n_con), (slots[rows, 0], slots.ravel())), shape=(P, P))
    _, label = connected_components(graph, directed=False)
    row_label = label[slots[:, 0]]
    K = len(np.unique(row_label))
    assert o["K"] == K
    comp_of_row = np.repeat(np.arange(K), np.diff(o["comp_con"]))  # of the rows in the order here
    order = o["order"]
    assert np.array_equal(np.sort(order), np.arange(n_con))
    for k in range(K):
        mine = order[comp_of_row == k]
        assert len(set(row_label[mine])) == 1 and len(mine) == int((row_label == row_label[mine[0]]).sum())  # one component, all of it
        assert np.all(np.diff(mine) > 0)  # the caller's order inside a component
    assert np.all(np.diff(order[o["comp_con"][:-1]]) > 0)  # components in the order of their first row
    # rows carry their data along
    assert np.array_equal(o["pt"], slots[order]) and np.array_equal(o["dist"], dist[order]) and np.array_equal(o["wgt"], wgt[order])
    # local numbering: every point of a component once, in the order the rows name it
    m = np.diff(o["comp_con"])
    for k in range(K):
        pts = o["comp_pts"][o["comp_pt"][k] : o["comp_pt"][k + 1]]
        rows_k = slice(o["comp_con"][k], o["comp_con"][k + 1])
        named = o["pt"][rows_k].ravel()
        _, first_seen = np.unique(named, return_index=True)
        assert np.array_equal(pts, named[np.sort(first_seen)])
        assert np.array_equal(pts[o["lp"][rows_k]], o["pt"][rows_k])
    assert np.array_equal(o["comp_m"], np.concatenate([[0], np.cumsum(m.astype(np.int64) ** 2)]))
    n_pts = np.diff(o["comp_pt"])
    assert o["max_m"] == m.max() and o["max_pts"] == n_pts.max() and o["big"] == (n_pts.max() > 20)
    for lds_points in (int(n_pts.max()) - 1, int(n_pts.max())):  # global scratch only when a component's points exceed the LDS copy
        assert _con(lib, P, 24, ga, gb, dist, wgt, pt_start, lds_points=lds_points)["big"] == (lds_points < n_pts.max())
    # orphans: constrained points nobody observes, in the order of comp_pts
    assert np.array_equal(o["orphan"], o["comp_pts"][counts[o["comp_pts"]] == 0]) and len(o["orphan"]) > 0


def test_constraint_limits_and_indices(lib):
    ones = lambda n: np.ones(n)  # noqa: E731
    chain = lambda n: (np.tile(np.arange(4, dtype=np.int32), (n, 1)), np.tile(np.arange(4, 8, dtype=np.int32), (n, 1)))  # noqa: E731  (n rows, one component)
    m = 1 << 14  # sum of m^2 = 2^28: the last that fits
    o = _con(lib, 8, 24, *chain(m), ones(m), ones(m))
    assert o["K"] == 1 and o["comp_m"][-1] == 1 << 28 and o["max_m"] == m and o["max_pts"] == 8
    rc, msg = _con(lib, 8, 24, *chain(m + 1), ones(m + 1), ones(m + 1))
    assert rc == ERR_UNSUPPORTED and f"sum of m^2 = {(m + 1) ** 2}" in msg and "the limits are 2 GB and 4 GB" in msg
    ncp = (1 << 28) - 1  # 2 rows x (ncp + 1) = 2^29 doubles of camera coupling: the last that fits
    assert _con(lib, 8, ncp, *chain(2), ones(2), ones(2))["K"] == 1
    rc, msg = _con(lib, 8, ncp + 1, *chain(2), ones(2), ones(2))
    assert rc == ERR_UNSUPPORTED and f"(2 rows x {ncp + 1} camera parameters)" in msg
    ga, gb = chain(3)
    for bad in (-1, 8):
        gb[2, 1] = bad
        assert _con(lib, 8, 24, ga, gb, ones(3), ones(3)) == (ERR_INVALID, "cba_set_constraints: point index out of range in constraint 2")


# ---- mapped host mailbox ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncp", [6, 24, 36, 96, 2043, 4095])
def test_mailbox_layout(lib, ncp):
    out = np.zeros(6, dtype=np.int64)
    lib.sp_mail_layout(ncp, _p(out, I64P))
    cam, flags, bcam, total, scalars, seq = (int(v) for v in out)
    # what cba_create spelled out: scalars (64 doubles) | three camera blocks + sequence (3 ncp + 8) | flags (4 ints) | four camera blocks
    assert (cam, flags, bcam, total) == (64, 64 + (3 * ncp + 8), 64 + (3 * ncp + 8) + 2, 64 + (3 * ncp + 8) + 2 + 4 * ncp)
    regions = [(0, scalars), (cam, cam + 3 * ncp + 8), (flags, flags + 4 * 4 // 8), (bcam, bcam + 4 * ncp)]
    assert all(a[1] <= b[0] for a, b in zip(regions, regions[1:])) and regions[-1][1] == total
    # the kernels write the sequence word of a packet to slot 63 of the scalar block
    assert seq == 63 < scalars and len(re.findall(r"host_scal\)\[63\] = (?:pub\.)?seq;", _KERNELS)) == 2


# ---- problem description, through the CPU build of the ABI ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_lib():
    return compile_native(NATIVE / "cpu_library.cpp", CSRC / "cba_solve.cpp", flags=("-pthread",), include=(INCLUDE,))


def test_every_rejection_of_a_problem_description(cpu_lib):
    body = """
        import ctypes as C, json
        import numpy as np
        from caliscope_amd import _lib
        lib = _lib.load()
        def attempt(**change):
            n_cams, n_points = 3, 5
            a = dict(cam_n_params=np.full(n_cams, 6, dtype=np.int32), cam_model=np.zeros(n_cams, dtype=np.int32), cam_const=np.tile(np.r_[800.0, 800.0, 320.0, 240.0, np.zeros(8)], n_cams),
                     obs_cam=np.tile(np.arange(n_cams, dtype=np.int32), n_points), obs_pt=np.repeat(np.arange(n_points, dtype=np.int32), n_cams),
                     obs_uv=np.zeros(2 * n_cams * n_points))
            s = dict(n_cams=n_cams, n_points=n_points, n_obs=n_cams * n_points, loss=0, f_scale=1.0)
            for key, value in change.items():
                if key in s: s[key] = value
                elif value is None: a[key] = None
                else: a[key][value[0]] = value[1]
            ptr = lambda k, t: a[k].ctypes.data_as(t) if a[k] is not None else t()
            d = _lib.ProblemDesc(s["n_cams"], s["n_points"], s["n_obs"], ptr("cam_n_params", _lib.c_int32_p), ptr("cam_model", _lib.c_int32_p), ptr("cam_const", _lib.c_double_p),
                                 ptr("obs_cam", _lib.c_int32_p), ptr("obs_pt", _lib.c_int32_p), ptr("obs_uv", _lib.c_double_p), s["loss"], s["f_scale"])
            handle = C.c_void_p()
            rc = lib.cba_create(C.byref(d), None, C.byref(handle))
            msg = _lib.last_error(lib) if rc else ""
            if handle: lib.cba_destroy(handle)
            return [rc, msg, bool(handle)]
        cases = dict(valid=dict(), no_cams=dict(n_cams=0), no_points=dict(n_points=0), no_obs=dict(n_obs=0), too_many=dict(n_obs=1 << 31), huber=dict(loss=1, f_scale=2.0),
                     null_uv=dict(obs_uv=None), null_model=dict(cam_model=None), loss_low=dict(loss=-1), loss_high=dict(loss=5), f_scale=dict(loss=1, f_scale=0.0),
                     f_scale_nan=dict(loss=3, f_scale=float("nan")), linear_ignores_f_scale=dict(f_scale=0.0), n_params=dict(cam_n_params=(1, 7)), model=dict(cam_model=(2, 5)),
                     free_fisheye=dict(cam_model=(1, 1), cam_n_params=(1, 9)), locked_fisheye=dict(cam_model=(1, 1)), fx=dict(cam_const=(24, 0.0)), fx_nan=dict(cam_const=(12, float("nan"))))
        print(json.dumps({name: attempt(**change) for name, change in cases.items()}))
    """
    env = dict(os.environ, CALISCOPE_BA_LIB=str(cpu_lib), PYTHONPATH=str(ROOT))
    proc = subprocess.run([sys.executable, "-c", textwrap.dedent(body)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stderr[-3000:]
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    for name in ("valid", "huber", "linear_ignores_f_scale", "locked_fisheye"):
        assert got.pop(name) == [0, "", True], name
    expected = dict(
        no_cams=(ERR_INVALID, "cba_create: empty problem (cams=0 points=5 obs=15)"), no_points=(ERR_INVALID, "cba_create: empty problem (cams=3 points=0 obs=15)"),
        no_obs=(ERR_INVALID, "cba_create: empty problem (cams=3 points=5 obs=0)"), too_many=(ERR_UNSUPPORTED, "cba_create: more than 2^31 observations"),
        null_uv=(ERR_INVALID, "cba_create: null array"), null_model=(ERR_INVALID, "cba_create: null array"), loss_low=(ERR_INVALID, "cba_create: unknown loss -1"),
        loss_high=(ERR_INVALID, "cba_create: unknown loss 5"), f_scale=(ERR_INVALID, "cba_create: f_scale must be positive"),
        f_scale_nan=(ERR_INVALID, "cba_create: f_scale must be positive"), n_params=(ERR_INVALID, "camera 1: n_params must be 6 or 9, got 7"),
        model=(ERR_INVALID, "camera 2: unknown model 5"), free_fisheye=(ERR_INVALID, "camera 1: fisheye cameras are always locked (6 params)"),
        fx=(ERR_INVALID, "camera 2: fx_initial must be positive"), fx_nan=(ERR_INVALID, "camera 1: fx_initial must be positive"))
    assert set(got) == set(expected)
    for name, (code, message) in expected.items():
        assert got[name] == [code, message, False], name
