"""The LDS layouts and the kernel routes of the bundle-adjustment engine (csrc/kernel_plan.h: what a kernel's carve-up of its dynamic LDS, the byte
count of its launch and the choices of cba_create share) on the CPU: compiled by g++ behind tests/native/kernel_plan_harness.cpp and checked
against Python restatements of the host formulas and of the route rules the library had before they moved into that header."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.native_build import NATIVE, load_native

I32P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_long)
KIB = 1024
ROW = 8
COST, BUILD, BUILD_CS, JV, TPREP, BACKSUB, BACKSUB_REC, SMALL_SOLVE = range(8)
CAMG, DET, UGLOB = 1, 2, 4
CAMERAS = {6: np.arange(1, 1101, dtype=np.int32), 9: np.arange(1, 501, dtype=np.int32)}  # past every threshold, the 160 KiB refusal included
PMAX, NVS = (1, 256, 512), (1, 2)

# ---- the constants the formulas are written with (cba_kernels.h / kernel_plan.h) -------------------------------------------------------
CHUNK, WAVE, BLOCK, NB = 256, 64, 256, 32
CAMTAB_LDS = 37
DET_PARK = 9 * (CHUNK + 1)  # DET_ROUND * DET_LD
STRIDE = {6: 27, 9: 54}  # UPack<NC>::STRIDE
STAGE = {6: 4 * WAVE * 5 * 2, 9: 2 * WAVE * 11 * 2}  # SchurRec<NC>::STAGE_WAVES * WAVE * STAGE * 2, doubles
BSR_NP, BSR_CSS = {6: 5, 9: 11}, {6: 8, 9: 9}
SMALL_N = 96


def ncp_pad_of(cams, nc):
    """camera_layout's rule (host_plan.h), every camera with nc parameters"""
    return ((cams * nc + 31) // 32 * 32).astype(np.int32)


@pytest.fixture(scope="module")
def lib():
    lib = load_native(NATIVE / "kernel_plan_harness.cpp")
    lib.kp_layout.restype = C.c_int
    lib.kp_layout.argtypes = [C.c_int, C.c_int, C.c_int, I32P, I32P, C.c_int, C.c_int, C.c_int, I64P, I64P]
    lib.kp_single.restype = None
    lib.kp_single.argtypes = [C.c_int, C.c_int, I64P]
    lib.kp_routes.restype = None
    lib.kp_routes.argtypes = [C.c_int, I32P, C.c_int, I32P] + [C.c_int] * 9 + [I32P, I64P]
    lib.kp_refusal.restype = C.c_int
    lib.kp_refusal.argtypes = [C.c_long, C.c_char_p, C.c_int]
    return lib


def _layout(lib, family, nc, cams, pmax=0, nv=0, flags=0):
    """(boundaries [n][k] in bytes, bytes() [n]) of one family at every camera count"""
    pad = ncp_pad_of(cams, nc)
    out, nbytes = np.zeros((len(cams), ROW), dtype=np.int64), np.zeros(len(cams), dtype=np.int64)
    k = lib.kp_layout(family, nc, len(cams), cams.ctypes.data_as(I32P), pad.ctypes.data_as(I32P), pmax, nv, flags, out.ctypes.data_as(I64P), nbytes.ctypes.data_as(I64P))
    assert 2 <= k <= ROW
    return out[:, :k], nbytes


# ---- the host formulas as cba_lib.hip had them (lds_cost, lds_build*, lds_jv, lds_tprep, lds_backsub, BsrCfg::lds_bytes, kSmallSolveLds) -----------
def _tab(cams, tab_global):
    return np.where(tab_global, 0, cams.astype(np.int64) * CAMTAB_LDS)


def lds_cost(cams, tab_global):
    return (_tab(cams, tab_global) + 8) * 8


def lds_build_camg(cams, nc):
    return (cams.astype(np.int64) * STRIDE[nc] + 9 * CHUNK + 8) * 8


def lds_build_with_tab(cams, nc):
    return (cams.astype(np.int64) * CAMTAB_LDS + cams.astype(np.int64) * STRIDE[nc] + 9 * CHUNK + 8) * 8


def lds_build_det(cams):
    return (cams.astype(np.int64) * CAMTAB_LDS + DET_PARK + 9 * CHUNK + 8) * 8 + (CHUNK + cams.astype(np.int64) + 1) * 4


def lds_build_cs(cams, nc, pmax, camg, uglob):
    c = cams.astype(np.int64)
    return ((0 if camg else c * CAMTAB_LDS) + (0 if uglob else c * STRIDE[nc]) + 12 * pmax + 8) * 8


def lds_jv(cams, pad, nv, tab_global):
    return (_tab(cams, tab_global) + nv * pad.astype(np.int64) + 8) * 8


def lds_tprep(cams, nc, pad, det, tab_global):
    if det:
        return (STAGE[nc] + cams.astype(np.int64) * CAMTAB_LDS + DET_PARK) * 8 + (CHUNK + cams.astype(np.int64) + 1) * 4
    return (STAGE[nc] + _tab(cams, tab_global) + pad.astype(np.int64)) * 8


def lds_backsub(cams, pad, tab_global):
    return (_tab(cams, tab_global) + pad.astype(np.int64) + 3 * CHUNK) * 8


def lds_backsub_rec(cams, nc):
    return (BLOCK * BSR_NP[nc] * 2 + 2 * 3 * CHUNK + cams.astype(np.int64) * BSR_CSS[nc] + 8) * 8


SMALL_SOLVE_LDS = ((SMALL_N + 1) * (SMALL_N + 1) + 2 * NB * (NB + 1) + ((SMALL_N + NB - 1) // NB) * NB * (NB + 1) + 2 * SMALL_N) * 8


def _cases(nc):
    """(family, pmax, nv, flags, bytes the parent's host formula gives, bytes of every region as its kernel uses them) over CAMERAS[nc]"""
    cams = CAMERAS[nc]
    c, pad = cams.astype(np.int64), ncp_pad_of(cams, nc).astype(np.int64)
    zero, red = 0 * c, 0 * c + 64
    for camg in (False, True):
        tab = zero if camg else c * CAMTAB_LDS * 8
        f = CAMG if camg else 0
        yield COST, 0, 0, f, lds_cost(cams, camg), [tab, red]
        yield BUILD, 0, 0, f, lds_build_camg(cams, nc) if camg else lds_build_with_tab(cams, nc), [tab, c * STRIDE[nc] * 8, zero + 9 * CHUNK * 8, red]
        for nv in NVS:
            yield JV, 0, nv, f, lds_jv(cams, pad, nv, camg), [tab, nv * pad * 8, red]
        yield TPREP, 0, 0, f, lds_tprep(cams, nc, pad, False, camg), [zero + STAGE[nc] * 8, tab, pad * 8]
        yield BACKSUB, 0, 0, f, lds_backsub(cams, pad, camg), [tab, pad * 8, zero + 3 * CHUNK * 8]
        for pmax in PMAX:
            for uglob in ((False, True) if camg else (False,)):  # (UGLOB implies CAMG: k_build_cs's static_assert)
                yield (BUILD_CS, pmax, 0, f | (UGLOB if uglob else 0), lds_build_cs(cams, nc, pmax, camg, uglob),
                       [tab, zero if uglob else c * STRIDE[nc] * 8, zero + 9 * pmax * 8, zero + 3 * pmax * 8, red])
    # the fixed-order forms keep the table in LDS; their int tables lie behind the doubles
    tab = c * CAMTAB_LDS * 8
    ints = [zero, zero + CHUNK * 4, (c + 1) * 4]
    yield BUILD, 0, 0, DET, lds_build_det(cams), [tab, zero + DET_PARK * 8, zero + 9 * CHUNK * 8, red] + ints
    yield TPREP, 0, 0, DET, lds_tprep(cams, nc, pad, True, False), [zero + STAGE[nc] * 8, tab, zero + DET_PARK * 8] + ints
    yield BACKSUB_REC, 0, 0, 0, lds_backsub_rec(cams, nc), [zero + BLOCK * BSR_NP[nc] * 16, zero + 2 * 3 * CHUNK * 8, c * BSR_CSS[nc] * 8, red]
    yield (SMALL_SOLVE, 0, 0, 0, zero + SMALL_SOLVE_LDS,
           [zero + (SMALL_N + 1) * (SMALL_N + 1) * 8, zero + 2 * NB * (NB + 1) * 8, zero + 3 * NB * (NB + 1) * 8, zero + SMALL_N * 8, zero + SMALL_N * 4, zero + SMALL_N * 4])


@pytest.mark.parametrize("nc", [6, 9])
def test_bytes_equal_the_host_formulas(lib, nc):
    """bytes() of every layout, for every flag combination of its family, at every camera count: exactly what the host formula gave."""
    n = 0
    for family, pmax, nv, flags, want, _ in _cases(nc):
        _, got = _layout(lib, family, nc, CAMERAS[nc], pmax, nv, flags)
        np.testing.assert_array_equal(got, want, err_msg=f"family {family} pmax {pmax} nv {nv} flags {flags}")
        n += 1
    assert n == 2 * (1 + 1 + 2 + 1 + 1) + 3 * 3 + 4


def test_single_region_kernels(lib):
    out = np.zeros(4, dtype=np.int64)
    for a, b in [(1, 1), (54, 7), (96, 64), (6600, 256), (9000, 1)]:
        lib.kp_single(a, b, out.ctypes.data_as(I64P))
        assert out.tolist() == [a * 3 * 8 + a * 4, a * 8, a * 8, (9 * a + 2 * b) * 8]


@pytest.mark.parametrize("nc", [6, 9])
def test_regions_tile_the_allocation(lib, nc):
    """Offsets ascend from 0, every region is as large as its kernel uses it (so none overlaps the next), the last ends at bytes(); what a kernel
    reads as double2 — k_tprep's record stage, k_backsub_rec's record buffer — starts on 16 bytes."""
    for family, pmax, nv, flags, want, sizes in _cases(nc):
        bounds, nbytes = _layout(lib, family, nc, CAMERAS[nc], pmax, nv, flags)
        what = f"family {family} pmax {pmax} nv {nv} flags {flags}"
        assert bounds.shape[1] == len(sizes) + 1, what
        assert (bounds[:, 0] == 0).all() and (np.diff(bounds, axis=1) >= 0).all(), what
        np.testing.assert_array_equal(np.diff(bounds, axis=1), np.stack(sizes, axis=1), err_msg=what)
        np.testing.assert_array_equal(bounds[:, -1], nbytes, err_msg=what)
        assert (bounds % 4 == 0).all(), what
        if family in (TPREP, BACKSUB_REC):
            assert (bounds[:, 0] % 16 == 0).all(), what


# ---- routes: the rules of configure_kernels, build_camg, build_cs_camg, build_cs_uglob and cba_get_info as cba_lib.hip had them ----------------
def parent_routes(nc, cams, det, n_heavy, n_sc, pmax, eval_only, fragments, sw_tab, sw_camg, sw_rec):
    """(tab_global, cs, point-ordered camg, cs camg, cs uglob, backsub_rec, cba_info's camg bit, first byte count over 160 KiB or 0), arrays over cams.
    A switch is -1 (not set), 0 or 1."""
    pad = ncp_pad_of(cams, nc)
    no, yes = np.zeros(len(cams), dtype=bool), np.ones(len(cams), dtype=bool)
    worst = np.maximum(np.maximum(lds_jv(cams, pad, 2, no), lds_backsub(cams, pad, no)), lds_tprep(cams, nc, pad, det, no))
    tab_global = (worst > 150 * KIB) & (not det)
    if sw_tab >= 0:
        tab_global = yes & (sw_tab != 0 and not det)
    with_tab = lds_build_with_tab(cams, nc)
    if sw_camg >= 0:
        rule = yes & (sw_camg != 0 and not det)
    else:
        rule = (((with_tab > 80 * KIB) & (lds_build_camg(cams, nc) <= 80 * KIB)) | (with_tab > 160 * KIB)) & (not det)
    pt_camg = tab_global | rule
    lds_build = np.where(pt_camg, lds_build_camg(cams, nc), lds_build_det(cams) if det else with_tab)
    use_cs = bool(n_sc) and not det and not n_heavy
    uglob = lds_build_cs(cams, nc, pmax, True, False) > 160 * KIB
    cs_camg = tab_global | (lds_build_cs(cams, nc, pmax, False, False) > 80 * KIB)
    rec = yes & ((nc == 6 or sw_rec == 1) and not eval_only and not fragments and sw_rec != 0) & (lds_backsub_rec(cams, nc) <= 150 * KIB)
    # allow_lds in the order of configure_kernels: the first request over 160 KiB is the one reported
    asked = [lds_cost(cams, tab_global)]
    if use_cs:
        asked.append(np.where(uglob, lds_build_cs(cams, nc, pmax, True, True), np.where(cs_camg, lds_build_cs(cams, nc, pmax, True, False), lds_build_cs(cams, nc, pmax, False, False))))
    asked.append(np.where(uglob, 0, lds_build) if use_cs else lds_build)
    if det:
        asked.append(lds_tprep(cams, nc, pad, True, no))
    asked += [lds_jv(cams, pad, 1, tab_global), lds_jv(cams, pad, 2, tab_global), lds_tprep(cams, nc, pad, det, tab_global), lds_backsub(cams, pad, tab_global)]
    refused = np.zeros(len(cams), dtype=np.int64)
    for a in asked:
        refused = np.where((refused == 0) & (a > 160 * KIB), a, refused)
    cs = yes & use_cs
    return tab_global, cs, pt_camg, cs & cs_camg, cs & uglob, rec, np.where(cs, cs_camg, pt_camg), refused


def _routes(lib, nc, cams, det, n_heavy, n_sc, pmax, eval_only, fragments, sw_tab, sw_camg, sw_rec):
    pad = ncp_pad_of(cams, nc)
    bits, refused = np.zeros(len(cams), dtype=np.int32), np.zeros(len(cams), dtype=np.int64)
    lib.kp_routes(len(cams), cams.ctypes.data_as(I32P), nc, pad.ctypes.data_as(I32P), 3 if det else 0, n_heavy, n_sc, pmax, int(eval_only), int(fragments), sw_tab, sw_camg,
                  sw_rec, bits.ctypes.data_as(I32P), refused.ctypes.data_as(I64P))
    return [(bits & (1 << k)) != 0 for k in range(7)], refused


CS_PLANS = [(0, 0)] + [(5, pmax) for pmax in PMAX]  # (n_sc, pmax): no camera-sorted plan, or one


@pytest.mark.parametrize("nc", [6, 9])
def test_routes_equal_the_parent_rules(lib, nc):
    """KernelRoutes at every camera count, crossed with the fixed-order mode, heavy points, fragments, evaluation-only, the camera-sorted plan and each
    value of the three switches: the routes, cba_info's bits and the refusal are what the rules gave when they stood in cba_lib.hip."""
    cams = CAMERAS[nc]
    for det, n_heavy, eval_only, fragments, (n_sc, pmax) in itertools.product((False, True), (0, 3), (False, True), (False, True), CS_PLANS):
        for sw in itertools.product((-1, 0, 1), repeat=3):
            args = (nc, cams, det, n_heavy, n_sc, pmax, eval_only, fragments, *sw)
            want = parent_routes(*args)
            got, refused = _routes(lib, *args)
            for k, name in enumerate(("tab_global", "build_cs", "build_pt_camg", "build_cs_camg", "build_uglob", "backsub_rec", "build_camg()")):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} at {args[2:]}")
            np.testing.assert_array_equal(refused, want[7], err_msg=f"refusal at {args[2:]}")


def test_route_flips_and_the_counts_other_tests_name(lib):
    """Where each route flips with no switch set (printed), and the counts that tests/test_gpu_parity.py::test_limits_are_reported_not_crashed and
    the comments name: 320 six-parameter cameras take the vector-cache table, 800 the global accumulators; beyond, the 160 KiB refusal."""
    names = ("tab_global", "build_cs", "build_pt_camg", "build_cs_camg", "build_uglob", "backsub_rec", "build_camg()")
    for nc in (6, 9):
        cams = CAMERAS[nc]
        for n_sc, pmax in CS_PLANS:
            got, refused = _routes(lib, nc, cams, False, 0, n_sc, pmax, False, False, -1, -1, -1)
            flips = {name: cams[1:][got[k][1:] != got[k][:-1]].tolist() for k, name in enumerate(names)}
            first_refused = int(cams[refused != 0][0]) if (refused != 0).any() else None
            print(f"nc {nc} n_sc {n_sc} pmax {pmax}: flips at {flips}, refused from {first_refused}")
            if nc == 6:
                at = lambda k, n: bool(got[k][n - 1])  # noqa: E731
                assert at(6, 320), "320 six-parameter cameras read the camera table through the vector cache in the build"
                assert at(0, 800) and (not n_sc or at(4, 800)), "800 six-parameter cameras: global table, and the global accumulators of k_build_cs"
                assert not n_sc or refused[800 - 1] == 0
    # the point-ordered build keeps the accumulators in LDS: 800 six-parameter cameras are refused there, with the message callers match
    _, refused = _routes(lib, 6, CAMERAS[6], False, 0, 0, 0, False, False, -1, -1, -1)
    assert refused[800 - 1] == lds_build_camg(CAMERAS[6], 6)[800 - 1] > 160 * KIB
    buf = C.create_string_buffer(128)
    lib.kp_refusal(int(refused[800 - 1]), buf, len(buf))
    assert "bytes of LDS (> 160 KiB)" in buf.value.decode() and str(int(refused[800 - 1])) in buf.value.decode()
