"""tan_portable, undistort_one and sym4_null_vector (csrc/ba_math.h) and the loop of k_triangulate, built by g++
(tests/triangulation_native.py), against the 60-digit fixture of tests/golden/make_triangulation_edge_fixtures.py and the oracle.

Limits.  Two are derived (a third, for tan_portable beyond pi / 2, in the docstring of its test):

* tan_portable: relative error <= 4 * 2^-52 * (1 + 1 / cos x).  tan x = 2 s c / (c^2 - s^2) with s, c of x / 2: the difference
  c^2 - s^2 = cos x cancels, so the roundings of c^2 and s^2 (2^-53 each, of numbers below 1) come back divided by cos x; the 4
  covers the few ulp of the two series.
* the DLT: max |xyz - exact| <= 4 * 2^-52 * l4 / (l2 - l1) * (1 + |X|^2), l1 <= .. <= l4 the eigenvalues of A^T A and X the exact
  point, both from the fixture (triangulation_native.dlt_bound has the derivation).

One is measured: the fisheye inverse against the fixture's root.  The reference that was measured is the oracle
(oracle.triangulation.undistort_fisheye in float64: the same Newton iteration with the maths library's tan) on the fixture's inputs:
its worst relative error of the scale tan(theta) / theta_d is 1.369e-14 (61.6 * 2^-52, at the coefficient set whose root for
theta_d = 1.55 lies 0.01 below pi / 2, where tan multiplies an error of theta by 170).  The limit is 4 times that, 5.476e-14: the two
differ only in tan.  test_fisheye_inverse_against_the_fixture measures the oracle again and holds it to the recorded figure.

One more is reasoned in the docstring of its test: the residual of the fisheye root on a dense sweep of theta_d.

The other figures are the oracle comparisons the suite already had (1e-12 for the same algorithm in the same order, 1e-10 for the
round trip of tests/test_triangulation.py) and the ones the issue states."""
import ctypes as C

import numpy as np
import pytest

from caliscope_amd.synthetic import WEBCAM_DIST, WEBCAM_FOCAL
from oracle import triangulation as otri
from oracle.camera_model import project_fisheye, project_pinhole
from tests import triangulation_native as T
from tests.native_build import NATIVE, load_native

K = np.array([[WEBCAM_FOCAL, 0.0, 960.0], [0.0, WEBCAM_FOCAL, 540.0], [0.0, 0.0, 1.0]])
UNIT = np.eye(3)
ORACLE_FISHEYE_WORST = 1.369e-14
FISHEYE_LIMIT = 4.0 * ORACLE_FISHEYE_WORST
RECORDING_FISHEYE = np.array([0.05, -0.02, 0.004, 0.001])


# ---- tan_portable ------------------------------------------------------------------------------------------------------------------------
def test_tan_portable_error_bound():
    fx = T.fixture()
    x, ref = fx["tan_x"], fx["tan_ref"]
    assert len(x) == 2013 and np.array_equal(x[:2001], np.linspace(0.0, 1.5, 2001)) and np.array_equal(x[2001:], np.pi / 2 - 10.0 ** -np.arange(1.0, 13.0))
    got = T.tan_portable(x)
    rel = np.abs(got - ref) / np.where(ref == 0.0, 1.0, ref)
    bound = 4.0 * T.EPS * (1.0 + 1.0 / np.cos(x))
    print(f"tan_portable: worst error / bound {np.max(rel / bound):.3f}; on [0, 1.5] {np.max(rel[:2001]) / T.EPS:.1f} ulp")
    assert np.all(rel <= bound), (x[rel > bound], (rel / bound).max())


def test_tan_portable_beyond_half_pi():
    """x leaves [-pi/2, pi/2] when undistort_one's Newton iteration does: the nearest multiple of pi comes off first.  The reduced
    argument r carries the roundings of the two subtractions, at most 2^-52 * pi/2 in all for these k <= 13 (k * 1.2e-10 * 2^-53 and
    the 7e-27 of the two-part pi are far below), and tan turns an error d of r into the relative error d / (sin r cos r)."""
    fx = T.fixture()
    x, ref = fx["tan_wide_x"], fx["tan_wide_ref"]
    assert len(x) == 400 and x.min() == 1.6 and x.max() == 40.0 and (ref < 0).sum() > 100 < (ref > 0).sum()
    rel = np.abs(T.tan_portable(x) - ref) / np.abs(ref)
    bound = 4.0 * T.EPS * (1.0 + 1.0 / np.abs(np.cos(x))) + T.EPS * (np.pi / 2) / np.abs(np.sin(x) * np.cos(x))
    print(f"tan_portable on [1.6, 40]: worst error / bound {np.max(rel / bound):.3f}")
    assert np.all(rel <= bound), x[rel > bound]
    assert np.array_equal(T.tan_portable(-x), -T.tan_portable(x))


def test_tan_portable_special_values():
    at_half_pi, at_zero = T.tan_portable([np.pi / 2, 0.0])
    assert np.isfinite(at_half_pi) and at_half_pi >= 1e15
    assert at_zero == 0.0 and not np.signbit(at_zero)
    assert np.array_equal(T.tan_portable([-0.3, -1.2]), -T.tan_portable([0.3, 1.2]))  # odd, to the bit


# ---- undistort_one, pinhole --------------------------------------------------------------------------------------------------------------
CORNERS = np.array([[0.0, 0.0], [1919.0, 0.0], [0.0, 1079.0], [1919.0, 1079.0], [960.0, 0.0], [0.0, 540.0], [1500.3, 900.7], [961.0, 540.0]])
PINHOLE_CASES = {
    "webcam": np.array(WEBCAM_DIST),
    "k3": np.array([0.05, -0.02, 0.0, 0.0, 0.08]),
    "tangential": np.array([0.0, 0.0, 0.004, -0.003, 0.0]),
    "zero": np.zeros(5),
}


@pytest.mark.parametrize("case", list(PINHOLE_CASES))
def test_pinhole_matches_the_oracle(case):
    dist = PINHOLE_CASES[case]
    got = T.undistort(CORNERS, K, dist, False)
    want = otri.undistort_pinhole(CORNERS, K, dist, float32_io=False)
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-12
    assert np.abs(got).max() > 0.65  # the corners are corners


@pytest.mark.parametrize("case", list(PINHOLE_CASES))
def test_pinhole_principal_point_is_exactly_zero(case):
    got = T.undistort([[960.0, 540.0]], K, PINHOLE_CASES[case], False)
    assert np.array_equal(got, np.zeros((1, 2)))


def test_pinhole_without_distortion_is_the_plain_quotient():
    got = T.undistort(CORNERS, K, np.zeros(5), False)
    want = np.c_[(CORNERS[:, 0] - 960.0) / WEBCAM_FOCAL, (CORNERS[:, 1] - 540.0) / WEBCAM_FOCAL]
    assert np.array_equal(T.bits(got), T.bits(want))


def _board_pixels(project, dist):
    i = np.arange(300)
    X = np.c_[0.5 * np.sin(1.7 * i), 0.3 * np.cos(2.3 * i + 0.4), 3.0 + np.sin(0.9 * i)]
    return project(X, np.zeros(3), np.zeros(3), K, dist)[0], X[:, :2] / X[:, 2:]


@pytest.mark.parametrize("case", ["webcam", "k3", "tangential"])
def test_pinhole_round_trip(case):
    uv, normalised = _board_pixels(project_pinhole, PINHOLE_CASES[case])
    assert np.abs(T.undistort(uv, K, PINHOLE_CASES[case], False) - normalised).max() < 1e-10


@pytest.mark.parametrize("fisheye,dist", [(False, np.array(WEBCAM_DIST)), (True, T.FISHEYE_DIST)])
def test_float32_io_rounds_input_and_output(fisheye, dist):
    uv, _ = _board_pixels(project_fisheye if fisheye else project_pinhole, dist)
    uv = np.vstack([uv, CORNERS])
    got = T.undistort(uv, K, dist, fisheye, float32_io=True)
    want = otri.undistort_points(uv, K, dist, fisheye, float32_io=True)
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    assert not np.array_equal(got, T.undistort(uv, K, dist, fisheye, float32_io=False))
    # the input is rounded too: the pixels and their float32 roundings give the same bits
    rounded = uv.astype(np.float32).astype(np.float64)
    assert not np.array_equal(rounded, uv)
    assert np.array_equal(T.bits(got), T.bits(T.undistort(rounded, K, dist, fisheye, float32_io=True)))


# ---- undistort_one, fisheye --------------------------------------------------------------------------------------------------------------
def _scales(undistort, coeffs, theta_d):
    """x / x0 of the points (theta_d, 0) through a camera with unit intrinsics: theta_d arrives exactly (sqrt(t * t) == t)."""
    theta_d = np.asarray(theta_d, dtype=np.float64)
    return undistort(np.c_[theta_d, np.zeros(len(theta_d))], coeffs)[:, 0] / theta_d


def _harness_fisheye(p, k):
    return T.undistort(p, UNIT, k, True)


def _oracle_fisheye(p, k):
    return otri.undistort_fisheye(p, UNIT, k, float32_io=False)


def test_fisheye_inverse_against_the_fixture():
    fx = T.fixture()
    assert np.array_equal(fx["fe_coeffs"][0], T.FISHEYE_DIST) and not fx["fe_coeffs"][1].any() and len(fx["fe_coeffs"]) >= 2
    assert np.array_equal(fx["fe_theta_d"], [2e-8, 1e-4, 0.5, 1.0, 1.4, 1.55])
    worst = {}
    for name, f in (("oracle", _oracle_fisheye), ("harness", _harness_fisheye)):
        err = np.array([np.abs(_scales(f, k, fx["fe_theta_d"]) - want) / want for k, want in zip(fx["fe_coeffs"], fx["fe_scale"])])
        worst[name] = err.max()
        print(f"{name}: worst relative error of tan(theta) / theta_d {err.max():.4e} ({err.max() / T.EPS:.1f} eps); per theta_d", err.max(axis=0) / T.EPS)
    assert worst["oracle"] <= ORACLE_FISHEYE_WORST  # the figure the limit was taken from still holds for the reference
    assert worst["harness"] <= FISHEYE_LIMIT
    # the second coordinate and a direction off the axes: the same scale on both
    p = np.array([[0.3, 0.4], [-0.6, 0.8], [0.0, -1.4]])
    got, want = _harness_fisheye(p, T.FISHEYE_DIST), _oracle_fisheye(p, T.FISHEYE_DIST)
    assert np.abs(got - want).max() <= FISHEYE_LIMIT * np.abs(want).max() and got[2, 0] == 0.0


def test_fisheye_root_residual_on_a_dense_sweep():
    """The six theta_d of the fixture say little about where Newton stops: whether the last step taken lies just below the 1e-8 of
    the stop depends on theta_d.  So 3081 evenly spaced theta_d in [0.01, 1.55] per coefficient set, and the residual of the root
    itself: theta = atan(scale * theta_d) is put back into theta (1 + k1 theta^2 + ..) in np.longdouble.  Going back through atan is
    well conditioned — a relative error d of tan moves theta by d sin theta cos theta — so the tan_portable bound
    4 * 2^-52 * (1 + 1 / cos theta) moves theta by at most 8 * 2^-52; the division, the product, atan and the last ulp of theta add
    less than 4 * 2^-52 more, and the residual of a theta that is off by e is f'(theta) e.  A converged iteration cannot do better
    than the roundings of its own residual, six terms of the size of theta_d: 4 * 2^-52 * theta_d.  Together
    |residual| <= 2^-52 * (16 f'(theta) + 4 theta_d), with a margin of 4 / 3 on the first term.  (A stop at 1e-6 leaves up to 1e-13.)"""
    fx = T.fixture()
    theta_d = np.linspace(0.01, 1.55, 3081)
    for k in fx["fe_coeffs"]:
        theta = np.arctan(_scales(_harness_fisheye, k, theta_d) * theta_d).astype(np.longdouble)
        t2 = theta * theta
        residual = np.abs(theta * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - theta_d).astype(np.float64)
        slope = (1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))).astype(np.float64)
        limit = T.EPS * (16.0 * slope + 4.0 * theta_d)
        print(f"coefficients {k}: worst residual / limit {np.max(residual / limit):.3f}")
        assert np.all(residual <= limit), (k, theta_d[residual > limit][:5])


@pytest.mark.parametrize("coeffs", [T.FISHEYE_DIST, RECORDING_FISHEYE, np.zeros(4)], ids=["fisheye_dist", "recording", "zero"])
def test_fisheye_gate_at_1e_8(coeffs):
    """Below 1e-8 the scale is 1; just above, Newton and tan run and give 1 to rounding."""
    s = _scales(_harness_fisheye, coeffs, [0.9e-8, 1.1e-8])
    assert s[0] == 1.0 and abs(s[1] - 1.0) < 1e-15
    assert np.all(np.abs(_scales(_oracle_fisheye, coeffs, [0.9e-8, 1.1e-8]) - 1.0) < 1e-15)


@pytest.mark.parametrize("coeffs", [T.FISHEYE_DIST, RECORDING_FISHEYE], ids=["fisheye_dist", "recording"])
def test_fisheye_clip_at_half_pi(coeffs):
    """theta_d is clipped to pi / 2: 1.58 and 2.5 undistort as pi / 2 does (the same theta, divided by the clipped theta_d)."""
    theta_d = np.array([1.55, np.pi / 2, 1.58, 2.5])
    p = np.c_[0.6 * theta_d, -0.8 * theta_d]
    got, want = _harness_fisheye(p, coeffs), _oracle_fisheye(p, coeffs)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[2] / 1.58, got[1] / (np.pi / 2), rtol=1e-12, atol=0)


# ---- inputs outside the model ------------------------------------------------------------------------------------------------------------
def _equal_or_non_finite_together(got, want):
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), (got, want)
    m = np.isfinite(want)
    np.testing.assert_allclose(got[m], want[m], rtol=1e-9, atol=0)
    return m


def test_pinhole_radial_factor_crossing_zero():
    """k1 = -0.4: 1 + k1 r^2 passes zero at r^2 = 2.5 and the fixed-point iteration has nothing to converge to.  What cv2 returns
    there is not pinned (oracle/triangulation.py); the routine and the oracle do the same arithmetic and must say the same."""
    dist = np.array([-0.4, 0.0, 0.0, 0.0, 0.0])
    r = np.sqrt(np.array([1.5, 2.0, 2.4, 2.49, 2.5, 2.51, 2.6, 3.0, 4.0]))
    p = np.vstack([np.c_[r, np.zeros(len(r))], np.c_[0.6 * r, 0.8 * r], np.c_[-0.8 * r, 0.6 * r]])
    got, want = T.undistort(p, UNIT, dist, False), otri.undistort_pinhole(p, UNIT, dist, float32_io=False)
    m = _equal_or_non_finite_together(got, want)
    assert m.all() and np.abs(want).max() > 5.0 and np.abs(want).min() < 1e-30  # the inputs do leave the model


def test_fisheye_newton_leaving_the_interval():
    """k1 = -0.5: theta (1 - 0.5 theta^2) peaks at 0.544 (theta = 0.816), so theta_d = 1.4 has no root and Newton wanders."""
    dist = np.array([-0.5, 0.0, 0.0, 0.0])
    theta_d = np.array([0.5, 0.54, 0.55, 1.0, 1.4])
    p = np.vstack([np.c_[theta_d, np.zeros(5)], np.c_[0.6 * theta_d, 0.8 * theta_d]])
    got, want = _harness_fisheye(p, dist), _oracle_fisheye(p, dist)
    _equal_or_non_finite_together(got, want)


# ---- sym4_null_vector and the DLT --------------------------------------------------------------------------------------------------------
def test_null_vector_of_a_diagonal_matrix():
    """No rotation happens: the answer is the unit vector of the smallest entry, wherever it stands."""
    for k in range(4):
        d = np.array([5.0, 3.0, 4.0, 6.0])
        d[k] = 1e-3
        assert np.array_equal(T.sym4_null_vector(np.diag(d)), np.eye(4)[k : k + 1])


def _normal_matrices(t: T.Table):
    P = t.cam_P[t.obs_cam]
    r0, r1 = t.obs_xy[:, :1] * P[:, 8:12] - P[:, 0:4], t.obs_xy[:, 1:] * P[:, 8:12] - P[:, 4:8]
    M = np.zeros((t.n_points, 4, 4))
    np.add.at(M, np.repeat(np.arange(t.n_points), t.views), r0[:, :, None] * r0[:, None, :] + r1[:, :, None] * r1[:, None, :])
    return M


def test_dlt_against_the_fixture():
    fx = T.fixture()
    names = fx["dlt_scene_names"][fx["dlt_scene"]]
    assert {"ring6", "adjacent2", "opposed2", "baseline5cm", "baseline5cm_clean", "offset130", "static1000", "same_camera2"} == set(names)
    t, _ = T.fixture_table()
    assert t.views.max() == 1000 and np.linalg.norm(fx["dlt_exact"][names == "offset130"], axis=1).min() > 125.0
    xyz, und = T.triangulate(t)
    assert np.array_equal(T.bits(und), T.bits(t.obs_xy))  # cam_intr == NULL: the coordinates pass through
    w = T.sym4_null_vector(_normal_matrices(t))
    alone = w[:, :3] / w[:, 3:]
    bound = T.dlt_bound(fx["dlt_eig"], fx["dlt_exact"])
    check = names != "same_camera2"  # two rays from one centre: the null vector is the centre, nothing is asserted about it
    for what, got in (("th_triangulate", xyz), ("sym4_null_vector", alone)):
        ratio = np.abs(got - fx["dlt_exact"]).max(axis=1) / bound
        for s in np.unique(names[check]):
            print(f"{what} {s}: worst error / bound {ratio[names == s].max():.4f} (bound up to {bound[names == s].max():.3e})")
        assert np.all(ratio[check] <= 1.0), (what, names[check][ratio[check] > 1.0])


def test_fewer_than_two_views_give_nan():
    t, _ = T.fixture_table(["ring6"])
    starts = np.array([0, 0, 1, 3, 3, 9, 10, 10])  # 0, 1, 2, 0, 6, 1, 0 views
    xyz, _ = T.triangulate(T.Table(t.cam_P, starts, t.obs_cam[:10], t.obs_xy[:10]))
    assert np.array_equal(np.isnan(xyz), np.repeat(np.diff(starts) < 2, 3).reshape(-1, 3))


def test_sweep_scene_on_the_cpu_build():
    """The scene of the device's shape sweep through the harness: NaN exactly below two views, the rest within the bound of the
    np.longdouble evaluation (of the fixture for the 1000-view point), which itself reproduces the fixture."""
    fx = T.fixture()
    ft, _ = T.fixture_table()
    ld, eig = T.longdouble_dlt(ft.cam_P, ft.pt_start, ft.obs_cam, ft.obs_xy)
    ok = fx["dlt_scene_names"][fx["dlt_scene"]] != "same_camera2"
    assert np.all(np.abs(ld - fx["dlt_exact"]).max(axis=1)[ok] <= 1e-3 * T.dlt_bound(fx["dlt_eig"], fx["dlt_exact"])[ok])
    np.testing.assert_allclose(eig[ok, 1:], fx["dlt_eig"][ok, 1:], rtol=1e-13)
    t = T.sweep_table(257, big_at=(0, 100), views_at={255: 0, 256: 1})
    assert set(t.views) == {0, 1, 2, 3, 12, 1000} and T.UNUSED_CAMERA not in t.obs_cam and t.obs_cam.max() == len(t.cam_P) - 1
    assert set(t.cam_model[np.unique(t.obs_cam)]) == {0, 1}
    xyz, und = T.triangulate(t)
    assert np.array_equal(T.bits(und[:1000]), T.bits(t.obs_xy[:1000]))  # unit intrinsics: the fixture's coordinates arrive untouched
    want, bound = T.sweep_reference(t, und, big_at=(0, 100))
    assert np.array_equal(np.isnan(xyz), np.repeat(t.views < 2, 3).reshape(-1, 3))
    seen = t.views >= 2
    assert np.all(np.abs(xyz - want).max(axis=1)[seen] <= bound[seen])
    assert np.array_equal(xyz[0], xyz[100])



# ---- the point table of a call -----------------------------------------------------------------------------------------------------------
def _starts_ok(starts):
    lib = load_native(NATIVE / "setup_harness.cpp", flags=("-pthread",))
    lib.sp_triangulate_starts_ok.restype = C.c_int
    lib.sp_triangulate_starts_ok.argtypes = [C.c_long, C.POINTER(C.c_long)]
    lib.sp_last_error.restype = C.c_char_p
    a = np.ascontiguousarray(starts, dtype=np.int64)
    rc = lib.sp_triangulate_starts_ok(len(a) - 1, a.ctypes.data_as(C.POINTER(C.c_long)))
    return rc, lib.sp_last_error().decode()


BAD_STARTS = {"first entry 1": ([1, 2, 4], "pt_start[0] is 1"), "decreasing pair": ([0, 3, 2, 5], "pt_start[2] = 2 is below pt_start[1] = 3"),
              "negative end": ([0, 2, -4], "pt_start[2] = -4 is below pt_start[1] = 2")}


def test_triangulate_starts_ok():
    for good in ([0, 0], [0, 2], [0, 0, 0, 0], [0, 2, 2, 5, 1005], list(range(0, 600, 2))):
        assert _starts_ok(good)[0] == 0, good
    for name, (bad, text) in BAD_STARTS.items():
        rc, msg = _starts_ok(bad)
        assert rc == -1 and text in msg, (name, rc, msg)
