"""csrc/epipolar_math.h on the CPU (the g++ harness): essential RANSAC of one pair, the four-way decomposition, the Sampson
distance, the sampler and RANSAC resection, against ground truth, numpy and scipy."""
import numpy as np
import pytest
from scipy.optimize import least_squares

from caliscope_amd.cameras import rvec_to_matrix
from tests.epipolar_native import HarnessEpipolar, decompose, sample, sampson


def _pair_scene(n=300, seed=0, noise_px=0.0, outliers=0.0, f=1600.0, half_width=0.5):
    """The reference unit test's scene: points uniform in [-0.5, 0.5]^2 x [4, 6], rvec (0.05, 0.35, -0.1), t (1.2, 0.1, 0.3)
    (``half_width`` widens the cloud)."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-half_width, half_width, (n, 2)), rng.uniform(4, 6, n)])
    R, t = rvec_to_matrix(np.array([0.05, 0.35, -0.1])), np.array([1.2, 0.1, 0.3])
    Xb = X @ R.T + t
    a, b = X[:, :2] / X[:, 2:], Xb[:, :2] / Xb[:, 2:]
    a = a + rng.normal(0, noise_px / f, a.shape)
    b = b + rng.normal(0, noise_px / f, b.shape)
    bad = rng.random(n) < outliers
    b[bad] = rng.uniform(-0.4, 0.4, (int(bad.sum()), 2))
    return a, b, R, t, ~bad


def _essential_one(a, b, f=1600.0, thr_px=3.0, n_hyp=1024, seed=0):
    """One pair through the harness with K = diag(f, f, 1) pixels and no distortion."""
    n = len(a)
    intr = np.array([[f, f, 0, 0, 0, 0, 0, 0, 0]] * 2, dtype=float)
    xy = np.vstack([a, b]) * f
    return HarnessEpipolar().essential_batch(np.zeros(2, np.int32), intr, xy, np.repeat([0, 1], n), np.array([0, n]), np.arange(n),
                                             n + np.arange(n), np.array([thr_px / f]), n_hyp, seed)


def _angle_deg(R1, R2):
    return np.degrees(np.arccos(np.clip((np.trace(R1 @ R2.T) - 1) / 2, -1, 1)))


def test_noiseless_pair_recovers_the_pose():
    a, b, R, t, _ = _pair_scene()
    out = _essential_one(a, b)
    assert out["status"][0] == 0
    np.testing.assert_allclose(out["pose"][0, :9].reshape(3, 3), R, atol=1e-8)
    np.testing.assert_allclose(out["pose"][0, 9:], t / np.linalg.norm(t), atol=1e-8)
    assert out["n_inliers"][0] == 300 and out["n_cheiral"][0] == 300
    assert out["conditioning"][0] > 0.9
    # the two-view points are the scene in camera A's frame at baseline 1
    X = np.column_stack([a, np.ones(len(a))]) * out["xyz"][:, 2:]
    np.testing.assert_allclose(out["xyz"], X, atol=1e-9)
    assert np.isfinite(out["xyz"]).all() and np.all(out["xyz"][:, 2] > 0)


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_noisy_pair_with_outliers(seed):
    """0.5 px noise, 30 % gross outliers.  (The cloud is widened to +-2 m: at +-0.5 m the view angle is ~12 degrees and the
    maximum-likelihood pose itself lies ~0.2-0.3 degrees from the truth at this noise.)"""
    a, b, R, t, good = _pair_scene(n=400, seed=seed, noise_px=0.5, outliers=0.3, half_width=2.0)
    out = _essential_one(a, b)
    assert out["status"][0] == 0
    Rh, th = out["pose"][0, :9].reshape(3, 3), out["pose"][0, 9:]
    assert _angle_deg(Rh, R) < 0.1
    assert np.degrees(np.arccos(np.clip(th @ t / np.linalg.norm(t), -1, 1))) < 2.0
    flag = out["flag"]
    assert (flag[good] >= 1).mean() >= 0.95
    # no flagged point beyond the gate
    E = np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]]) @ Rh
    d = np.array([sampson(E, *a[i], *b[i]) for i in range(len(a))])
    thr = 3.0 / 1600.0
    assert (d[flag >= 1] <= thr**2).all() and (d[flag == 0] > thr**2).all()


@pytest.mark.parametrize("case", range(4))
def test_decomposition_picks_the_true_branch(case):
    """Scenes whose true (R, t) is each of the four candidates of the decomposition in turn."""
    rng = np.random.default_rng(case)
    picked = set()
    for trial in range(40):
        R = rvec_to_matrix(rng.normal(0, 0.6, 3))
        t = rng.normal(0, 1, 3)
        t /= np.linalg.norm(t)
        X = np.column_stack([rng.uniform(-1, 1, (60, 2)), rng.uniform(3, 6, 60)])
        Xb = X @ R.T + t
        if (Xb[:, 2] <= 0.5).any():
            continue
        a, b = X[:, :2] / X[:, 2:], Xb[:, :2] / Xb[:, 2:]
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        E = E * rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
        k, rt, cnt = decompose(E, a, b)
        assert cnt[k] == 60
        np.testing.assert_allclose(rt[k, :9].reshape(3, 3), R, atol=1e-9)
        np.testing.assert_allclose(rt[k, 9:], t, atol=1e-9)
        picked.add(k)
        if case in picked:
            break
    assert case in picked, picked


def test_sampson_matches_numpy():
    rng = np.random.default_rng(5)
    for _ in range(50):
        E = rng.normal(size=(3, 3))
        xa, ya, xb, yb = rng.normal(0, 0.5, 4)
        pa, pb = np.array([xa, ya, 1.0]), np.array([xb, yb, 1.0])
        Ea, Etb = E @ pa, E.T @ pb
        ref = (pb @ E @ pa) ** 2 / (Ea[0] ** 2 + Ea[1] ** 2 + Etb[0] ** 2 + Etb[1] ** 2)
        assert abs(sampson(E, xa, ya, xb, yb) - ref) <= 1e-14 * max(1.0, ref)


def test_sampler_draws_distinct_reproducible_indices():
    for n, k in ((8, 8), (9, 8), (50, 8), (100000, 8), (6, 6), (60, 6)):
        seen = set()
        for h in range(64):
            idx = sample(7, 3, h, n, k)
            assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < n
            assert np.array_equal(idx, sample(7, 3, h, n, k))
            seen.add(tuple(sorted(idx.tolist())))
        assert n <= k + 1 or len(seen) > 32
    assert not np.array_equal(sample(7, 3, 0, 1000, 8), sample(8, 3, 0, 1000, 8))
    assert not np.array_equal(sample(7, 3, 0, 1000, 8), sample(7, 4, 0, 1000, 8))


def test_resection_agrees_with_scipy_on_its_inliers():
    rng = np.random.default_rng(2)
    n = 200
    X = rng.uniform(-1, 1, (n, 3)) + [0, 0, 0]
    R, t = rvec_to_matrix(np.array([0.2, -0.4, 0.1])), np.array([0.1, -0.2, 5.0])
    Xc = X @ R.T + t
    uv = Xc[:, :2] / Xc[:, 2:] + rng.normal(0, 0.3 / 1000, (n, 2))
    bad = rng.random(n) < 0.2
    uv[bad] += rng.uniform(-0.05, 0.05, (int(bad.sum()), 2))
    thr = 3.0 / 1000
    out = HarnessEpipolar().resect_batch(np.array([0, n]), X, uv, np.array([thr]), 200, 50, 0)
    assert out["status"][0] == 0
    Rh, th = out["pose"][0, :9].reshape(3, 3), out["pose"][0, 9:]
    assert _angle_deg(Rh, R) < 0.2 and np.linalg.norm(th - t) < 0.05
    assert out["n_inliers"][0] >= 0.95 * (~bad).sum()
    # LM on the inliers of the winning hypothesis: the same minimum scipy finds on the final inliers
    inl = out["err"] <= thr
    def res(p):
        Rp = rvec_to_matrix(p[:3])
        Y = X[inl] @ Rp.T + p[3:]
        return (Y[:, :2] / Y[:, 2:] - uv[inl]).ravel()
    from scipy.spatial.transform import Rotation

    sol = least_squares(res, np.concatenate([Rotation.from_matrix(Rh).as_rotvec(), th]), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    np.testing.assert_allclose(rvec_to_matrix(sol.x[:3]), Rh, atol=1e-6)
    np.testing.assert_allclose(sol.x[3:], th, atol=1e-6)


def test_too_few_and_degenerate_jobs_report_a_status():
    a, b, _, _, _ = _pair_scene(n=7)
    assert _essential_one(a, b)["status"][0] == 1
    out = HarnessEpipolar().resect_batch(np.array([0, 5]), np.zeros((5, 3)), np.zeros((5, 2)), np.array([0.01]), 10, 6, 0)
    assert out["status"][0] == 1 and np.isnan(out["err"]).all()
