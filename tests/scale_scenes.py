"""Scenes and bounds shared by the CPU and GPU tests of cba_scale_errors (tests/test_anchoring.py, tests/test_anchoring_gpu.py).

Bounds on the statistics (derived, not tuned).  u = 2^-53, L the largest measured or true distance of a group, m its pair count,
tau = 16 u L: a distance carries at most 3.5 u relative error, an err at most about 7 u L, two correct evaluations differ by at
most twice that.  max|err| and D_ref: tau.  sum err: m tau + 2 m u sum|err|.  sum err^2: 2 tau sum|err| + m tau^2 + 2 m u sum err^2.
A centroid coordinate: 2 n u max|coordinate|.  Derived values inherit them through sqrt and division (``derived_bounds``).  float64
``pdist`` summed sequentially in shuffled order stays below 0.12 of every bound against ``np.longdouble`` (group sizes 2 to 2 049,
object scales 0.05 to 5 m, noise 0 to 0.2 m): the reference alone is inside with an 8-fold margin."""
import numpy as np
from scipy.spatial.distance import pdist

U = 2.0 ** -53


def stat_bounds(L, m, sum_abs, sum_sq, n, max_coord):
    """Bounds on (sum err, sum err^2, max|err|, D_ref, centroid coordinate) between two correct evaluations (module docstring)."""
    tau = 16 * U * L
    return dict(s1=m * tau + 2 * m * U * sum_abs, s2=2 * tau * sum_abs + m * tau * tau + 2 * m * U * sum_sq, mx=tau, dref=tau,
                centroid=2 * n * U * max_coord)


def reference_stats(world, obj, dtype=np.float64):
    """(stats[8], bounds) of one group from numpy alone: pdist in float64, or every step in np.longdouble."""
    world, obj = np.asarray(world, dtype=np.float64), np.asarray(obj, dtype=np.float64)
    n = len(world)
    if dtype is np.float64:
        dm, dt = pdist(world), pdist(obj)
    else:
        i, j = np.triu_indices(n, 1)
        w, o = world.astype(dtype), obj.astype(dtype)
        dm, dt = np.sqrt(((w[i] - w[j]) ** 2).sum(axis=1)), np.sqrt(((o[i] - o[j]) ** 2).sum(axis=1))
    err = dm - dt
    m = len(err)
    stats = np.array([err.sum(), (err * err).sum(), np.abs(err).max(), dt.max(), *world.astype(dtype).mean(axis=0), m], dtype=dtype)
    L = float(max(dm.max(), dt.max()))
    return stats, stat_bounds(L, m, float(np.abs(err).sum()), float((err * err).sum()), n, float(np.abs(world).max())), err


def assert_stats(got, want, b, what=""):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    assert got[7] == want[7], f"{what}: pair count {got[7]} != {want[7]}"
    for k, key in ((0, "s1"), (1, "s2"), (2, "mx"), (3, "dref"), (4, "centroid"), (5, "centroid"), (6, "centroid")):
        assert abs(got[k] - want[k]) <= b[key], f"{what}: statistic {k} off by {float(abs(got[k] - want[k])):.3e}, bound {b[key]:.3e}"


def derived_bounds(stats, b):
    """Bounds on a FrameScaleError's floats from those of the statistics: sqrt and division propagated, plus 4 u relative for the
    roundings of the few operations that form them."""
    s1, s2, mx, dref, m = stats[0], stats[1], stats[2], stats[3], stats[7]
    rmse = np.sqrt(s2 / m)
    d_rmse = min(np.sqrt(b["s2"] / m), b["s2"] / (m * rmse) if rmse > 0 else np.inf)  # |sqrt a - sqrt b| <= min(sqrt|a - b|, |a - b| / sqrt a)
    rel = s2 / dref ** 2 if dref > 0 else 0.0
    d_rel = (b["s2"] / dref ** 2 + 2 * rel * b["dref"] / dref * 1.01) if dref > 0 else 0.0
    return dict(distance_rmse_mm=1000 * d_rmse + 4 * U * 1000 * rmse, distance_mean_signed_error_mm=1000 * b["s1"] / m + 4 * U * 1000 * abs(s1 / m),
                distance_max_error_mm=1000 * b["mx"] + 4 * U * 1000 * mx, sum_squared_errors_m2=b["s2"], sum_squared_relative_errors=d_rel + 4 * U * rel,
                centroid=b["centroid"])


def noisy_group(rng, n, scale, noise):
    obj = rng.uniform(-scale, scale, size=(n, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return obj @ q.T + rng.normal(size=3) + rng.normal(size=(n, 3)) * noise, obj


def uniform_scale_scene(rng, n):
    """Object points at least 0.02 m apart; world points a rigid motion of 1.001 x them: every err = 0.001 d_true >= 2e-5."""
    obj = np.zeros((0, 3))
    while len(obj) < n:
        cand = rng.uniform(-1.0, 1.0, size=(4 * n, 3))
        for p in cand:
            if len(obj) == 0 or ((obj - p) ** 2).sum(axis=1).min() >= 0.02 ** 2:
                obj = np.vstack([obj, p])
                if len(obj) == n:
                    break
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return 1.001 * obj @ q.T + rng.normal(size=3), obj
