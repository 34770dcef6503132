"""Writes tests/golden/triangulation_edge_fixtures.npz: inputs and 60-digit expectations (mpmath) of the three routines behind
``cba_triangulate`` — ``tan_portable``, the fisheye inverse of ``undistort_one`` and the DLT null vector of ``sym4_null_vector``.

    python tests/golden/make_triangulation_edge_fixtures.py

Run on a CPU; the tests read the file and never import mpmath.  Everything a test needs is stored (inputs too), so a reader depends
on no random-generator stream.  Every expectation is the exact result for the stored float64 inputs, rounded once to float64.

tan        ``tan_x`` [2013]: 2001 evenly spaced x in [0, 1.5], then pi/2 - 10^-k for k = 1..12 (as float64); ``tan_ref`` = tan(x).
           ``tan_wide_x`` [400]: evenly spaced in [1.6, 40] (up to 13 periods beyond the interval), ``tan_wide_ref`` = tan(x).
fisheye    ``fe_coeffs`` [n_sets][4] (every set has theta (1 + k1 theta^2 + ..) increasing on [0, pi/2]), ``fe_theta_d`` [6];
           ``fe_theta`` [n_sets][6] the root of theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = theta_d and
           ``fe_scale`` = tan(theta) / theta_d.
DLT        one table of points over all scenes: ``dlt_P`` [n_cams][12] normalised [R | t] of every scene's cameras one after the
           other, ``dlt_pt_start`` [n_points + 1], ``dlt_cam`` [n_obs] (index into dlt_P), ``dlt_xy`` [n_obs][2] normalised
           coordinates, ``dlt_scene`` [n_points] index into ``dlt_scene_names``, ``dlt_truth`` [n_points][3] the point the views
           were projected from.  Expectations: with rows x P[2] - P[0], y P[2] - P[1] formed exactly from the float64 x, y and P,
           ``dlt_eig`` [n_points][4] the eigenvalues l1 <= .. <= l4 of A^T A and ``dlt_exact`` [n_points][3] its eigenvector of l1,
           dehomogenised.
           scenes: ring6 (six cameras on a 2 m ring, 0.3 px noise at f = 1394.6), adjacent2 (two neighbours of the ring), opposed2,
           baseline5cm / baseline5cm_clean (two cameras 5 cm apart, 10 m away, with and without noise), offset130 (ring6 with the
           world origin moved to (100, -80, 30)), static1000 (one point, the ring repeated with fresh noise, 1000 views),
           same_camera2 (two views of the same camera index with different coordinates: the null vector is the camera centre).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
from mpmath import mp, mpf

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
OUT = Path(__file__).resolve().parent / "triangulation_edge_fixtures.npz"

mp.dps = 60
FOCAL = 1394.6
DRAWS = 20


def tan_table():
    x = np.concatenate([np.linspace(0.0, 1.5, 2001), [np.pi / 2 - 10.0**-k for k in range(1, 13)]])
    wide = np.linspace(1.6, 40.0, 400)
    return x, np.array([float(mp.tan(mpf(float(v)))) for v in x]), wide, np.array([float(mp.tan(mpf(float(v)))) for v in wide])


FISHEYE_SETS = np.array([
    [0.05, -0.01, 0.003, -0.001],   # FISHEYE_DIST of tests/test_triangulation.py
    [0.0, 0.0, 0.0, 0.0],
    [0.05, -0.02, 0.004, 0.001],    # the fisheye of the trajectory recording
    [-0.005, 0.001, -0.0002, 0.00005],  # barrel: theta_d grows slower than theta, the root of 1.55 is 0.01 short of pi/2
    [0.3, 0.05, 0.01, 0.002],       # strong
])
THETA_D = np.array([2e-8, 1e-4, 0.5, 1.0, 1.4, 1.55])


def fisheye_table():
    theta, scale = np.zeros((len(FISHEYE_SETS), len(THETA_D))), np.zeros((len(FISHEYE_SETS), len(THETA_D)))
    for i, k in enumerate(FISHEYE_SETS):
        k1, k2, k3, k4 = (mpf(float(v)) for v in k)
        for t in np.linspace(0.0, np.pi / 2, 2001):  # increasing on [0, pi/2]
            t2 = float(t) ** 2
            assert 1 + 3 * k[0] * t2 + 5 * k[1] * t2**2 + 7 * k[2] * t2**3 + 9 * k[3] * t2**4 > 0.05, (i, t)
        for j, td in enumerate(THETA_D):
            tdm = mpf(float(td))
            f = lambda th: th * (1 + k1 * th**2 + k2 * th**4 + k3 * th**6 + k4 * th**8) - tdm  # noqa: E731
            root = mp.findroot(f, tdm, tol=mpf(10) ** -50)
            assert 0 < root < mp.pi / 2 and abs(f(root)) < mpf(10) ** -48, (i, j, root)
            theta[i, j], scale[i, j] = float(root), float(mp.tan(root) / tdm)
    return theta, scale


def look_at(position, target):
    fwd = target - position
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.vstack([right, down / np.linalg.norm(down), fwd])


def camera(position, target):
    R = look_at(np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64))
    return np.hstack([R, (-R @ np.asarray(position, dtype=np.float64)).reshape(3, 1)]).reshape(12)


def ring(n=6, radius=2.0, height=0.5, target=(0.0, 0.0, 0.6)):
    return [camera((radius * np.cos(2 * np.pi * i / n), radius * np.sin(2 * np.pi * i / n), height), target) for i in range(n)]


def shifted(P, offset):
    """The camera after the world origin moved: X' = X + offset, so t' = t - R offset."""
    M = P.reshape(3, 4).copy()
    M[:, 3] -= M[:, :3] @ offset
    return M.reshape(12)


def view(P, X, noise, rng):
    Xc = P.reshape(3, 4) @ np.append(X, 1.0)
    return Xc[:2] / Xc[2] + rng.normal(0.0, noise, 2)


def exact(P_list, xy):
    """(eigenvalues ascending, dehomogenised eigenvector of the smallest) of A^T A, rows formed exactly from the float64 inputs."""
    M = mp.zeros(4, 4)
    for P, (x, y) in zip(P_list, xy):
        p = [mpf(float(v)) for v in P]
        xm, ym = mpf(float(x)), mpf(float(y))
        for row in ([xm * p[8 + c] - p[c] for c in range(4)], [ym * p[8 + c] - p[4 + c] for c in range(4)]):
            for r in range(4):
                for c in range(4):
                    M[r, c] += row[r] * row[c]
    E, Q = mp.eigsy(M)
    order = sorted(range(4), key=lambda i: E[i])
    w = [Q[r, order[0]] for r in range(4)]
    lam = [float(E[i]) for i in order]
    return lam, [float(w[r] / w[3]) for r in range(3)]


def main():
    rng = np.random.default_rng(20261018)
    noise = 0.3 / FOCAL
    offset = np.array([100.0, -80.0, 30.0])
    cams, scenes = [], []  # cameras of all scenes; (name, first camera, cameras, draws, point sampler, X -> [(local camera, xy)])

    def add_scene(name, P_list, draws, sampler, views_of):
        first = len(cams)
        cams.extend(P_list)
        scenes.append((name, first, P_list, draws, sampler, views_of))

    near = lambda: np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(0.2, 1.0)])  # noqa: E731
    every = lambda P_list, sigma: (lambda X: [(c, view(P, X, sigma, rng)) for c, P in enumerate(P_list)])  # noqa: E731
    r6 = ring()
    add_scene("ring6", r6, DRAWS, near, every(r6, noise))
    add_scene("adjacent2", r6[:2], DRAWS, near, every(r6[:2], noise))
    add_scene("opposed2", [r6[0], r6[3]], DRAWS, near, every([r6[0], r6[3]], noise))
    pair = [camera((-0.025, 0.0, 0.0), (-0.025, 10.0, 0.0)), camera((0.025, 0.0, 0.0), (0.025, 10.0, 0.0))]
    far = lambda: np.array([rng.uniform(-1.0, 1.0), 10.0 + rng.uniform(-0.5, 0.5), rng.uniform(-1.0, 1.0)])  # noqa: E731
    add_scene("baseline5cm", pair, DRAWS, far, every(pair, noise))
    add_scene("baseline5cm_clean", pair, DRAWS, far, every(pair, 0.0))
    r6o = [shifted(P, offset) for P in r6]
    add_scene("offset130", r6o, DRAWS, lambda: near() + offset, every(r6o, noise))
    add_scene("static1000", r6, 1, lambda: np.array([0.1, -0.2, 0.5]),
              lambda X: [(i % 6, view(r6[i % 6], X, noise, rng)) for i in range(1000)])
    add_scene("same_camera2", r6, 1, lambda: np.array([0.1, -0.2, 0.5]),
              lambda X: [(2, view(r6[2], X, 0.0, rng)), (2, view(r6[2], X + np.array([0.05, 0.02, 0.0]), 0.0, rng))])

    pt_start, obs_cam, obs_xy, scene_of, truth, eig, xyz = [0], [], [], [], [], [], []
    for s, (name, first, P_list, draws, sampler, views_of) in enumerate(scenes):
        for _ in range(draws):
            X = sampler()
            views = views_of(X)
            lam, w = exact([P_list[c] for c, _ in views], [xy for _, xy in views])
            obs_cam.extend(first + c for c, _ in views)
            obs_xy.extend(xy for _, xy in views)
            pt_start.append(len(obs_cam))
            scene_of.append(s); truth.append(X); eig.append(lam); xyz.append(w)
        print(f"{name}: {draws} points, worst |exact - truth| {max(np.abs(np.array(xyz[-draws:]) - np.array(truth[-draws:])).max(), 0):.3e}, "
              f"l4 / (l2 - l1) up to {max(e[3] / (e[1] - e[0]) for e in eig[-draws:]):.3e}")
    tan_x, tan_ref, tan_wide_x, tan_wide_ref = tan_table()
    fe_theta, fe_scale = fisheye_table()
    np.savez_compressed(
        OUT, tan_x=tan_x, tan_ref=tan_ref, tan_wide_x=tan_wide_x, tan_wide_ref=tan_wide_ref, fe_coeffs=FISHEYE_SETS, fe_theta_d=THETA_D, fe_theta=fe_theta, fe_scale=fe_scale,
        dlt_P=np.array(cams), dlt_pt_start=np.array(pt_start, dtype=np.int64), dlt_cam=np.array(obs_cam, dtype=np.int32),
        dlt_xy=np.array(obs_xy), dlt_scene=np.array(scene_of, dtype=np.int32), dlt_scene_names=np.array([s[0] for s in scenes]),
        dlt_truth=np.array(truth), dlt_eig=np.array(eig), dlt_exact=np.array(xyz))
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
