"""The recorded reference of the MANY_POINTS scene of tests/covariance_edge_scenes.py (three six-wide cameras x 65 793 points), for which a
dense pseudo-inverse is out of reach: blocks of pinv(J^T J) from the bordered system

    [ H    N ] [ X ]   [ E ]
    [ N^T  0 ] [ M ] = [ 0 ]        H = J^T J (sparse, from the oracle's joint_jacobian), N = covariance_native.gauge_matrix

factored once with scipy.sparse.linalg.splu and solved for the unit columns E of the 18 camera parameters and of the sampled points:
X = pinv(H) E, because the seven columns of N span the null space of H.  Written to tests/golden/covariance_many_points.npz (a few
kilobytes): the 18 x 18 camera block, the sampled 3 x 3 point blocks and their indices, dof, cost, sigma0^2 and the SHA-256 of the
scene's x, cam, obj and uv bytes, which the tests require of the scene they rebuild from its seed.

CPU only, no device, not collected by pytest.  Run time: six to seven minutes on one core (233 s for the factorisation, 130 to 190 s for
the 42 solves); that is why the result is recorded and not computed by the suite.  A second run reproduced the file bit for bit.

    python tests/golden/make_covariance_many_points_fixture.py [output file]
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def bordered_solve(sc, point_index, report=print):
    """(pinv(H)[:ncp, :ncp], the 3 x 3 diagonal blocks of pinv(H) at ``point_index``) by a sparse LU of the bordered system."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu

    from oracle.residuals import joint_jacobian
    from tests import covariance_native as cn

    par, x = sc["par"], sc["x"]
    ncp, n = par.n_camera_params, len(x)
    J = joint_jacobian(x, par, sc["cam"], sc["uv"], sc["obj"]).tocsc()
    N = sp.csc_matrix(cn.gauge_matrix(par, x))
    K = sp.bmat([[J.T @ J, N], [N.T, None]], format="csc")
    t0 = time.perf_counter()
    lu = splu(K)
    report(f"factored {K.shape[0]} unknowns in {time.perf_counter() - t0:.0f} s")
    cols = np.concatenate([np.arange(ncp)] + [ncp + 3 * p + np.arange(3) for p in point_index])
    E = np.zeros((K.shape[0], len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    t0 = time.perf_counter()
    X = lu.solve(E)
    report(f"solved {len(cols)} columns in {time.perf_counter() - t0:.0f} s; |N^T X| = {np.abs(N.T @ X[:n]).max():.1e}")
    cc = X[:ncp, :ncp]
    pp = np.stack([X[ncp + 3 * p: ncp + 3 * p + 3, ncp + 3 * i: ncp + 3 * i + 3] for i, p in enumerate(point_index)])  # (column block i belongs to point p)
    return 0.5 * (cc + cc.T), 0.5 * (pp + np.swapaxes(pp, 1, 2))


def main(out_file):
    from oracle.residuals import joint_residuals
    from tests import covariance_edge_scenes as es
    from tests import covariance_native as cn

    sc = cn.key_scene(es.MANY_POINTS)
    cc, pp = bordered_solve(sc, es.MANY_POINTS_SAMPLE)
    f = joint_residuals(sc["x"], sc["par"], sc["cam"], sc["uv"], sc["obj"])
    cost = 0.5 * float(f @ f)
    dof = len(f) - len(sc["x"]) + 7
    np.savez(out_file, cam_block=cc, point_blocks=pp, point_index=np.asarray(es.MANY_POINTS_SAMPLE, dtype=np.int64), dof=np.int64(dof),
             cost=np.float64(cost), sigma0_sq=np.float64(2.0 * cost / dof), sha256=np.str_(es.scene_hash(sc)))
    print(out_file, cc.shape, pp.shape, dof, cost)


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).resolve().parent / "covariance_many_points.npz")
