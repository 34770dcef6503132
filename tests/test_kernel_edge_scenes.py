"""The scenes of tests/test_kernel_edges_gpu.py have the planning properties their GPU tests rely on (no GPU needed): a scene that stopped having
its property would fail here instead of quietly testing another route on the device."""
import numpy as np
import pytest

from tests.edge_scenes import CHUNK, CON_SMALL_LDS, CON_SMALL_M, CS_MAX_PTS, con_small_lds_bytes, sparse_id_scene
from tests.test_library_abi import _plan, lib  # noqa: F401 - the module fixture that builds and loads the library


def _ranges(lib, sc):
    par = sc["par"]
    nch, order, pstart, cstart = _plan(lib, par.n_points, sc["obj"], CHUNK, sc["cam"], len(par.blocks))
    assert nch > 0
    pts = sc["obj"][order]
    first, last = pts[cstart[:-1]], pts[cstart[1:] - 1]
    return first, last, pstart, cstart


@pytest.mark.parametrize("stride, heavy_obs, lo, hi", [(5, 256, CHUNK, CS_MAX_PTS), (8, 256, CS_MAX_PTS, None), (5, 257, CHUNK, CS_MAX_PTS),
                                                      (5, None, CHUNK, CS_MAX_PTS), (8, None, CS_MAX_PTS, None)])
def test_sparse_id_scenes_reach_the_padded_range_branches(lib, stride, heavy_obs, lo, hi):  # noqa: F811
    sc = sparse_id_scene(stride, heavy_obs=heavy_obs)
    first, last, pstart, cstart = _ranges(lib, sc)
    span = last - first + 1
    # the largest chunk range: above 256 ids (the loops over points beyond the first 256 of a chunk), and above 512 for stride 8 (k_build_cs off)
    assert span.max() > lo and (hi is None or span.max() <= hi), span.max()
    # the runs of unobserved ids in front of the first and behind the last observed point lie outside every chunk range
    ids = np.arange(sc["par"].n_points)
    in_range = np.zeros(len(ids), dtype=bool)
    for a, b in zip(first, last):
        in_range[a:b + 1] = True
    assert sc["lead"] > CHUNK and sc["tail"] > CHUNK
    assert not in_range[: sc["lead"]].any() and not in_range[-sc["tail"]:].any()
    assert np.all(in_range[sc["observed"]])
    # the static-marker point: 256 observations are one chunk of their own, 257 are split into fragments (k_backsub_rec is then off)
    counts = np.diff(pstart)
    if heavy_obs is None:
        assert counts.max() <= 3
        return
    h = sc["heavy_id"]
    assert np.flatnonzero(counts > 3).tolist() == [h]
    assert pstart[h + 1] - pstart[h] == heavy_obs
    starts_inside = np.count_nonzero((cstart > pstart[h]) & (cstart < pstart[h + 1]))
    assert starts_inside == (0 if heavy_obs <= CHUNK else 1)
    assert np.isin(pstart[h], cstart) and np.isin(pstart[h + 1], cstart)


# (m rows, points, camera parameters, k_con_schur_small's LDS bytes or None beyond CON_SMALL_M rows, small route)
COMPONENT_TABLE = [
    (1, 2, 12, 26136, True), (31, 8, 12, 56184, True), (32, 8, 12, 58112, True), (33, 8, 12, 59048, True), (64, 4, 12, 113152, True),
    (64, 8, 12, 120832, True), (65, 4, 12, None, False), (55, 12, 24, 119832, True), (56, 12, 24, 123200, False), (33, 8, 36, 76328, True),
    (53, 8, 36, 119688, True), (54, 8, 36, 123056, False), (48, 12, 24, 104192, True),  # (the last: the mixed handle's max_m / max_np)
]


@pytest.mark.parametrize("m, npts, ncp, nbytes, small", COMPONENT_TABLE)
def test_component_shapes_fall_on_the_intended_side_of_the_small_kernel_limits(m, npts, ncp, nbytes, small):
    """The routes tests/test_kernel_edges_gpu.py expects of its constraint components, from the layout of k_con_schur_small: at most
    CON_SMALL_M = 64 rows and 120 KB of LDS."""
    got = con_small_lds_bytes(m, npts, ncp)
    if nbytes is not None:
        assert got == nbytes
    assert (m <= CON_SMALL_M and got <= CON_SMALL_LDS) == small
