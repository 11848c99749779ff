"""The model of tests/decimate_ref.py against the numbers a prototype of it gave when the service was specified, the
properties that follow from the definition, and one case small enough to do by hand.  Inputs come from the model of the
triangulation (tests/mesh_ref.py), as the device's inputs come from smx_recon_triangulate."""
import numpy as np
import pytest

import decimate_ref as dr
import mesh_ref as mr
from common import small_pre


@pytest.fixture(scope="module")
def sphere():
    m = mr.sphere_map()
    return m, mr.triangulate(*m)[0]


@pytest.fixture(scope="module")
def plane():
    m = mr.plane_map()
    return m, mr.triangulate(*m)[0]


@pytest.fixture(scope="module")
def grown(orc):
    from oracle_pipeline import OraclePipeline
    from test_golden import G, run_golden_stream
    fx, fy, cx, cy = [float(v) for v in G["intr"]]
    h, w = G["depth"].shape[1:]
    po = OraclePipeline(w, h, fx, fy, cx, cy, 30000, small_pre(w))
    run_golden_stream(po)
    m = mr.map_of_rows(po.recon.surfels(), po.recon.surfels_size)
    return m, mr.triangulate(*m)[0]


def _run(fixture, cell):
    (pos, _, r2), tri = fixture
    out, vmap, st = dr.decimate(pos, r2, tri, cell)
    print("cell %g: %s" % (cell, st))
    dr.check_properties(out, vmap, st)
    assert out.dtype == np.uint32 and vmap.dtype == np.uint32 and vmap.shape == (pos.shape[0],)
    return out, vmap, st


def test_sphere(sphere):
    assert sphere[1].shape[0] == 6739
    out, vmap, st = _run(sphere, 0.1)
    assert st == dict(n_in=6739, n_not_live=0, n_used_vertices=3995, n_cells=1345, n_collapsed=4614, n_duplicates=13, n_triangles=2112)
    _, _, st = _run(sphere, 0.03)
    assert st == dict(n_in=6739, n_not_live=0, n_used_vertices=3995, n_cells=3525, n_collapsed=680, n_duplicates=0, n_triangles=6059)
    out4, _, st = _run(sphere, 4.0)
    assert st["n_cells"] == 8 and st["n_triangles"] == 9
    # what is not promised: an edge may lie in more than two triangles
    edges = np.sort(np.concatenate([out[:, [0, 1]], out[:, [1, 2]], out[:, [0, 2]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert int(np.sum(counts > 2)) == 21
    # a second, coarser level on the output: the representatives of 0.1 are the used vertices of the next call
    pos, _, r2 = sphere[0]
    out2, vmap2, st2 = dr.decimate(pos, r2, out, 0.2)
    dr.check_properties(out2, vmap2, st2)
    assert st2["n_in"] == 2112 and st2["n_used_vertices"] <= 1345 and 0 < st2["n_triangles"] < 2112


def test_plane(plane):
    (pos, _, r2), tri = plane
    out, vmap, st = _run(plane, 0.5)
    assert st["n_cells"] == st["n_used_vertices"] and st["n_collapsed"] == 0 and st["n_duplicates"] == 0
    assert out.tobytes() == tri.tobytes()          # every vertex alone in its cell
    used = np.unique(tri)
    assert np.array_equal(vmap[used], used)
    _, _, st = _run(plane, 2.0)
    assert st["n_cells"] == 429 and st["n_duplicates"] == 1 and st["n_triangles"] == 766
    with pytest.raises(dr.CellRangeError):
        dr.decimate(pos, r2, tri, 1e-5)


def test_grown_map(grown):
    _, _, st = _run(grown, 0.05)
    assert st["n_cells"] == 2855 and st["n_triangles"] == 5349
    _, _, st = _run(grown, 0.1)
    assert st["n_cells"] == 766 and st["n_triangles"] == 1343


def test_by_hand():
    # slots 0-3: four points at (+-0.25, +-0.25, 0) + 0.5 in the unit cell (0, 0, 0), all at the same distance from its
    # centre: the lowest slot wins.  Slots 4, 5 and 6, 7: one point each in cells of their own; 8 is merged, 9 unused.
    pos = np.array([[0.75, 0.75, 0.5], [0.25, 0.75, 0.5], [0.25, 0.25, 0.5], [0.75, 0.25, 0.5],
                    [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [2.5, 0.5, 0.5], [2.5, 1.5, 0.5], [1.5, 1.5, 0.5], [9.0, 9.0, 9.0]])
    r2 = np.ones(10)
    r2[8] = -1.0
    tri = np.array([[3, 4, 5],      # -> (0, 4, 5)
                    [0, 2, 4],      # two corners in one cell: collapsed
                    [5, 4, 2],      # -> (5, 4, 0) = (0, 5, 4): the corners of the first in the opposite winding, later: dropped
                    [4, 8, 5],      # a corner that is not live
                    [7, 6, 4],      # -> (4, 7, 6)
                    [4, 5, 1]],     # -> (4, 5, 0) = (0, 4, 5): the same winding, later: dropped too
                   np.uint32)
    out, vmap, st = dr.decimate(pos, r2, tri, 1.0)
    dr.check_properties(out, vmap, st)
    assert out.tolist() == [[0, 4, 5], [4, 7, 6]]
    assert vmap.tolist() == [0, 0, 0, 0, 4, 5, 6, 7, 0xFFFFFFFF, 0xFFFFFFFF]
    assert st == dict(n_in=6, n_not_live=1, n_used_vertices=8, n_cells=5, n_collapsed=1, n_duplicates=2, n_triangles=2)
    # the other order of the two windings: the earlier one stays, whichever it is
    out, vmap, _ = dr.decimate(pos, r2, tri[[2, 0]], 1.0)
    assert out.tolist() == [[2, 5, 4]] and vmap[:4].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 2, 2]      # (of U: slots 0 and 1 are in no triangle)
    # nothing in, nothing out; bad arguments
    out, vmap, st = dr.decimate(pos, r2, np.zeros((0, 3), np.uint32), 1.0)
    assert out.shape == (0, 3) and np.all(vmap == 0xFFFFFFFF) and st["n_triangles"] == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dr.decimate(pos, r2, tri, bad)
    with pytest.raises(ValueError):
        dr.decimate(pos, r2, np.array([[0, 1, 10]], np.uint32), 1.0)
