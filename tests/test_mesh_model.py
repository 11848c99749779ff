"""The model of tests/mesh_ref.py against what it must reproduce without any kernel: the global Delaunay triangulation
of a planar map, the two-triangles-per-edge property on a noisy sphere, and the output order and winding rules."""
import numpy as np

import mesh_ref as mr


def test_model_reproduces_the_global_delaunay_triangulation_of_a_plane():
    pos, nrm, r2 = mr.plane_map()
    # all of them with the angle limits open (the limits cut slivers along the hull, which the global triangulation has)
    tri, stats, _ = mr.triangulate(pos, nrm, r2, mr.Params(**mr.NO_ANGLE_LIMITS))
    want = mr.global_delaunay_short(pos, r2)
    assert want.shape[0] == 3079
    assert mr.as_set(tri) == mr.as_set(want)
    # ... and with the default limits exactly those of them that pass the limits
    tri, stats, _ = mr.triangulate(pos, nrm, r2)
    want = mr.global_delaunay_short(pos, r2, nrm, mr.Params())
    assert 3000 < want.shape[0] < 3079
    assert mr.as_set(tri) == mr.as_set(want)
    assert stats["n_live"] == 1600 and stats["star_overflow"] == 0 and stats["truncated_lists"] == 0
    assert stats["n_star_triangles"] >= stats["n_triangles"] == tri.shape[0]
    mr.check_properties(tri, pos, nrm, r2)


def test_model_on_a_noisy_sphere_keeps_edges_manifold():
    pos, nrm, r2 = mr.sphere_map()
    tri, stats, _ = mr.triangulate(pos, nrm, r2)
    print("sphere: %d star triangles, %d agreed (%.1f %%), overflow %d, truncated %d" % (
        stats["n_star_triangles"], tri.shape[0], 100.0 * tri.shape[0] / stats["n_star_triangles"], stats["star_overflow"],
        stats["truncated_lists"]))
    assert tri.shape[0] > 0.7 * stats["n_star_triangles"] > 4000
    mr.check_properties(tri, pos, nrm, r2)      # (at most two triangles per edge among them)
    # the same input rounded differently gives the same mesh: nothing here hangs on a last bit
    tri2, _, _ = mr.triangulate(pos.astype(np.float32).astype(np.float64), nrm, r2)
    assert np.array_equal(tri, tri2)


def test_output_order_and_winding():
    pos, nrm, r2 = mr.plane_map(side=8)
    tri, _, _ = mr.triangulate(pos, nrm, r2)
    assert tri.dtype == np.uint32 and tri.shape[0] > 50
    assert np.all(tri[:, 0] < tri[:, 1]) and np.all(tri[:, 0] < tri[:, 2])
    assert [tuple(t) for t in tri] == sorted(tuple(t) for t in tri)
    P = pos[tri.astype(np.int64)]
    z = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])[:, 2]
    assert np.all(z > 0)                       # counter-clockwise seen from +z, where the normals point
    tri_down, _, _ = mr.triangulate(pos, -nrm, r2)
    assert mr.as_set(tri_down) == mr.as_set(tri)
    Pd = pos[tri_down.astype(np.int64)]
    assert np.all(np.cross(Pd[:, 1] - Pd[:, 0], Pd[:, 2] - Pd[:, 0])[:, 2] < 0)
    # merged and non-finite slots are not part of anything
    r2m, posm = r2.copy(), pos.copy()
    r2m[10] = -1.0
    posm[20, 1] = np.nan
    tri_m, stats, _ = mr.triangulate(posm, nrm, r2m)
    assert stats["n_live"] == 62 and not np.isin(tri_m, [10, 20]).any()
    # parameters: a normal threshold nobody passes leaves nothing
    tri_none, _, _ = mr.triangulate(pos, nrm, r2, mr.Params(max_angle_between_normals_deg=1e-3))
    tilted = nrm.copy()
    tilted[::2] = [0.0, np.sin(0.1), np.cos(0.1)]
    assert mr.triangulate(pos, tilted, r2, mr.Params(max_angle_between_normals_deg=1.0))[0].shape[0] < tri.shape[0]
    assert tri_none.shape[0] == tri.shape[0]   # (identical normals: the angle between them is 0)
