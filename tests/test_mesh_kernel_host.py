"""The arithmetic of smx_mesh.hip without a GPU: smx_mesh.hpp holds projection, in-circle test, star construction, ring
lookup and triangle filters as plain inline functions, so this test compiles them for the host with the project's
-ffp-contract=off, drives them the way k_mesh_star / k_mesh_agree do (a "lane" per candidate, a "lane" per slot), and
compares stars and accepted triangles with the float64 / Qhull model of tests/mesh_ref.py -- the comparison
tests/test_gpu_mesh.py makes on the device, with the same cap."""
import math

import numpy as np

import mesh_ref as mr
from common import small_pre
from mesh_host import host, host_triangulate  # noqa: F401  (the host build, shared with test_mesh_cases.py)


def _compare(L, pos, nrm, r2, prm, what):
    got, got_stars, st = host_triangulate(L, pos, nrm, r2, prm)
    want, wst, want_stars = mr.triangulate(pos, nrm, r2, prm)
    print("%s: model %d triangles of %d star triangles, host %d of %d" % (what, want.shape[0], len(want_stars), got.shape[0],
                                                                         len(got_stars)))
    assert want.shape[0] > 100
    star_diff = got_stars ^ want_stars
    assert len(star_diff) <= math.ceil(0.001 * len(want_stars)), sorted(sorted(t) for t in star_diff)[:20]
    d = mr.assert_sets_close(got, want, what)
    assert st["n_star_triangles"] == len(got_stars)
    assert st["star_overflow"] == wst["star_overflow"] and st["truncated_lists"] == wst["truncated_lists"]
    mr.check_properties(got, pos, nrm, r2, prm)
    if d == 0:      # the same set: then the same array, order and winding included
        assert np.array_equal(got, want)
    return got, wst


def test_plane_on_the_host(host):
    pos, nrm, r2 = mr.plane_map()
    got, _ = _compare(host, pos, nrm, r2, mr.Params(), "plane")
    assert mr.as_set(got) == mr.as_set(mr.global_delaunay_short(pos, r2, nrm, mr.Params()))
    got, _ = _compare(host, pos, nrm, r2, mr.Params(**mr.NO_ANGLE_LIMITS), "plane, no angle limits")
    assert got.shape[0] == 3079 and mr.as_set(got) == mr.as_set(mr.global_delaunay_short(pos, r2))


def test_sphere_on_the_host(host):
    pos, nrm, r2 = mr.sphere_map()
    _compare(host, pos, nrm, r2, mr.Params(), "sphere")
    _compare(host, pos, nrm, r2, mr.Params(search_radius_factor=1.5), "sphere, factor 1.5")
    _, st = _compare(host, pos, nrm, r2, mr.Params(max_neighbors=16, search_radius_factor=1.5), "sphere, 16 neighbours")
    assert st["truncated_lists"] > 0
    _compare(host, pos, nrm, r2, mr.Params(max_angle_between_normals_deg=30.0), "sphere, 30 degrees")
    _, st5 = _compare(host, pos, nrm, r2, mr.Params(max_angle_between_normals_deg=5.0), "sphere, 5 degrees")
    assert st5["n_triangles"] < 6000      # (a threshold that does drop candidates)


def test_oracle_grown_map_on_the_host(host, orc):
    from oracle_pipeline import OraclePipeline
    from test_golden import G, run_golden_stream
    fx, fy, cx, cy = [float(v) for v in G["intr"]]
    h, w = G["depth"].shape[1:]
    po = OraclePipeline(w, h, fx, fy, cx, cy, 30000, small_pre(w))
    run_golden_stream(po)
    n = po.recon.surfels_size
    assert po.recon.merge_count > 0
    pos, nrm, r2 = mr.map_of_rows(po.recon.surfels(), n)
    got, _ = _compare(host, pos, nrm, r2, mr.Params(), "grown map")
    assert np.all(r2[got.astype(np.int64)] >= 0)
    _compare(host, pos, nrm, r2, mr.Params(search_radius_factor=2.0), "grown map, factor 2")
