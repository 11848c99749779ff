"""The arithmetic of smx_decimate.hip without a GPU: smx_decimate.hpp holds the cell coordinate, key, centre, d2, value
word, hashes and the canonical rotation as plain inline functions, so the harness of tests/decimate_host.py compiles them
for the host with the project's -ffp-contract=off and walks the passes of the kernels one "lane" after the other -- the same
two open-addressing tables, with a compare-and-swap and a minimum that one lane at a time makes trivial -- here in forward
and in reverse lane order on the maps of the device tests.  The output has to equal the model of tests/decimate_ref.py
exactly, as on the device.  (The hand-built cases: tests/test_decimate_cases.py.)"""
import numpy as np
import pytest

import decimate_host as dh
import decimate_ref as dr
import mesh_ref as mr
from common import small_pre
from decimate_host import host_decimate


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return dh.host_library(tmp_path_factory.mktemp("decimate_host"))


def _compare(L, m, tri, cell, what):
    pos, _, r2 = m
    want, wmap, wst = dr.decimate(pos, r2, tri, cell)
    for reverse in (0, 1):
        got, vmap, st = host_decimate(L, pos, r2, tri, cell, reverse)
        print("%s, cell %g, lanes %s: %s" % (what, cell, "downwards" if reverse else "upwards", st))
        assert st == wst and got.tobytes() == want.tobytes() and vmap.tobytes() == wmap.tobytes()
    return wst


def test_sphere_on_the_host(host):
    m = mr.sphere_map()
    tri = mr.triangulate(*m)[0]
    assert _compare(host, m, tri, 0.03, "sphere")["n_triangles"] == 6059
    assert _compare(host, m, tri, 0.1, "sphere")["n_triangles"] == 2112
    # a stale array: a tenth of the slots merged
    r2 = m[2].copy()
    r2[::10] = -1.0
    assert _compare(host, (m[0], m[1], r2), tri, 0.1, "sphere, stale")["n_not_live"] > 0


def test_plane_on_the_host(host):
    m = mr.plane_map()
    tri = mr.triangulate(*m)[0]
    assert _compare(host, m, tri, 2.0, "plane")["n_triangles"] == 766
    assert host_decimate(host, m[0], m[2], tri, 1e-5)[0] == -2           # the coordinate range
    bad = tri.copy()
    bad[5, 1] = m[0].shape[0]
    assert host_decimate(host, m[0], m[2], bad, 2.0)[0] == -1


def test_oracle_grown_map_on_the_host(host, orc):
    from oracle_pipeline import OraclePipeline
    from test_golden import G, run_golden_stream
    fx, fy, cx, cy = [float(v) for v in G["intr"]]
    h, w = G["depth"].shape[1:]
    po = OraclePipeline(w, h, fx, fy, cx, cy, 30000, small_pre(w))
    run_golden_stream(po)
    m = mr.map_of_rows(po.recon.surfels(), po.recon.surfels_size)
    tri = mr.triangulate(*m)[0]
    assert _compare(host, m, tri, 0.05, "grown map")["n_triangles"] == 5349
