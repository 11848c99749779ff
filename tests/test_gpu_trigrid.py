"""The shared build of the triangle grid at the sizes where it can go wrong: every case of
tests/trigrid_cases.py goes through smx_recon_mesh_distance, smx_recon_raycast_mesh and a scene on the same map, and each
result is compared byte for byte, statistics included, with the brute-force models of distance_ref.py and raycast_ref.py and
the numpy grids; an index out of range is refused by all three with one text, nothing written."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import mesh_ref as mr
import raycast_ref as rr
import rayscene_ref as sr
import trigrid_cases as tc

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
GRID = ("n_wide", "n_entries", "n_cells")
STEP1 = ("n_in", "n_not_live", "n_repeated", "n_out_of_range")


@pytest.fixture(scope="module")
def rec(smx):
    pos, nrm, r2, _ = tc.world()
    rows = mr.rows_of_map(pos, nrm, r2)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + 100, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(r2 < 0)))
    yield rec
    rec.close()


def _same_bytes(got, want, what):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


@pytest.mark.parametrize("name", list(tc.cases()))
def test_the_three_services_equal_the_models(rec, name):
    pos, nrm, r2, _ = tc.world()
    pts, rays = tc.queries()
    case = tc.cases()[name]
    tri, md = case["tri"], case["max_distance"]
    t0, t1 = tc.T_RANGE
    want_d = dr.answer(dr.brute(pos, r2, tri, pts), md, True)
    want_r = rr.answer(rr.brute(pos, r2, tri, rays, t0, t1), 0)
    for cs in case["cells"]:
        what = "%s cell %g" % (name, cs)
        # the distance: its own lower bound on c, the boxes as they are
        got = rec.MeshDistance(None, tri, pts, md, cs, True, return_closest=True)
        c = tc.distance_cell(pos, r2, tri, cs, md)
        wst = dict(want_d[3], cell_size_used=c, **dr.structure(pos, r2, tri, c, md))
        assert got[3] == wst, (what, got[3], wst)
        _same_bytes(got[:3], want_d[:3], what)
        # the ray caster and the scene: the other lower bound, the boxes inflated
        got = rec.RaycastMesh(None, tri, rays, t0, t1, cs, 0, return_uv=True)
        c = tc.raycast_cell(pos, r2, tri, cs)
        grid = rr.structure(pos, r2, tri, c)
        gst = dict(got[3])
        assert all(gst.pop(k) >= 0 for k in rr.WORK_NAMES)
        wst = dict(want_r[3], cell_size_used=c, **grid)
        assert gst == wst, (what, gst, wst)
        _same_bytes(got[:3], want_r[:3], what)
        g = sr.grid(pos, r2, tri, c)
        for occ in (0, 1):
            with rec.BuildRayScene(None, tri, cs, occ) as sc:
                bst = sc.stats
                assert {k: bst[k] for k in STEP1 + GRID} == {k: wst[k] for k in STEP1 + GRID} and bst["cell_size_used"] == c, (what, bst)
                k = bst["occupancy_log2"]
                assert k == 0 if occ == 1 else k in (-1, sr.smallest(g)), (what, bst)
                assert bst["n_blocks_set"] == (sr.blocks_set(g, k) if k >= 0 else 0), (what, bst)
                assert bst["occupancy_bytes"] == (4 * ((sr.bits(g, k) + 31) // 32) if k >= 0 else 0), (what, bst)
                hit, t, uv, cst = sc.Cast(None, rays, t0, t1, 0, return_uv=True)
                _same_bytes((hit, t, uv), want_r[:3], what)
                assert all(cst[k] == want_r[3][k] for k in ("n_rays", "n_bad_rays", "n_hit", "n_front_hits", "max_t_bits")), (what, cst)
                assert cst["n_layers"] == got[3]["n_layers"] and cst["n_pair_tests"] == got[3]["n_pair_tests"], (what, cst)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_an_index_out_of_range_is_refused_alike_by_all_three(smx, rec):
    from surfelmeshing_amd import _lib
    pos, nrm, r2, sheet = tc.world()
    pts, rays = tc.queries()
    bad = sheet[:257].copy()
    bad[192, 1] = pos.shape[0]                     # the first index past the map, in the fourth wavefront
    L, n_in, P = _lib.load(), bad.shape[0], pts.shape[0]
    texts = []

    def refused(rc):
        assert rc == -1
        texts.append(L.smx_last_error().decode())

    out = [np.full(P + 4, GUARD, np.uint32), np.full(P + 4, GUARD, np.uint32), np.full(3 * P + 4, GUARD, np.uint32)]
    prm, st = _lib.DistanceParams(tc.MAX_DISTANCE, 0.0, 1), _lib.DistanceStats()
    refused(L.smx_recon_mesh_distance(rec._h, None, C.byref(prm), _ptr(bad), C.c_uint32(n_in), _ptr(pts), C.c_uint32(P), _ptr(out[0]), _ptr(out[1]),
                                      _ptr(out[2]), C.c_int32(0), C.byref(st)))
    t = rec.debug_distance_timings()
    assert all(np.all(a == GUARD) for a in out) and t["mark"] >= 0 and t["index"] == t["query"] == t["stats"] == 0.0, t

    out = [np.full(P + 4, GUARD, np.uint32), np.full(P + 4, GUARD, np.uint32), np.full(2 * P + 4, GUARD, np.uint32)]
    prm, st = _lib.RaycastParams(*tc.T_RANGE, 0.0, 0), _lib.RaycastStats()
    refused(L.smx_recon_raycast_mesh(rec._h, None, C.byref(prm), _ptr(bad), C.c_uint32(n_in), _ptr(rays), C.c_uint32(P), _ptr(out[0]), _ptr(out[1]),
                                     _ptr(out[2]), C.c_int32(0), C.byref(st)))
    t = rec.debug_raycast_timings()
    assert all(np.all(a == GUARD) for a in out) and t["mark"] >= 0 and t["index"] == t["cast"] == t["stats"] == 0.0, t

    with rec.BuildRayScene(None, sheet[:257], 0.0, 0) as sc:
        want = sc.Cast(None, rays, *tc.T_RANGE)
        with pytest.raises(smx.SmxError) as e:
            rec.BuildRayScene(None, bad, 0.0, 0, scene=sc)
        texts.append(str(e.value).split(": ", 1)[1])
        t = sc.debug_timings()
        assert sc.stats is None and t["mark"] >= 0 and t["index"] == t["occupancy"] == 0.0, t
        with pytest.raises(smx.SmxError):
            sc.Cast(None, rays, *tc.T_RANGE)       # the refused build left the scene empty
        rec.BuildRayScene(None, sheet[:257], 0.0, 0, scene=sc)
        again = sc.Cast(None, rays, *tc.T_RANGE)
        assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes()
    assert len(set(texts)) == 1 and texts[0] == "triangles holds an index >= the %d slots of the map" % pos.shape[0], texts
