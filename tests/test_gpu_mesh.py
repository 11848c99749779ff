"""smx_recon_triangulate on the device: against the global Delaunay triangulation of planar maps (independent of the
model), against the float64 / Qhull model of tests/mesh_ref.py on a noisy sphere and on a grown map, and the properties,
determinism, capacity and compaction rules of include/smx.h.  Set comparisons allow a symmetric difference of at most
ceil(0.001 T_reference) triangles (float32 against float64 signs on near-cocircular quadruples; mesh_ref.assert_sets_close
prints what differs); the property checks apply to every output in full."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as mr

pytestmark = pytest.mark.gpu


def _pod(smx, prm):
    from surfelmeshing_amd._lib import MeshParams
    return MeshParams.defaults(max_angle_between_normals_deg=prm.max_angle_between_normals_deg,
                               min_triangle_angle_deg=prm.min_triangle_angle_deg,
                               max_triangle_angle_deg=prm.max_triangle_angle_deg,
                               search_radius_factor=prm.search_radius_factor, max_neighbors=prm.max_neighbors)


def _rec_of(smx, pos, nrm, r2, spare=1000):
    rows = mr.rows_of_map(pos, nrm, r2)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(160, 120, 131.25, 131.25, 80.0, 60.0))
    rec.debug_upload_surfels(rows, int(np.sum(r2 < 0)))
    return rec


def _mesh(smx, rec, prm, cell_size=None):
    tri, stats = rec.Triangulate(None, _pod(smx, prm), cell_size=cell_size)
    assert tri.dtype == np.uint32 and tri.shape == (stats["n_triangles"], 3)
    return tri, stats


def _against_model(smx, rec, pos, nrm, r2, prm, what, cell_size=None):
    got, st = _mesh(smx, rec, prm, cell_size)
    want, wst, want_stars = mr.triangulate(pos, nrm, r2, prm)
    print("%s: GPU %s, model %s" % (what, st, wst))
    assert want.shape[0] > 100
    d = mr.assert_sets_close(got, want, what)
    mr.check_properties(got, pos, nrm, r2, prm)
    assert st["n_live"] == wst["n_live"] and st["star_overflow"] == wst["star_overflow"]
    assert st["truncated_lists"] == wst["truncated_lists"]
    assert abs(st["n_star_triangles"] - wst["n_star_triangles"]) <= int(np.ceil(0.001 * wst["n_star_triangles"]))
    if d == 0:
        assert np.array_equal(got, want)          # the same set: then the same array, order and winding included
    return got, st


@pytest.mark.parametrize("side", [40, 1100])
def test_plane_against_the_global_delaunay_triangulation(smx, side):
    pos, nrm, r2 = mr.plane_map(side=side)
    rec = _rec_of(smx, pos, nrm, r2)
    cell = 2.5      # (the map's unit is the grid spacing; results do not depend on the cell size)
    open_prm = mr.Params(**mr.NO_ANGLE_LIMITS)
    got, st = _mesh(smx, rec, open_prm, cell)
    want = mr.global_delaunay_short(pos, r2)
    if side == 40:
        assert want.shape[0] == 3079
    mr.assert_sets_close(got, want, "plane %d, angle limits open" % side)
    mr.check_properties(got, pos, nrm, r2, open_prm)
    assert st["n_live"] == side * side and st["star_overflow"] == 0 and st["truncated_lists"] == 0
    assert st["n_star_triangles"] >= st["n_triangles"] == got.shape[0]
    got, st = _mesh(smx, rec, mr.Params(), cell)
    want = mr.global_delaunay_short(pos, r2, nrm, mr.Params())
    mr.assert_sets_close(got, want, "plane %d, default limits" % side)
    mr.check_properties(got, pos, nrm, r2, mr.Params())
    # the cell size of the index changes nothing
    again, _ = _mesh(smx, rec, mr.Params(), 4.0)
    assert np.array_equal(again, got)
    rec.close()


def test_sphere_against_the_model_with_default_and_other_parameters(smx):
    pos, nrm, r2 = mr.sphere_map()
    rec = _rec_of(smx, pos, nrm, r2)
    _against_model(smx, rec, pos, nrm, r2, mr.Params(), "sphere")
    _against_model(smx, rec, pos, nrm, r2, mr.Params(search_radius_factor=1.5), "sphere, factor 1.5")
    _, st = _against_model(smx, rec, pos, nrm, r2, mr.Params(search_radius_factor=1.5, max_neighbors=16), "sphere, 16 neighbours")
    assert st["truncated_lists"] > 0
    _against_model(smx, rec, pos, nrm, r2, mr.Params(max_angle_between_normals_deg=30.0), "sphere, 30 degrees")
    got, _ = _against_model(smx, rec, pos, nrm, r2, mr.Params(max_angle_between_normals_deg=5.0), "sphere, 5 degrees")
    assert got.shape[0] < 6000      # (a threshold that does drop candidates)
    rec.close()


def _grown(smx):
    from common import small_stream
    from test_gpu_parity import _pipes
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    _, pg = _pipes(smx, s, 60000)
    for f in range(0, 38):
        pg.upload(f, *s.frame(f))
    for f in range(4, 34):
        pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    rec = pg.reconstruction
    assert rec.stats()["merge_count"] > 0
    return pg, rec


def test_grown_map_against_the_model_and_across_a_compaction(smx):
    pg, rec = _grown(smx)
    n = rec.surfels_size()
    pos, nrm, r2 = mr.map_of_rows(rec.debug_download_surfels(n), n)
    assert np.any(r2 < 0)
    got, st = _against_model(smx, rec, pos, nrm, r2, mr.Params(), "grown map")
    assert np.all(r2[got.astype(np.int64)] >= 0)                  # merged slots never appear
    assert st["n_live"] == rec.surfel_count()
    # determinism: the same bytes and counts
    again, st2 = _mesh(smx, rec, mr.Params())
    assert again.tobytes() == got.tobytes() and st2 == st
    # a passed-in index is rebuilt and gives the same
    nn = smx.SurfelNeighborIndex()
    third, _ = rec.Triangulate(None, None, index=nn)
    assert np.array_equal(third, got)
    # after a compaction: exactly the previous array through old_to_new (slot order is kept, so is the array order)
    old_to_new, new_size, _ = rec.Compact(None)
    assert new_size < n
    after, st3 = rec.Triangulate(None, None, index=nn)
    nn.close()
    assert np.array_equal(after, old_to_new[got.astype(np.int64)])
    assert st3["n_live"] == st["n_live"] == new_size and st3["n_triangles"] == st["n_triangles"]
    pos2, nrm2, r22 = mr.map_of_rows(rec.debug_download_surfels(new_size), new_size)
    mr.check_properties(after, pos2, nrm2, r22)


def test_capacity_rule_and_guard_words(smx):
    from surfelmeshing_amd import _lib
    pos, nrm, r2 = mr.sphere_map(n=1500)
    rec = _rec_of(smx, pos, nrm, r2)
    ref, _ = _mesh(smx, rec, mr.Params())
    T = ref.shape[0]
    assert T > 1000
    L, nn, p = _lib.load(), smx.SurfelNeighborIndex(), _lib.MeshParams.defaults()

    def call(buf, capacity):
        n, st = C.c_uint32(0), _lib.MeshStats()
        rc = L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p),
                                     buf.ctypes.data_as(C.c_void_p) if buf is not None else None, C.c_uint32(capacity),
                                     C.c_int32(0), C.byref(n), C.byref(st))
        return rc, n.value, st
    guard = 0xA5A5A5A5
    rc, n, st = call(None, 0)                                     # the count-only form
    assert rc == -1 and n == T and st.n_triangles == T
    buf = np.full(3 * T + 8, guard, np.uint32)
    rc, n, _ = call(buf, 0)
    assert rc == -1 and n == T and np.all(buf == guard)           # nothing is written
    rc, n, _ = call(buf, T - 1)
    assert rc == -1 and n == T and np.all(buf == guard)
    rc, n, _ = call(buf, T)
    assert rc == 0 and n == T
    assert np.array_equal(buf[:3 * T].reshape(T, 3), ref) and np.all(buf[3 * T:] == guard)
    # the device-pointer form writes the same bytes, and nothing behind them
    dbuf = smx.CUDABuffer(1, 3 * T + 8, np.uint32)
    dbuf.Upload(np.full((1, 3 * T + 8), guard, np.uint32))
    n = C.c_uint32(0)
    _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dbuf.ToCUDA().address),
                                       C.c_uint32(T), C.c_int32(1), C.byref(n), None))
    back = dbuf.Download()[0]
    assert n.value == T and np.array_equal(back[:3 * T].reshape(T, 3), ref) and np.all(back[3 * T:] == guard)
    # bad parameters are refused by the library itself
    for bad in (dict(max_neighbors=65), dict(max_neighbors=0), dict(search_radius_factor=0.5), dict(search_radius_factor=2.5),
                dict(max_star_degree=8), dict(min_triangle_angle_deg=120.0, max_triangle_angle_deg=60.0)):
        with pytest.raises(_lib.SmxError):
            rec.Triangulate(None, _lib.MeshParams.defaults(**bad), index=nn)
    t = rec.debug_mesh_timings()
    assert set(t) == {"index_build", "list_query", "star", "agree_write"} and all(v >= 0 for v in t.values())
    nn.close()
    dbuf.close()
    rec.close()


def test_empty_and_all_merged_maps_give_no_triangles(smx):
    rec = smx.CUDASurfelReconstruction(1000, smx.PinholeCamera4f(160, 120, 131.25, 131.25, 80.0, 60.0))
    tri, st = rec.Triangulate(None)
    assert tri.shape == (0, 3) and st["n_live"] == 0
    pos, nrm, r2 = mr.plane_map(side=8)
    rec.debug_upload_surfels(mr.rows_of_map(pos, nrm, np.full(64, -1.0)), 64)
    tri, st = rec.Triangulate(None, cell_size=2.5)
    assert tri.shape == (0, 3) and st["n_live"] == 0 and st["n_star_triangles"] == 0
    rec.close()
