"""smx_recon_decimate_mesh on the device.  The contract (include/smx.h) is made of integers and of float32 expressions that
numpy reproduces bit for bit, so everything here is compared for EQUALITY with the model of tests/decimate_ref.py: the
triangle array, the vertex map and every statistic.  The inputs are what smx_recon_triangulate returns on the uploaded map."""
import ctypes as C

import numpy as np
import pytest

import decimate_ref as dr
import mesh_ref as mr

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


def _equals_model(rec, pos, r2, tri, cell, what):
    got, st, vmap = rec.DecimateMesh(None, tri, cell, return_vertex_map=True)
    want, wmap, wst = dr.decimate(pos, r2, tri, cell)
    print("%s, cell %g: GPU %s" % (what, cell, st))
    assert got.dtype == np.uint32 and got.shape == (st["n_triangles"], 3)
    assert st == wst
    assert got.tobytes() == want.tobytes()
    assert vmap.tobytes() == wmap.tobytes()
    dr.check_properties(got, vmap, st)
    return got, st, vmap


@pytest.fixture(scope="module")
def sphere(smx):
    m = mr.sphere_map()
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    assert tri.shape[0] > 6000
    yield m, rec, tri
    rec.close()


@pytest.fixture(scope="module")
def plane(smx):
    m = mr.plane_map()
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None, cell_size=2.5)
    assert tri.shape[0] > 3000
    yield m, rec, tri
    rec.close()


def _raw(rec, cell, tin, n_in, out, capacity, vmap, on_device=0):
    """The C call itself; tin / out / vmap: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    n, st = C.c_uint32(0xDEAD), _lib.DecimateStats()
    rc = _lib.load().smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), ptr(tin), C.c_uint32(n_in), ptr(out),
                                             C.c_uint32(capacity), ptr(vmap), C.c_int32(on_device), C.byref(n), C.byref(st))
    return rc, n.value, st


@pytest.mark.parametrize("cell", [0.03, 0.1, 4.0])
def test_sphere_equals_the_model(sphere, cell):
    (pos, _, r2), rec, tri = sphere
    _, st, _ = _equals_model(rec, pos, r2, tri, cell, "sphere")
    if cell == 4.0:
        assert st["n_cells"] == 8
    else:
        assert 1000 < st["n_cells"] < st["n_used_vertices"] and st["n_collapsed"] > 0


@pytest.mark.parametrize("cell", [0.5, 2.0])
def test_plane_equals_the_model(plane, cell):
    (pos, _, r2), rec, tri = plane
    got, st, _ = _equals_model(rec, pos, r2, tri, cell, "plane")
    if cell == 0.5:      # every vertex alone in its cell: the input comes back byte for byte
        assert got.tobytes() == tri.tobytes() and st["n_cells"] == st["n_used_vertices"]
    else:
        assert st["n_duplicates"] > 0


def test_grown_map_equals_the_model(smx):
    from test_gpu_mesh import _grown
    pg, rec = _grown(smx)
    n = rec.surfels_size()
    pos, _, r2 = mr.map_of_rows(rec.debug_download_surfels(n), n)
    assert np.any(r2 < 0)
    tri, _ = rec.Triangulate(None)
    assert tri.shape[0] > 10000
    rows_before, stats_before = rec.debug_download_surfels(n), rec.stats()
    _, st, _ = _equals_model(rec, pos, r2, tri, 0.05, "grown map")
    assert st["n_not_live"] == 0 and st["n_collapsed"] > 0 and st["n_triangles"] > 1000
    # the call changes no map state and no statistic
    assert rec.stats() == stats_before and rec.surfels_size() == n
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()


def test_large_plane_across_workgroups_sort_tiles_and_probe_chains(smx):
    m = mr.plane_map(side=300)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None, cell_size=2.5)
    assert tri.shape[0] > 170000          # hundreds of workgroups, dozens of sort tiles in, a dozen out
    _, st, _ = _equals_model(rec, m[0], m[2], tri, 2.0, "plane 300")
    assert st["n_cells"] > 20000 and st["n_triangles"] > 2048 * 8
    rec.close()


def test_host_and_device_arrays_two_calls_and_a_second_level(smx, sphere):
    (pos, _, r2), rec, tri = sphere
    got, st, vmap = _equals_model(rec, pos, r2, tri, 0.1, "sphere")
    again, st2, vmap2 = rec.DecimateMesh(None, tri, 0.1, return_vertex_map=True)
    assert again.tobytes() == got.tobytes() and st2 == st and vmap2.tobytes() == vmap.tobytes()
    # the device-pointer form: the same bytes, nothing behind them
    T, n_in, n = got.shape[0], tri.shape[0], pos.shape[0]
    din, dout, dmap = (smx.CUDABuffer(1, k, np.uint32) for k in (3 * n_in, 3 * T + 8, n + 8))
    din.Upload(tri.reshape(1, -1))
    dout.Upload(np.full((1, 3 * T + 8), GUARD, np.uint32))
    dmap.Upload(np.full((1, n + 8), GUARD, np.uint32))
    rc, nt, dst = _raw(rec, 0.1, din.ToCUDA().address, n_in, dout.ToCUDA().address, T, dmap.ToCUDA().address, on_device=1)
    assert rc == 0 and nt == T and {k: int(getattr(dst, k)) for k in st} == st
    back, mback = dout.Download()[0], dmap.Download()[0]
    assert back[:3 * T].tobytes() == got.tobytes() and np.all(back[3 * T:] == GUARD)
    assert mback[:n].tobytes() == vmap.tobytes() and np.all(mback[n:] == GUARD)
    assert din.Download()[0].tobytes() == tri.tobytes()          # the input is left alone
    for b in (din, dout, dmap):
        b.close()
    # a second level: the output of 0.1 decimated at 0.2
    second, st3, _ = _equals_model(rec, pos, r2, got, 0.2, "sphere, second level")
    assert st3["n_in"] == T and st3["n_not_live"] == 0 and 0 < second.shape[0] < T
    t = rec.debug_decimate_timings()
    assert set(t) == {"cluster", "remap_dedupe", "survivors", "order"} and all(np.isfinite(v) and v >= 0 for v in t.values())


def test_capacity_rule_count_only_and_empty_input(sphere):
    (pos, _, r2), rec, tri = sphere
    want, wmap, wst = dr.decimate(pos, r2, tri, 0.1)
    T, n_in, n = want.shape[0], tri.shape[0], pos.shape[0]
    out, vmap = np.full(3 * T + 8, GUARD, np.uint32), np.full(n + 8, GUARD, np.uint32)
    rc, nt, st = _raw(rec, 0.1, tri, n_in, out, T - 1, vmap)
    assert rc == -1 and nt == T and st.n_triangles == T and st.n_cells == wst["n_cells"]
    assert np.all(out == GUARD) and np.all(vmap == GUARD)         # nothing is written
    rc, nt, st = _raw(rec, 0.1, tri, n_in, None, 0, None)          # the count-only form
    assert rc == -1 and nt == T and st.n_duplicates == wst["n_duplicates"]
    rc, nt, st = _raw(rec, 0.1, tri, n_in, out, T, vmap)
    assert rc == 0 and nt == T
    assert out[:3 * T].tobytes() == want.tobytes() and np.all(out[3 * T:] == GUARD)
    assert vmap[:n].tobytes() == wmap.tobytes() and np.all(vmap[n:] == GUARD)
    rc, nt, st = _raw(rec, 0.1, tri, n_in, out, T + 2, None)       # room to spare, no vertex map
    assert rc == 0 and nt == T and np.all(out[3 * T:] == GUARD)
    # n_in = 0: valid, nothing out, nobody is used
    vmap[:] = GUARD
    rc, nt, st = _raw(rec, 0.1, None, 0, out, T, vmap)
    assert rc == 0 and nt == 0 and st.n_in == 0 and st.n_used_vertices == 0
    assert np.all(vmap[:n] == 0xFFFFFFFF) and np.all(vmap[n:] == GUARD)
    got, st = rec.DecimateMesh(None, np.zeros((0, 3), np.uint32), 0.1)
    assert got.shape == (0, 3) and st["n_triangles"] == 0


def test_refusals_write_nothing(smx, sphere, plane):
    from surfelmeshing_amd import _lib
    (pos, _, r2), rec, tri = sphere
    n_in, n = tri.shape[0], pos.shape[0]
    out, vmap = np.full(3 * n_in + 8, GUARD, np.uint32), np.full(n + 8, GUARD, np.uint32)

    def refused(rc):
        assert rc == -1 and np.all(out == GUARD) and np.all(vmap == GUARD)
    # an index >= surfels_size(), anywhere
    for where in (0, 3 * (n_in // 2) + 1, 3 * n_in - 1):
        bad = tri.copy()
        bad.reshape(-1)[where] = n
        refused(_raw(rec, 0.1, bad, n_in, out, n_in, vmap)[0])
        assert b"index" in _lib.load().smx_last_error()
    # cell_size of 0, negative, NaN or infinite
    for cell in (0.0, -0.1, float("nan"), float("inf")):
        refused(_raw(rec, cell, tri, n_in, out, n_in, vmap)[0])
    with pytest.raises(_lib.SmxError):
        rec.DecimateMesh(None, tri, 0.0)
    # overlapping in and out (host pointers here: the same array, and one that starts inside it)
    both = tri.copy()
    rc, _, _ = _raw(rec, 0.1, both, n_in, both, n_in, None)
    assert rc == -1 and both.tobytes() == tri.tobytes()
    rc, _, _ = _raw(rec, 0.1, both, n_in, both.reshape(-1)[3 * (n_in - 1):], 1, None)
    assert rc == -1 and both.tobytes() == tri.tobytes()
    # the coordinate range: the plane (extent 40) at a cell of 1e-5
    (ppos, _, pr2), prec, ptri = plane
    pout, pmap = np.full(3 * ptri.shape[0], GUARD, np.uint32), np.full(ppos.shape[0], GUARD, np.uint32)
    rc, _, _ = _raw(prec, 1e-5, ptri, ptri.shape[0], pout, ptri.shape[0], pmap)
    assert rc == -1 and np.all(pout == GUARD) and np.all(pmap == GUARD)
    assert b"too small" in _lib.load().smx_last_error()
    with pytest.raises(dr.CellRangeError):
        dr.decimate(ppos, pr2, ptri, 1e-5)


def test_stale_array_and_compaction(smx):
    m = mr.sphere_map()
    pos, nrm, r2 = m
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    # a tenth of the slots merged since the array was made
    r2m = r2.copy()
    r2m[np.random.default_rng(3).permutation(pos.shape[0])[:pos.shape[0] // 10]] = -1.0
    rec.debug_upload_surfels(mr.rows_of_map(pos, nrm, r2m), int(np.sum(r2m < 0)))
    got, st, _ = _equals_model(rec, pos, r2m, tri, 0.1, "stale array")
    assert st["n_not_live"] > 500 and np.all(r2m[got.astype(np.int64)] >= 0)
    # after a compaction: the (still valid part of the) input through old_to_new, against the model on the compacted map
    old_to_new, new_size, _ = rec.Compact(None)
    assert new_size == pos.shape[0] - pos.shape[0] // 10
    kept = tri[np.all(r2m[tri.astype(np.int64)] >= 0, axis=1)]
    mapped = old_to_new[kept.astype(np.int64)]
    pos2, _, r22 = mr.map_of_rows(rec.debug_download_surfels(new_size), new_size)
    after, st2, _ = _equals_model(rec, pos2, r22, mapped, 0.1, "compacted")
    assert st2["n_not_live"] == 0 and st2["n_triangles"] == st["n_triangles"]
    assert after.tobytes() == old_to_new[got.astype(np.int64)].tobytes()      # slot order is kept, so is everything else
    rec.close()


def test_independent_of_the_incremental_mesher(smx):
    m = mr.sphere_map()
    rec = _rec_of(smx, m)
    nn = smx.SurfelNeighborIndex()
    tri, st, us = rec.TriangulateUpdate(None, index=nn)
    assert us["mode"] == 1
    rec.DecimateMesh(None, tri, 0.1)
    again, st2, us2 = rec.TriangulateUpdate(None, index=nn)
    assert us2["mode"] == 0 and us2["n_changed"] == 0 and again.tobytes() == tri.tobytes() and st2 == st
    nn.close()
    rec.close()


def test_map_mesher_decimates_beside_the_full_mesh_and_export_uses_only_referenced_vertices(smx, tmp_path):
    from surfelmeshing_amd import export, meshing
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    mesher = meshing.MapMesher(rec)
    assert len(mesher.update()) == 3 and mesher.decimated is None
    tri, _, _, coarse = mesher.update(cell_size=0.2)
    want, _, wst = dr.decimate(m[0], m[2], tri, 0.2)
    assert coarse.tobytes() == want.tobytes() and mesher.decimate_stats == wst
    assert meshing.decimate_map_mesh(rec, tri, 0.2)[0].tobytes() == want.tobytes()
    path = str(tmp_path / "coarse.obj")
    export.SaveMeshAsOBJ(rec, path, triangles=coarse, referenced_only=True)
    lines = open(path).read().split("\n")
    n_v, faces = sum(ln.startswith("v ") for ln in lines), [ln.split()[1:] for ln in lines if ln.startswith("f ")]
    assert n_v == wst["n_cells"] == np.unique(coarse).size and len(faces) == coarse.shape[0]
    assert {int(v) for f in faces for v in f} == set(range(1, n_v + 1))
    mesher.close()
    rec.close()


def test_memory_returns_after_destroy(smx):
    before = smx.DebugLiveAllocations()
    m = mr.plane_map(side=20)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None, cell_size=2.5)
    held = smx.DebugLiveAllocations()
    rec.DecimateMesh(None, tri, 2.0)
    assert smx.DebugLiveAllocations()[0] > held[0]              # the workspace belongs to the object ...
    grown = smx.DebugLiveAllocations()
    rec.DecimateMesh(None, tri, 3.0)
    assert smx.DebugLiveAllocations() == grown                  # ... is reused ...
    rec.close()
    assert smx.DebugLiveAllocations() == before                 # ... and goes with it
