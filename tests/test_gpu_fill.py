"""smx_recon_fill_holes on the device.  The contract (include/smx.h) is made of integers and of float32 expressions that numpy
reproduces bit for bit, so everything here is compared for EQUALITY with the model of tests/fill_ref.py: the triangle
array, the table of listed loops and every statistic; the consequences of the contract's item 6 are asserted on every
output."""
import ctypes as C

import numpy as np
import pytest

import components_ref as cr
import decimate_ref as dr
import fill_cases as fc
import fill_ref as fr
import mesh_ref as mr

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
INVALID = 0xFFFFFFFF
PARAMS = [dict(), dict(min_triangle_angle_deg=1.0, max_triangle_angle_deg=179.0), dict(max_hole_edges=4), dict(max_hole_edges=32)]
IDS = lambda p: ",".join("%s=%s" % kv for kv in p.items()) or "default"      # noqa: E731


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def world(smx):
    """One map: the noisy sphere (slots 0 .. 3999, triangulated on the device) and the holed plane of tests/fill_cases.py with
    its islands, pinch, taken diagonal, third triangle on an edge and dead slot (scaled to the sphere's spacing, placed apart)."""
    sp, sn, sr = mr.sphere_map()
    pp, pn, pr, ptri = fc.holed_plane()
    pos = np.concatenate([sp, _f32(pp * 0.05 + np.array([3.0, 0.0, 0.0]))])
    nrm = np.concatenate([sn, pn])
    r2 = np.concatenate([sr, _f32(np.where(pr < 0, -1.0, pr * 0.0025))])
    m = (pos, nrm, r2)
    rec = _rec_of(smx, m)
    meshed, _ = rec.Triangulate(None)
    sphere = meshed[np.all(meshed < sp.shape[0], axis=1)]
    assert 6500 < sphere.shape[0] < 7000 and pos.shape[0] == 5624
    tri = np.ascontiguousarray(np.concatenate([sphere, ptri + np.uint32(sp.shape[0])]), np.uint32)
    yield dict(m=m, rec=rec, tri=tri, models={})
    rec.close()


def _model(world, tri, key=None, **p):
    """The model's answer, computed once per (array, parameters), shared and left unchanged."""
    k = (key, tuple(sorted(p.items())))
    if key is None or k not in world["models"]:
        ans = fr.fill(*world["m"], tri, **p)
        fr.check_properties(*world["m"], tri, *ans, **p)
        for a in (ans[0], ans[2]):
            a.setflags(write=False)
        if key is None:
            return ans
        world["models"][k] = ans
    return world["models"][k]


def _equals_model(world, tri, what, key=None, **p):
    got, st, holes = world["rec"].FillHoles(None, tri, return_holes=True, **p)
    want, wkept, wholes, wst = _model(world, tri, key, **p)
    kept = st.pop("n_kept")
    print("%s %s: GPU %s, kept %d; listed loop lengths %s" % (what, p, st, kept, np.bincount(holes["n_edges"], minlength=4)[3:].tolist()))
    assert got.dtype == np.uint32 and got.shape == (st["n_triangles"], 3)
    assert st == wst and kept == wkept
    assert holes.dtype.itemsize == 12 and holes.tobytes() == wholes.tobytes()
    assert got.tobytes() == want.tobytes()
    return got, kept, holes, st


@pytest.mark.parametrize("p", PARAMS, ids=IDS)
def test_one_map_with_everything_equals_the_model(world, p):
    got, kept, holes, st = _equals_model(world, world["tri"], "everything", key="all", **p)
    assert st["n_not_live"] > 0 and st["n_nonmanifold_edges"] == 1 and st["n_pinched_vertices"] > 100
    assert st["n_rejected_diagonal"] >= 1 and st["n_rejected_filter"] >= 3 and st["n_filled_loops"] >= 20
    if not p:
        assert st["n_listed_loops"] >= 100 and set(holes["n_edges"].tolist()) >= {3, 4, 5, 6, 8}
    if p == dict(max_hole_edges=32):
        assert int(holes["n_edges"].max()) == 32
    if p == dict(max_hole_edges=4):
        assert int(holes["n_edges"].max()) == 4


@pytest.mark.parametrize("order", ["shuffled", "reversed"])
def test_the_input_order_only_moves_the_kept_triangles(world, order):
    tri = world["tri"]
    arr = tri[::-1].copy() if order == "reversed" else tri[np.random.default_rng(5).permutation(tri.shape[0])]
    got, kept, holes, st = _equals_model(world, arr, order)
    want, wkept, wholes, _ = _model(world, tri, "all")
    live = fr.live_mask(world["m"][0].astype(np.float32), world["m"][2])
    assert holes.tobytes() == wholes.tobytes() and got[kept:].tobytes() == want[wkept:].tobytes()
    assert got[:kept].tobytes() == arr[np.all(live[arr.astype(np.int64)], axis=1)].tobytes()


def test_a_large_plane_with_many_holes(smx):
    """160 x 160 slots, a hole at every 8th interior vertex: about 50 000 triangles in about 200 workgroups, several loops per
    wavefront of the fill kernel."""
    m = mr.plane_map(side=160)
    rec = _rec_of(smx, m)
    full, _ = rec.Triangulate(None)
    gone = [y * 160 + x for x in range(8, 152, 8) for y in range(8, 152, 8)]
    tri = fc.without_vertices(full, gone)
    assert tri.shape[0] > 64 * 256 * 2
    world = dict(rec=rec, m=m, models={})
    got, kept, holes, st = _equals_model(world, tri, "plane 160")
    assert st["n_listed_loops"] == len(gone) and st["n_filled_loops"] > 300 and st["n_pinched_vertices"] == 0
    assert st["n_new_triangles"] > 1000 and not np.any(np.isin(got, gone))
    _equals_model(world, tri[np.random.default_rng(8).permutation(tri.shape[0])], "plane 160 shuffled", max_hole_edges=6)
    t = rec.debug_fill_timings()
    assert set(t) == {"edges", "loops", "fill", "write"} and all(np.isfinite(v) and v >= 0 for v in t.values())
    # what the fill added comes back as what was taken, where a single triangle was taken
    one = np.delete(full, 12345, axis=0)
    back, k1, h1, s1 = _equals_model(world, one, "one triangle deleted")
    assert s1["n_listed_loops"] == 1 and back[k1:].tolist() == [full[12345].tolist()]
    rec.close()


def test_composition_with_cleaning_decimation_and_the_mesh_render(world):
    from surfelmeshing_amd import render
    rec, tri, (pos, nrm, r2) = world["rec"], world["tri"], world["m"]
    clean, _ = rec.MeshComponents(None, tri, min_triangles=3)
    assert clean.tobytes() == cr.components(pos, r2, tri, min_triangles=3)[0].tobytes()
    filled, kept, holes, st = _equals_model(world, clean, "cleaned")
    assert st["n_new_triangles"] > 50
    coarse, dst = rec.DecimateMesh(None, filled, 0.1)
    want, _, wst = dr.decimate(pos, r2, filled, 0.1)
    assert coarse.tobytes() == want.tobytes() and dst == wst
    pose = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -4.0]], np.float32)
    index = render.render_mesh_view(rec, filled, *CAM, pose, outputs=("index",))["index"]
    covered = index[index != INVALID]
    assert covered.size > 1000 and int(covered.max()) < filled.shape[0]
    # a decimated (non-manifold) mesh goes into FillHoles
    _equals_model(world, coarse, "decimated", max_hole_edges=16)


def test_after_a_compaction_the_mapped_output_is_refilled_as_an_identity(smx):
    pos, nrm, r2 = mr.sphere_map(n=1500)
    rec = _rec_of(smx, (pos, nrm, r2))
    tri, _ = rec.Triangulate(None)
    r2m = r2.copy()
    r2m[np.random.default_rng(3).permutation(pos.shape[0])[:150]] = -1.0
    rec.debug_upload_surfels(mr.rows_of_map(pos, nrm, r2m), 150)
    world = dict(rec=rec, m=(pos, nrm, r2m), models={})
    got, kept, holes, st = _equals_model(world, tri, "stale array")
    assert st["n_not_live"] > 100 and st["n_filled_loops"] > 0
    old_to_new, new_size, _ = rec.Compact(None)
    assert new_size == pos.shape[0] - 150
    mapped = old_to_new[got.astype(np.int64)]
    assert int(mapped.max()) < new_size
    rows = rec.debug_download_surfels(new_size)
    world2 = dict(rec=rec, m=mr.map_of_rows(rows, new_size), models={})
    again, kept2, holes2, st2 = _equals_model(world2, mapped, "compacted")
    assert st2["n_new_triangles"] == 0 and st2["n_not_live"] == 0 and again.tobytes() == mapped.tobytes()
    assert holes2["label"].tolist() == old_to_new[holes["label"][holes["status"] != fr.FILLED].astype(np.int64)].tolist()
    rec.close()


def _raw(rec, p, tin, n_in, out, capacity, table, table_capacity, on_device=0, stats=True):
    """The C call itself; tin / out / table: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    prm = _lib.FillParams(p.get("max_hole_edges", 8), p.get("min_triangle_angle_deg", 10.0), p.get("max_triangle_angle_deg", 170.0))
    n, kept, nh, st = C.c_uint32(0xDEAD), C.c_uint32(0xDEAD), C.c_uint32(0xDEAD), _lib.FillStats()
    rc = _lib.load().smx_recon_fill_holes(rec._h, None, C.byref(prm), ptr(tin), C.c_uint32(n_in), ptr(out), C.c_uint32(capacity),
                                          ptr(table), C.c_uint32(table_capacity), C.c_int32(on_device), C.byref(n), C.byref(kept),
                                          C.byref(nh), C.byref(st) if stats else None)
    return rc, n.value, kept.value, nh.value, st


def test_calling_rules_on_host_arrays(world):
    rec, tri = world["rec"], world["tri"]
    p = dict(max_hole_edges=32)
    want, wkept, wholes, wst = _model(world, tri, "all", **p)
    T, H, n_in, n = want.shape[0], wholes.shape[0], tri.shape[0], world["m"][0].shape[0]
    out, table = np.full(3 * T + 8, GUARD, np.uint32), np.full(3 * (H + 2), GUARD, np.uint32)

    def untouched():
        return np.all(out == GUARD) and np.all(table == GUARD)
    # count only
    rc, nt, nk, nh, st = _raw(rec, p, tri, n_in, None, 0, None, 0)
    assert rc == -1 and (nt, nk, nh) == (T, wkept, H) and {k: int(getattr(st, k)) for k in wst} == wst
    # a short capacity; a short table: all counts, nothing written
    rc, nt, nk, nh, st = _raw(rec, p, tri, n_in, out, T - 1, table, H)
    assert rc == -1 and (nt, nk, nh) == (T, wkept, H) and untouched()
    rc, nt, nk, nh, st = _raw(rec, p, tri, n_in, out, T, table, H - 1)
    assert rc == -1 and (nt, nk, nh) == (T, wkept, H) and st.n_listed_loops == H and untouched()
    # an index >= n, anywhere
    for where in (0, 3 * (n_in // 2) + 1, 3 * n_in - 1):
        bad = tri.copy()
        bad.reshape(-1)[where] = n
        assert _raw(rec, p, bad, n_in, out, T, table, H)[0] == -1 and untouched()
    # parameters the library refuses
    for q in (dict(max_hole_edges=2), dict(max_hole_edges=33), dict(min_triangle_angle_deg=-1.0), dict(max_triangle_angle_deg=float("nan")),
              dict(min_triangle_angle_deg=50.0, max_triangle_angle_deg=50.0)):
        assert _raw(rec, q, tri, n_in, out, T, table, H)[0] == -1 and untouched()
    # overlapping in and out
    both = np.concatenate([tri, np.zeros((T - n_in + 4, 3), np.uint32)])
    snapshot = both.copy()
    assert _raw(rec, p, both, n_in, both, T, None, 0)[0] == -1 and both.tobytes() == snapshot.tobytes()
    assert _raw(rec, p, both, n_in, both.reshape(-1)[3 * (n_in - 1):], 1, None, 0)[0] == -1 and both.tobytes() == snapshot.tobytes()
    # the full call, with NULL stats; room to spare stays untouched
    rc, nt, nk, nh, _ = _raw(rec, p, tri, n_in, out, T + 2, table, H + 2, stats=False)
    assert rc == 0 and (nt, nk, nh) == (T, wkept, H)
    assert out[:3 * T].tobytes() == want.tobytes() and np.all(out[3 * T:] == GUARD)
    assert table[:3 * H].tobytes() == wholes.tobytes() and np.all(table[3 * H:] == GUARD)
    # no table
    out[:] = GUARD
    rc, nt, nk, nh, st = _raw(rec, p, tri, n_in, out, T, None, 0)
    assert rc == 0 and nh == H and out[:3 * T].tobytes() == want.tobytes()
    # n_in = 0: valid, nothing out
    out[:] = GUARD
    table[:] = GUARD
    rc, nt, nk, nh, st = _raw(rec, p, None, 0, out, T, table, H)
    assert rc == 0 and (nt, nk, nh) == (0, 0, 0) and st.n_in == 0 and st.n_edges == 0 and untouched()
    got, st = rec.FillHoles(None, np.zeros((0, 3), np.uint32))
    assert got.shape == (0, 3) and st["n_triangles"] == 0 and st["n_kept"] == 0


def test_device_arrays(smx, world):
    rec, tri = world["rec"], world["tri"]
    p = dict()
    want, wkept, wholes, wst = _model(world, tri, "all", **p)
    T, H, n_in = want.shape[0], wholes.shape[0], tri.shape[0]
    din, dout, dtab = (smx.CUDABuffer(1, k, np.uint32) for k in (3 * n_in, 3 * T + 8, 3 * H + 8))
    din.Upload(tri.reshape(1, -1))
    for b, k in ((dout, 3 * T + 8), (dtab, 3 * H + 8)):
        b.Upload(np.full((1, k), GUARD, np.uint32))
    a = [b.ToCUDA().address for b in (din, dout, dtab)]
    rc, nt, nk, nh, st = _raw(rec, p, a[0], n_in, None, 0, None, 0, on_device=1)
    assert rc == -1 and (nt, nk, nh) == (T, wkept, H)
    rc, nt, nk, nh, st = _raw(rec, p, a[0], n_in, a[1], T - 1, a[2], H, on_device=1)
    assert rc == -1 and (nt, nk, nh) == (T, wkept, H)
    rc, nt, nk, nh, st = _raw(rec, p, a[0], n_in, a[1], T, a[2], H - 1, on_device=1)
    assert rc == -1 and (nt, nk, nh) == (T, wkept, H)
    assert all(np.all(b.Download()[0] == GUARD) for b in (dout, dtab))
    rc, nt, nk, nh, st = _raw(rec, p, a[0], n_in, a[1], T, a[2], H, on_device=1)
    assert rc == 0 and (nt, nk, nh) == (T, wkept, H) and {k: int(getattr(st, k)) for k in wst} == wst
    back, tback = dout.Download()[0], dtab.Download()[0]
    assert back[:3 * T].tobytes() == want.tobytes() and np.all(back[3 * T:] == GUARD)
    assert tback[:3 * H].tobytes() == wholes.tobytes() and np.all(tback[3 * H:] == GUARD)
    assert din.Download()[0].tobytes() == tri.tobytes()          # the input is left alone
    # an index out of range on the device: nothing written
    bad = tri.copy()
    bad[n_in // 3, 2] = world["m"][0].shape[0]
    din.Upload(bad.reshape(1, -1))
    dout.Upload(np.full((1, 3 * T + 8), GUARD, np.uint32))
    assert _raw(rec, p, a[0], n_in, a[1], T, a[2], H, on_device=1)[0] == -1 and np.all(dout.Download()[0] == GUARD)
    # overlap on the device; n_in = 0
    assert _raw(rec, p, a[0], n_in, a[0] + 12, n_in - 1, None, 0, on_device=1)[0] == -1
    rc, nt, nk, nh, st = _raw(rec, p, None, 0, a[1], T, a[2], H, on_device=1)
    assert rc == 0 and (nt, nk, nh) == (0, 0, 0) and np.all(dout.Download()[0] == GUARD)
    for b in (din, dout, dtab):
        b.close()


def test_no_side_effects(smx):
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    nn = smx.SurfelNeighborIndex()
    tri, st, us = rec.TriangulateUpdate(None, index=nn)
    assert us["mode"] == 1
    n = rec.surfels_size()
    rec.SetDeltaTracking(None, True)
    rec.TransferChangedToCPU(None, 1)                            # enabling marks every slot; the hand-off clears the marks
    rows_before, stats_before = rec.debug_download_surfels(n), rec.stats()
    first = rec.FillHoles(None, tri, max_hole_edges=12, return_holes=True)
    again = rec.FillHoles(None, tri, max_hole_edges=12, return_holes=True)
    assert first[1] == again[1] and first[1]["n_filled_loops"] > 0 and all(first[k].tobytes() == again[k].tobytes() for k in (0, 2))
    assert rec.stats() == stats_before and rec.surfels_size() == n and rec.surfel_count() == n
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()
    assert rec.TransferChangedToCPU(None, 2).count == 0
    mesh_again, st2, us2 = rec.TriangulateUpdate(None, index=nn)
    assert us2["mode"] == 0 and us2["n_changed"] == 0 and mesh_again.tobytes() == tri.tobytes() and st2 == st
    nn.close()
    rec.close()


def test_map_mesher_fills_between_cleaning_and_decimation(smx):
    from surfelmeshing_amd import meshing
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    mesher = meshing.MapMesher(rec)
    tri, _, _, filled = mesher.update(clean=dict(min_triangles=4), fill=dict(max_hole_edges=6))
    clean = cr.components(m[0], m[2], tri, min_triangles=4)[0]
    want, wkept, _, wst = fr.fill(*m, clean, max_hole_edges=6)
    stats = dict(mesher.fill_stats)
    assert stats.pop("n_kept") == wkept and stats == wst and filled.tobytes() == want.tobytes() and mesher.decimated is None
    _, _, _, coarse = mesher.update(cell_size=0.2, clean=dict(min_triangles=4), fill=dict(max_hole_edges=6))
    assert coarse.tobytes() == dr.decimate(m[0], m[2], want, 0.2)[0].tobytes()
    assert meshing.fill_map_mesh(rec, clean, max_hole_edges=6)[0].tobytes() == want.tobytes()
    assert len(mesher.update()) == 3 and mesher.filled is None
    mesher.close()
    rec.close()


def test_a_failed_allocation_writes_nothing_and_the_next_call_succeeds(smx):
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    p = dict(max_hole_edges=10)
    want, wkept, wholes, wst = fr.fill(*m, tri, **p)
    T, H, n_in = want.shape[0], wholes.shape[0], tri.shape[0]
    assert wst["n_new_triangles"] > 0
    out, table = np.full(3 * T, GUARD, np.uint32), np.full(3 * H, GUARD, np.uint32)
    try:
        for nth in range(40):
            smx.DebugFailAllocation(nth)
            rc = _raw(rec, p, tri, n_in, out, T, table, H)[0]
            if rc == 0:
                break
            assert np.all(out == GUARD) and np.all(table == GUARD), nth
            # the next call succeeds and equals the model
            smx.DebugFailAllocation(-1)
            got, st, holes = rec.FillHoles(None, tri, return_holes=True, **p)
            st.pop("n_kept")
            assert st == wst and got.tobytes() == want.tobytes() and holes.tobytes() == wholes.tobytes()
            rec.close()                       # a fresh object for the next allocation in line
            rec = _rec_of(smx, m)
    finally:
        smx.DebugFailAllocation(-1)
    assert rc == 0 and 12 <= nth < 40, "the call reached %d allocations" % nth
    assert out.tobytes() == want.tobytes() and table.tobytes() == wholes.tobytes()
    rec.close()
    assert smx.DebugLiveAllocations() == base


def test_create_call_destroy_frees_everything(smx):
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    for _ in range(2):
        rec = _rec_of(smx, m)
        tri, _ = rec.Triangulate(None)
        got, st = rec.FillHoles(None, tri)
        assert st["n_new_triangles"] > 0 and smx.DebugLiveAllocations() > base
        rec.close()
        assert smx.DebugLiveAllocations() == base
