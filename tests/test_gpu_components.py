"""smx_recon_mesh_components on the device.  The contract (include/smx.h) is made of integers and of float32 expressions that
numpy reproduces bit for bit, so everything here is compared for EQUALITY with the model of tests/components_ref.py: the
triangle array, the vertex labels, the component table and every statistic."""
import ctypes as C

import numpy as np
import pytest

import components_ref as cr
import decimate_ref as dr
import mesh_ref as mr

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
INVALID = 0xFFFFFFFF
STRIP = 4096


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _everything():
    """The sphere, the plane (scaled to the sphere's spacing and placed apart), and spare slots on a grid so coarse against
    their radius that the mesher leaves them alone; over the spare slots the hand-made triangles."""
    sp, sn, sr = mr.sphere_map()
    pp, pn, pr = mr.plane_map()
    pp = _f32(pp * 0.05 + np.array([3.0, 0.0, 0.0]))
    pr = _f32(pr * 0.0025)
    n_spare = 3 + 4 + (STRIP + 2) + 5 + 7
    g = np.arange(n_spare)
    spare = _f32(np.stack([g % 17, (g // 17) % 17, g // 289], axis=1) * 0.1 + np.array([-1.0, 3.0, 0.0]))
    base = sp.shape[0] + pp.shape[0]
    pos = np.concatenate([sp, pp, spare])
    nrm = np.concatenate([sn, pn, np.tile([0.0, 0.0, 1.0], (n_spare, 1))])
    r2 = np.concatenate([sr, pr, np.full(n_spare, 1e-8)])
    b = base
    hand = [np.array([[b, b + 1, b + 2]])]                                         # one isolated triangle
    b += 3
    hand.append(np.array([[b, b + 1, b + 2], [b + 1, b + 3, b + 2]]))             # a two-triangle strip
    b += 4
    k = np.arange(STRIP)
    top = b + STRIP + 1
    hand.append(np.stack([top - k, top - k - 1, top - k - 2], axis=1))             # the strip whose indices descend along it
    b += STRIP + 2
    hand.append(np.array([[b, b + 1, b + 2], [b + 2, b + 3, b + 4]]))             # a bowtie
    b += 5
    r2[b + 3] = -1.0
    hand.append(np.array([[b + 4, b + 5, b + 6], [b + 2, b + 3, b + 4], [b, b + 1, b + 2]]))   # a bridge with a dead corner
    assert b + 7 == pos.shape[0]
    return (pos, nrm, _f32(r2)), np.concatenate(hand).astype(np.uint32), sp.shape[0], pp.shape[0]


@pytest.fixture(scope="module")
def world(smx):
    m, hand, n_sphere, n_plane = _everything()
    rec = _rec_of(smx, m)
    meshed, _ = rec.Triangulate(None)
    assert meshed.shape[0] > 9000 and int(meshed.max()) < n_sphere + n_plane       # the spare slots are left alone
    tri = np.concatenate([meshed, hand])
    yield dict(m=m, rec=rec, tri=tri, meshed=meshed, n_sphere=n_sphere, n_plane=n_plane, models={})
    rec.close()


def _model(world, tri, key=None, **p):
    """The model's answer, computed once per (array, parameters) and shared."""
    k = (key, tuple(sorted(p.items())))
    if key is None or k not in world["models"]:
        pos, _, r2 = world["m"]
        ans = cr.components(pos, r2, tri, **p)
        if key is None:
            return ans
        world["models"][k] = ans
    return world["models"][k]


def _equals_model(world, tri, what, key=None, rec=None, m=None, **p):
    rec = rec or world["rec"]
    got, st, labels, table = rec.MeshComponents(None, tri, return_labels=True, return_components=True, **p)
    if m is None:
        want, wlabels, wtable, wst = _model(world, tri, key, **p)
    else:
        want, wlabels, wtable, wst = cr.components(m[0], m[2], tri, **p)
    print("%s %s: GPU %s" % (what, p, st))
    assert got.dtype == np.uint32 and got.shape == (st["n_triangles"], 3)
    assert st == wst
    assert got.tobytes() == want.tobytes()
    assert labels.tobytes() == wlabels.tobytes()
    assert table.dtype.itemsize == 40 and table.tobytes() == wtable.tobytes()
    cr.check_properties(tri, got, labels, table, st)
    return got, st, labels, table


PARAMS = [dict(), dict(min_triangles=3), dict(min_triangles=4097), dict(min_diagonal=0.25), dict(min_diagonal=2.5),
          dict(keep_largest=1), dict(keep_largest=2), dict(min_triangles=2, min_diagonal=0.15, keep_largest=4)]


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: ",".join("%s=%s" % kv for kv in p.items()) or "default")
def test_one_map_with_everything_equals_the_model(world, p):
    got, st, labels, table = _equals_model(world, world["tri"], "everything", key="all", **p)
    if not p:
        # sphere, plane, isolated triangle, two-strip, long strip, bowtie, the two halves of the bridge
        assert st["n_components"] == 8 and st["n_not_live"] == 1 and st["n_kept_components"] == 8
        assert sorted(int(v) for v in table["n_triangles"])[:5] == [1, 1, 1, 2, 2] and STRIP in table["n_triangles"]
        assert got.tobytes() == np.delete(world["tri"], world["tri"].shape[0] - 2, axis=0).tobytes()
    if p == dict(keep_largest=2):
        assert sorted(int(v) for v in table["n_triangles"][table["kept"] == 1])[0] == STRIP


def _interleaved(tri, comp, stride):
    """tri reordered so that neighbouring rows alternate between its `stride` largest components (comp: the component of
    every row); the rest follows."""
    ids, sizes = np.unique(comp, return_counts=True)
    big = ids[np.argsort(-sizes, kind="stable")][:stride]
    runs = [np.flatnonzero(comp == c) for c in big]
    m = min(r.size for r in runs)
    mixed = np.stack([r[:m] for r in runs], axis=1).reshape(-1)
    order = np.concatenate([mixed, np.setdiff1d(np.arange(tri.shape[0]), mixed)])
    assert np.array_equal(np.sort(order), np.arange(tri.shape[0])) and m > 1000
    return tri[order]


@pytest.mark.parametrize("stride", [2, 5])
def test_mixed_labels_in_one_wavefront(world, stride):
    """Neighbouring lanes alternate between `stride` components: the aggregation loop takes `stride` or more trips."""
    # the long strip cut in three (two neighbouring triangles taken out separate what is left of them): five large pieces
    tri = world["tri"]
    first = world["meshed"].shape[0] + 3                                 # the strip comes after the isolated triangle and the two-strip
    cuts = [first + STRIP // 3, first + STRIP // 3 + 1, first + 2 * STRIP // 3, first + 2 * STRIP // 3 + 1]
    tri = np.delete(tri, cuts, axis=0)
    _, labels, table, wst = _model(world, tri, "cut")
    assert wst["n_components"] == 10 and sorted(int(v) for v in table["n_triangles"])[5] > 1000
    comp = labels[tri[:, 0].astype(np.int64)]
    arr = _interleaved(tri, comp, stride)
    assert len(set(labels[arr[:stride, 0].astype(np.int64)])) == stride
    got, st, _, _ = _equals_model(world, arr, "interleaved by %d" % stride, min_triangles=2)
    assert st["n_components"] == 10 and st["n_kept_components"] == 7
    shuffled = tri[np.random.default_rng(stride).permutation(tri.shape[0])]
    _equals_model(world, shuffled, "shuffled", keep_largest=3)           # (output order follows the input: the bytes are compared)


def test_a_single_component_above_64_workgroups(smx):
    m = mr.sphere_map(n=11000)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    world = dict(rec=rec, m=m, models={})
    _, st, _, _ = _equals_model(world, tri, "sphere 11000")
    assert st["n_largest_triangles"] > 64 * 256
    # the same from the far end, and shuffled: many workgroups hook into one root in another order
    _equals_model(world, tri[::-1].copy(), "sphere 11000 reversed", min_triangles=10)
    _equals_model(world, tri[np.random.default_rng(2).permutation(tri.shape[0])], "sphere 11000 shuffled", keep_largest=1)
    t = rec.debug_components_timings()
    assert set(t) == {"mark_link", "flatten_number", "measure", "write"} and all(np.isfinite(v) and v >= 0 for v in t.values())
    rec.close()


def test_composition_with_decimation_and_the_mesh_render(smx, world):
    from surfelmeshing_amd import render
    rec, tri, meshed, (pos, _, r2) = world["rec"], world["tri"], world["meshed"], world["m"]
    # keep_largest = 1 on sphere + plane: the sphere's own triangulation, byte for byte
    sphere = _rec_of(smx, mr.sphere_map())
    own, _ = sphere.Triangulate(None)
    sphere.close()
    got, st = rec.MeshComponents(None, meshed, keep_largest=1)
    assert st["n_components"] == 2 and got.tobytes() == own.tobytes()
    # the cleaned array goes into DecimateMesh and RenderMesh as it is
    clean, _ = rec.MeshComponents(None, tri, min_triangles=3)
    coarse, dst = rec.DecimateMesh(None, clean, 0.1)
    want, _, wst = dr.decimate(pos, r2, clean, 0.1)
    assert coarse.tobytes() == want.tobytes() and dst == wst
    pose = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -4.0]], np.float32)
    index = render.render_mesh_view(rec, clean, *CAM, pose, outputs=("index",))["index"]
    covered = index[index != INVALID]
    assert covered.size > 1000 and int(covered.max()) < clean.shape[0]
    # a decimated (non-manifold) mesh goes into MeshComponents
    _equals_model(world, coarse, "decimated", min_triangles=2)
    _equals_model(world, coarse, "decimated", keep_largest=1)


def _raw(rec, p, tin, n_in, out, capacity, labels, table, table_capacity, on_device=0, stats=True):
    """The C call itself; tin / out / labels / table: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    prm = _lib.ComponentsParams(p.get("min_triangles", 0), p.get("min_diagonal", 0.0), p.get("keep_largest", 0))
    n, nc, st = C.c_uint32(0xDEAD), C.c_uint32(0xDEAD), _lib.ComponentsStats()
    rc = _lib.load().smx_recon_mesh_components(rec._h, None, C.byref(prm), ptr(tin), C.c_uint32(n_in), ptr(out), C.c_uint32(capacity),
                                               ptr(labels), ptr(table), C.c_uint32(table_capacity), C.c_int32(on_device),
                                               C.byref(n), C.byref(nc), C.byref(st) if stats else None)
    return rc, n.value, nc.value, st


def test_calling_rules_on_host_arrays(world):
    rec, tri = world["rec"], world["tri"]
    p = dict(min_triangles=3)
    want, wlabels, wtable, wst = _model(world, tri, "all", **p)
    T, Cn, n_in, n = want.shape[0], wtable.shape[0], tri.shape[0], wlabels.shape[0]
    out, labels = np.full(3 * n_in + 8, GUARD, np.uint32), np.full(n + 8, GUARD, np.uint32)
    table = np.full(10 * (Cn + 2), GUARD, np.uint32)

    def untouched():
        return np.all(out == GUARD) and np.all(labels == GUARD) and np.all(table == GUARD)
    # count only
    rc, nt, nc, st = _raw(rec, p, tri, n_in, None, 0, None, None, 0)
    assert rc == -1 and nt == T and nc == Cn and st.n_triangles == T and st.n_kept_components == wst["n_kept_components"]
    # a short capacity; a short component capacity: both counts, nothing written
    rc, nt, nc, st = _raw(rec, p, tri, n_in, out, T - 1, labels, table, Cn)
    assert rc == -1 and nt == T and nc == Cn and untouched()
    rc, nt, nc, st = _raw(rec, p, tri, n_in, out, T, labels, table, Cn - 1)
    assert rc == -1 and nt == T and nc == Cn and st.n_components == Cn and untouched()
    # an index >= n, anywhere
    for where in (0, 3 * (n_in // 2) + 1, 3 * n_in - 1):
        bad = tri.copy()
        bad.reshape(-1)[where] = n
        rc, nt, nc, _ = _raw(rec, p, bad, n_in, out, n_in, labels, table, Cn)
        assert rc == -1 and untouched()
    # min_diagonal negative, NaN or infinite
    for d in (-0.5, float("nan"), float("inf")):
        assert _raw(rec, dict(min_diagonal=d), tri, n_in, out, n_in, labels, table, Cn)[0] == -1 and untouched()
    # overlapping in and out
    both = tri.copy()
    assert _raw(rec, p, both, n_in, both, n_in, None, None, 0)[0] == -1 and both.tobytes() == tri.tobytes()
    assert _raw(rec, p, both, n_in, both.reshape(-1)[3 * (n_in - 1):], 1, None, None, 0)[0] == -1 and both.tobytes() == tri.tobytes()
    # the full call, with NULL stats; room to spare stays untouched
    rc, nt, nc, _ = _raw(rec, p, tri, n_in, out, n_in, labels, table, Cn + 2, stats=False)
    assert rc == 0 and nt == T and nc == Cn
    assert out[:3 * T].tobytes() == want.tobytes() and np.all(out[3 * T:] == GUARD)
    assert labels[:n].tobytes() == wlabels.tobytes() and np.all(labels[n:] == GUARD)
    assert table[:10 * Cn].tobytes() == wtable.tobytes() and np.all(table[10 * Cn:] == GUARD)
    # no table, no labels
    out[:] = GUARD
    rc, nt, nc, st = _raw(rec, p, tri, n_in, out, T, None, None, 0)
    assert rc == 0 and nt == T and nc == Cn and out[:3 * T].tobytes() == want.tobytes()
    # n_in = 0: valid, nothing out, nobody is used
    labels[:] = GUARD
    out[:] = GUARD
    rc, nt, nc, st = _raw(rec, p, None, 0, out, n_in, labels, table, Cn)
    assert rc == 0 and nt == 0 and nc == 0 and st.n_in == 0 and st.n_used_vertices == 0 and st.n_largest_triangles == 0
    assert np.all(labels[:n] == INVALID) and np.all(labels[n:] == GUARD) and np.all(out == GUARD)
    got, st = rec.MeshComponents(None, np.zeros((0, 3), np.uint32), keep_largest=1)
    assert got.shape == (0, 3) and st["n_components"] == 0


def test_device_arrays(smx, world):
    rec, tri = world["rec"], world["tri"]
    p = dict(keep_largest=2)
    want, wlabels, wtable, wst = _model(world, tri, "all", **p)
    T, Cn, n_in, n = want.shape[0], wtable.shape[0], tri.shape[0], wlabels.shape[0]
    din, dout, dlab, dtab = (smx.CUDABuffer(1, k, np.uint32) for k in (3 * n_in, 3 * T + 8, n + 8, 10 * Cn + 8))
    din.Upload(tri.reshape(1, -1))
    for b, k in ((dout, 3 * T + 8), (dlab, n + 8), (dtab, 10 * Cn + 8)):
        b.Upload(np.full((1, k), GUARD, np.uint32))
    a = [b.ToCUDA().address for b in (din, dout, dlab, dtab)]
    rc, nt, nc, st = _raw(rec, p, a[0], n_in, a[1], T - 1, a[2], a[3], Cn, on_device=1)
    assert rc == -1 and nt == T and nc == Cn
    assert all(np.all(b.Download()[0] == GUARD) for b in (dout, dlab, dtab))
    rc, nt, nc, st = _raw(rec, p, a[0], n_in, a[1], T, a[2], a[3], Cn, on_device=1)
    assert rc == 0 and nt == T and nc == Cn and {k: int(getattr(st, k)) for k in wst} == wst
    back, lback, tback = dout.Download()[0], dlab.Download()[0], dtab.Download()[0]
    assert back[:3 * T].tobytes() == want.tobytes() and np.all(back[3 * T:] == GUARD)
    assert lback[:n].tobytes() == wlabels.tobytes() and np.all(lback[n:] == GUARD)
    assert tback[:10 * Cn].tobytes() == wtable.tobytes() and np.all(tback[10 * Cn:] == GUARD)
    assert din.Download()[0].tobytes() == tri.tobytes()          # the input is left alone
    # overlap on the device
    assert _raw(rec, p, a[0], n_in, a[0] + 12, n_in - 1, None, None, 0, on_device=1)[0] == -1
    for b in (din, dout, dlab, dtab):
        b.close()


def test_no_side_effects(smx):
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    nn = smx.SurfelNeighborIndex()
    tri, st, us = rec.TriangulateUpdate(None, index=nn)
    assert us["mode"] == 1
    n = rec.surfels_size()
    rows_before, stats_before = rec.debug_download_surfels(n), rec.stats()
    first = rec.MeshComponents(None, tri, min_triangles=5, keep_largest=3, return_labels=True, return_components=True)
    again = rec.MeshComponents(None, tri, min_triangles=5, keep_largest=3, return_labels=True, return_components=True)
    assert first[1] == again[1] and all(first[k].tobytes() == again[k].tobytes() for k in (0, 2, 3))
    assert rec.stats() == stats_before and rec.surfels_size() == n
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()
    mesh_again, st2, us2 = rec.TriangulateUpdate(None, index=nn)
    assert us2["mode"] == 0 and us2["n_changed"] == 0 and mesh_again.tobytes() == tri.tobytes() and st2 == st
    nn.close()
    rec.close()


def test_map_mesher_cleans_before_it_decimates(smx):
    from surfelmeshing_amd import meshing
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    mesher = meshing.MapMesher(rec)
    tri, _, _, clean = mesher.update(clean=dict(min_triangles=4))
    want, _, _, wst = cr.components(m[0], m[2], tri, min_triangles=4)
    assert clean.tobytes() == want.tobytes() and mesher.clean_stats == wst and mesher.decimated is None
    _, _, _, coarse = mesher.update(cell_size=0.2, clean=dict(min_triangles=4))
    assert coarse.tobytes() == dr.decimate(m[0], m[2], want, 0.2)[0].tobytes()
    assert meshing.clean_map_mesh(rec, tri, min_triangles=4)[0].tobytes() == want.tobytes()
    assert len(mesher.update()) == 3 and mesher.cleaned is None
    mesher.close()
    rec.close()


def test_a_failed_allocation_writes_nothing_and_the_next_call_succeeds(smx):
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    pos, _, r2 = m
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    p = dict(min_triangles=2, keep_largest=2)
    want, wlabels, wtable, wst = cr.components(pos, r2, tri, **p)
    T, Cn, n_in, n = want.shape[0], wtable.shape[0], tri.shape[0], pos.shape[0]
    out, labels, table = np.full(3 * n_in, GUARD, np.uint32), np.full(n, GUARD, np.uint32), np.full(10 * Cn, GUARD, np.uint32)
    try:
        for nth in range(40):
            smx.DebugFailAllocation(nth)
            rc, nt, nc, _ = _raw(rec, p, tri, n_in, out, n_in, labels, table, Cn)
            if rc == 0:
                break
            assert rc != 0 and np.all(out == GUARD) and np.all(labels == GUARD) and np.all(table == GUARD), nth
            # the next call succeeds and equals the model
            smx.DebugFailAllocation(-1)
            got, st, glabels, gtable = rec.MeshComponents(None, tri, return_labels=True, return_components=True, **p)
            assert st == wst and got.tobytes() == want.tobytes() and glabels.tobytes() == wlabels.tobytes()
            assert gtable.tobytes() == wtable.tobytes()
            rec.close()                       # a fresh object for the next allocation in line
            rec = _rec_of(smx, m)
    finally:
        smx.DebugFailAllocation(-1)
    assert rc == 0 and 8 <= nth < 40, "the call reached %d allocations" % nth
    assert out[:3 * T].tobytes() == want.tobytes() and labels.tobytes() == wlabels.tobytes() and table.tobytes() == wtable.tobytes()
    rec.close()
    assert smx.DebugLiveAllocations() == base
