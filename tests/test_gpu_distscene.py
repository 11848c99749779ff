"""smx_distscene on the device.  A scene answers what smx_recon_mesh_distance answers on the map as it stood at the build, so
everything here is compared for EQUALITY: with the brute-force model of tests/distance_ref.py (nearest, distance, closest and
every statistic; the grid's three counts whenever the cell size is given) and with rec.MeshDistance at the scene's
cell_size_used (every word, cell_size_used included)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distance_ref as dr
import distscene_ref as sr
import mesh_ref as mr
from common import ROOT

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
GRID = ("n_wide", "n_entries", "n_cells")
BUILD_STATS = ("n_in", "n_not_live", "n_repeated", "n_out_of_range") + GRID + ("cell_size_used",)


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


@pytest.fixture(scope="module")
def world(smx):
    """One map for the module: the world of tests/distance_ref.py (sphere, holed plane, the twelve hand-made triangles)."""
    pos, nrm, r2, tri, info = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    yield dict(m=(pos, nrm, r2), rec=rec, tri=tri, info=info)
    rec.close()


def _same(got, want, what):
    """(nearest, distance, closest, stats) twice: the same bytes and the same words."""
    assert got[3] == want[3], (what, got[3], want[3])
    for k, name in enumerate(("nearest", "distance", "closest")):
        assert got[k].tobytes() == want[k].tobytes(), (what, name, int(np.sum(got[k].view(np.uint32) != want[k].view(np.uint32))))


def _against_model(got, want, m, tri, bound, cell_size, what):
    gst, wst = dict(got[3]), dict(want[3])
    used = gst.pop("cell_size_used")
    if cell_size > 0:
        assert used == float(dr.cell_used(cell_size, bound)), what
        wst.update(dr.structure(m[0], m[2], tri, cell_size, bound))       # (the structure is the build's, whatever q is)
    else:
        assert used >= float(dr.cell_used(0.0, bound)), what
        for k in GRID:
            gst.pop(k)
    assert gst == wst, (what, gst, wst)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32 and got[2].dtype == np.float32
    for k, name in enumerate(("nearest", "distance", "closest")):
        assert got[k].tobytes() == want[k].tobytes(), (what, name, int(np.sum(got[k].view(np.uint32) != want[k].view(np.uint32))))


@pytest.mark.parametrize("bound,cell", sr.BUILDS)
def test_every_point_set_equals_the_model_and_the_call(world, bound, cell):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    for cs in (cell,) + sr.OTHER_CELLS:
        with rec.BuildDistanceScene(None, tri, bound, cs) as scene:
            st = scene.stats
            assert st["max_distance"] == float(dr.F(bound)) and st["n_in"] == tri.shape[0] and st["device_bytes"] > 48 * (st["n_entries"] + st["n_wide"])
            if cs > 0:
                assert {k: st[k] for k in GRID} == dr.structure(m[0], m[2], tri, cs, bound) and st["cell_size_used"] == float(dr.cell_used(cs, bound))
            if cs == cell:       # where the winners come from: the wide list for nearly all, both, cell records only
                assert (st["n_wide"] > 9000, 0 < st["n_wide"] < 1000, st["n_wide"] == 0)[sr.BUILDS.index((bound, cell))]
            for q in sr.queries(bound):
                matched = unmatched = 0
                for name, pts in dr.point_sets().items():
                    model = dr.model_of(name)
                    for signed in (False, True):
                        what = "%s bound %g cell %g q %g signed %d" % (name, bound, cs, q, signed)
                        got = scene.Query(None, pts, q, signed, return_closest=True)
                        want = dr.answer(model, q, signed)
                        _against_model(got, want, m, tri, bound, cs, what)
                        _same(got, rec.MeshDistance(None, tri, pts, q, st["cell_size_used"], signed, return_closest=True), what)
                        assert {k: got[3][k] for k in BUILD_STATS} == {k: st[k] for k in BUILD_STATS}
                    matched, unmatched = matched + want[3]["n_matched"], unmatched + want[3]["n_points"] - want[3]["n_matched"]
                print("bound %g cell %g q %g: %d matched, %d not, n_wide %d n_entries %d" % (bound, cs, q, matched, unmatched, st["n_wide"], st["n_entries"]))
                assert matched > 0 and unmatched > 0
            t = scene.debug_timings()
            assert set(t) == {"mark", "index", "first", "query", "stats"} and all(np.isfinite(v) and v >= 0 for v in t.values())
            assert t["first"] > 0 and t["query"] > 0


def test_the_edges_of_the_256_point_workgroup(world):
    rec, tri = world["rec"], world["tri"]
    pts, model = dr.point_sets()[sr.TILE_SET], dr.model_of(sr.TILE_SET)
    with rec.BuildDistanceScene(None, tri, 0.02, 0.0225) as scene:
        for q in sr.queries(0.02):
            wn, wd, wc, _ = dr.answer(model, q, True)
            for n in sr.TILE_PREFIXES:
                nearest, distance, closest, st = scene.Query(None, pts[:n], q, True, return_closest=True)
                assert nearest.tobytes() == wn[:n].tobytes() and distance.tobytes() == wd[:n].tobytes() and closest.tobytes() == wc[:n].tobytes(), (q, n)
                assert st["n_points"] == n and st["n_matched"] == int(np.sum(wn[:n] != dr.INVALID))


def _raw_query(scene, pts, n_points, nearest, distance, closest, max_distance=0.02, cell_size=0.0, signed=0, on_device=0, stats=True):
    """The C call itself; arrays: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    prm, st = _lib.DistanceParams(max_distance, cell_size, signed), _lib.DistanceStats()
    rc = _lib.load().smx_distscene_query(scene._h, None, C.byref(prm), ptr(pts), C.c_uint32(n_points), ptr(nearest), ptr(distance), ptr(closest),
                                         C.c_int32(on_device), C.byref(st) if stats else None)
    return rc, st


def _raw_build(rec, scene, tri, n_in, max_distance=0.02, cell_size=0.0, on_device=0):
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    prm, st = _lib.DistSceneParams(max_distance, cell_size), _lib.DistSceneStats()
    rc = _lib.load().smx_recon_build_distscene(rec._h, None, scene._h, C.byref(prm), ptr(tri), C.c_uint32(n_in), C.c_int32(on_device), C.byref(st))
    return rc, st


def _guards(P, extra=4):
    return np.full(P + extra, GUARD, np.uint32), np.full(P + extra, GUARD, np.uint32), np.full(3 * P + extra, GUARD, np.uint32)


def test_a_query_above_the_bound_is_refused_and_writes_nothing(smx, world):
    rec, tri = world["rec"], world["tri"]
    pts = dr.point_sets()["around the hand-made triangles"]
    P = pts.shape[0]
    with rec.BuildDistanceScene(None, tri, 0.02) as scene:
        for q in (0.5, float(np.nextafter(np.float32(0.02), np.float32(1.0)))):
            g = _guards(P)
            assert _raw_query(scene, pts, P, *g, max_distance=q)[0] == -1 and all(np.all(a == GUARD) for a in g), q
            with pytest.raises(ValueError):
                scene.Query(None, pts, q)
        scene.stats = dict(scene.stats, max_distance=16.0)       # past the wrapper's own check: the library refuses too
        with pytest.raises(smx.SmxError):
            scene.Query(None, pts, 0.5)
        g = _guards(P)
        assert _raw_query(scene, pts, P, *g, cell_size=0.05)[0] == -1 and all(np.all(a == GUARD) for a in g)
        assert _raw_query(scene, pts, P, *g, max_distance=0.02)[0] == 0 and np.all(g[0][P:] == GUARD) and not np.all(g[0][:P] == GUARD)


def test_a_scene_is_a_snapshot(smx):
    """Build, query; then every position moved and a third of the slots killed, then Compact, then the reconstruction closed: the
    same query gives the same bytes.  A fresh MeshDistance on the changed map gives different ones."""
    pos, nrm, r2, tri, _ = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    name = "vertices 0 / 1 / 5 mm"
    pts, model = dr.point_sets()[name], dr.model_of(name)
    scene = rec.BuildDistanceScene(None, tri, 0.02)
    want = dr.answer(model, 0.02, True)
    first = scene.Query(None, pts, 0.02, True, return_closest=True)
    assert all(first[k].tobytes() == want[k].tobytes() for k in range(3)) and want[3]["n_matched"] == 900
    moved_r2 = r2.copy()
    moved_r2[::3] = -1.0
    rec.debug_upload_surfels(mr.rows_of_map(pos + np.array([0.004, -0.003, 0.002]), nrm, moved_r2), int(np.sum(moved_r2 < 0)))
    _same(scene.Query(None, pts, 0.02, True, return_closest=True), first, "after the upload")
    changed = rec.MeshDistance(None, tri, pts, 0.02, scene.stats["cell_size_used"], True, return_closest=True)
    assert changed[0].tobytes() != first[0].tobytes() and changed[1].tobytes() != first[1].tobytes() and changed[3] != first[3]
    rec.Compact(None)
    _same(scene.Query(None, pts, 0.02, True, return_closest=True), first, "after Compact")
    rec.close()
    _same(scene.Query(None, pts, 0.02, True, return_closest=True), first, "after the reconstruction is gone")
    _same(scene.Query(None, pts, 0.002, True, return_closest=True)[:3] + (None,), dr.answer(model, 0.002, True)[:3] + (None,), "a smaller q, later")
    scene.close()


def test_rebuild_in_place_two_scenes_at_once_and_a_call_in_between(world):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    pts = dr.point_sets()["random in the box"]
    half = tri[: tri.shape[0] // 2]
    want_all = rec.MeshDistance(None, tri, pts, 0.5, 0.5625, return_closest=True)
    want_half = dr.answer(dr.brute(m[0], m[2], half, pts), 0.02)
    a = rec.BuildDistanceScene(None, tri, 0.5, 0.5625)
    b = rec.BuildDistanceScene(None, half, 0.02)
    _same(a.Query(None, pts, 0.5, return_closest=True), want_all, "a")
    got = b.Query(None, pts, 0.02, return_closest=True)
    assert all(got[k].tobytes() == want_half[k].tobytes() for k in range(3)) and got[3]["n_in"] == half.shape[0]
    rec.MeshDistance(None, half, pts[:100], 0.002)                         # the call shares the build's workspace with neither scene
    _same(a.Query(None, pts, 0.5, return_closest=True), want_all, "a after b and a call")
    assert rec.BuildDistanceScene(None, half, 0.02, scene=a) is a           # rebuilt in place: now it answers for `half`
    assert a.stats["n_in"] == half.shape[0] and a.stats["max_distance"] == float(dr.F(0.02))
    _same(a.Query(None, pts, 0.02, return_closest=True), got, "a rebuilt")
    _same(b.Query(None, pts, 0.02, return_closest=True), got, "b after a's rebuild")
    with pytest.raises(ValueError):
        a.Query(None, pts, 0.5)
    a.close()
    b.close()


def test_calling_rules_on_host_and_device_arrays(smx, world):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    name = "around the hand-made triangles"
    pts = dr.point_sets()[name]
    P, n_in, n = pts.shape[0], tri.shape[0], m[0].shape[0]
    wn, wd, wc, wst = dr.answer(dr.model_of(name), 0.02, True)
    scene = smx.DistanceScene()
    # never built: empty
    g = _guards(P)
    assert _raw_query(scene, pts, P, *g)[0] == -1 and all(np.all(a == GUARD) for a in g)
    # an index >= n: the build is refused and the scene stays empty; so does a scene that held a build before
    bad = tri.copy()
    bad.reshape(-1)[3 * (n_in // 2) + 1] = n
    assert _raw_build(rec, scene, bad, n_in)[0] == -1 and _raw_query(scene, pts, P, *g)[0] == -1
    assert _raw_build(rec, scene, tri, n_in)[0] == 0 and _raw_query(scene, pts, P, *_guards(P))[0] == 0
    assert _raw_build(rec, scene, bad, n_in)[0] == -1 and _raw_query(scene, pts, P, *g)[0] == -1 and all(np.all(a == GUARD) for a in g)
    rc, bst = _raw_build(rec, scene, tri, n_in)
    assert rc == 0 and bst.n_in == n_in and bst.n_repeated == 1 and bst.n_out_of_range == 1 and bst.max_distance == np.float32(0.02)
    # host arrays pre-filled with a guard word; room to spare stays untouched
    nearest, distance, closest = _guards(P)
    rc, st = _raw_query(scene, pts, P, nearest, distance, closest, signed=1)
    assert rc == 0 and nearest[:P].tobytes() == wn.tobytes() and distance[:P].tobytes() == wd.tobytes() and closest[:3 * P].tobytes() == wc.tobytes()
    assert np.all(nearest[P:] == GUARD) and np.all(distance[P:] == GUARD) and np.all(closest[3 * P:] == GUARD)
    gst = smx.distance_stats_dict(st)
    assert {k: gst[k] for k in wst if k != "max_distance"} == {k: v for k, v in wst.items() if k != "max_distance"}
    # closest = NULL and stats = NULL leave the other outputs as they are
    n2, d2, _ = _guards(P)
    rc, _ = _raw_query(scene, pts, P, n2, d2, None, signed=1, stats=False)
    assert rc == 0 and n2.tobytes() == nearest.tobytes() and d2.tobytes() == distance.tobytes()
    # an output over the points: refused, nothing written
    both = np.concatenate([pts.reshape(-1).view(np.uint32), np.full(8, GUARD, np.uint32)])
    snapshot = both.copy()
    g = _guards(P)
    assert _raw_query(scene, both, P, g[0], g[1], both[3 * P - 1:])[0] == -1 and both.tobytes() == snapshot.tobytes()
    # n_points == 0: only the structure's statistics
    rc, st = _raw_query(scene, None, 0, None, None, None)
    assert rc == 0 and st.n_points == 0 and st.n_matched == 0 and st.n_in == n_in and st.n_entries == bst.n_entries and st.n_wide == bst.n_wide
    # device arrays give the same bytes, for the build and for the query
    din, dpt = smx.CUDABuffer(1, 3 * n_in, np.uint32), smx.CUDABuffer(1, 3 * P, np.uint32)
    outs = [smx.CUDABuffer(1, k, np.uint32) for k in (P + 4, P + 4, 3 * P + 4)]
    din.Upload(tri.reshape(1, -1))
    dpt.Upload(pts.reshape(1, -1).view(np.uint32))
    for b, k in zip(outs, (P + 4, P + 4, 3 * P + 4)):
        b.Upload(np.full((1, k), GUARD, np.uint32))
    a = [b.ToCUDA().address for b in [din, dpt] + outs]
    rc, dst = _raw_build(rec, scene, a[0], n_in, on_device=1)
    assert rc == 0 and all(getattr(dst, k) == getattr(bst, k) for k in BUILD_STATS)
    rc, st = _raw_query(scene, a[1], P, a[2], a[3], a[4], signed=1, on_device=1)
    back = [b.Download()[0] for b in outs]
    assert rc == 0 and back[0].tobytes() == nearest.tobytes() and back[1].tobytes() == distance.tobytes() and back[2].tobytes() == closest.tobytes()
    assert din.Download()[0].tobytes() == tri.tobytes() and dpt.Download()[0].tobytes() == pts.tobytes()
    assert _raw_query(scene, a[1], P, a[1] + 8, a[3], a[4], on_device=1)[0] == -1          # overlap on the device
    assert dpt.Download()[0].tobytes() == pts.tobytes()
    for b in [din, dpt] + outs:
        b.close()
    # device tensors through the Python calls
    import torch
    tt, tp = torch.from_numpy(tri.astype(np.int32)).cuda(), torch.from_numpy(pts.copy()).cuda()
    with rec.BuildDistanceScene(None, tt, 0.02) as ts:
        tn, td, tc, tst = ts.Query(None, tp, signed=True, return_closest=True)
        torch.cuda.synchronize()
        assert tn.cpu().numpy().view(np.uint32).tobytes() == wn.tobytes() and td.cpu().numpy().tobytes() == wd.tobytes()
        assert tc.cpu().numpy().tobytes() == wc.tobytes() and tst["n_matched"] == wst["n_matched"]
    scene.close()


def test_no_triangles_and_no_points(world):
    rec = world["rec"]
    pts = dr.point_sets()["NaN, inf and 65 m"]
    P = pts.shape[0]
    with rec.BuildDistanceScene(None, np.zeros((0, 3), np.uint32), 0.02) as scene:
        assert scene.stats["n_in"] == 0 and scene.stats["n_entries"] == 0 and scene.stats["n_wide"] == 0
        nearest, distance, closest, st = scene.Query(None, pts, 0.02, return_closest=True)
        assert np.all(nearest == dr.INVALID) and np.all(np.isinf(distance)) and np.all(np.isnan(closest))
        assert st["n_matched"] == 0 and st["n_points"] == P and st["n_bad_points"] == 7
        nearest, distance, st = scene.Query(None, np.zeros((0, 3), np.float32))
        assert nearest.size == 0 and distance.size == 0 and st["n_points"] == 0


def test_a_failed_allocation_leaves_the_scene_empty_or_writes_nothing_and_destroy_frees_everything(smx):
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    pts = np.ascontiguousarray((m[0][:200] * 1.002).astype(np.float32))
    wn, wd, wc, wst = dr.answer(dr.brute(m[0], m[2], tri, pts), 0.02)
    P, n_in = pts.shape[0], tri.shape[0]
    failed_builds, failed_queries = [], []
    try:
        # every allocation of a build, on a fresh object and a fresh scene each time
        for nth in range(40):
            scene = smx.DistanceScene()
            smx.DebugFailAllocation(nth)
            rc = _raw_build(rec, scene, tri, n_in)[0]
            smx.DebugFailAllocation(-1)
            if rc == 0:
                break
            failed_builds.append(rc)
            g = _guards(P, 0)
            assert rc == -2 and _raw_query(scene, pts, P, *g)[0] == -1 and all(np.all(a == GUARD) for a in g), nth     # empty
            assert _raw_build(rec, scene, tri, n_in)[0] == 0                    # the next build succeeds
            assert _raw_query(scene, pts, P, *g)[0] == 0
            assert g[0].tobytes() == wn.tobytes() and g[1].tobytes() == wd.tobytes() and g[2].tobytes() == wc.tobytes()
            scene.close()
            rec.close()
            rec = _rec_of(smx, m)
        # from the scene's counters to first_rec, behind the cell table
        assert rc == 0 and 10 <= len(failed_builds) < 40, "the build reached %d allocations" % len(failed_builds)
        scene.close()
        # every allocation of a query, on a fresh scene each time
        for nth in range(40):
            scene = rec.BuildDistanceScene(None, tri, 0.02)
            g = _guards(P, 0)
            smx.DebugFailAllocation(nth)
            rc = _raw_query(scene, pts, P, *g)[0]
            smx.DebugFailAllocation(-1)
            if rc == 0:
                break
            failed_queries.append(rc)
            assert rc == -2 and all(np.all(a == GUARD) for a in g), nth       # the allocation error, nothing written
            got = scene.Query(None, pts, 0.02, return_closest=True)            # the next query succeeds
            assert got[0].tobytes() == wn.tobytes() and got[1].tobytes() == wd.tobytes() and got[2].tobytes() == wc.tobytes()
            scene.close()
        # the counters, the keys, the sort's five buffers, the point staging and the three output stagings
        assert rc == 0 and 8 <= len(failed_queries) < 40, "the query reached %d allocations" % len(failed_queries)
        assert g[0].tobytes() == wn.tobytes() and g[1].tobytes() == wd.tobytes() and g[2].tobytes() == wc.tobytes()
    finally:
        smx.DebugFailAllocation(-1)
    assert smx.DebugLiveAllocations() > base
    rec.close()
    assert smx.DebugLiveAllocations() > base          # the scene outlives the object, with its memory
    scene.close()
    assert smx.DebugLiveAllocations() == base


@pytest.mark.parametrize("other,max_distance,cell_size", (("coarse10", 0.5, 0.0), ("coarse3", 0.02, 0.05), ("filled", 0.02, 0.0)))
def test_compare_to_a_scene_equals_the_side_of_compare_meshes(world, other, max_distance, cell_size):
    """The fixtures of tests/test_gpu_compare.py: the world's triangle array against three meshes derived from it."""
    from surfelmeshing_amd import meshing
    rec, fine = world["rec"], world["tri"]
    onto = dict(coarse10=lambda: rec.DecimateMesh(None, fine, 0.1)[0], coarse3=lambda: rec.DecimateMesh(None, fine, 0.03)[0],
                filled=lambda: rec.FillHoles(None, fine)[0])[other]()
    N, SEED = 600, 17
    with meshing.build_distance_scene(rec, onto, max_distance, cell_size) as scene:
        used = scene.stats["cell_size_used"]
        want = rec.CompareMeshes(None, fine, onto, max_distance, N, SEED, used, directions=1)
        got = rec.CompareToDistanceScene(None, fine, scene, max_distance, N, SEED)
        assert got == want["a_to_b"], (got, want["a_to_b"])
        assert got["distance"]["n_matched"] > N // 2 and got["sum_d"] > 0 and got["distance"]["cell_size_used"] == used
        # the helper with scene_b=: the A -> B side from the scene, the other side as without one
        both = meshing.compare_meshes(rec, fine, onto, max_distance, N, SEED, used, directions=3)
        assert meshing.compare_meshes(rec, fine, onto, max_distance, N, SEED, used, directions=3, scene_b=scene) == both
        assert meshing.compare_meshes(rec, fine, onto, max_distance, N, SEED, used, directions=1, scene_b=scene) == want
        two = meshing.compare_meshes(rec, fine, onto, max_distance, N, SEED, used, directions=2)
        assert meshing.compare_meshes(rec, fine, onto, max_distance, N, SEED, used, directions=2, scene_b=scene) == two
        # device tensors
        import torch
        tf = torch.from_numpy(fine.astype(np.int32)).cuda()
        assert rec.CompareToDistanceScene(None, tf, scene, max_distance, N, SEED) == got
        # a smaller distance than the bound, and no samples
        if max_distance > 0.02:
            small = rec.CompareToDistanceScene(None, fine, scene, 0.02, N, SEED)
            assert small == rec.CompareMeshes(None, fine, onto, 0.02, N, SEED, used, directions=1)["a_to_b"]
        none = rec.CompareToDistanceScene(None, fine, scene, max_distance, 0, SEED)
        assert none["sample"]["n_samples"] == 0 and none["distance"]["n_points"] == 0 and none["sum_d"] == 0


def test_compare_to_a_scene_stages_host_triangles_and_nothing_else(smx):
    """With host triangles the call stages them and hands the sampler device arrays: the samples are drawn straight into the
    comparison's workspace, so the host call holds one block more than the device call (the staged triangles), not a second
    set of sample buffers."""
    import torch
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    fine, _ = rec.Triangulate(None)
    coarse, _ = rec.DecimateMesh(None, fine, 0.2)
    with rec.BuildDistanceScene(None, fine, 0.3) as scene:
        on_device = rec.CompareToDistanceScene(None, torch.from_numpy(coarse.astype(np.int32)).cuda(), scene, 0.3, 500, 5)
        blocks = smx.DebugLiveAllocations()[0]
        on_host = rec.CompareToDistanceScene(None, coarse, scene, 0.3, 500, 5)
        assert on_host == on_device and on_host["distance"]["n_matched"] > 250
        assert smx.DebugLiveAllocations()[0] == blocks + 1
        assert on_host == rec.CompareMeshes(None, coarse, fine, 0.3, 500, 5, scene.stats["cell_size_used"], directions=1)["a_to_b"]
    rec.close()


def test_the_helpers_with_a_scene_equal_themselves_without(smx):
    from surfelmeshing_amd import meshing
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    fine, _ = rec.Triangulate(None)
    coarse, _ = rec.DecimateMesh(None, fine, 0.2)
    pts = np.ascontiguousarray((m[0][:300] * 1.01).astype(np.float32))
    with meshing.build_distance_scene(rec, coarse, 0.3, 0.4) as scene:
        assert scene.stats["cell_size_used"] == float(dr.cell_used(0.4, 0.3)) and scene.device_bytes == scene.stats["device_bytes"] > 0
        want = meshing.decimation_error(rec, fine, coarse, 0.3, cell_size=0.4)
        got = meshing.decimation_error(rec, fine, None, 0.3, scene=scene)
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]
        for q, signed in ((0.3, False), (0.05, True)):
            want = meshing.mesh_distance(rec, coarse, pts, q, 0.4, signed, return_closest=True)
            _same(meshing.mesh_distance(None, None, pts, q, signed=signed, return_closest=True, scene=scene), want, (q, signed))
        with pytest.raises(ValueError):
            meshing.mesh_distance(rec, coarse, pts, 0.5, scene=scene)
    rec.close()


LINE = r"(\d+) of (\d+) points matched \(([0-9.]+) %\): mean ([0-9.]+) mm, rms ([0-9.]+) mm, max ([0-9.]+) mm; 50 / 90 / 99 % below ([0-9.]+) mm / ([0-9.]+) mm / ([0-9.]+) mm"


def _run_tum(tmp_path, frames):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "8",
                        "--outlier_filtering_frame_count", "2", "--mesh", "--mesh_eval", "0.05", "--mesh_eval_frames", str(frames)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    one = re.search(r"surface error within 0.05 m, ground truth of (\d+) frames to the mesh \(true poses\): " + LINE, r.stdout)
    assert one, r.stdout[-1500:]
    lines = re.findall(r"scene points of frame (\d+): " + LINE, r.stdout)
    total = re.search(r"scene points of (\d+) frames: " + LINE, r.stdout)
    assert total and re.search(r"scene points: one scene of \d+ triangles \(\d+ bytes on the device\) built in", r.stdout), r.stdout[-1500:]
    return one.groups(), lines, total.groups()


def test_run_tum_measures_the_points_of_several_frames_against_one_scene(tmp_path):
    """--mesh_eval_frames 3: three lines and a total.  The --mesh_eval line measures the points of ALL integrated frames (six
    here) in one call, so it is the TOTAL of a run over all six frames that has its figures, which the next test checks; what
    holds at 3 is that the total adds up from the lines and that the last line is the last integrated frame's."""
    one, lines, total = _run_tum(tmp_path, 3)
    assert len(lines) == 3 and [int(ln[0]) for ln in lines] == [4, 5, 6], lines
    assert int(total[0]) == 3 and int(total[1]) == sum(int(ln[1]) for ln in lines) and int(total[2]) == sum(int(ln[2]) for ln in lines)
    assert int(one[0]) == 6 and int(total[2]) < int(one[2])
    print("\n".join(" ".join(ln) for ln in lines))


def test_run_tum_over_every_integrated_frame_totals_to_the_mesh_eval_line(tmp_path):
    one, lines, total = _run_tum(tmp_path, 6)
    assert len(lines) == 6 and [int(ln[0]) for ln in lines] == [1, 2, 3, 4, 5, 6], lines
    assert total == one, (total, one)
