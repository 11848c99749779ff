"""smx_recon_mesh_distance on the device.  The contract (include/smx.h) is made of integers and of float32 expressions that numpy
reproduces bit for bit, and its answer is the minimum over ALL triangles, so everything here is compared for EQUALITY with the
brute-force model of tests/distance_ref.py: nearest, distance, closest and every statistic (the grid's three counts whenever the
cell size is given; cell_size_used never)."""
import ctypes as C

import numpy as np
import pytest

import components_ref as cr
import decimate_ref as dr_dec
import distance_ref as dr
import fill_ref as fr
import mesh_ref as mr

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
GRID = ("n_wide", "n_entries", "n_cells")


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


def _cells(max_distance):
    return (0.0, float(dr.MARGIN * dr.F(max_distance)), 1e-3, 100.0)


def _check(got, want, m, tri, max_distance, cell_size, what):
    """got / want: (nearest, distance, closest, stats)."""
    gst, wst = dict(got[3]), dict(want[3])
    used = gst.pop("cell_size_used")
    if cell_size > 0:
        assert used == float(dr.cell_used(cell_size, max_distance)), what
        wst.update(dr.structure(m[0], m[2], tri, cell_size, max_distance))
    else:
        assert used >= float(dr.cell_used(0.0, max_distance)), what
        for k in GRID:
            gst.pop(k)
    assert gst == wst, (what, gst, wst)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32 and got[2].dtype == np.float32
    for k, name in enumerate(("nearest", "distance", "closest")):
        assert got[k].tobytes() == want[k].tobytes(), (what, name, int(np.sum(got[k].view(np.uint32) != want[k].view(np.uint32))))


@pytest.mark.parametrize("name", list(dr.point_sets()))
def test_every_point_set_equals_the_model(world, name):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    pts, model = dr.point_sets()[name], dr.model_of(name)
    for signed in (False, True):
        for md in dr.MAX_DISTANCES:
            want = dr.answer(model, md, signed)
            for cs in _cells(md):
                got = rec.MeshDistance(None, tri, pts, md, cs, signed, return_closest=True)
                _check(got, want, m, tri, md, cs, "%s max %g cell %g signed %d" % (name, md, cs, signed))
            print("%s max %g signed %d: %d of %d matched, bad %d, dropped %d / %d / %d" % (
                name, md, signed, want[3]["n_matched"], want[3]["n_points"], want[3]["n_bad_points"], want[3]["n_not_live"],
                want[3]["n_repeated"], want[3]["n_out_of_range"]))
    t = rec.debug_distance_timings()
    assert set(t) == {"mark", "index", "query", "stats"} and all(np.isfinite(v) and v >= 0 for v in t.values())


def _raw(rec, tri, n_in, pts, n_points, nearest, distance, closest, max_distance=0.02, cell_size=0.0, signed=0, on_device=0, stats=True):
    """The C call itself; arrays: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    prm, st = _lib.DistanceParams(max_distance, cell_size, signed), _lib.DistanceStats()
    rc = _lib.load().smx_recon_mesh_distance(rec._h, None, C.byref(prm), ptr(tri), C.c_uint32(n_in), ptr(pts), C.c_uint32(n_points),
                                             ptr(nearest), ptr(distance), ptr(closest), C.c_int32(on_device), C.byref(st) if stats else None)
    return rc, st


def _guards(P, extra=4):
    return np.full(P + extra, GUARD, np.uint32), np.full(P + extra, GUARD, np.uint32), np.full(3 * P + extra, GUARD, np.uint32)


def test_calling_rules_on_host_and_device_arrays(smx, world):
    from surfelmeshing_amd import api
    rec, tri, m = world["rec"], world["tri"], world["m"]
    name = "around the hand-made triangles"
    pts = dr.point_sets()[name]
    P, n_in, n = pts.shape[0], tri.shape[0], m[0].shape[0]
    wn, wd, wc, wst = dr.answer(dr.model_of(name), 0.02, True)
    # host arrays pre-filled with a guard word; room to spare stays untouched
    nearest, distance, closest = _guards(P)
    rc, st = _raw(rec, tri, n_in, pts, P, nearest, distance, closest, signed=1)
    assert rc == 0 and nearest[:P].tobytes() == wn.tobytes() and distance[:P].tobytes() == wd.tobytes() and closest[:3 * P].tobytes() == wc.tobytes()
    assert np.all(nearest[P:] == GUARD) and np.all(distance[P:] == GUARD) and np.all(closest[3 * P:] == GUARD)
    gst = api.distance_stats_dict(st)
    assert {k: gst[k] for k in wst if k != "max_distance"} == {k: v for k, v in wst.items() if k != "max_distance"}
    # closest = NULL and stats = NULL leave the other outputs as they are
    n2, d2, _ = _guards(P)
    rc, _ = _raw(rec, tri, n_in, pts, P, n2, d2, None, signed=1, stats=False)
    assert rc == 0 and n2.tobytes() == nearest.tobytes() and d2.tobytes() == distance.tobytes()
    # an index >= n, anywhere: refused, nothing written
    for where in (0, 3 * (n_in // 2) + 1, 3 * n_in - 1):
        bad = tri.copy()
        bad.reshape(-1)[where] = n
        g = _guards(P)
        assert _raw(rec, bad, n_in, pts, P, *g)[0] == -1 and all(np.all(a == GUARD) for a in g)
    # an output over an input: refused, nothing written
    both = np.concatenate([pts.reshape(-1).view(np.uint32), np.full(8, GUARD, np.uint32)])
    snapshot = both.copy()
    g = _guards(P)
    assert _raw(rec, tri, n_in, both, P, g[0], g[1], both[3 * P - 1:])[0] == -1 and both.tobytes() == snapshot.tobytes()
    # n_in == 0: every point is "none"; n_points == 0: only the triangles' statistics
    g = _guards(P)
    rc, st = _raw(rec, None, 0, pts, P, *g)
    assert rc == 0 and np.all(g[0][:P] == dr.INVALID) and np.all(np.isinf(g[1][:P].view(np.float32))) and np.all(np.isnan(g[2][:3 * P].view(np.float32)))
    assert st.n_matched == 0 and st.n_in == 0 and st.n_points == P and st.n_bad_points == wst["n_bad_points"] and np.all(g[0][P:] == GUARD)
    g = _guards(P)
    rc, st = _raw(rec, tri, n_in, None, 0, None, None, None, cell_size=0.05)
    assert rc == 0 and st.n_points == 0 and st.n_not_live == wst["n_not_live"] and st.n_repeated == 1 and st.n_out_of_range == 1
    assert {k: int(getattr(st, k)) for k in GRID} == dr.structure(m[0], m[2], tri, 0.05, 0.02)
    # device arrays give the same bytes
    din, dpt = smx.CUDABuffer(1, 3 * n_in, np.uint32), smx.CUDABuffer(1, 3 * P, np.uint32)
    outs = [smx.CUDABuffer(1, k, np.uint32) for k in (P + 4, P + 4, 3 * P + 4)]
    din.Upload(tri.reshape(1, -1))
    dpt.Upload(pts.reshape(1, -1).view(np.uint32))
    for b, k in zip(outs, (P + 4, P + 4, 3 * P + 4)):
        b.Upload(np.full((1, k), GUARD, np.uint32))
    a = [b.ToCUDA().address for b in [din, dpt] + outs]
    rc, st = _raw(rec, a[0], n_in, a[1], P, a[2], a[3], a[4], signed=1, on_device=1)
    back = [b.Download()[0] for b in outs]
    assert rc == 0 and back[0].tobytes() == nearest.tobytes() and back[1].tobytes() == distance.tobytes() and back[2].tobytes() == closest.tobytes()
    assert din.Download()[0].tobytes() == tri.tobytes() and dpt.Download()[0].tobytes() == pts.tobytes()
    bad = tri.copy()
    bad[n_in // 3, 2] = n
    din.Upload(bad.reshape(1, -1))
    outs[0].Upload(np.full((1, P + 4), GUARD, np.uint32))
    assert _raw(rec, a[0], n_in, a[1], P, a[2], a[3], a[4], on_device=1)[0] == -1 and np.all(outs[0].Download()[0] == GUARD)
    assert _raw(rec, a[0], n_in, a[1], P, a[1] + 8, a[3], a[4], on_device=1)[0] == -1          # overlap on the device
    for b in [din, dpt] + outs:
        b.close()
    # device tensors through the Python call
    import torch
    tt, tp = torch.from_numpy(tri.astype(np.int32)).cuda(), torch.from_numpy(pts.copy()).cuda()
    tn, td, tc, tst = rec.MeshDistance(None, tt, tp, 0.02, signed=True, return_closest=True)
    torch.cuda.synchronize()
    assert tn.cpu().numpy().view(np.uint32).tobytes() == wn.tobytes() and td.cpu().numpy().tobytes() == wd.tobytes()
    assert tc.cpu().numpy().tobytes() == wc.tobytes() and tst["n_matched"] == wst["n_matched"]


def test_on_the_outputs_of_the_mesh_services(world):
    """One case each: Triangulate's, DecimateMesh's, MeshComponents' and FillHoles' array of the same map."""
    rec, m, info = world["rec"], world["m"], world["info"]
    pos, nrm, r2 = m
    pts = dr.point_sets()["centroids moved both ways"][:300]
    meshed, _ = rec.Triangulate(None)
    clean, _ = rec.MeshComponents(None, meshed, min_triangles=3)
    filled, _ = rec.FillHoles(None, clean)
    coarse, _ = rec.DecimateMesh(None, meshed, 0.1)
    assert clean.tobytes() == cr.components(pos, r2, meshed, min_triangles=3)[0].tobytes()
    assert filled.tobytes() == fr.fill(pos, nrm, r2, clean)[0].tobytes() and coarse.tobytes() == dr_dec.decimate(pos, r2, meshed, 0.1)[0].tobytes()
    for what, arr, md in (("triangulated", meshed, 0.02), ("cleaned", clean, 0.02), ("filled", filled, 0.02), ("decimated", coarse, 0.5)):
        want = dr.answer(dr.brute(pos, r2, arr, pts), md, True)
        got = rec.MeshDistance(None, arr, pts, md, 0.0, True, return_closest=True)
        _check(got, want, m, arr, md, 0.0, what)
        print("%s: %d triangles, %d of %d matched" % (what, arr.shape[0], want[3]["n_matched"], pts.shape[0]))
        assert want[3]["n_matched"] > 100


def test_decimation_error_of_the_sphere_equals_the_model(smx):
    from surfelmeshing_amd import meshing
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    fine, _ = rec.Triangulate(None)
    coarse, _ = rec.DecimateMesh(None, fine, 0.2)
    summary, nearest, distance, stats = meshing.decimation_error(rec, fine, coarse, 0.3, cell_size=0.4)
    used = np.unique(fine)
    pts = m[0].astype(np.float32)[used.astype(np.int64)]
    wn, wd, _, wst = dr.answer(dr.brute(m[0], m[2], coarse, pts), 0.3)
    wst.update(dr.structure(m[0], m[2], coarse, 0.4, 0.3))
    stats.pop("cell_size_used")
    assert stats == wst and nearest.tobytes() == wn.tobytes() and distance.tobytes() == wd.tobytes()
    want = meshing.distance_summary(wd, wst)
    print("decimation at 0.2 m of the unit sphere (%d -> %d triangles): %s" % (fine.shape[0], coarse.shape[0], meshing.format_distance_summary(summary)))
    assert summary == want and summary["n_matched"] == used.size and 0.0 < summary["mean"] < 0.05
    rec.close()


def test_two_calls_give_the_same_bytes_and_a_smaller_call_reuses_the_workspace(smx, world):
    rec, tri = world["rec"], world["tri"]
    pts = dr.point_sets()["random in the box"]
    first = rec.MeshDistance(None, tri, pts, 0.5, 0.0, True, return_closest=True)
    live = smx.DebugLiveAllocations()
    again = rec.MeshDistance(None, tri, pts, 0.5, 0.0, True, return_closest=True)
    assert first[3] == again[3] and all(first[k].tobytes() == again[k].tobytes() for k in range(3))
    small = rec.MeshDistance(None, tri[:2000], pts[:100], 0.5, 0.0, True, return_closest=True)
    assert smx.DebugLiveAllocations() == live
    m = world["m"]
    _check(small, dr.answer(dr.brute(m[0], m[2], tri[:2000], pts[:100]), 0.5, True), m, tri[:2000], 0.5, 0.0, "smaller")


def test_a_failed_allocation_writes_nothing_and_close_frees_everything(smx):
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    pts = np.ascontiguousarray((m[0][:200] * 1.002).astype(np.float32))
    wn, wd, wc, wst = dr.answer(dr.brute(m[0], m[2], tri, pts), 0.02)
    P, n_in = pts.shape[0], tri.shape[0]
    failed = []
    try:
        for nth in range(40):
            g = _guards(P, 0)
            smx.DebugFailAllocation(nth)
            rc = _raw(rec, tri, n_in, pts, P, *g)[0]
            if rc == 0:
                break
            failed.append(rc)
            assert rc == -2 and all(np.all(a == GUARD) for a in g), nth        # the allocation error, nothing written
            smx.DebugFailAllocation(-1)
            got = rec.MeshDistance(None, tri, pts, 0.02, return_closest=True)    # the next call succeeds
            assert got[0].tobytes() == wn.tobytes() and got[1].tobytes() == wd.tobytes() and got[2].tobytes() == wc.tobytes()
            rec.close()                       # a fresh object for the next allocation in line
            rec = _rec_of(smx, m)
    finally:
        smx.DebugFailAllocation(-1)
    # from the first allocation of the call (the counters) to its last (the cell table)
    assert rc == 0 and 15 <= len(failed) < 40, "the call reached %d allocations" % len(failed)
    assert g[0].tobytes() == wn.tobytes() and g[1].tobytes() == wd.tobytes() and g[2].tobytes() == wc.tobytes()
    assert smx.DebugLiveAllocations() > base
    rec.close()
    assert smx.DebugLiveAllocations() == base


def test_no_side_effects(smx):
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    nn = smx.SurfelNeighborIndex()
    full, full_st = rec.Triangulate(None)                        # (before the update state exists: the full call does not keep it)
    tri, st, us = rec.TriangulateUpdate(None, index=nn)
    assert us["mode"] == 1
    n = rec.surfels_size()
    rec.SetDeltaTracking(None, True)
    rec.TransferChangedToCPU(None, 1)                            # enabling marks every slot; the hand-off clears the marks
    rows_before, stats_before = rec.debug_download_surfels(n), rec.stats()
    pts = np.ascontiguousarray((m[0][:500] * 0.999).astype(np.float32))
    out = rec.MeshDistance(None, tri, pts, 0.05, signed=True)
    assert out[2]["n_matched"] == 500 and int(np.sum(out[1] < 0)) > 0
    assert rec.stats() == stats_before and rec.surfels_size() == n and rec.surfel_count() == n
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()
    assert rec.TransferChangedToCPU(None, 2).count == 0
    mesh_again, st2, us2 = rec.TriangulateUpdate(None, index=nn)
    assert us2["mode"] == 0 and us2["n_changed"] == 0 and mesh_again.tobytes() == tri.tobytes() and st2 == st
    full2, full_st2 = rec.Triangulate(None)
    assert full2.tobytes() == full.tobytes() and full_st2 == full_st
    nn.close()
    rec.close()


def test_a_synthetic_reconstruction_against_its_ground_truth(smx):
    """Eight frames of the 160 x 120 synthetic stream integrated at the true poses, meshed, and the noise-free surface points of
    those frames measured against the mesh.  The accuracy figures are printed, not gated; at least half of the points match."""
    from common import small_pre, small_stream
    from surfelmeshing_amd import meshing
    from surfelmeshing_amd.pipeline import FramePipeline
    s = small_stream()
    pipe = FramePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, small_pre(s.width))
    frames = list(range(4, 12))
    for f in range(0, 16):
        pipe.upload(f, *s.frame(f))
    for f in frames:
        pipe.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    rec = pipe.reconstruction
    tri, _ = meshing.mesh_map(rec)
    truth = np.concatenate([s.surface_points(f, 2) for f in frames])
    nearest, distance, closest, stats = rec.MeshDistance(None, tri, truth, 0.05, return_closest=True)
    summary = meshing.distance_summary(distance, stats)
    print("%d surfels, %d triangles; %s" % (rec.surfels_size(), tri.shape[0], meshing.format_distance_summary(summary)))
    assert summary["matched_fraction"] >= 0.5
    n = rec.surfels_size()
    pos, nrm, r2 = mr.map_of_rows(rec.debug_download_surfels(n), n)
    sub = np.random.default_rng(2).permutation(truth.shape[0])[:2048]
    step = max(1, dr.MAX_PAIRS // max(1, tri.shape[0]))          # (the model takes at most MAX_PAIRS pairs at a time)
    for lo in range(0, sub.size, step):
        part = sub[lo:lo + step]
        wn, wd, wc, _ = dr.answer(dr.brute(pos, r2, tri, truth[part]), 0.05)
        assert nearest[part].tobytes() == wn.tobytes() and distance[part].tobytes() == wd.tobytes() and closest[part].tobytes() == wc.tobytes()
