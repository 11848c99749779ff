"""smx_recon_import_points on the device: every case of tests/import_cases.py against the model of tests/import_ref.py byte for
byte (all 25 rows of every slot, point_to_slot through host and device pointers, every statistic), in all three modes of the
neighbour search and twice for the same bytes; the refusals; and what comes after an import: triangulation, a merge, the frame
loop, the delta hand-off and the command-line tool.  All comparisons are equalities."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import import_cases as ic
import import_ref as ir
import merge_ref as mr
import mesh_ref
from common import ROOT, small_pre, small_stream
from test_gpu_parity import _compare_state, _pipes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def modelled():
    """{case name: (case, model answer)}, computed once and left unchanged."""
    return {c.name: (c, c.model()) for c in ic.cases()}


@pytest.fixture(scope="module")
def sphere():
    pos, nrm, r2 = mesh_ref.sphere_map()
    P = np.ascontiguousarray(pos.astype(np.float32))
    kw = dict(k=16, search_radius=0.2, radius_rank=8, radius_scale_squared=2.0, orient=ir.ORIENT_ORIGINS)
    rows, p2s, st, ex = ir.import_model(P, None, 2.0 * P, ir.params(**kw))
    tri = mesh_ref.triangulate(*mesh_ref.map_of_rows(rows))[0]
    return P, kw, rows, st, tri


def _camera(smx):
    return smx.PinholeCamera4f(96, 72, 80.0, 80.0, 48.0, 36.0)


def _map(smx, rows, capacity, merge_count=0):
    rec = smx.CUDASurfelReconstruction(max(int(capacity), 1), _camera(smx))
    if rows.shape[1]:
        rec.debug_upload_surfels(np.ascontiguousarray(rows, np.float32), merge_count)
    return rec


def _pod(p):
    from surfelmeshing_amd import _lib
    return _lib.ImportParams(p["cell_size"], p["search_radius"], p["k"], p["min_neighbors"], p["max_surface_variation"], p["radius_rank"],
                             p["radius_scale_squared"], p["confidence"], p["default_color"], p["frame_index"], p["orient"],
                             (C.c_float * 3)(*p["view_point"]))


def _assert_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = ir.comparable(got), ir.comparable(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d words differ, first at row %d slot %d (%08x vs %08x)" % (
        what, len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])])


def _import(smx, c, query_mode=None, device=False):
    """One import of case c into a fresh object: (rows afterwards, point_to_slot or None, stats, failed)."""
    from surfelmeshing_amd import _lib
    rec = _map(smx, c.old_rows, c.max_surfels)
    nn = smx.SurfelNeighborIndex()
    try:
        if query_mode is not None:
            nn.set_query_mode(query_mode)
        n = c.points.shape[0]
        failed = False
        if device:
            import torch
            dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()
            pts, col, org = dev(c.points), dev(c.colors), dev(c.origins)
            out = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            addr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
            st = _lib.ImportStats()
            rc = _lib.load().smx_recon_import_points(rec._h, None, nn._h, addr(pts), addr(col), addr(org), C.c_uint32(n), C.c_int32(1),
                                                     C.byref(_pod(c.prm)), C.c_void_p(out.data_ptr()), C.c_uint32(n), C.c_int32(1), C.byref(st))
            stats, failed = smx.import_stats_dict(st), rc != 0
            p2s = out.cpu().numpy().view(np.uint32)[:n].copy()
        else:
            try:
                stats, p2s = rec.ImportPoints(None, c.points, c.colors, c.origins, index=nn, return_map=True, params=_pod(c.prm))
            except _lib.SmxError:
                stats, p2s, failed = rec.last_import_stats, None, True
        assert rec.surfels_size() == stats["new_size"]
        rows = rec.debug_download_surfels(stats["new_size"]) if stats["new_size"] else ir.blank_rows(0)
        return rows, (None if failed else p2s), stats, failed
    finally:
        nn.close()
        rec.close()


def _check(c, model, got, what):
    rows, p2s, st, ex = model
    grows, gp2s, gst, failed = got
    assert failed == ex["failed"], what
    assert gst == st, (what, gst, st)
    _assert_rows(grows, rows, what)
    if not failed:
        assert np.array_equal(gp2s, p2s), what


@pytest.mark.parametrize("name", [c.name for c in ic.cases()])
def test_every_case_equals_the_model(smx, modelled, name):
    c, model = modelled[name]
    first = _import(smx, c)
    _check(c, model, first, (name, "host pointers"))
    _check(c, model, _import(smx, c, device=True), (name, "device pointers"))
    for query_mode in (0, 1, 2):
        _check(c, model, _import(smx, c, query_mode=query_mode), (name, "query mode %d" % query_mode))
    again = _import(smx, c)
    assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32)) and first[2] == again[2]


def test_refusals_leave_the_map_unchanged(smx, modelled):
    from surfelmeshing_amd import _lib
    gc.collect()       # (objects other tests dropped go now, not in the middle of the count)
    blocks0 = smx.DebugLiveAllocations()[0]
    c, model = modelled["non_empty_map"]
    n_old, n = c.old_rows.shape[1], c.points.shape[0]
    rec, nn = _map(smx, c.old_rows, c.max_surfels, merge_count=3), smx.SurfelNeighborIndex()
    pod = _pod(c.prm)

    def unchanged(what):
        assert rec.surfels_size() == n_old and rec.stats()["merge_count"] == 3, what
        _assert_rows(rec.debug_download_surfels(n_old), c.old_rows, what)

    # a point_to_slot that is too small
    small = np.zeros(n - 1, np.uint32)
    st = _lib.ImportStats()
    rc = _lib.load().smx_recon_import_points(rec._h, None, nn._h, c.points.ctypes.data_as(C.c_void_p), c.colors.ctypes.data_as(C.c_void_p), None,
                                             C.c_uint32(n), C.c_int32(0), C.byref(pod), small.ctypes.data_as(C.c_void_p), C.c_uint32(n - 1),
                                             C.c_int32(0), C.byref(st))
    assert rc == -1 and not small.any()
    unchanged("capacity of point_to_slot")
    # a bad parameter with a live object
    with pytest.raises(_lib.SmxError):
        rec.ImportPoints(None, c.points, index=nn, params=_lib.ImportParams.defaults(k=3))
    unchanged("k = 3")
    # an allocation that fails, at every position of the call's allocations
    failures = 0
    for nth in range(64):
        smx.DebugFailAllocation(nth)
        try:
            stats, p2s = rec.ImportPoints(None, c.points, c.colors, index=nn, return_map=True, params=pod)
        except _lib.SmxError:
            failures += 1
            unchanged("allocation %d failed" % nth)
            continue
        finally:
            smx.DebugFailAllocation(-1)
        break
    else:
        raise AssertionError("the call never got through")
    assert failures >= 10, failures      # (the workspace's blocks, the staging of host inputs, the index)
    assert stats == model[2] and np.array_equal(p2s, model[1])
    assert rec.stats()["merge_count"] == 3 and rec.surfels_size() == stats["new_size"]
    _assert_rows(rec.debug_download_surfels(stats["new_size"]), model[0], "after the failures")
    timings = rec.debug_import_timings()
    assert timings["whole"] > 0 and abs(sum(v for k, v in timings.items() if k != "whole") - timings["whole"]) < 1e-3 * timings["whole"] + 1e-3
    # an empty cloud changes nothing
    assert rec.ImportPoints(None, np.zeros((0, 3), np.float32), index=nn)["new_size"] == stats["new_size"]
    _assert_rows(rec.debug_download_surfels(stats["new_size"]), model[0], "after an empty cloud")
    for o in (nn, rec):
        o.close()
    # over-full: the counts say how much room was needed
    c, model = modelled["capacity_one_short"]
    rows, p2s, stats, failed = _import(smx, c)
    assert failed and stats["n_imported"] == 40 and stats["old_size"] == stats["new_size"] == 3
    _assert_rows(rows, c.old_rows, "over-full")
    assert smx.DebugLiveAllocations()[0] == blocks0


def test_sphere_import_then_triangulate(smx, sphere):
    from surfelmeshing_amd import meshing
    P, kw, rows, st, tri = sphere
    rec, gst = meshing.map_from_points(P, origins=2.0 * P, **kw)
    assert gst == st
    _assert_rows(rec.debug_download_surfels(gst["new_size"]), rows, "sphere")
    got, ts = rec.Triangulate(None)
    assert ts["truncated_lists"] == 0 and ts["star_overflow"] == 0
    mesh_ref.assert_sets_close(got, tri, "sphere")
    rec.close()


def test_import_then_merge_into_the_other_half(smx, sphere):
    """The imported half z >= -0.1 of the sphere into a map holding the half z <= 0.1: merge_ref on the imported rows."""
    from surfelmeshing_amd import meshing
    P, kw, rows, st, tri = sphere
    upper = P[:, 2] >= -0.1
    lower_rows = np.ascontiguousarray(rows[:, P[:, 2] <= 0.1])
    src, ist = meshing.map_from_points(P[upper], origins=2.0 * P[upper], **kw)
    src_rows = src.debug_download_surfels(ist["new_size"])
    want_src = ir.import_model(P[upper], None, 2.0 * P[upper], ir.params(**kw))[0]
    _assert_rows(src_rows, want_src, "upper half")
    dst = _map(smx, lower_rows, 8192)
    T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    stats = meshing.merge_maps(dst, src, T.reshape(3, 4), mode="blend", frame_index=3)
    want_rows, _, want_stats, _ = mr.merge_model(lower_rows, want_src, T, mr.params(mode=mr.BLEND, frame_index=3))
    assert stats == want_stats and stats["n_matched"] > 100 and stats["n_appended"] > 1000
    got = dst.debug_download_surfels(stats["new_size"])
    assert np.array_equal(mr.comparable(got), mr.comparable(want_rows))
    # the same through the helper that imports into a temporary object
    dst2 = _map(smx, lower_rows, 8192)
    ist2, mst2 = meshing.merge_points(dst2, P[upper], T.reshape(3, 4), origins=2.0 * P[upper], import_params=kw, mode="blend", frame_index=3)
    assert ist2 == ist and mst2 == want_stats
    assert np.array_equal(mr.comparable(dst2.debug_download_surfels(mst2["new_size"])), mr.comparable(want_rows))
    for o in (src, dst, dst2):
        o.close()


def _grow(smx, s, frames):
    from surfelmeshing_amd.pipeline import FramePipeline
    p = FramePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, small_pre(s.width))
    for f in range(min(frames) - 4, max(frames) + 5):
        p.upload(f, *s.frame(f))
    for f in frames:
        p.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    return p


def test_frame_loop_after_an_import_matches_oracle(smx):
    """A grown from the first half of the stream; the surfel positions of B, grown from the second half, imported into A as a
    cloud; then further frames: A, a fresh object that received the same rows by upload, and the oracle stay equal."""
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    pa, pb = _grow(smx, s, list(range(4, 14))), _grow(smx, s, list(range(14, 24)))
    ra, rb = pa.reconstruction, pb.reconstruction
    cloud = rb.debug_download_surfels(rb.surfels_size())
    cloud = np.ascontiguousarray(cloud[3:6, ~(cloud[7] < 0)].T)[:4000]
    merge_count = ra.stats()["merge_count"]
    old = ra.debug_download_surfels(ra.surfels_size())
    kw = dict(search_radius=0.05, k=16, frame_index=24, orient=ir.ORIENT_VIEW_POINT, cell_size=0.02)
    stats = ra.ImportPoints(pa.stream, cloud, params=_pod(ir.params(**kw)))
    want_rows, _, want_stats, _ = ir.import_model(cloud, None, None, ir.params(**kw), old_rows=old)
    assert stats == want_stats and stats["n_imported"] > 1000 and ra.stats()["merge_count"] == merge_count
    n = stats["new_size"]
    rows = ra.debug_download_surfels(n)
    _assert_rows(rows, want_rows, "import into a grown map")
    po, pf = _pipes(smx, s, 60000)
    pf.reconstruction.debug_upload_surfels(rows, merge_count)
    po.recon.surfels()[:, :n] = rows
    po.recon.set_counts(n, merge_count)
    frames = list(range(25, 33))
    for f in range(frames[0] - 4, frames[-1] + 5):
        d, c = s.frame(f)
        for p in (pa, po, pf):
            p.upload(f, d, c)
    for f in frames:
        others, T, pose = s.outlier_frames(f), s.others_TR_reference(f), s.pose(f)
        for p in (po, pf, pa):
            p.process(f, others, T, pose)
        _compare_state(po, pf)
        _compare_state(po, pa)
    assert po.recon.surfels_size > n


def test_delta_hand_off_delivers_the_appended_slots(smx, modelled):
    c, model = modelled["non_empty_map"]
    rec = _map(smx, c.old_rows, c.max_surfels)
    rec.SetDeltaTracking(None, True)
    assert rec.TransferChangedToCPU(None, 1).count == c.old_rows.shape[1]
    assert rec.TransferChangedToCPU(None, 2).count == 0
    stats = rec.ImportPoints(None, c.points, c.colors, params=_pod(c.prm))
    d = rec.TransferChangedToCPU(None, 3)
    want = model[3]["dirty"]
    assert d.count == want.size == stats["n_imported"] and d.surfel_count == stats["new_size"]
    assert np.array_equal(d.surfel_index[:d.count], want)
    assert np.array_equal(d.x[:d.count].view(np.uint32), model[0][3, want].view(np.uint32))
    assert np.array_equal(d.last_update_stamp[:d.count], ir.u32(model[0])[18, want])
    assert rec.TransferChangedToCPU(None, 4).count == 0
    rec.close()


def test_mesh_ply_tool(smx, sphere, tmp_path):
    from surfelmeshing_amd import export
    P, kw, rows, st, tri = sphere
    # (the tool orients by one view point; from the centre every normal of the sphere points inwards, consistently)
    want_rows = ir.import_model(P, None, None, ir.params(k=16, search_radius=0.2, orient=ir.ORIENT_VIEW_POINT))[0]
    want = mesh_ref.triangulate(*mesh_ref.map_of_rows(want_rows))[1]["n_triangles"]
    ply, obj = tmp_path / "sphere.ply", tmp_path / "sphere.obj"
    export.write_ply(str(ply), P)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mesh_ply.py"), str(ply), "--export_mesh", str(obj), "--search_radius", "0.2",
                        "--view_point", "0,0,0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "imported 4000 of 4000 points (bad 0, sparse 0, degenerate 0, rough 0; 4000 lists full)" in r.stdout
    lines = obj.read_text().splitlines()
    faces = sum(1 for l in lines if l.startswith("f "))
    assert sum(1 for l in lines if l.startswith("v ")) == 4000
    assert abs(faces - want) <= int(np.ceil(0.001 * want)), (faces, want)      # (mesh_ref.assert_sets_close's rule for float32 against float64)
