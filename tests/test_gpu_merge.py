"""smx_recon_merge_map on the device: every case of tests/merge_cases.py against the model of tests/merge_ref.py byte for byte
(rows, src_to_dst through host and device pointers, every statistic, src untouched), independence of the query chunk and of the
neighbour search's mode, the refusals, the frame loop after a merge against the oracle, the delta hand-off and what comes after
a merge downstream (triangulation, the kept mesh, a remapped source mesh, a scene built before).  All comparisons are equalities."""
import ctypes as C
import gc

import numpy as np
import pytest

import merge_cases as mc
import merge_ref as mr
from common import small_pre, small_stream
from test_gpu_parity import _compare_state, _pipes

pytestmark = pytest.mark.gpu

MODES = {"keep": mr.KEEP_DST, "blend": mr.BLEND}


@pytest.fixture(scope="module")
def modelled():
    """{(case name, mode): (case, model answer)}, computed once and left unchanged."""
    out = {}
    for c in mc.cases():
        for mode in MODES.values():
            out[c.name, mode] = (c, mr.merge_model(c.dst, c.src, c.T, c.params(mode), c.max_surfels))
    return out


def _camera(smx):
    return smx.PinholeCamera4f(96, 72, 80.0, 80.0, 48.0, 36.0)


def _map(smx, rows, capacity, merge_count=0):
    rec = smx.CUDASurfelReconstruction(max(int(capacity), 1), _camera(smx))
    rec.debug_upload_surfels(np.ascontiguousarray(rows, np.float32), merge_count)
    return rec


def _pod(smx, p):
    from surfelmeshing_amd import _lib
    return _lib.MergeParams(p["cell_size"], p["radius_factor_squared"], p["max_normal_angle_deg"], p["k"], p["mode"], p["confidence_cap"],
                            p["frame_index"])


def _assert_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = mr.comparable(got), mr.comparable(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d words differ, first at row %d slot %d (%08x vs %08x)" % (
        what, len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])])


def _merge(smx, c, mode, chunk=None, query_mode=None, device_map=False):
    """One merge of case c on fresh objects: (dst rows afterwards, src_to_dst or None, stats, failed)."""
    from surfelmeshing_amd import _lib
    dst, src = _map(smx, c.dst, c.max_surfels), _map(smx, c.src, c.src.shape[1])
    nn = smx.SurfelNeighborIndex()
    try:
        if chunk is not None:
            dst.debug_set_merge_chunk(chunk)
        if query_mode is not None:
            nn.set_query_mode(query_mode)
        n = c.src.shape[1]
        failed = False
        if device_map:
            buf = smx.CUDABuffer(1, max(n, 1), np.uint32)
            st = _lib.MergeStats()
            T = np.ascontiguousarray(c.T, np.float32)
            rc = _lib.load().smx_recon_merge_map(dst._h, None, nn._h, src._h, T.ctypes.data_as(C.c_void_p), C.byref(_pod(smx, c.params(mode))),
                                                 C.c_void_p(buf.ToCUDA().address), C.c_uint32(n), C.c_int32(1), C.byref(st))
            stats, failed = smx.merge_stats_dict(st), rc != 0
            s2d = buf.Download(None)[0][:n].copy()
            buf.close()
        else:
            try:
                stats, s2d = dst.MergeMap(None, src, c.T.reshape(3, 4), index=nn, return_map=True, params=_pod(smx, c.params(mode)))
            except _lib.SmxError:
                stats, s2d, failed = dst.last_merge_stats, None, True
        assert dst.surfels_size() == stats["new_size"]
        rows = dst.debug_download_surfels(stats["new_size"])
        _assert_rows(src.debug_download_surfels(n), c.src, c.name + ": src")      # read only
        assert src.surfels_size() == n
        return rows, (None if failed else s2d), stats, failed
    finally:
        nn.close()
        dst.close()
        src.close()


def _check(c, mode, model, got, what):
    rows, s2d, st, ex = model
    grows, gs2d, gst, failed = got
    assert failed == ex["failed"], what
    assert gst == st, (what, gst, st)
    _assert_rows(grows, rows, what)
    if not failed:
        assert np.array_equal(gs2d, s2d), what


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [c.name for c in mc.cases()])
def test_every_case_equals_the_model(smx, modelled, name, mode):
    c, model = modelled[name, MODES[mode]]
    _check(c, MODES[mode], model, _merge(smx, c, MODES[mode]), (name, mode, "host map"))
    _check(c, MODES[mode], model, _merge(smx, c, MODES[mode], device_map=True), (name, mode, "device map"))


def test_the_same_call_twice_gives_the_same_bytes(smx, modelled):
    c, _ = modelled["src_three_segments_interleaved", mr.BLEND]
    a, b = _merge(smx, c, mr.BLEND), _merge(smx, c, mr.BLEND)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("chunk,names", [(1, ("links_of_each_kind", "pose_rotation_translation", "k64_dense_patch")),
                                         (64, ("src_three_segments_interleaved", "blend_7_onto_one")),
                                         (1000, ("src_three_segments_interleaved", "dst_1024_append_across_segment")),
                                         (0, ("src_three_segments_interleaved",))])
def test_results_do_not_depend_on_the_chunk(smx, modelled, chunk, names):
    for name in names:
        for mode in MODES.values():
            c, model = modelled[name, mode]
            _check(c, mode, model, _merge(smx, c, mode, chunk=chunk), (name, mode, "chunk %d" % chunk))


@pytest.mark.parametrize("query_mode", [0, 1, 2])
def test_results_do_not_depend_on_the_query_mode(smx, modelled, query_mode):
    for name in ("src_three_segments_interleaved", "k64_dense_patch", "k1_dense_patch", "equal_d2_lower_index_wins", "on_the_ball_and_one_ulp_outside",
                 "pose_rotation_translation"):
        c, model = modelled[name, mr.BLEND]
        _check(c, mr.BLEND, model, _merge(smx, c, mr.BLEND, query_mode=query_mode), (name, "query mode %d" % query_mode))


def test_refusals_leave_dst_unchanged(smx, modelled):
    from surfelmeshing_amd import _lib
    gc.collect()       # (objects other tests dropped go now, not in the middle of the count)
    blocks0 = smx.DebugLiveAllocations()[0]
    c, model = modelled["src_three_segments_interleaved", mr.BLEND]
    dst, src, nn = _map(smx, c.dst, c.max_surfels, merge_count=3), _map(smx, c.src, c.src.shape[1]), smx.SurfelNeighborIndex()
    n_dst, n = c.dst.shape[1], c.src.shape[1]

    def unchanged(what):
        assert dst.surfels_size() == n_dst and dst.stats()["merge_count"] == 3, what
        _assert_rows(dst.debug_download_surfels(n_dst), c.dst, what)

    # a src_to_dst that is too small
    small = np.zeros(n - 1, np.uint32)
    st = _lib.MergeStats()
    T = np.ascontiguousarray(c.T, np.float32)
    pod = _pod(smx, c.params(mr.BLEND))
    rc = _lib.load().smx_recon_merge_map(dst._h, None, nn._h, src._h, T.ctypes.data_as(C.c_void_p), C.byref(pod), small.ctypes.data_as(C.c_void_p),
                                         C.c_uint32(n - 1), C.c_int32(0), C.byref(st))
    assert rc == -1 and not small.any()
    unchanged("capacity of src_to_dst")
    # an allocation that fails, at every position of the call's allocations
    failures = 0
    for nth in range(64):
        smx.DebugFailAllocation(nth)
        try:
            stats, s2d = dst.MergeMap(None, src, c.T.reshape(3, 4), index=nn, return_map=True, params=pod)
        except _lib.SmxError:
            failures += 1
            unchanged("allocation %d failed" % nth)
            continue
        finally:
            smx.DebugFailAllocation(-1)
        break
    else:
        raise AssertionError("the call never got through")
    assert failures >= 10, failures      # (the workspace's blocks, the staging buffer, the index and its query workspace)
    assert stats == model[2] and np.array_equal(s2d, model[1])
    assert dst.stats()["merge_count"] == 3 and dst.surfels_size() == stats["new_size"]
    _assert_rows(dst.debug_download_surfels(stats["new_size"]), model[0], "after the failures")
    for o in (nn, dst, src):
        o.close()
    # over-full: the model's refusal case ran in test_every_case_equals_the_model; here the counts say how much room was needed
    c, model = modelled["capacity_one_short", mr.KEEP_DST]
    rows, s2d, stats, failed = _merge(smx, c, mr.KEEP_DST)
    assert failed and stats["n_appended"] == 12 and stats["old_size"] == stats["new_size"] == 30
    assert smx.DebugLiveAllocations()[0] == blocks0


def _grow(smx, s, frames, handover):
    from surfelmeshing_amd.pipeline import FramePipeline
    p = FramePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, small_pre(s.width))
    if handover == "event_handover":
        p.reconstruction.set_handover_mode(0)
    for f in range(min(frames) - 4, max(frames) + 5):
        p.upload(f, *s.frame(f))
    for f in frames:
        p.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    return p


@pytest.mark.parametrize("mode", ["keep", "blend"])
@pytest.mark.parametrize("handover", ["default", "event_handover"])
def test_frame_loop_after_a_merge_matches_oracle(smx, mode, handover):
    """A and B grown from two halves of the stream (true poses: the identity), B merged into A, then further frames: A, a fresh
    object that received the merged rows by upload, and the oracle from the same rows stay equal after every frame."""
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    pa, pb = _grow(smx, s, list(range(4, 14)), handover), _grow(smx, s, list(range(14, 24)), handover)
    ra, rb = pa.reconstruction, pb.reconstruction
    merge_count = ra.stats()["merge_count"]
    stats = ra.MergeMap(pa.stream, rb, np.eye(4, dtype=np.float32)[:3], mode=mode, frame_index=24, cell_size=0.02)
    assert stats["n_matched"] > 100 and stats["n_appended"] > 100 and stats["new_size"] == ra.surfels_size()
    assert ra.stats()["merge_count"] == merge_count
    n = stats["new_size"]
    rows = ra.debug_download_surfels(n)
    po, pf = _pipes(smx, s, 60000)
    if handover == "event_handover":
        pf.reconstruction.set_handover_mode(0)
    pf.reconstruction.debug_upload_surfels(rows, merge_count)
    po.recon.surfels()[:, :n] = rows
    po.recon.set_counts(n, merge_count)
    frames = list(range(25, 37))
    for f in range(frames[0] - 4, frames[-1] + 5):
        pa.upload(f, *s.frame(f))

    def both(f):
        _compare_state(po, pf)
        _compare_state(po, pa)

    lo, hi = frames[0] - 4, frames[-1] + 4
    for f in range(lo, hi + 1):
        d, c = s.frame(f)
        po.upload(f, d, c)
        pf.upload(f, d, c)
    for f in frames:
        others, T, pose = s.outlier_frames(f), s.others_TR_reference(f), s.pose(f)
        for p in (po, pf, pa):
            p.process(f, others, T, pose)
        both(f)
    assert po.recon.surfels_size > n


@pytest.mark.parametrize("mode", ["keep", "blend"])
def test_delta_hand_off_delivers_the_appended_and_blended_slots(smx, modelled, mode):
    c, model = modelled["src_three_segments_interleaved", MODES[mode]]
    dst, src = _map(smx, c.dst, c.max_surfels), _map(smx, c.src, c.src.shape[1])
    dst.SetDeltaTracking(None, True)
    first = dst.TransferChangedToCPU(None, 1)
    assert first.count == c.dst.shape[1]
    assert dst.TransferChangedToCPU(None, 2).count == 0
    stats = dst.MergeMap(None, src, c.T.reshape(3, 4), params=_pod(smx, c.params(MODES[mode])))
    d = dst.TransferChangedToCPU(None, 3)
    want = model[3]["dirty"]
    assert d.count == want.size == stats["n_appended"] + stats["n_blended_dst"] and d.surfel_count == stats["new_size"]
    assert np.array_equal(d.surfel_index[:d.count], want)
    rows = model[0]
    assert np.array_equal(d.x[:d.count].view(np.uint32), rows[3, want].view(np.uint32))
    assert np.array_equal(d.last_update_stamp[:d.count], mr.u32(rows)[18, want])
    assert dst.TransferChangedToCPU(None, 4).count == 0
    dst.close()
    src.close()


def _wide_planes():
    r2 = float((1.5 * mc.STEP) ** 2)
    whole = mc.plane(600, r2=r2)
    jitter = np.random.default_rng(3).uniform(-0.25, 0.25, (2, 600)).astype(np.float32) * mc.STEP   # (a lattice has no unique Delaunay triangulation)
    whole[0:2] += jitter
    whole[3:5] = whole[0:2]
    return whole[:, :400].copy(), whole[:, 200:].copy()


def test_downstream_of_a_merge(smx):
    """Triangulate on the merged map equals Triangulate on a fresh object with the merged rows; MapMesher.update after a merge
    equals the full call; a source mesh through src_to_dst indexes live slots of dst; a scene built before answers as before."""
    from surfelmeshing_amd import meshing
    a, b = _wide_planes()
    dst, src = _map(smx, a, 4096), _map(smx, b, 400)
    mesher = meshing.MapMesher(dst)
    tri_before = mesher.update()[0]
    tri_src = src.Triangulate(None)[0]
    assert tri_before.shape[0] > 300 and tri_src.shape[0] > 300
    scene = meshing.build_distance_scene(dst, tri_before, 0.05)
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, 0.5, 300), rng.uniform(0, 0.2, 300), rng.uniform(-0.03, 0.03, 300)], axis=1).astype(np.float32)
    answer = meshing.mesh_distance(dst, tri_before, pts, 0.05, scene=scene)
    stats, s2d = meshing.merge_maps(dst, src, mc.IDENTITY.reshape(3, 4), return_map=True, mode="blend", frame_index=2)
    want_rows, want_s2d, want_stats, _ = mr.merge_model(a, b, mc.IDENTITY, mr.params(mode=mr.BLEND, frame_index=2))
    assert stats["n_matched"] >= 200 and stats["n_appended"] > 100      # (the overlap, and the source slots next to dst's edge)
    n = stats["new_size"]
    rows = dst.debug_download_surfels(n)
    _assert_rows(rows, want_rows, "wide planes")
    assert np.array_equal(s2d, want_s2d) and stats == want_stats
    fresh = _map(smx, rows, 4096)
    tri_fresh, tri_merged = fresh.Triangulate(None)[0], dst.Triangulate(None)[0]
    assert tri_merged.shape[0] > tri_before.shape[0] and np.array_equal(tri_merged, tri_fresh)
    assert np.array_equal(mesher.update()[0], tri_merged)
    moved = meshing.remap_triangles(tri_src, s2d)
    assert moved.shape == tri_src.shape and int(moved.max()) < n and not (rows[7, moved.reshape(-1)] < 0).any()
    again = meshing.mesh_distance(dst, tri_before, pts, 0.05, scene=scene)
    for x, y in zip(answer[:2], again[:2]):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    timings = dst.debug_merge_timings()
    assert timings["whole"] > 0 and abs(sum(v for k, v in timings.items() if k != "whole") - timings["whole"]) < 1e-3 * timings["whole"] + 1e-3
    scene.close()
    mesher.close()
    for o in (fresh, dst, src):
        o.close()
