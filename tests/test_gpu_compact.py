"""smx_recon_compact: removing the merged slots from the map (not in the reference).  The GPU result is checked
against the numpy model of tests/compact_ref.py, and the frame loop after a compaction against the oracle whose state
was compacted in place by the same model."""
import ctypes as C

import numpy as np
import pytest

import compact_ref as cr
from common import RESULT_ROWS, assert_surfels_match, run_both, small_pre, small_stream
from test_gpu_parity import _compare_state, _pipes

pytestmark = pytest.mark.gpu


def _assert_rows_equal(got, want, rows=RESULT_ROWS):
    assert got.shape[1] == want.shape[1], (got.shape, want.shape)
    for r in rows:
        bad = np.nonzero(got[r].view(np.uint32) != want[r].view(np.uint32))[0]
        assert bad.size == 0, "row %d: %d mismatches, first at slot %d" % (r, bad.size, bad[0])


def _check_exact_effect(rec):
    n = rec.surfels_size()
    before = rec.debug_download_surfels(n)
    want, want_map, want_dropped = cr.compact_rows(before, n)
    old_to_new, new_size, dropped = rec.Compact(None)
    k = want.shape[1]
    assert new_size == k == rec.surfels_size() == rec.surfel_count()
    assert rec.stats()["merge_count"] == 0
    assert np.array_equal(old_to_new, want_map)
    assert dropped == want_dropped
    _assert_rows_equal(rec.debug_download_surfels(k), want)
    return n, k, dropped


def test_compact_exact_effect_on_a_grown_map(smx):
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    po, pg = _pipes(smx, s, 60000)
    for f in range(0, 34):
        pg.upload(f, *s.frame(f))
    for f in range(4, 29):
        pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    assert pg.reconstruction.stats()["merge_count"] > 0
    n, k, _ = _check_exact_effect(pg.reconstruction)
    assert k < n


def test_compact_exact_effect_on_a_large_map(smx):
    """> 1 M slots (a thousand segments and more), about one in ten merged, links to everywhere."""
    n, cap = 1_200_000, 1_300_000
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((25, n)).astype(np.float32)
    rows[7] = np.abs(rows[7]) + 1e-3
    merged = rng.random(n) < 0.1
    rows[7, merged] = -1.0
    links = rng.integers(0, n, size=(4, n), dtype=np.uint64).astype(np.uint32)
    links[rng.random((4, n)) < 0.2] = cr.INVALID
    rows[19:23] = links.view(np.float32)
    for r in (14, 15, 16, 23):       # (rows without storage read back as 0)
        rows[r] = 0
    rec = smx.CUDASurfelReconstruction(cap, smx.PinholeCamera4f(640, 480, 525.0, 525.0, 320.0, 240.0))
    rec.debug_upload_surfels(rows, int(merged.sum()))
    n_, k, dropped = _check_exact_effect(rec)
    assert n_ == n and k == n - int(merged.sum()) and dropped > 0
    # a second call finds nothing to remove: identity map
    old_to_new, new_size, dropped = rec.Compact(None)
    assert new_size == k and dropped == 0 and np.array_equal(old_to_new, np.arange(k, dtype=np.uint32))
    rec.close()


def _compact_both(po, pg, stream=None):
    n = po.recon.surfels_size
    orc_rows = po.recon.surfels()[:, :n].copy()
    want_map, want_dropped = cr.compact_oracle(po.recon)
    old_to_new, new_size, dropped = pg.reconstruction.Compact(stream)
    assert np.array_equal(old_to_new, want_map) and dropped == want_dropped
    assert new_size == po.recon.surfels_size
    return orc_rows, old_to_new


@pytest.mark.parametrize("mode", ["default", "event_handover", "no_overlap", "second_stream"])
def test_frame_loop_after_compaction_matches_oracle(smx, mode):
    """Compaction in the middle of a run, then 40 frames (longer than the 30-frame regulariser window) compared with
    the oracle after every frame."""
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    po, pg = _pipes(smx, s, 60000)
    if mode == "event_handover":
        pg.reconstruction.set_handover_mode(0)
    if mode == "no_overlap":
        pg.reconstruction.set_overlap(0)
    run_both(po, pg, s, list(range(4, 18)), None)
    assert po.recon.merge_count > 0
    if mode == "second_stream":   # straight behind the last Integrate, no synchronisation, on another stream
        other = smx.Stream()
        _compact_both(po, pg, other)
        other.synchronize()
    else:
        _compare_state(po, pg)
        _compact_both(po, pg)
    assert pg.reconstruction.stats()["merge_count"] == 0
    run_both(po, pg, s, list(range(18, 58)), lambda f: _compare_state(po, pg))
    assert po.recon.merge_count > 0


def test_compaction_lets_a_clamped_map_grow_again(smx):
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    cap = 10000                                        # (reached in frame 11, 50 merged slots by frame 12)
    po, pg = _pipes(smx, s, cap)
    run_both(po, pg, s, list(range(4, 13)), None)
    assert po.recon.surfels_size == cap and po.recon.merge_count > 0
    assert pg.reconstruction.stats()["capacity_clamped"] == 1
    _compare_state(po, pg)
    _compact_both(po, pg)
    k = po.recon.surfels_size
    assert k < cap
    run_both(po, pg, s, list(range(13, 17)), lambda f: _compare_state(po, pg))
    assert po.recon.surfels_size > k


def test_compaction_is_a_relabelling_without_zombie_links(smx):
    """Two objects start from the same state (merged slots' links cleared); one is compacted (links_dropped == 0).
    After 10 frames the uncompacted one's rows, mapped through old_to_new (later slots shifted down by the number
    removed), equal the compacted one's, and the neighbour candidates commute with the map."""
    from surfelmeshing_amd.pipeline import FramePipeline
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    po, pg = _pipes(smx, s, 60000)
    run_both(po, pg, s, list(range(4, 16)), None)
    n_old = po.recon.surfels_size
    rows = pg.reconstruction.debug_download_surfels(n_old)
    cr.clear_zombie_links(rows, n_old)
    pa, pb = (FramePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, small_pre(s.width)) for _ in range(2))
    for p in (pa, pb):
        p.reconstruction.debug_upload_surfels(rows, po.recon.merge_count)
    old_to_new, k, dropped = pb.compact()
    assert dropped == 0 and k == po.recon.surfel_count
    for f in range(12, 30):
        for p in (pa, pb):
            p.upload(f, *s.frame(f))
    for f in range(16, 26):
        for p in (pa, pb):
            p.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    n = pa.reconstruction.surfels_size()
    got = pb.reconstruction.debug_download_surfels(pb.reconstruction.surfels_size())
    _assert_rows_equal(got, cr.relabel(pa.reconstruction.debug_download_surfels(n), n, old_to_new, n_old))
    # neighbour candidates of the kept old slots, after rebuilding both indices
    removed = n_old - k
    full = np.concatenate([old_to_new, np.arange(n_old, n, dtype=np.uint32) - np.uint32(removed)])
    slots_a = np.nonzero(full != cr.INVALID)[0][::7].astype(np.uint32)
    r2 = got[7][got[7] > 0]
    cell = 2.0 * float(np.sqrt(np.median(r2)))
    res = []
    for p, slots in ((pa, slots_a), (pb, full[slots_a])):
        nn = smx.SurfelNeighborIndex()
        nn.BuildFromReconstruction(p.reconstruction, cell)
        res.append(nn.FindNeighborCandidates(p.reconstruction, slots, 4.0, 16))
        nn.close()
    (ca, da, ia), (cb, db, ib) = res
    assert np.array_equal(ca, cb) and ca.sum() > 0
    for q in range(len(slots_a)):
        assert np.array_equal(da[q, :ca[q]].view(np.uint32), db[q, :cb[q]].view(np.uint32))
        assert np.array_equal(full[ia[q, :ca[q]]], ib[q, :cb[q]])


def test_boundary_outputs_after_compaction_match_the_oracle(smx):
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    po, pg = _pipes(smx, s, 60000)
    rec = pg.reconstruction
    rec.SetDeltaTracking(None, True)
    run_both(po, pg, s, list(range(4, 16)), None)
    n = rec.surfels_size()
    pos0, col0 = smx.CUDABuffer(1, 3 * n, np.float32), smx.CUDABuffer(1, 3 * n, np.uint8)
    rec.ExportVertices(None, pos0, col0)
    pos0, col0 = pos0.Download()[0].reshape(n, 3), col0.Download()[0].reshape(n, 3)
    rec.TransferChangedToCPU(None, 15)              # (drain the marks of the frames so far)
    _compact_both(po, pg)
    k = rec.surfels_size()
    # TransferAllToCPU against the oracle's transfer of its compacted state
    cpu = smx.CUDASurfelsCPU(60000)
    cpu.LockWriteBuffers()
    rec.TransferAllToCPU(None, 15, cpu)
    smx.StreamSynchronize(None)
    cpu.UnlockWriteBuffers()
    cpu.WaitForLockAndSwapBuffers()
    rb, t = cpu.read_buffers(), po.recon.transfer_all()
    assert rb.surfel_count == t["surfel_count"] == k
    pairs = (("surfel_x_buffer", "x"), ("surfel_y_buffer", "y"), ("surfel_z_buffer", "z"),
             ("surfel_radius_squared_buffer", "radius_squared"), ("surfel_normal_x_buffer", "normal_x"),
             ("surfel_normal_y_buffer", "normal_y"), ("surfel_normal_z_buffer", "normal_z"),
             ("surfel_last_update_stamp_buffer", "last_update_stamp"))
    for a, b in pairs:
        assert np.array_equal(getattr(rb, a)[:k].view(np.uint32), t[b].view(np.uint32)), a
    # ExportVertices: the earlier export without its NaN (merged) rows, and the oracle's
    pos, col = smx.CUDABuffer(1, 3 * k, np.float32), smx.CUDABuffer(1, 3 * k, np.uint8)
    rec.ExportVertices(None, pos, col)
    pos, col = pos.Download()[0], col.Download()[0]
    keep = ~np.isnan(pos0[:, 0])
    assert keep.sum() == k
    assert np.array_equal(pos.view(np.uint32), pos0[keep].reshape(-1).view(np.uint32))
    assert np.array_equal(col, col0[keep].reshape(-1))
    opos, ocol = po.recon.export_vertices()
    assert np.array_equal(pos.view(np.uint32), opos.view(np.uint32)) and np.array_equal(col, ocol)
    # the next delta holds every slot of the compacted map and patches a truncated mirror into the oracle's arrays
    delta = rec.TransferChangedToCPU(None, 15)
    assert delta.count == k == delta.surfel_count
    assert np.array_equal(delta.surfel_index[:k], np.arange(k, dtype=np.uint32))
    mirror = smx.CUDASurfelBuffersCPU(60000)
    for a, _ in pairs:
        getattr(mirror, a)[:] = 0
    delta.ApplyTo(mirror)
    assert mirror.surfel_count == k
    for a, b in pairs:
        assert np.array_equal(getattr(mirror, a)[:k].view(np.uint32), t[b].view(np.uint32)), a
    # ... and the frame loop's deltas go on from there
    run_both(po, pg, s, [16, 17], None)
    delta = rec.TransferChangedToCPU(None, 17)
    assert delta.count > 0 and np.all(np.diff(delta.surfel_index[:delta.count].astype(np.int64)) > 0)
    rec.SetDeltaTracking(None, False)


def _raw_compact(rec, ptr, capacity, on_device):
    from surfelmeshing_amd import _lib
    new_size, dropped = C.c_uint32(0), C.c_uint32(0)
    return _lib.load().smx_recon_compact(rec._h, None, C.c_void_p(ptr) if ptr else None, C.c_uint32(capacity),
                                         C.c_int32(on_device), C.byref(new_size), C.byref(dropped)), new_size.value


def test_compaction_edge_cases(smx):
    cam = smx.PinholeCamera4f(160, 120, 131.25, 131.25, 80.0, 60.0)
    rec = smx.CUDASurfelReconstruction(5000, cam)
    # an empty map
    old_to_new, new_size, dropped = rec.Compact(None)
    assert old_to_new.size == 0 and new_size == 0 and dropped == 0 and rec.surfels_size() == 0
    rng = np.random.default_rng(3)
    n = 3000
    rows = rng.standard_normal((25, n)).astype(np.float32)
    rows[7] = -1.0
    rows[19:23] = rng.integers(0, n, size=(4, n), dtype=np.uint64).astype(np.uint32).view(np.float32)
    # all slots merged
    rec.debug_upload_surfels(rows, n)
    old_to_new, new_size, dropped = rec.Compact(None)
    assert new_size == 0 and rec.surfels_size() == 0 and np.all(old_to_new == cr.INVALID) and dropped == 4 * n
    # capacity too small: an error, and the map is unchanged
    rows[7] = np.abs(rows[7]) + 0.5
    rows[7, ::5] = -1.0
    for r in (14, 15, 16, 23):
        rows[r] = 0
    rec.debug_upload_surfels(rows, n // 5)
    rc, _ = _raw_compact(rec, np.zeros(n - 1, np.uint32).ctypes.data, n - 1, 0)
    assert rc != 0
    assert rec.surfels_size() == n and rec.surfel_count() == n - n // 5
    _assert_rows_equal(rec.debug_download_surfels(n), rows)
    # old_to_new on the device
    want, want_map, _ = cr.compact_rows(rows, n)
    dev = smx.CUDABuffer(1, n, np.uint32)
    rc, new_size = _raw_compact(rec, dev.ToCUDA().address, n, 1)
    assert rc == 0 and new_size == want.shape[1]
    assert np.array_equal(dev.Download()[0], want_map)
    _assert_rows_equal(rec.debug_download_surfels(new_size), want)
    rec.close()


def test_compaction_without_merged_slots_is_the_identity(smx):
    s = small_stream()
    po, pg = _pipes(smx, s, 60000)
    run_both(po, pg, s, [4], None)
    n = po.recon.surfels_size
    assert po.recon.merge_count == 0 and n > 0
    before = pg.reconstruction.debug_download_surfels(n)
    old_to_new, new_size, dropped = pg.reconstruction.Compact(None)
    assert new_size == n and dropped == 0 and np.array_equal(old_to_new, np.arange(n, dtype=np.uint32))
    assert_surfels_match(pg.reconstruction.debug_download_surfels(n), before, n)
    run_both(po, pg, s, [5, 6], lambda f: _compare_state(po, pg))
