"""The viewer buffers (smx_recon_update_visualization_buffers) and the headless render (smx_recon_render) on the GPU,
against the numpy restatements of tests/viz_ref.py, on maps built from small_stream with the obstacle (merges and
replacements included)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import splat_ref as sp
import viz_ref as vr
from common import ROOT, assert_surfels_match, run_both, small_stream
from test_gpu_parity import _compare_state, _pipes
from test_render_api import RAYCAST_MEDIAN_REL_ERR, RAYCAST_MIN_COVERAGE, RAYCAST_P95_REL_ERR, raycast_agreement

pytestmark = pytest.mark.gpu
INT_MAX = 2 ** 31 - 1
GUARD = 0xA5A5A5A5


def _grown(smx, frames=range(4, 16), **kw):
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0, **kw)
    _, pg = _pipes(smx, s, 60000)
    for f in range(min(frames) - 4, max(frames) + 5):
        pg.upload(f, *s.frame(f))
    for f in frames:
        pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    rec = pg.reconstruction
    assert rec.stats()["merge_count"] > 0
    return s, pg, rec


@pytest.fixture(scope="module")
def grown(smx):
    return _grown(smx)


def _vis(smx, rec, n, cap, frame, tri, mesh_count, window, flags, which=("v", "i", "n")):
    """Runs the fill into guard-filled device buffers of `cap` slots + 64 guard slots; returns the host copies."""
    sizes = {"v": 4, "i": 8, "n": 6}
    bufs = {k: smx.CUDABuffer(1, (cap + 64) * sizes[k], np.uint32) for k in which}
    for b in bufs.values():
        b.Clear(GUARD)
    get = {k: ((bufs[k].ToCUDA().address, cap) if k in bufs else None) for k in "vin"}
    rec.UpdateVisualizationBuffers(None, frame, tri, mesh_count, window,
                                   bool(flags & vr.VIS_LAST_UPDATE), bool(flags & vr.VIS_CREATION),
                                   bool(flags & vr.VIS_RADII), bool(flags & vr.VIS_NORMALS),
                                   vertex_buffer=get["v"], neighbor_index_buffer=get["i"], normal_vertex_buffer=get["n"])
    return {k: b.Download().reshape(cap + 64, sizes[k]) for k, b in bufs.items()}


@pytest.mark.parametrize("window", [INT_MAX, 10])
def test_vertex_buffers_bit_exact_for_every_flag_combination(smx, grown, window):
    s, pg, rec = grown
    n = rec.surfels_size()
    rows = rec.debug_download_surfels(n)
    creation = rows[17, :n].view(np.uint32)
    tri = int(np.median(creation))                       # both sides of creation_stamp > latest_triangulated
    mesh_count = n // 2                                  # ... and of slot < latest_mesh_surfel_count
    frame = 15
    assert (creation > tri).any() and (creation <= tri).any()
    for flags in range(16):
        got = _vis(smx, rec, n, n, frame, tri, mesh_count, window, flags)
        want_v = vr.vertex_buffer(rows, n, frame, tri, mesh_count, window, flags)
        assert vr.equal_nan_aware(got["v"][:n], want_v, float_cols=[0, 1, 2]), flags
        assert np.isnan(got["v"][:n, 0].view(np.float32)).any()
        assert np.array_equal(got["i"][:n], vr.neighbor_buffer(rows, n))
        assert vr.equal_nan_aware(got["n"][:n], vr.normal_vertex_buffer(rows, n), float_cols=list(range(6)))
        for k in "vin":
            assert np.all(got[k][n:] == GUARD), k
    merged = rows[7, :n] < 0
    assert merged.any()
    nv = vr.normal_vertex_buffer(rows, n).view(np.float32)
    assert np.isnan(nv[merged, 3:]).all()


def test_vertex_buffers_capacity_and_null_buffers(smx, grown):
    s, pg, rec = grown
    n = rec.surfels_size()
    rows = rec.debug_download_surfels(n)
    cap = n // 3
    got = _vis(smx, rec, n, cap, 15, 15, 0, INT_MAX, vr.VIS_RADII)
    assert vr.equal_nan_aware(got["v"][:cap], vr.vertex_buffer(rows, n, 15, 15, 0, INT_MAX, vr.VIS_RADII)[:cap], [0, 1, 2])
    assert np.array_equal(got["i"][:cap], vr.neighbor_buffer(rows, n)[:cap])
    for k in "vin":
        assert np.all(got[k][cap:] == GUARD), k
    got = _vis(smx, rec, n, n, 15, 15, 0, INT_MAX, 0, which=("i",))
    assert np.array_equal(got["i"][:n], vr.neighbor_buffer(rows, n)) and np.all(got["i"][n:] == GUARD)
    rec.UpdateVisualizationBuffers(None, 15, 0, 0, 30)   # (nothing given: a no-op, as before)


def _render(smx, rec, w, h, fx, fy, cx, cy, T, stream=None, **opts):
    from surfelmeshing_amd import render
    return render.render_view(rec, w, h, fx, fy, cx, cy, T, stream=stream, **opts)


def _off_pose(s):
    from surfelmeshing_amd import render
    return render.look_at([0.2, -0.3, -0.4], [1.2, 0.3, 2.4])


CASES = [("square", 0.0), ("square", 3.0), ("disc", 3.0)]
SIZES = [(160, 120), (200, 77), (320, 240)]


@pytest.mark.parametrize("mode,h", CASES)
@pytest.mark.parametrize("size", SIZES)
def test_render_matches_the_reference(smx, grown, mode, h, size):
    s, pg, rec = grown
    n = rec.surfels_size()
    rows = rec.debug_download_surfels(n)
    w, hh = size
    sc = w / 640.0
    fx = fy = 525.0 * sc
    cx, cy = 320.0 * sc, 0.5 * hh
    for T in (s.pose(15), _off_pose(s)):
        got = _render(smx, rec, w, hh, fx, fy, cx, cy, T, splat_mode=mode, splat_half_extent_in_pixels=h, color="radii",
                      frame_index=15)
        ref = vr.render(rows, n, w, hh, fx, fy, cx, cy, T, mode=vr.SPLAT_DISC if mode == "disc" else vr.SPLAT_SQUARE,
                        half_extent=h)
        cov_ref = ref["index"] != vr.INVALID
        assert cov_ref.sum() > 0.1 * w * hh   # (h = 0 at 320 x 240: about 15 %)
        diff = got["index"] != ref["index"]
        unstable = vr.unstable(ref)
        assert not (diff & ~unstable).any(), np.argwhere(diff & ~unstable)[:5]
        assert diff.sum() <= 0.005 * cov_ref.sum(), (diff.sum(), cov_ref.sum())
        same = ~diff & cov_ref
        rel = np.abs(got["depth"][same] - ref["depth"][same]) / ref["depth"][same]
        assert rel.max() <= 1e-5, rel.max()
        _check_invariants(got, rows, T, vr.VIS_RADII, 15, INT_MAX)
        # ... and bit for bit against the exact model: no tolerance, no pixel excused
        exact = sp.render(rows, n, w, hh, fx, fy, cx, cy, T, mode=sp.DISC if mode == "disc" else sp.SQUARE, half_extent=h,
                          color_flags=vr.VIS_RADII, frame_index=15)
        for k in sp.IMAGES:
            assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(exact[k]).tobytes(), (k, T)


def _check_invariants(got, rows, T, flags, frame, window):
    idx = got["index"]
    empty = idx == vr.INVALID
    assert np.array_equal(empty, got["depth"] == 0) and np.array_equal(empty, got["color"][..., 3] == 0)
    assert np.all(got["color"][empty] == 0) and np.all(got["normal"][empty] == 0)
    assert np.all(got["color"][~empty][:, 3] == 255)
    sl = idx[~empty].astype(np.int64)
    assert np.all(rows[7, sl] >= 0)                     # no merged slot appears
    want_c = vr.vis_color(rows, sl, flags, frame, window)
    got_c = got["color"][~empty].copy().view(np.uint32).ravel() & 0x00FFFFFF
    assert np.array_equal(got_c, want_c & 0x00FFFFFF)
    R = np.asarray(T, np.float32).reshape(3, 4)[:, :3]
    n = rows[8:11, sl].astype(np.float32)
    want_n = np.stack([((R[0, k] * n[0]).astype(np.float32) + (R[1, k] * n[1]).astype(np.float32)).astype(np.float32)
                       + (R[2, k] * n[2]).astype(np.float32) for k in range(3)], axis=1).astype(np.float32)
    assert np.array_equal(got["normal"][~empty][:, :3], want_n)


def test_render_of_a_capture_pose_matches_the_raycast_depth(smx):
    """The oracle-built map of test_render_api, rendered on the GPU, within the bounds measured there."""
    s = small_stream(obstacle_until=8)
    po, pg = _pipes(smx, s, 60000)
    run_both(po, pg, s, list(range(4, 12)), None)
    got = _render(smx, pg.reconstruction, s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.pose(11), splat_mode="disc")
    cov, err, _ = raycast_agreement(s, 11, got["depth"])
    assert cov >= RAYCAST_MIN_COVERAGE and np.median(err) <= RAYCAST_MEDIAN_REL_ERR
    assert np.percentile(err, 95) <= RAYCAST_P95_REL_ERR


@pytest.mark.parametrize("mode", ["handover1", "handover0", "no_overlap"])
def test_render_straight_after_integrate_is_ordered_and_deterministic(smx, mode):
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    _, pg = _pipes(smx, s, 60000)
    rec = pg.reconstruction
    rec.set_handover_mode(0 if mode == "handover0" else 1)
    if mode == "no_overlap":
        rec.set_overlap(0)
    for f in range(0, 20):
        pg.upload(f, *s.frame(f))
    for f in range(4, 15):
        pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    a = _render(smx, rec, 160, 120, s.fx, s.fy, s.cx, s.cy, s.pose(14), stream=pg.stream, splat_mode="disc")
    smx.StreamSynchronize(None)
    b = _render(smx, rec, 160, 120, s.fx, s.fy, s.cx, s.cy, s.pose(14), stream=pg.stream, splat_mode="disc")
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("handover", [0, 1])
def test_renders_and_buffer_updates_do_not_change_the_frame_loop(smx, handover):
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    po, pg = _pipes(smx, s, 60000)
    rec = pg.reconstruction
    rec.set_handover_mode(handover)
    _, pq = _pipes(smx, s, 60000)
    pq.reconstruction.set_handover_mode(handover)
    rec.SetDeltaTracking(pg.stream, True)
    pq.reconstruction.SetDeltaTracking(pq.stream, True)
    vbuf = smx.CUDABuffer(1, 60000 * 4, np.float32)

    def between(f):
        if f % 2 == 0:
            _render(smx, rec, 160, 120, s.fx, s.fy, s.cx, s.cy, s.pose(f), stream=pg.stream, splat_mode="disc")
        else:
            rec.UpdateVisualizationBuffers(pg.stream, f, f, 0, 30, True, False, False, False, vertex_buffer=vbuf)
        if f % 5 == 0:
            da = rec.TransferChangedToCPU(pg.stream, f)
            db = pq.reconstruction.TransferChangedToCPU(pq.stream, f)
            assert da.count == db.count and np.array_equal(da.surfel_index[:da.count], db.surfel_index[:db.count])
    lo, hi = 0, 28
    for f in range(lo, hi):
        d, c = s.frame(f)
        po.upload(f, d, c); pg.upload(f, d, c); pq.upload(f, d, c)
    for f in range(4, 24):
        for p in (po, pg, pq):
            p.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
        between(f)
    _compare_state(po, pg)
    n = po.recon.surfels_size
    assert_surfels_match(rec.debug_download_surfels(n), po.recon.surfels(), n)


def test_render_after_compaction_is_a_relabelling(smx):
    s, pg, rec = _grown(smx)
    T = s.pose(15)
    before = _render(smx, rec, 160, 120, s.fx, s.fy, s.cx, s.cy, T, splat_mode="disc")
    old_to_new, _, _ = pg.compact()
    after = _render(smx, rec, 160, 120, s.fx, s.fy, s.cx, s.cy, T, splat_mode="disc")
    cov = before["index"] != vr.INVALID
    assert np.array_equal(after["index"][cov], old_to_new[before["index"][cov]])
    assert np.array_equal(after["index"][~cov], before["index"][~cov])
    assert np.array_equal(after["depth"], before["depth"])


def test_render_edge_cases(smx):
    from surfelmeshing_amd import _lib
    rec = smx.CUDASurfelReconstruction(1000, smx.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    got = _render(smx, rec, 33, 17, 30.0, 30.0, 16.0, 8.0, T)
    assert np.all(got["index"] == vr.INVALID) and np.all(got["depth"] == 0) and np.all(got["color"] == 0)
    lib = _lib.load()
    good = smx.make_render_params(33, 17, 30.0, 30.0, 16.0, 8.0, T)
    d = smx.CUDABuffer(17, 33, np.float32)
    wrong = smx.CUDABuffer(17, 32, np.float32)
    assert lib.smx_recon_render(rec._h, None, None, None, None, None, None) == -1
    assert lib.smx_recon_render(rec._h, None, C.byref(good), C.byref(wrong.ToCUDA()), None, None, None) == -1
    assert lib.smx_recon_render(rec._h, None, C.byref(good), None, None, C.byref(d.ToCUDA()), None) == -1  # (16 B/px)
    for field, bad in (("width", 0), ("height", -3), ("near_z", 0.0), ("far_z", 0.01), ("splat_mode", 2),
                       ("max_splat_extent_in_pixels", 0.0), ("splat_half_extent_in_pixels", -1.0)):
        p = smx.make_render_params(33, 17, 30.0, 30.0, 16.0, 8.0, T)
        setattr(p, field, bad)
        assert lib.smx_recon_render(rec._h, None, C.byref(p), C.byref(d.ToCUDA()), None, None, None) == -1, field
    assert lib.smx_recon_render(rec._h, None, C.byref(good), C.byref(d.ToCUDA()), None, None, None) == 0
    smx.StreamSynchronize(None)
    rec.close()


def test_run_tum_writes_renders(tmp_path):
    out = tmp_path / "renders"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "20",
                        "--render_dir", str(out), "--render_every", "5", "--render_splat", "disc", "--render_overview"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    from surfelmeshing_amd import tum
    pngs = sorted(p for p in os.listdir(out) if p.startswith("render_"))
    assert len(pngs) >= 3 and "render_overview.png" in pngs
    for p in pngs:
        img = tum.read_png(str(out / p))
        assert img.shape[:2] == (240, 320)
        assert (img.reshape(-1, img.shape[-1]).max(axis=1) > 0).mean() > 0.05, p
