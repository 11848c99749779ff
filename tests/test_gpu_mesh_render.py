"""smx_recon_render_mesh on the device.  Coverage is integer arithmetic and every floating-point quantity of the contract
(include/smx.h) is a float64 expression that numpy reproduces bit for bit, so everything here is compared for EQUALITY with the
model of tests/mesh_raster_ref.py: the four images and every statistic.  There is no allowance for unstable pixels.

The sphere fixture's mesh from smx_recon_triangulate is not closed (6 739 triangles where a closed surface over 4 000 vertices
has 7 996), and decimating it at 0.1 does not close it: seen from (0, 0, 0.9) at 320 x 240 it covers 60 880 of the 76 800 pixels
in the model.  The full-coverage assertion of the large-path case is therefore made on the fixture's convex hull decimated at
0.1 (76 800 of 76 800); the decimated mesher output is compared for equality beside it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_raster_ref as rr
import mesh_ref as mr
from common import ROOT, small_stream

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
EMPTY = 0xFFFFFFFF
IMAGES = {"depth": (np.float32, 1), "index": (np.uint32, 1), "normal": (np.float32, 4), "color": (np.uint8, 4)}
EYE = np.eye(4, dtype=np.float32)[:3]


def _pose(z):
    return np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, z]], np.float32)


def _cam(w, h, f, T, cx=None, cy=None):
    return dict(width=w, height=h, fx=f, fy=f, cx=0.5 * w if cx is None else cx, cy=0.5 * h if cy is None else cy, global_T_camera=T)


OUTSIDE = _cam(160, 120, 131.25, _pose(-3))
OFF_AXIS = _cam(200, 77, 164.0, rr.look_at([1.5, -1.0, -2.2], [0.1, 0.0, 0.0]))
INSIDE = _cam(320, 240, 262.5, _pose(0.9))


def _rec_of(smx, rows, spare=1000):
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(rows[7] < 0)))
    return rec


def _params(smx, cam, cull_back_faces=False, normal_mode=0, color_flags=0, frame_index=0, window=2 ** 31 - 1, **kw):
    return smx.make_mesh_render_params(cull_back_faces=cull_back_faces, normal_mode=normal_mode, color_flags=color_flags,
                                       frame_index=frame_index, surfel_integration_active_window_size=window, **cam, **kw)


def _gpu(smx, rec, tri, cam, stream=None, **opts):
    """The four images and the statistics of one call."""
    bufs = {k: smx.CUDABuffer(cam["height"], cam["width"], *IMAGES[k]) for k in IMAGES}
    st = rec.RenderMesh(stream, _params(smx, cam, **opts), tri, return_stats=True, **bufs)
    out = {k: b.Download(stream) for k, b in bufs.items()}
    for b in bufs.values():
        b.close()
    out["stats"] = st
    return out


def _same(a, b, what=""):
    for k in IMAGES:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, int(np.sum(a[k] != b[k])))
    assert a["stats"] == b["stats"], what


def _equals_model(smx, rec, tri, cam, what, **opts):
    n = rec.surfels_size()
    rows = rec.debug_download_surfels(n)
    got = _gpu(smx, rec, tri, cam, **opts)
    want = rr.render_mesh(rows, n, tri, **cam, **opts)
    print("%s %s: GPU %s" % (what, opts, got["stats"]))
    assert got["stats"] == want["stats"]
    _same(got, want, what)
    return got


@pytest.fixture(scope="module")
def sphere(smx):
    rows = rr.rows_with_colors(*mr.sphere_map())
    rec = _rec_of(smx, rows)
    tri, _ = rec.Triangulate(None)
    assert tri.shape[0] > 6000
    yield rows, rec, tri
    rec.close()


def _hull(rows):
    from scipy.spatial import ConvexHull
    pos = rows[3:6].T.astype(np.float64)
    tri = ConvexHull(pos).simplices.copy()
    P = pos[tri]
    inwards = np.sum(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) * P[:, 0], axis=1) < 0
    tri[inwards] = tri[inwards][:, ::-1]
    return tri.astype(np.uint32)


@pytest.mark.parametrize("opts", [dict(), dict(cull_back_faces=True, normal_mode=rr.NORMAL_FACE, color_flags=4),
                                  dict(cull_back_faces=True), dict(normal_mode=rr.NORMAL_FACE, color_flags=1, frame_index=45, window=30)],
                         ids=["vertex-both-color", "face-cull-radii", "vertex-cull-color", "face-both-age"])
@pytest.mark.parametrize("view", ["outside", "off_axis"])
def test_sphere_equals_the_model(smx, sphere, view, opts):
    rows, rec, tri = sphere
    got = _equals_model(smx, rec, tri, OUTSIDE if view == "outside" else OFF_AXIS, "sphere " + view, **opts)
    if view == "outside":
        assert got["stats"]["n_covered_pixels"] > 0.25 * 160 * 120
    assert got["stats"]["n_drawn"] > 500 and got["stats"]["n_large"] == 0


def test_large_path_sphere_from_inside(smx, sphere):
    rows, rec, tri = sphere
    coarse_hull, _ = rec.DecimateMesh(None, _hull(rows), 0.1)
    got = _equals_model(smx, rec, coarse_hull, INSIDE, "hull decimated at 0.1, from inside")
    assert got["stats"]["n_large"] > 0 and got["stats"]["n_covered_pixels"] == 320 * 240
    _equals_model(smx, rec, coarse_hull, INSIDE, "hull decimated at 0.1, from inside", normal_mode=rr.NORMAL_FACE, color_flags=4)
    coarse, _ = rec.DecimateMesh(None, tri, 0.1)
    got = _equals_model(smx, rec, coarse, INSIDE, "mesher output decimated at 0.1, from inside")
    assert got["stats"]["n_large"] > 0 and got["stats"]["n_clipped"] > 0
    # from the centre: a hundred and more large triangles beside small ones
    got = _equals_model(smx, rec, coarse_hull, _cam(320, 240, 262.5, _pose(0.0)), "hull decimated at 0.1, from the centre")
    assert got["stats"]["n_large"] > 100 and got["stats"]["n_drawn"] > got["stats"]["n_large"]


def test_two_triangles_cover_a_640_x_480_image(smx):
    px = np.array([(-10.0, -10.0), (650.0, -10.0), (-10.0, 490.0), (650.0, 490.0)])
    z = 2.0
    pos = np.concatenate([(px - [320.0, 240.0]) / 500.0 * z, np.full((4, 1), z)], axis=1)
    rec = _rec_of(smx, rr.rows_with_colors(pos, np.tile([0.0, 0.0, -1.0], (4, 1)), np.full(4, 0.01)), spare=60)
    tri = np.array([[0, 2, 1], [1, 2, 3]], np.uint32)
    got = _equals_model(smx, rec, tri, _cam(640, 480, 500.0, EYE), "two triangles")
    assert got["stats"]["n_large"] == 2 and got["stats"]["n_covered_pixels"] == 640 * 480
    assert np.all(got["depth"] == np.float32(z)) and set(np.unique(got["index"])) == {0, 1}
    rec.close()


def test_grown_map_changes_nothing_and_agrees_with_the_splat_render(smx):
    from surfelmeshing_amd import render
    from test_gpu_mesh import _grown
    pg, rec = _grown(smx)
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    nn = smx.SurfelNeighborIndex()
    tri, mesh_stats, us = rec.TriangulateUpdate(None, index=nn)
    assert us["mode"] == 1 and tri.shape[0] > 10000
    n = rec.surfels_size()
    rows_before, stats_before = rec.debug_download_surfels(n), rec.stats()
    assert np.any(rows_before[7] < 0)
    for what, T in (("capture pose", s.pose(33)), ("off pose", render.look_at([0.2, -0.3, -0.4], [1.2, 0.3, 2.4]))):
        cam = _cam(s.width, s.height, s.fx, T, s.cx, s.cy)
        got = _equals_model(smx, rec, tri, cam, "grown map, " + what, color_flags=4)
        splat = render.render_view(rec, s.width, s.height, s.fx, s.fy, s.cx, s.cy, T, splat_mode="disc", outputs=("depth",))["depth"]
        both = (got["depth"] > 0) & (splat > 0)
        rel = np.abs(got["depth"][both] - splat[both]) / splat[both]
        print("%s: mesh covers %d pixels, discs %d, both %d; median relative depth difference %.3g" % (
            what, int((got["depth"] > 0).sum()), int((splat > 0).sum()), int(both.sum()), float(np.median(rel))))
        assert both.sum() > 0.5 * (splat > 0).sum()
    # no map state, statistic or kept mesher state has changed
    assert rec.stats() == stats_before and rec.surfels_size() == n
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()
    again, st2, us2 = rec.TriangulateUpdate(None, index=nn)
    assert us2["mode"] == 0 and us2["n_changed"] == 0 and again.tobytes() == tri.tobytes() and st2 == mesh_stats
    nn.close()


def test_large_plane_hundreds_of_workgroups(smx):
    m = mr.plane_map(side=300)
    rec = _rec_of(smx, rr.rows_with_colors(*m))
    tri, _ = rec.Triangulate(None, cell_size=2.5)
    assert tri.shape[0] > 170000
    got = _equals_model(smx, rec, tri, _cam(320, 240, 262.5, np.array([[1, 0, 0, 150], [0, 1, 0, 150], [0, 0, 1, -240]], np.float32)),
                        "plane 300, fronto-parallel")
    assert got["stats"]["n_covered_pixels"] == 320 * 240 and got["stats"]["n_drawn"] > 50000
    got = _equals_model(smx, rec, tri, _cam(320, 240, 262.5, rr.look_at([150.0, 420.0, -120.0], [150.0, 150.0, 0.0])),
                        "plane 300, tilted", normal_mode=rr.NORMAL_FACE)
    assert got["stats"]["n_covered_pixels"] > 0.4 * 320 * 240
    rec.close()


@pytest.mark.parametrize("reverse", [False, True])
def test_grid_is_covered_exactly_once(smx, reverse):
    rows, tri, cam = rr.grid_case(reverse)
    rec = _rec_of(smx, rows, spare=28)
    got = _equals_model(smx, rec, tri, cam, "grid")
    assert got["stats"]["n_covered_pixels"] == 1600 and np.all(got["index"][1:40, 1:40] != EMPTY)
    assert np.all(got["index"][40:] == EMPTY) and np.all(got["index"][:, 40:] == EMPTY)
    _equals_model(smx, rec, tri, cam, "grid", cull_back_faces=True)
    rec.close()


def test_stale_and_dirty_arrays_are_counted_not_drawn(smx, sphere):
    rows, _, tri = sphere
    stale = rows.copy()
    stale[7, np.random.default_rng(3).permutation(rows.shape[1])[:rows.shape[1] // 10]] = -1.0
    rec = _rec_of(smx, stale)
    n = rows.shape[1]
    bad = tri.copy()
    bad[::7, 1] = n + 5
    bad[3::11, 2] = EMPTY
    bad[5::13, 0] = n                   # (slots n .. n + 999 exist in the allocation but not in the map)
    got = _equals_model(smx, rec, bad, INSIDE, "stale, from inside")   # most of the sphere lies behind this camera
    st = got["stats"]
    assert st["n_out_of_range"] > 1000 and st["n_not_live"] > 500 and st["n_clipped"] > 1000 and st["n_drawn"] > 0
    # triangles that straddle the near plane: a near plane through the cap in front of the camera
    got = _equals_model(smx, rec, bad, INSIDE, "stale, near plane through the cap", near_z=0.09)
    assert 0 < got["stats"]["n_drawn"] < st["n_drawn"]
    drawn = np.unique(got["index"][got["index"] != EMPTY]).astype(np.int64)
    assert np.all(bad[drawn] < n) and np.all(stale[7][bad[drawn].astype(np.int64)] >= 0)
    got = _equals_model(smx, rec, bad, OUTSIDE, "stale, from outside", cull_back_faces=True)
    assert got["stats"]["n_culled"] > 0
    # ... and through old_to_new after a compaction: the same depth image, and the same index image (t is the array position)
    before = _gpu(smx, rec, tri, OUTSIDE)
    old_to_new, new_size, _ = rec.Compact(None)
    assert new_size == n - n // 10
    mapped = old_to_new[tri.astype(np.int64)]
    after = _equals_model(smx, rec, mapped, OUTSIDE, "compacted")
    assert after["depth"].tobytes() == before["depth"].tobytes() and after["index"].tobytes() == before["index"].tobytes()
    assert after["stats"]["n_out_of_range"] == before["stats"]["n_not_live"] > 0
    rec.close()


def test_device_array_equals_host_array_and_two_calls_agree(smx, sphere):
    rows, rec, tri = sphere
    a = _gpu(smx, rec, tri, OFF_AXIS, color_flags=4)
    b = _gpu(smx, rec, tri, OFF_AXIS, color_flags=4)
    _same(a, b, "two calls")
    dev = smx.CUDABuffer(1, tri.size, np.uint32)
    dev.Upload(tri.reshape(1, -1))
    c = _gpu(smx, rec, (dev.ToCUDA().address, tri.shape[0]), OFF_AXIS, color_flags=4)
    _same(a, c, "device array")
    # without statistics nothing is read back; the images are the same
    bufs = {k: smx.CUDABuffer(OFF_AXIS["height"], OFF_AXIS["width"], *IMAGES[k]) for k in IMAGES}
    assert rec.RenderMesh(None, _params(smx, OFF_AXIS, color_flags=4), (dev.ToCUDA().address, tri.shape[0]), **bufs) is None
    for k, buf in bufs.items():
        assert buf.Download().tobytes() == a[k].tobytes(), k
        buf.close()
    assert dev.Download()[0].tobytes() == tri.tobytes()          # the input is left alone
    t = rec.debug_mesh_render_timings()
    assert set(t) == {"small", "large", "resolve"} and all(np.isfinite(v) and v >= 0 for v in t.values())
    # an empty array: empty images
    e = _gpu(smx, rec, np.zeros((0, 3), np.uint32), OFF_AXIS)
    assert np.all(e["index"] == EMPTY) and not e["depth"].any() and not e["color"].any() and not e["normal"].any()
    assert e["stats"] == dict.fromkeys(rr.STAT_KEYS, 0)
    dev.close()


@pytest.mark.parametrize("mode", ["handover1", "handover0", "no_overlap"])
def test_straight_after_integrate_is_ordered(smx, mode):
    from test_gpu_parity import _pipes
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    _, pg = _pipes(smx, s, 60000)
    rec = pg.reconstruction
    rec.set_handover_mode(0 if mode == "handover0" else 1)
    if mode == "no_overlap":
        rec.set_overlap(0)
    for f in range(0, 20):
        pg.upload(f, *s.frame(f))
    for f in range(4, 14):
        pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    tri, _ = rec.Triangulate(pg.stream)
    pg.process(14, s.outlier_frames(14), s.others_TR_reference(14), s.pose(14))
    cam = _cam(s.width, s.height, s.fx, s.pose(14), s.cx, s.cy)
    a = _gpu(smx, rec, tri, cam, stream=pg.stream)          # (behind the integration just enqueued, no synchronisation before)
    smx.StreamSynchronize(None)
    b = _gpu(smx, rec, tri, cam, stream=pg.stream)
    _same(a, b, mode)
    assert a["stats"]["n_covered_pixels"] > 0.3 * s.width * s.height


def test_interleaved_with_splat_renders_and_tracking_on_two_streams(smx):
    from surfelmeshing_amd import _lib
    from test_gpu_mesh import _grown
    pg, rec = _grown(smx)
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    tri, _ = rec.Triangulate(None)
    pg.preprocess(34, [], None)
    smx.StreamSynchronize(None)
    w, h = s.width, s.height
    other = smx.Stream()
    splat_params = smx.make_render_params(w, h, s.fx, s.fy, s.cx, s.cy, s.pose(33), splat_mode=smx.SMX_SPLAT_DISC)
    mesh_params = _params(smx, _cam(w, h, s.fx, s.pose(30), s.cx, s.cy), color_flags=4)
    track_params = _lib.TrackParams.defaults()

    def run(sync):
        bufs = {k: [smx.CUDABuffer(h, w, np.float32) for _ in range(2)] for k in ("splat", "mesh")}
        idx = [smx.CUDABuffer(h, w, np.uint32) for _ in range(2)]
        rec.Render(pg.stream, splat_params, depth=bufs["splat"][0]); sync()
        rec.RenderMesh(other, mesh_params, tri, depth=bufs["mesh"][0], index=idx[0]); sync()
        out = rec.Track(pg.stream, s.depth_scaling, pg.depth_final, pg.normals, s.pose(33), track_params); sync()
        rec.RenderMesh(other, mesh_params, tri, depth=bufs["mesh"][1], index=idx[1]); sync()
        rec.Render(pg.stream, splat_params, depth=bufs["splat"][1])
        smx.StreamSynchronize(pg.stream)
        other.synchronize()
        got = [b.Download().tobytes() for k in ("splat", "mesh") for b in bufs[k]] + [b.Download().tobytes() for b in idx]
        for b in bufs["splat"] + bufs["mesh"] + idx:
            b.close()
        return got, (out.status, out.inliers, out.global_T_frame.tobytes())

    def everything():
        smx.StreamSynchronize(pg.stream)
        other.synchronize()
    one_at_a_time = run(everything)
    interleaved = run(lambda: None)
    assert one_at_a_time[1] == interleaved[1] and one_at_a_time[1][1] > 1000
    assert one_at_a_time[0] == interleaved[0]
    assert one_at_a_time[0][0] == one_at_a_time[0][1] and one_at_a_time[0][2] == one_at_a_time[0][3]
    other.close()


def _block(smx, words):
    b = smx.CUDABuffer(1, words, np.uint32)
    b.Upload(np.full((1, words), GUARD, np.uint32))
    return b


def test_pitched_outputs_null_outputs_and_refusals(smx):
    from surfelmeshing_amd import _lib
    rows, tri, cam = rr.grid_case()
    rec = _rec_of(smx, rows, spare=28)
    W, H = cam["width"], cam["height"]
    want = rr.render_mesh(rows, 36, tri, **cam)
    want_words = {"depth": want["depth"].view(np.uint32), "index": want["index"], "normal": want["normal"].view(np.uint32).reshape(H, 4 * W),
                  "color": want["color"].view(np.uint32).reshape(H, W)}
    per_px = {"depth": 1, "index": 1, "normal": 4, "color": 1}
    lead, extra = 8, 12                      # words before the image, and between its rows (multiples of 4: float4 stays aligned)
    blocks = {k: _block(smx, lead + H * (per_px[k] * W + extra) + 8) for k in IMAGES}

    def desc(k, **kw):
        d = dict(address=blocks[k].ToCUDA().address + 4 * lead, height=H, width=W, pitch=4 * (per_px[k] * W + extra))
        d.update(kw)
        return _lib.BufferDesc(d["address"], d["height"], d["width"], d["pitch"])

    def contents(k):
        flat = blocks[k].Download()[0]
        body = flat[lead:lead + H * (per_px[k] * W + extra)].reshape(H, per_px[k] * W + extra)
        return flat[:lead], body[:, :per_px[k] * W], body[:, per_px[k] * W:], flat[lead + H * (per_px[k] * W + extra):]

    def refill():
        for b in blocks.values():
            b.Upload(np.full((1, b.width()), GUARD, np.uint32))
    # every combination of outputs: the wanted ones hold the model's images, the guard words around them and all of an
    # unwanted block stay as they were
    for mask in range(16):
        refill()
        wanted = [k for j, k in enumerate(IMAGES) if mask & (1 << j)]
        rec.RenderMesh(None, _params(smx, cam), tri, **{k: desc(k) for k in wanted})
        smx.StreamSynchronize(None)
        for k in IMAGES:
            head, image, gaps, tail = contents(k)
            assert np.all(head == GUARD) and np.all(gaps == GUARD) and np.all(tail == GUARD), (mask, k)
            assert (image.tobytes() == want_words[k].tobytes()) if k in wanted else np.all(image == GUARD), (mask, k)
    # refusals: nothing is launched, so nothing is written
    refill()
    L = _lib.load()

    def raw(p=None, t=tri, n_in=None, **descs):
        p = p if p is not None else _params(smx, cam)
        d = {k: C.byref(descs[k]) if k in descs else C.byref(desc(k)) for k in IMAGES}
        return L.smx_recon_render_mesh(rec._h, None, C.byref(p), t.ctypes.data_as(C.c_void_p) if t is not None else None,
                                       C.c_uint32(tri.shape[0] if n_in is None else n_in), C.c_int32(0), d["depth"], d["index"], d["normal"],
                                       d["color"], None)
    for field, bad in (("width", 0), ("height", -3), ("width", W + 1), ("fx", 0.0), ("cy", float("nan")), ("near_z", 0.0), ("far_z", 0.01),
                       ("color_flags", 16), ("cull_back_faces", 2), ("normal_mode", 2), ("normal_mode", -1)):
        p = _params(smx, cam)
        setattr(p, field, bad)
        assert raw(p) == -1, field
    assert raw(t=None) == -1
    assert raw(depth=desc("depth", width=W - 1)) == -1 and raw(index=desc("index", pitch=4 * W - 4)) == -1
    assert raw(normal=desc("normal", address=blocks["normal"].ToCUDA().address + 4)) == -1         # not 16-byte aligned
    assert raw(color=desc("color", address=0)) == -1 and raw(normal=desc("normal", pitch=4 * W)) == -1
    smx.StreamSynchronize(None)
    for k in IMAGES:
        assert np.all(blocks[k].Download() == GUARD), k
    assert raw() == 0 and raw(t=None, n_in=0) == 0
    smx.StreamSynchronize(None)
    for b in blocks.values():
        b.close()
    rec.close()


def test_memory_returns_after_destroy(smx):
    before = smx.DebugLiveAllocations()
    rows, tri, cam = rr.grid_case()
    rec = _rec_of(smx, rows, spare=28)
    held = smx.DebugLiveAllocations()
    _gpu(smx, rec, tri, cam)
    grown = smx.DebugLiveAllocations()
    assert grown[0] > held[0]                                   # the workspace belongs to the object ...
    _gpu(smx, rec, tri[::2], cam)
    assert smx.DebugLiveAllocations() == grown                  # ... is reused ...
    rec.close()
    assert smx.DebugLiveAllocations() == before                 # ... and goes with it


def test_run_tum_writes_mesh_renders(tmp_path):
    out = tmp_path / "renders"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "12",
                        "--mesh_every", "4", "--render_source", "mesh", "--render_dir", str(out), "--render_every", "2",
                        "--render_overview"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    from surfelmeshing_amd import tum
    pngs = sorted(p for p in os.listdir(out) if p.startswith("render_"))
    assert len(pngs) >= 2 and "render_overview.png" in pngs
    for p in pngs:
        img = tum.read_png(str(out / p))
        assert img.shape[:2] == (240, 320)
        assert (img.reshape(-1, img.shape[-1]).max(axis=1) > 0).mean() > 0.05, p
