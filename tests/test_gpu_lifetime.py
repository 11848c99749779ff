"""Who owns device memory: every object gives back exactly what it took, whatever it was asked to do in between and
wherever an allocation failed on the way.  Measured with smx_debug_live_allocations (blocks and bytes the library's
objects hold, process-wide) against a baseline read at the start of each test -- other fixtures may be alive -- and
provoked with smx_debug_fail_allocation, which fails the nth next allocation on the host (HIP is not called).

Shapes: the 96 x 72 camera and the frames of tests/golden/stream_96x72.npz (at most 4 985 slots), 6 000 slots of capacity;
the meshing cases run on uploaded sphere maps of 1 500 .. 4 500 slots."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as mr
from common import small_pre
from test_golden import G

pytestmark = pytest.mark.gpu

CAPACITY = 6000
H, W = G["depth"].shape[1:]
INTR = [float(v) for v in G["intr"]]
SMX_ERR_HIP = -2


@pytest.fixture
def live(smx):
    """Returns the current (blocks, bytes); whatever the test does, no armed failure outlives it."""
    yield smx.DebugLiveAllocations
    smx.DebugFailAllocation(-1)


def _pipeline(smx, n_frames, after_frame=None):
    """A FramePipeline that has integrated the first n_frames frames of the golden stream (its image buffers are
    smx_buffers: not counted)."""
    from surfelmeshing_amd.pipeline import FramePipeline
    pg = FramePipeline(W, H, *INTR, CAPACITY, small_pre(W))
    for f in range(G["depth"].shape[0]):
        pg.upload(f, G["depth"][f], G["color"][f])
    for k in range(n_frames):
        f = int(G["frames"][k])
        pg.process(f, [f - 1, f - 2, f - 3, f - 4, f + 1, f + 2, f + 3, f + 4], G["others_T"][k], G["poses"][f])
        if after_frame is not None:
            after_frame(k + 1)
    return pg


def _upload(rec, m):
    rec.debug_upload_surfels(mr.rows_of_map(*m), 0)


def _track_raw(smx, pg, g):
    """smx_recon_track of frame g (preprocessed without the cull) at its own pose: (status code, the bytes of smx_track_result)."""
    from surfelmeshing_amd import _lib
    pg.preprocess(g, [], None)
    T = np.ascontiguousarray(np.asarray(G["poses"][g], np.float32).reshape(12))
    p, res = _lib.TrackParams.defaults(), _lib.TrackResult()
    rc = _lib.load().smx_recon_track(pg.reconstruction._h, C.c_void_p(0), C.c_float(pg.pre.depth_scaling),
                                     smx._d(pg.depth_final), smx._d(pg.normals), T.ctypes.data_as(C.c_void_p), C.byref(p),
                                     C.byref(res), C.c_int32(0), None, None)
    return rc, bytes(res)


def _track_rgbd_raw(smx, handle, pg, g, pose, weight, guard=0xA5, fail=-1):
    """smx_recon_track_rgbd on `handle` of frame g of pg (preprocessed without the cull) with its colour image, predicted at
    `pose`: (status code, the bytes of smx_track_rgbd_result, which start as `guard` bytes).  fail: the allocation of the call
    that fails (smx_debug_fail_allocation, armed after the preparations), -1 = none; likewise below."""
    from surfelmeshing_amd import _lib
    pg.preprocess(g, [], None)
    T = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(12))
    p, res = _lib.TrackRGBDParams.defaults(photometric_weight=weight), _lib.TrackRGBDResult()
    C.memset(C.addressof(res), guard, C.sizeof(res))
    smx.DebugFailAllocation(fail)
    rc = _lib.load().smx_recon_track_rgbd(handle, C.c_void_p(0), C.c_float(pg.pre.depth_scaling), smx._d(pg.depth_final),
                                          smx._d(pg.normals), smx._d(pg.color[g]), T.ctypes.data_as(C.c_void_p), C.byref(p),
                                          C.byref(res), C.c_int32(0), None, None, None)
    return rc, bytes(res)


def _decimate_raw(smx, rec, tri, cell, guard=0xA5A5A5A5, fail=-1):
    """One smx_recon_decimate_mesh call from host arrays with room for every input triangle: (status code, the whole output
    array, the whole vertex map -- both start as `guard` words -- the count, the bytes of smx_decimate_stats)."""
    from surfelmeshing_amd import _lib
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    out = np.full((tri.shape[0], 3), guard, np.uint32)
    vmap = np.full(rec.surfels_size(), guard, np.uint32)
    T, st = C.c_uint32(0), _lib.DecimateStats()
    smx.DebugFailAllocation(fail)
    rc = _lib.load().smx_recon_decimate_mesh(rec._h, C.c_void_p(0), C.c_float(cell), tri.ctypes.data_as(C.c_void_p),
                                             C.c_uint32(tri.shape[0]), out.ctypes.data_as(C.c_void_p), C.c_uint32(tri.shape[0]),
                                             vmap.ctypes.data_as(C.c_void_p), C.c_int32(0), C.byref(T), C.byref(st))
    return rc, out, vmap, T.value, bytes(st)


def _render_mesh_raw(smx, rec, tri, w, h, pose, bufs, guard=0xA5, fail=-1):
    """One smx_recon_render_mesh call from a host array into the four images `bufs` at w x h with the camera of the file
    scaled to it: (status code, the bytes of smx_mesh_render_stats, which start as `guard` bytes)."""
    from surfelmeshing_amd import _lib
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    k = w / W
    prm = smx.make_mesh_render_params(w, h, INTR[0] * k, INTR[1] * k, INTR[2] * k, INTR[3] * k, pose)
    st = _lib.MeshRenderStats()
    C.memset(C.addressof(st), guard, C.sizeof(st))
    smx.DebugFailAllocation(fail)
    rc = _lib.load().smx_recon_render_mesh(rec._h, C.c_void_p(0), C.byref(prm), tri.ctypes.data_as(C.c_void_p),
                                           C.c_uint32(tri.shape[0]), C.c_int32(0), *[smx._d(b) for b in bufs], C.byref(st))
    return rc, bytes(st)


def _mean_edge(tri, pos):
    e = np.concatenate([pos[tri[:, a]] - pos[tri[:, b]] for a, b in ((0, 1), (1, 2), (2, 0))])
    return float(np.sqrt((e * e).sum(axis=1)).mean())


EYE = np.eye(3, 4, dtype=np.float32)
MESH_IMAGES = ((np.float32, 1), (np.uint32, 1), (np.float32, 4), (np.uint8, 4))      # depth, index, normal, color


# ---- 1. everything comes back -----------------------------------------------------------------------------------------
def test_a_reconstruction_gives_back_everything_its_services_took(smx, live):
    from surfelmeshing_amd import render
    from surfelmeshing_amd._lib import MeshParams
    base = live()
    pg = _pipeline(smx, 3)
    rec, st = pg.reconstruction, pg.stream
    created = live()
    assert created[0] > base[0] and created[1] > base[1]
    f = int(G["frames"][2])
    pose = G["poses"][f]

    rec.SetDeltaTracking(st, True)
    d = rec.TransferChangedToCPU(st, f)
    n = rec.surfels_size()
    assert d.count == n > 2000                                       # (enabling marks every slot)
    cpu = smx.CUDASurfelsCPU(CAPACITY)
    cpu.LockWriteBuffers()
    rec.TransferAllToCPU(st, f, cpu)
    smx.StreamSynchronize(st)
    cpu.UnlockWriteBuffers()
    assert cpu.write_buffers().surfel_count == n
    for w, h in ((W, H), (2 * W, 2 * H)):                                # (the second one regrows the z-buffer)
        s = w / W
        img = render.render_view(rec, w, h, INTR[0] * s, INTR[1] * s, INTR[2] * s, INTR[3] * s, pose, stream=st, outputs=("depth",))
        assert (img["depth"] > 0).mean() > 0.2
    rc, _ = _track_raw(smx, pg, f + 1)
    assert rc == 0
    nn = smx.SurfelNeighborIndex()
    nn.BuildFromReconstruction(rec, 0.05, st)
    cnt, _, idx = nn.FindNeighborCandidates(rec, np.arange(0, n, 3), 4.0, 16, stream=st)
    assert cnt.max() > 1
    tri = np.stack([np.arange(0, 300), np.arange(1, 301), np.arange(2, 302)], axis=1)
    assert rec.CheckTrianglesForRemeshing(st, tri, 4.0).shape == (300,)
    _, new_size, _ = rec.Compact(st)
    assert new_size == rec.surfels_size()
    rec.DeformByCreationFrame(st, np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (32, 1)), np.zeros(32, np.uint8), f)
    pod = MeshParams.defaults()
    t_full, _ = rec.Triangulate(st, pod, index=nn)
    t_upd, _, us = rec.TriangulateUpdate(st, pod, index=nn)
    assert us["mode"] == 1 and t_upd.tobytes() == t_full.tobytes()
    rc, _ = _track_rgbd_raw(smx, rec._h, pg, f + 2, G["poses"][f + 2], 0.1)   # (a weight: the colour pair is allocated)
    assert rc == 0
    n = rec.surfels_size()
    cell = 3.0 * _mean_edge(t_full.astype(np.int64), rec.debug_download_surfels(n)[3:6].T.astype(np.float64))
    d_small, ds = rec.DecimateMesh(st, t_full, cell)
    assert 0 < d_small.shape[0] < t_full.shape[0] and ds["n_in"] == t_full.shape[0]
    _upload(rec, mr.sphere_map(4500))                                    # (more slots than the kept state has room for: reserve_keep)
    t_upd, _, us = rec.TriangulateUpdate(st, pod, index=nn)
    assert us["mode"] in (0, 4) and t_upd.shape[0] > 5000            # (the kept state was used: its first rows were copied over)
    t_again, _, us = rec.TriangulateUpdate(st, pod, index=nn)
    assert us["n_changed"] == 0 and t_again.tobytes() == t_upd.tobytes()
    d_large, ds = rec.DecimateMesh(st, t_upd, 3.0 * _mean_edge(t_upd.astype(np.int64), mr.sphere_map(4500)[0]))
    print("decimated %d of %d triangles, then %d of %d" % (d_small.shape[0], t_full.shape[0], d_large.shape[0], t_upd.shape[0]))
    assert 0 < d_large.shape[0] < t_upd.shape[0] and ds["n_in"] == t_upd.shape[0]
    # W x H (the z-buffer of the 2W x 2H splat render above is large enough: only the list, the counters and the staging
    # are allocated), then 4W x 4H, larger than anything rendered on this object, with no synchronisation in between: the
    # z-buffer regrows while the first mesh render is in flight
    depth = [smx.CUDABuffer(k * H, k * W, np.float32) for k in (1, 4)]
    for k, buf in zip((1, 4), depth):
        prm = smx.make_mesh_render_params(k * W, k * H, *[v * k for v in INTR], EYE)
        rec.RenderMesh(st, prm, t_upd, depth=buf)
    for b in depth:                                                      # (from the centre of the sphere: its inside)
        assert (b.Download(st) > 0).mean() > 0.2
        b.close()
    rec.SetDeltaTracking(st, False)
    grown = live()
    print("baseline %s, after create %s, after the services %s" % (base, created, grown))
    assert grown[0] > created[0]

    nn.close()
    rec.close()
    assert live() == base


def test_a_neighbor_index_gives_back_everything(smx, live):
    base = live()
    rng = np.random.default_rng(3)
    nn = smx.SurfelNeighborIndex()
    created = live()
    for n_points, n_queries in ((1000, 500), (3000, 1500)):             # (the second round regrows every buffer)
        p = rng.uniform(-1, 1, (n_points, 3)).astype(np.float32)
        nn.Build(p[:, 0], p[:, 1], p[:, 2], 0.1)
        cnt, _, _ = nn.FindNearestSurfelsWithinRadius(p[:n_queries] + 0.01, 0.04, 8)
        assert cnt.min() >= 1
    assert live()[1] > created[1] > base[1]
    nn.close()
    assert live() == base


# ---- 2. a failed create leaves nothing behind -----------------------------------------------------------------------------
def test_a_create_that_fails_at_any_of_its_allocations_leaves_nothing(smx, live):
    from surfelmeshing_amd import _lib
    L = _lib.load()
    base = live()

    def create():
        h = C.c_void_p()
        rc = L.smx_recon_create(C.c_uint32(CAPACITY), W, H, *[C.c_float(v) for v in INTR], C.c_int32(-1), C.byref(h))
        return rc, h

    for nth in range(201):
        smx.DebugFailAllocation(nth)
        rc, h = create()
        if rc == 0:
            break
        assert rc == SMX_ERR_HIP and not h.value, (nth, rc)
        assert live() == base, "allocation %d failed and something stayed behind" % nth
    smx.DebugFailAllocation(-1)
    assert rc == 0 and nth <= 200, "create still fails with allocation %d armed" % nth
    held = live()[0] - base[0]
    L.smx_recon_destroy(h)
    print("smx_recon_create makes %d allocations" % nth)
    assert nth == held > 50           # the loop has visited every allocation of create, and only those
    assert live() == base


# ---- 3. a failed lazy allocation is retried cleanly ---------------------------------------------------------------------
def test_track_is_retried_cleanly_after_a_failed_allocation(smx, live):
    base = live()
    pa, pb = _pipeline(smx, 3), _pipeline(smx, 3)
    g = int(G["frames"][3])
    before = live()
    smx.DebugFailAllocation(1)                                           # (the second of the four buffers)
    rc, _ = _track_raw(smx, pa, g)
    assert rc == SMX_ERR_HIP
    assert live() == before                                              # all four or none
    rc_a, res_a = _track_raw(smx, pa, g)
    rc_b, res_b = _track_raw(smx, pb, g)
    assert rc_a == 0 and rc_b == 0 and res_a == res_b
    assert live()[0] == before[0] + 2 * 5                                # (four buffers and the z-buffer, each)
    pa.reconstruction.close()
    pb.reconstruction.close()
    assert live() == base


def test_track_rgbd_colour_pair_is_allocated_whole_or_not_at_all(smx, live):
    """After a geometric call the four buffers and the z-buffer exist, so the first two allocations of a call with colour are
    the colour pair: failing the SECOND of them leaves what the call found, and the retry adds exactly the two."""
    base = live()
    pg = _pipeline(smx, 3)
    g = int(G["frames"][3])
    rc, _ = _track_raw(smx, pg, g)
    assert rc == 0
    before = live()
    rc, res = _track_rgbd_raw(smx, pg.reconstruction._h, pg, g, G["poses"][g], 0.1, fail=1)
    smx.DebugFailAllocation(-1)
    assert rc == SMX_ERR_HIP and res == b"\xA5" * len(res)
    assert live() == before                                              # both or none
    rc, _ = _track_rgbd_raw(smx, pg.reconstruction._h, pg, g, G["poses"][g], 0.1)
    assert rc == 0 and live()[0] == before[0] + 2
    pg.reconstruction.close()
    assert live() == base


def test_triangulate_and_update_are_retried_cleanly_after_a_failed_allocation(smx, live):
    from surfelmeshing_amd._lib import MeshParams, SmxError
    base = live()
    cam = smx.PinholeCamera4f(W, H, *INTR)
    a, b = smx.CUDASurfelReconstruction(CAPACITY, cam), smx.CUDASurfelReconstruction(CAPACITY, cam)
    na, nb = smx.SurfelNeighborIndex(), smx.SurfelNeighborIndex()
    pod = MeshParams.defaults()
    m = mr.sphere_map(1500)
    _upload(a, m)
    _upload(b, m)
    before = live()
    smx.DebugFailAllocation(0)                                           # (the workspace's first block)
    with pytest.raises(SmxError):
        a.Triangulate(None, pod, index=na)
    assert live() == before                                              # a complete workspace or none
    tri_a, st_a = a.Triangulate(None, pod, index=na)
    tri_b, st_b = b.Triangulate(None, pod, index=nb)
    assert tri_a.shape[0] > 2000 and tri_a.tobytes() == tri_b.tobytes() and st_a == st_b

    smx.DebugFailAllocation(2)
    with pytest.raises(SmxError):
        a.TriangulateUpdate(None, pod, index=na)
    up_a, ust_a, us_a = a.TriangulateUpdate(None, pod, index=na)
    up_b, ust_b, us_b = b.TriangulateUpdate(None, pod, index=nb)
    assert up_a.tobytes() == up_b.tobytes() == tri_b.tobytes() and ust_a == ust_b and us_a == us_b
    assert live()[0] > before[0]
    for o in (na, nb, a, b):
        o.close()
    assert live() == base


def test_the_new_services_are_retried_cleanly_after_a_failed_allocation(smx, live):
    """smx_recon_track_rgbd, smx_recon_decimate_mesh and smx_recon_render_mesh (the last two from host arrays) on object a,
    each with the failure armed at allocation 0, 1, 2, ... until the call succeeds, against object b that never sees one.
    A failed call returns SMX_ERR_HIP and leaves the guarded arrays, images and result structs as they were; the first call
    that succeeds returns what b returns.  Tracking allocates in groups that are complete or absent (the geometric four, then
    the colour pair, then the z-buffer), so the blocks the object holds more than at the start are 0, 4 or 6 after a failure,
    and a failure among the first four leaves exactly what the call found.  (A failure in the colour pair cannot leave
    "what the call found" when the same call has just completed the four: they stay, as they did before this test existed.)"""
    from surfelmeshing_amd._lib import MeshParams
    base = live()
    cam = smx.PinholeCamera4f(W, H, *INTR)
    a, b = smx.CUDASurfelReconstruction(CAPACITY, cam), smx.CUDASurfelReconstruction(CAPACITY, cam)
    na, nb = smx.SurfelNeighborIndex(), smx.SurfelNeighborIndex()
    m = mr.sphere_map(1500)
    _upload(a, m)
    _upload(b, m)
    tri, _ = a.Triangulate(None, MeshParams.defaults(), index=na)
    tri_b, _ = b.Triangulate(None, MeshParams.defaults(), index=nb)
    assert tri.shape[0] > 2000 and tri.tobytes() == tri_b.tobytes()
    pg = _pipeline(smx, 0)                                               # (the frame images of the tracking calls)
    g = int(G["frames"][0])
    cell = 3.0 * _mean_edge(tri.astype(np.int64), m[0])
    bufs = {o: [smx.CUDABuffer(2 * H, 2 * W, *spec) for spec in MESH_IMAGES] for o in (a, b)}

    def clear(o):
        for buf in bufs[o]:
            buf.Clear(0xA5)
        smx.StreamSynchronize()

    def images(o):
        return [buf.Download().tobytes() for buf in bufs[o]]

    def track(o, fail):
        rc, res = _track_rgbd_raw(smx, o._h, pg, g, EYE, 0.1, fail=fail)
        return rc, (res,), rc == 0 or res == b"\xA5" * len(res)

    def decimate(o, fail):
        rc, out, vmap, count, stats = _decimate_raw(smx, o, tri, cell, fail=fail)
        untouched = bool((out == 0xA5A5A5A5).all() and (vmap == 0xA5A5A5A5).all())
        return rc, (out[:count].tobytes(), vmap.tobytes(), count, stats), rc == 0 or untouched

    def render_mesh(o, fail):                                            # (2W x 2H: the tracking call's z-buffer regrows)
        clear(o)
        guard = images(o)
        rc, stats = _render_mesh_raw(smx, o, tri, 2 * W, 2 * H, EYE, bufs[o], fail=fail)
        smx.StreamSynchronize()
        got = images(o)
        return rc, (got, stats), rc == 0 or (got == guard and stats == b"\xA5" * len(stats))

    for name, call in (("track_rgbd", track), ("decimate_mesh", decimate), ("render_mesh", render_mesh)):
        start = live()
        for nth in range(41):
            assert nth < 40, "%s still fails with allocation %d armed" % (name, nth)
            before = live()
            rc, got, guarded = call(a, nth)
            smx.DebugFailAllocation(-1)
            assert guarded, "%s wrote to its outputs in a call that failed at allocation %d" % (name, nth)
            if rc == 0:
                break
            assert rc == SMX_ERR_HIP, (name, nth, rc)
            if name == "track_rgbd":
                # all or none, per group: a failure among the geometric four (they come first) leaves what the call found,
                # one in the colour pair behind them the complete four and nothing else, one in the z-buffer all six
                assert live()[0] - start[0] in (0, 4, 6), (nth, before, live())
                assert live() == before or nth >= 4, (nth, before, live())
        rc_b, want, _ = call(b, -1)
        assert rc_b == 0 and got == want, name
        # (blocks the object holds more than before the service's first call = the allocations of a first call that meets
        # no failure, less the z-buffer the mesh render replaces; the armed index at the first success is smaller where
        # groups completed by earlier failed calls were kept)
        print("%s: a first call makes %d allocations that stay (first success with allocation %d armed)"
              % (name, live()[0] - start[0], nth))

    for bl in bufs.values():
        for buf in bl:
            buf.close()
    for o in (na, nb, a, b, pg.reconstruction):
        o.close()
    assert live() == base


# ---- 4. the hook disarms ----------------------------------------------------------------------------------------------
def test_the_failure_hook_fires_once_and_can_be_disarmed(smx, live):
    from surfelmeshing_amd._lib import SmxError
    base = live()
    smx.DebugFailAllocation(0)
    with pytest.raises(SmxError):
        smx.SurfelNeighborIndex()
    assert live() == base
    nn = smx.SurfelNeighborIndex()                                       # (it has fired: the next allocation succeeds)
    nn.close()
    smx.DebugFailAllocation(1)
    smx.DebugFailAllocation(-1)                                          # (a pending one is disarmed)
    nn = smx.SurfelNeighborIndex()
    assert live()[0] == base[0] + 4
    nn.close()
    assert live() == base


# ---- 5. steady state allocates nothing ----------------------------------------------------------------------------------
def test_the_frame_loop_allocates_nothing_after_its_first_frames(smx, live):
    base = live()
    seen = {}
    pg = _pipeline(smx, 10, lambda k: seen.__setitem__(k, live()))
    print("after frame 3: %s, after frame 10: %s" % (seen[3], seen[10]))
    assert seen[3] == seen[10]
    assert pg.reconstruction.surfels_size() > 4000
    pg.reconstruction.close()
    assert live() == base
