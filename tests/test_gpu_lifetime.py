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
    _upload(rec, mr.sphere_map(4500))                                    # (more slots than the kept state has room for: reserve_keep)
    t_upd, _, us = rec.TriangulateUpdate(st, pod, index=nn)
    assert us["mode"] in (0, 4) and t_upd.shape[0] > 5000            # (the kept state was used: its first rows were copied over)
    t_again, _, us = rec.TriangulateUpdate(st, pod, index=nn)
    assert us["n_changed"] == 0 and t_again.tobytes() == t_upd.tobytes()
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
