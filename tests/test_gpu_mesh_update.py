"""smx_recon_triangulate_update on the device.  The contract is equality: after any sequence of changes the update returns
the bytes and the statistics smx_recon_triangulate returns on the same map.  "Equals full" below always means: tobytes()
of the triangles and the whole smx_mesh_stats equal those of Triangulate on a SECOND object that was uploaded the same rows.
The counts of the update (changed, D) are compared with the model of tests/mesh_update_ref.py, exactly."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as mr
import mesh_update_ref as mu

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
TRUNCATING = dict(search_radius_factor=1.5, max_neighbors=16)


def _pod(prm):
    from surfelmeshing_amd._lib import MeshParams
    return MeshParams.defaults(max_angle_between_normals_deg=prm.max_angle_between_normals_deg,
                               min_triangle_angle_deg=prm.min_triangle_angle_deg,
                               max_triangle_angle_deg=prm.max_triangle_angle_deg,
                               search_radius_factor=prm.search_radius_factor, max_neighbors=prm.max_neighbors)


def _upload(rec, m):
    rec.debug_upload_surfels(mr.rows_of_map(*m), int(np.sum(m[2] < 0)))


class Pair:
    """The object under test and the second object the full call runs on."""

    def __init__(self, smx, capacity=6000):
        self.rec = smx.CUDASurfelReconstruction(capacity, smx.PinholeCamera4f(*CAM))
        self.ref = smx.CUDASurfelReconstruction(capacity, smx.PinholeCamera4f(*CAM))
        self.nn = smx.SurfelNeighborIndex()

    def set_map(self, m):
        _upload(self.rec, m)
        _upload(self.ref, m)

    def update(self, prm=None, fraction=None, cell_size=None):
        pod = _pod(prm or mr.Params())
        tri, st, us = self.rec.TriangulateUpdate(None, pod, index=self.nn, cell_size=cell_size, full_above_fraction=fraction)
        want, wst = self.ref.Triangulate(None, pod)
        print("update %s, stats %s, full call %s" % (us, st, wst))
        assert tri.dtype == np.uint32 and tri.shape == want.shape
        assert tri.tobytes() == want.tobytes() and st == wst          # equals full
        return tri, st, us

    def close(self):
        self.nn.close()
        self.rec.close()
        self.ref.close()


@pytest.fixture(scope="module")
def sphere():
    return mr.sphere_map(4000)


@pytest.fixture(scope="module")
def cap_change(sphere):
    """The issue's perturbation in the cap z > 0.9, with 100 appended slots: 4000 -> 4100 slots."""
    cap = np.nonzero(sphere[0][:, 2] > 0.9)[0]
    new, picked = mu.perturb(sphere, cap, np.random.default_rng(11), n_append=100)
    return new, picked


def test_first_update_runs_the_full_path_and_the_second_finds_nothing(smx, sphere):
    pr = Pair(smx)
    pr.set_map(sphere)
    tri, st, us = pr.update()
    T = tri.shape[0]
    assert T > 5000 and us["mode"] == 1
    again, st2, us2 = pr.update()
    assert us2 == dict(mode=0, n_changed=0, n_dirty=0, n_reagreed=0, n_kept_triangles=T)
    assert again.tobytes() == tri.tobytes() and st2 == st
    pr.close()


# cell size: the balls of this map have radii of 0.11 .. 0.22.  With the default cell of 0.05 none is small enough for the
# coarse filter in front of the reverse test and every unchanged slot takes the exact test; with 0.5 all of them are
# filtered first.  n_dirty has to be the rule's value either way.
@pytest.mark.parametrize("cell_size", [None, 0.5], ids=["unfiltered", "coarse_filter"])
@pytest.mark.parametrize("params_kw", [{}, TRUNCATING], ids=["defaults", "truncated_lists"])
def test_perturbation_in_a_cap_is_incremental_and_equals_full(smx, sphere, cap_change, params_kw, cell_size):
    prm = mr.Params(**params_kw)
    new, picked = cap_change
    n = new[0].shape[0]
    assert sphere[0].shape[0] == 4000 and n == 4100        # across the 4096 boundary: 16 -> 17 workgroups of the scan
    pr = Pair(smx)
    pr.set_map(sphere)
    _, st0, us0 = pr.update(prm, cell_size=cell_size)
    assert us0["mode"] == 1
    if params_kw:
        assert st0["truncated_lists"] > 0
    pr.set_map(new)
    tri, st, us = pr.update(prm, cell_size=cell_size)
    assert us["mode"] == 0
    assert us["n_changed"] == picked.size + 100 == int(mu.changed_mask(sphere, new).sum())
    assert us["n_dirty"] == int(mu.dirty_mask(sphere, new, prm).sum())
    assert us["n_dirty"] <= us["n_reagreed"] <= n and us["n_dirty"] < n / 4 and us["n_kept_triangles"] > 0
    mr.check_properties(tri, *new, prm)
    pr.close()


def test_a_single_moved_slot(smx, sphere):
    pr = Pair(smx)
    pr.set_map(sphere)
    pr.update()
    # the first slot from 1234 on whose move gives a work list that is no multiple of the four wavefronts of a workgroup
    for slot in range(1234, 1300):
        pos, nrm, r2 = (a.copy() for a in sphere)
        pos[slot] = (pos[slot] * (1.0 + 0.05 * np.sqrt(r2[slot]))).astype(np.float32)      # moved along its direction
        moved = (pos, nrm, r2)
        want = int(mu.dirty_mask(sphere, moved, mr.Params()).sum())
        if want % 4 != 0:
            break
    assert 1 < want < 64 and want % 4 != 0
    pr.set_map(moved)
    tri, _, us = pr.update(cell_size=0.5)
    print("slot %d moved: a work list of %d slots" % (slot, want))
    assert us["mode"] == 0 and us["n_changed"] == 1 and us["n_dirty"] == want
    # A is D and at most 16 old and 16 new ring members of each of its slots; a triangle that is not kept is owned by a
    # slot of A, which owns at most 16
    assert want <= us["n_reagreed"] <= 33 * want
    assert tri.shape[0] - 16 * us["n_reagreed"] <= us["n_kept_triangles"] < tri.shape[0]
    pr.close()


def test_the_two_ends_of_the_path_choice(smx, sphere):
    rng = np.random.default_rng(5)
    pos, nrm, r2 = (a.copy() for a in sphere)
    pos = (pos + 1e-4 * rng.standard_normal(pos.shape)).astype(np.float32).astype(np.float64)
    jittered = (pos, nrm, r2)
    n = pos.shape[0]
    assert mu.changed_mask(sphere, jittered).all()
    for fraction, mode in ((1.0, 0), (0.0, 4)):
        pr = Pair(smx)
        pr.set_map(sphere)
        pr.update()
        pr.set_map(jittered)
        _, _, us = pr.update(fraction=fraction)       # (mode 0 here is the subset path over the whole map)
        assert us["mode"] == mode and us["n_changed"] == n and us["n_dirty"] == n and us["n_reagreed"] == n
        assert us["n_kept_triangles"] == 0
        pr.close()


def test_what_drops_the_state(smx, sphere, cap_change):
    new, _ = cap_change
    pr = Pair(smx)
    pr.set_map(sphere)
    assert pr.update()[2]["mode"] == 1
    assert pr.update()[2]["mode"] == 0
    pr.rec.Triangulate(None, _pod(mr.Params()))                   # the plain call shares the rings
    assert pr.update()[2]["mode"] == 1
    assert pr.update(mr.Params(**TRUNCATING))[2]["mode"] == 2      # other parameters
    assert pr.update(mr.Params(**TRUNCATING))[2]["mode"] == 0
    pr.rec.ResetTriangulation()
    assert pr.update(mr.Params(**TRUNCATING))[2]["mode"] == 1
    # fewer slots than kept: a compaction (the perturbed map has merged slots)
    pr.set_map(new)
    before, st, us = pr.update(mr.Params(**TRUNCATING))
    assert us["mode"] == 0
    n = new[0].shape[0]
    old_to_new, new_size, _ = pr.rec.Compact(None)
    assert new_size == n - 10
    rows = pr.rec.debug_download_surfels(new_size)
    pr.ref.debug_upload_surfels(rows, 0)
    after, st2, us2 = pr.update(mr.Params(**TRUNCATING))
    assert us2["mode"] == 3 and us2["n_kept_triangles"] == 0
    assert np.array_equal(after, old_to_new[before.astype(np.int64)])
    assert pr.update(mr.Params(**TRUNCATING))[2]["mode"] == 0
    pr.close()


def test_grown_map_followed_while_it_grows(smx):
    from common import small_stream
    from test_gpu_mesh import _grown
    pg, rec = _grown(smx)
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)      # (the stream _grown integrates)
    for f in range(0, 30):
        pg.release(f)
    for f in range(38, 44):
        pg.upload(f, *s.frame(f))
    ref = smx.CUDASurfelReconstruction(60000, smx.PinholeCamera4f(*CAM))
    nn = smx.SurfelNeighborIndex()
    pod = _pod(mr.Params())
    modes = []
    for step in range(3):
        if step:
            for f in (32 + 2 * step, 33 + 2 * step):
                pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
        # (the default fraction; whichever path it chooses, the result is the full call's)
        n = rec.surfels_size()
        rows = rec.debug_download_surfels(n)
        tri, st, us = rec.TriangulateUpdate(None, pod, index=nn)
        ref.debug_upload_surfels(rows, int(np.sum(rows[7] < 0)))
        want, wst = ref.Triangulate(None, pod)
        print("step %d: %d slots, update %s, stats %s" % (step, n, us, st))
        assert tri.tobytes() == want.tobytes() and st == wst
        assert st["n_live"] == rec.surfel_count()
        if step and us["mode"] == 4:
            print("step %d: the default fraction chose the full path (|D| = %d of %d slots)" % (step, us["n_dirty"], n))
        modes.append(us["mode"])
    assert modes[0] == 1 and all(m in (0, 4) for m in modes[1:])
    # two frames of integration touch a large share of this small map, so the default fraction may have chosen the full
    # path above: two more frames with the fraction 1 run the incremental path on a map that grew by integration
    for f in (38, 39):
        pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    n = rec.surfels_size()
    rows = rec.debug_download_surfels(n)
    tri, st, us = rec.TriangulateUpdate(None, pod, index=nn, full_above_fraction=1.0)
    ref.debug_upload_surfels(rows, int(np.sum(rows[7] < 0)))
    want, wst = ref.Triangulate(None, pod)
    print("fraction 1: %d slots, update %s" % (n, us))
    assert us["mode"] == 0 and 0 < us["n_changed"] <= us["n_dirty"] <= us["n_reagreed"] <= n
    assert tri.tobytes() == want.tobytes() and st == wst and st["n_live"] == rec.surfel_count()
    nn.close()
    ref.close()


def test_capacity_rule_and_guard_words(smx, sphere):
    from surfelmeshing_amd import _lib
    pr = Pair(smx)
    pr.set_map(sphere)
    ref, _ = pr.ref.Triangulate(None, _pod(mr.Params()))
    T = ref.shape[0]
    L, p = _lib.load(), _lib.MeshParams.defaults()

    def call(buf, capacity, on_device=0):
        n, st, us = C.c_uint32(0), _lib.MeshStats(), _lib.MeshUpdateStats()
        ptr = None if buf is None else (C.c_void_p(buf) if on_device else buf.ctypes.data_as(C.c_void_p))
        rc = L.smx_recon_triangulate_update(pr.rec._h, None, pr.nn._h, C.c_float(0.05), C.byref(p), C.c_float(-1.0), ptr,
                                            C.c_uint32(capacity), C.c_int32(on_device), C.byref(n), C.byref(st), C.byref(us))
        return rc, n.value, st, us
    guard = 0xA5A5A5A5
    buf = np.full(3 * T + 8, guard, np.uint32)
    rc, n, st, us = call(buf, T - 1)
    assert rc == -1 and n == T and st.n_triangles == T and us.mode == 1 and np.all(buf == guard)   # nothing is written
    rc, n, st, us = call(buf, T)                                   # the state had advanced: nothing changed since
    assert rc == 0 and n == T and us.mode == 0 and us.n_changed == 0 and us.n_kept_triangles == T
    assert buf[:3 * T].tobytes() == ref.tobytes() and np.all(buf[3 * T:] == guard)
    rc, n, _, us = call(None, 0)                                   # the count-only form, from the kept state
    assert rc == -1 and n == T and us.n_changed == 0
    # the device-pointer form: the same bytes, nothing behind them; on the recomputing path too
    dbuf = smx.CUDABuffer(1, 3 * T + 8, np.uint32)
    for reset in (False, True):
        if reset:
            pr.rec.ResetTriangulation()
        dbuf.Upload(np.full((1, 3 * T + 8), guard, np.uint32))
        rc, n, _, us = call(dbuf.ToCUDA().address, T, on_device=1)
        back = dbuf.Download()[0]
        assert rc == 0 and n == T and us.mode == (1 if reset else 0)
        assert back[:3 * T].tobytes() == ref.tobytes() and np.all(back[3 * T:] == guard)
    with pytest.raises(_lib.SmxError):
        pr.rec.TriangulateUpdate(None, _lib.MeshParams.defaults(), index=pr.nn, full_above_fraction=1.01)
    dbuf.close()
    pr.close()


def test_two_identical_sequences_give_identical_bytes_and_timings_are_reported(smx, sphere, cap_change):
    new, _ = cap_change
    recs = [smx.CUDASurfelReconstruction(6000, smx.PinholeCamera4f(*CAM)) for _ in range(2)]
    names = {"diff", "index_builds", "reverse_test", "subset_lists", "stars", "agree_merge"}
    for rec in recs:
        t = rec.debug_mesh_update_timings()
        assert set(t) == names and all(v == 0.0 for v in t.values())          # zeros before the first update
    outs = [[], []]
    for m in (sphere, new, new, sphere):          # (the last one has fewer slots than kept)
        for rec, out in zip(recs, outs):
            _upload(rec, m)
            tri, st, us = rec.TriangulateUpdate(None, _pod(mr.Params()))
            out.append((tri.tobytes(), st, us))
    assert outs[0] == outs[1]
    assert [o[2]["mode"] for o in outs[0]] == [1, 0, 0, 3]
    for rec in recs:
        t = rec.debug_mesh_update_timings()
        assert set(t) == names and all(np.isfinite(v) and v >= 0.0 for v in t.values())
        rec.close()


def test_empty_map_and_map_mesher(smx, sphere):
    from surfelmeshing_amd import meshing
    rec = smx.CUDASurfelReconstruction(6000, smx.PinholeCamera4f(*CAM))
    mesher = meshing.MapMesher(rec, meshing.MeshParams())
    tri, st, us = mesher.update()
    assert tri.shape == (0, 3) and st["n_live"] == 0
    _upload(rec, sphere)
    tri, st, us = mesher.update()
    want, wst = rec.Triangulate(None, index=mesher.index)
    assert us["mode"] == 1 and tri.tobytes() == want.tobytes() and st == wst and mesher.triangles is tri
    assert mesher.update()[2]["mode"] == 1            # (the plain call above dropped the state)
    assert mesher.update()[2]["mode"] == 0
    mesher.reset()
    assert mesher.triangles is None and mesher.update()[2]["mode"] == 1
    assert set(mesher.timings()) == {"diff", "index_builds", "reverse_test", "subset_lists", "stars", "agree_merge"}
    mesher.close()
    rec.close()
