"""smx_rayscene on the device: a scene built once answers every cast with the bytes of the brute-force model of
tests/raycast_ref.py and of smx_recon_raycast_mesh on the same inputs, for every ray set, cell size, occupancy setting and cull
mode; its work counters stand in the relations the contract fixes against that call's; it is a snapshot (the map may change or
go); and the calling rules and allocation failures write nothing."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distance_ref as dr
import mesh_ref as mr
import raycast_ref as rr
import rayscene_ref as sr
from common import ROOT

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
STEP1 = ("n_in", "n_not_live", "n_repeated", "n_out_of_range")
CAST = ("n_rays", "n_bad_rays", "n_hit", "n_front_hits", "max_t_bits")


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


def _check_build(st, g, cs, occ, what):
    """The build's statistics against the numpy grid g at the cell size used."""
    k = st["occupancy_log2"]
    if occ == -1:
        assert k == -1, what
    elif occ == 0:
        assert k in (-1, sr.smallest(g)), what
    else:
        assert k == occ - 1, what
    if k >= 0:
        assert st["n_blocks_set"] == sr.blocks_set(g, k) and st["occupancy_bytes"] == 4 * ((sr.bits(g, k) + 31) // 32), (what, st)
        if k == 0:
            assert st["n_blocks_set"] == st["n_cells"], what
    else:
        assert st["n_blocks_set"] == 0 and st["occupancy_bytes"] == 0, what
    assert st["n_cells"] == g["cells"].shape[0] and st["device_bytes"] >= st["occupancy_bytes"] + 48 * st["n_entries"], (what, st)


@pytest.fixture(scope="module")
def world(smx):
    """One map and one scene per (cell size, occupancy setting) for the module: many casts, one build."""
    pos, nrm, r2, tri, info = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    scenes = {}
    for cs in rr.CELL_SIZES:
        for occ in sr.SETTINGS:
            sc = rec.BuildRayScene(None, tri, cs, occ)
            g = sr.grid(pos, r2, tri, sc.stats["cell_size_used"])
            _check_build(sc.stats, g, cs, occ, "cell %g occupancy %d" % (cs, occ))
            if cs > 0:
                assert sc.stats["cell_size_used"] == float(rr.cell_used(cs))
                assert {k: sc.stats[k] for k in ("n_wide", "n_entries", "n_cells")} == rr.structure(pos, r2, tri, cs)
            scenes[(cs, occ)] = sc
        print("cell %g: the library's choice is k = %d; k = 0 has %d bits, k = 3 %d" % (
            cs, scenes[(cs, 0)].stats["occupancy_log2"], sr.bits(g, 0), sr.bits(g, 3)))
    yield dict(m=(pos, nrm, r2), rec=rec, tri=tri, info=info, scenes=scenes)
    for sc in scenes.values():
        sc.close()
    rec.close()


def _relations(st, k, base, what):
    """A cast's work counters against smx_recon_raycast_mesh's at the same c."""
    assert st["n_layers"] == base["n_layers"] and st["n_pair_tests"] == base["n_pair_tests"], (what, st, base)
    if k < 0:
        assert st["n_bit_tests"] == 0 and st["n_lookups"] == base["n_lookups"], (what, st, base)
    else:
        assert st["n_bit_tests"] == base["n_lookups"] and st["n_lookups"] <= base["n_lookups"], (what, st, base)
        if k == 0:
            assert st["n_lookup_misses"] == 0, (what, st)
    assert st["n_lookup_misses"] <= st["n_lookups"]
    return st["n_lookups"] - st["n_lookup_misses"]


@pytest.mark.parametrize("name", list(rr.ray_sets()))
def test_every_ray_set_equals_the_model_and_the_call(world, name):
    rec, tri, scenes = world["rec"], world["tri"], world["scenes"]
    (rays, t0, t1), model = rr.ray_sets()[name], rr.model_of(name)
    for cull in (0, 1, 2):
        wh, wt, wuv, wst = rr.answer(model, cull)
        for cs in rr.CELL_SIZES:
            bh, bt, buv, bst = rec.RaycastMesh(None, tri, rays, t0, t1, cs, cull, return_uv=True)
            found = set()
            for occ in sr.SETTINGS:
                sc = scenes[(cs, occ)]
                what = "%s cell %g occupancy %d cull %d" % (name, cs, occ, cull)
                hit, t, uv, st = sc.Cast(None, rays, t0, t1, cull, return_uv=True)
                assert hit.dtype == np.uint32 and t.dtype == np.float32 and uv.dtype == np.float32
                for got, want, other in ((hit, wh, bh), (t, wt, bt), (uv, wuv, buv)):
                    assert got.tobytes() == want.tobytes() and got.tobytes() == other.tobytes(), what
                assert {k: st[k] for k in CAST} == {k: wst[k] for k in CAST} == {k: bst[k] for k in CAST}, what
                assert {k: sc.stats[k] for k in STEP1} == {k: wst[k] for k in STEP1} == {k: bst[k] for k in STEP1}, what
                assert sc.stats["cell_size_used"] == bst["cell_size_used"] and all(sc.stats[k] == bst[k] for k in ("n_wide", "n_entries", "n_cells"))
                found.add(_relations(st, sc.stats["occupancy_log2"], bst, what))
            assert len(found) == 1, (name, cs, cull, found)
    t = scenes[(0.0, 4)].debug_timings()
    assert set(t) == {"mark", "index", "occupancy", "cast", "stats"} and all(np.isfinite(v) and v >= 0 for v in t.values())


def _cast_all(sc, cull=0):
    return [sc.Cast(None, rays, t0, t1, cull, return_uv=True) for rays, t0, t1 in rr.ray_sets().values()]


def _same(a, b):
    return all(x[k].tobytes() == y[k].tobytes() for x, y in zip(a, b) for k in range(3)) and all(x[3] == y[3] for x, y in zip(a, b))


def test_a_scene_is_a_snapshot(smx):
    pos, nrm, r2, tri, _ = dr.world()
    rays, t0, t1 = rr.ray_sets()["pinhole"]
    # the map overwritten with moved positions
    rec = _rec_of(smx, (pos, nrm, r2))
    with rec.BuildRayScene(None, tri, 0.0225, 4) as sc, rec.BuildRayScene(None, tri, 0.0, 0) as auto:
        before, before_auto = _cast_all(sc), _cast_all(auto)
        call = rec.RaycastMesh(None, tri, rays, t0, t1, 0.0225, 0, return_uv=True)
        assert all(call[k].tobytes() == before[list(rr.ray_sets()).index("pinhole")][k].tobytes() for k in range(3))
        moved = pos.copy()
        moved[:, 0] += np.float32(0.125)
        rec.debug_upload_surfels(mr.rows_of_map(moved, nrm, r2), int(np.sum(r2 < 0)))
        assert _same(_cast_all(sc), before) and _same(_cast_all(auto), before_auto)
        changed = rec.RaycastMesh(None, tri, rays, t0, t1, 0.0225, 0, return_uv=True)
        assert changed[1].tobytes() != call[1].tobytes()                       # (the test can fail: the map did change)
        # the object the scene was built from destroyed
        rec.close()
        assert _same(_cast_all(sc), before) and _same(_cast_all(auto), before_auto)
    # a map with merged slots compacted
    rec = _rec_of(smx, (pos, nrm, r2))
    assert int(np.sum(r2 < 0)) > 0
    with rec.BuildRayScene(None, tri, 0.0, 1) as sc:
        before = _cast_all(sc)
        call = rec.RaycastMesh(None, tri, rays, t0, t1, 0.0, 0, return_uv=True)
        _, new_size, _ = rec.Compact(None)
        assert new_size < pos.shape[0]
        assert _same(_cast_all(sc), before)
        try:
            after = rec.RaycastMesh(None, tri, rays, t0, t1, 0.0, 0, return_uv=True)
            differs = any(after[k].tobytes() != call[k].tobytes() for k in range(3))
        except smx.SmxError:
            differs = True                                                      # (an index past the compacted map: refused)
        assert differs
    rec.close()


def test_rebuild_in_place_two_scenes_and_a_call_in_between(smx, world):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    name = "inside-out"
    rays, t0, t1 = rr.ray_sets()[name]
    full = rr.answer(rr.model_of(name), 0)
    small_tri = tri[:2000]
    small = rr.answer(rr.brute(m[0], m[2], small_tri, rays, t0, t1), 0)

    def equals(sc, want, what):
        got = sc.Cast(None, rays, t0, t1, 0, return_uv=True)
        assert all(got[k].tobytes() == want[k].tobytes() for k in range(3)) and {k: got[3][k] for k in CAST} == {k: want[3][k] for k in CAST}, what
        return got
    a = rec.BuildRayScene(None, tri, 0.0225, 4)
    equals(a, full, "first build")
    assert rec.BuildRayScene(None, small_tri, 0.0225, 1, scene=a) is a and a.stats["n_in"] == 2000 and a.stats["occupancy_log2"] == 0
    equals(a, small, "rebuilt smaller")
    rec.BuildRayScene(None, tri, 0.2, -1, scene=a)
    assert a.stats["n_in"] == tri.shape[0] and a.stats["occupancy_log2"] == -1
    first = equals(a, full, "rebuilt larger")
    # a second scene of the same object, and a call of the sibling in between
    b = rec.BuildRayScene(None, small_tri, 0.0, 4)
    equals(b, small, "second scene")
    call = rec.RaycastMesh(None, small_tri, rays, t0, t1, 0.05, 0, return_uv=True)
    assert all(call[k].tobytes() == small[k].tobytes() for k in range(3))
    again = equals(a, full, "first scene after the second and the call")
    assert again[3] == first[3]
    equals(b, small, "second scene after the call")
    call2 = rec.RaycastMesh(None, small_tri, rays, t0, t1, 0.05, 0, return_uv=True)
    assert call2[3] == call[3] and all(call2[k].tobytes() == call[k].tobytes() for k in range(3))
    a.close()
    b.close()
    a.close()                                                                   # (closing twice is harmless)
    with pytest.raises(ValueError):
        a.Cast(None, rays)


def _lib_of():
    from surfelmeshing_amd import _lib
    return _lib


def _ptr(a):
    return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)


def _build_raw(rec, sc, tri, n_in, cell_size=0.0, occupancy=0, on_device=0, stats=True):
    _lib = _lib_of()
    prm, st = _lib.RaySceneParams(cell_size, occupancy), _lib.RaySceneStats()
    rc = _lib.load().smx_recon_build_rayscene(rec._h, None, sc, C.byref(prm), _ptr(tri), C.c_uint32(n_in), C.c_int32(on_device),
                                              C.byref(st) if stats else None)
    return rc, st


def _cast_raw(sc, rays, n_rays, hit, t, uv, t_min=0.0, t_max=2.0 ** 20, cell_size=0.0, cull=0, on_device=0, stats=True):
    _lib = _lib_of()
    prm, st = _lib.RaycastParams(t_min, t_max, cell_size, cull), _lib.RaySceneCastStats()
    rc = _lib.load().smx_rayscene_cast(sc, None, C.byref(prm), _ptr(rays), C.c_uint32(n_rays), _ptr(hit), _ptr(t), _ptr(uv), C.c_int32(on_device),
                                       C.byref(st) if stats else None)
    return rc, st


def _guards(P, extra=4):
    return np.full(P + extra, GUARD, np.uint32), np.full(P + extra, GUARD, np.uint32), np.full(2 * P + extra, GUARD, np.uint32)


def _untouched(g):
    return all(np.all(a == GUARD) for a in g)


def test_calling_rules_on_host_and_device_arrays(smx, world):
    _lib = _lib_of()
    L = _lib.load()
    rec, tri, m = world["rec"], world["tri"], world["m"]
    name = "around the hand-made triangles"
    rays, t0, t1 = rr.ray_sets()[name]
    P, n_in, n = rays.shape[0], tri.shape[0], m[0].shape[0]
    wh, wt, wuv, wst = rr.answer(rr.model_of(name), 1)
    sc = C.c_void_p()
    assert L.smx_rayscene_create(C.c_int32(-1), C.byref(sc)) == 0
    prm = _lib.RaySceneParams(1.0, 5)
    assert L.smx_rayscene_params_default(C.byref(prm)) == 0 and prm.cell_size == 0.0 and prm.occupancy == 0
    # a cast on a scene never built: refused, nothing written
    g = _guards(P)
    assert _cast_raw(sc, rays, P, *g)[0] == -1 and _untouched(g)
    rc, bst = _build_raw(rec, sc, tri, n_in, 0.0, 4)
    assert rc == 0 and bst.n_in == n_in and bst.occupancy_log2 == 3
    # host arrays pre-filled with a guard word; room to spare stays untouched
    hit, t, uv = _guards(P)
    rc, st = _cast_raw(sc, rays, P, hit, t, uv, cull=1)
    assert rc == 0 and hit[:P].tobytes() == wh.tobytes() and t[:P].tobytes() == wt.tobytes() and uv[:2 * P].tobytes() == wuv.tobytes()
    assert np.all(hit[P:] == GUARD) and np.all(t[P:] == GUARD) and np.all(uv[2 * P:] == GUARD)
    assert {k: int(getattr(st, k)) for k in CAST} == {k: wst[k] for k in CAST}
    # uv = NULL and stats = NULL leave the other outputs as they are
    h2, t2, _ = _guards(P)
    assert _cast_raw(sc, rays, P, h2, t2, None, cull=1, stats=False)[0] == 0 and h2.tobytes() == hit.tobytes() and t2.tobytes() == t.tobytes()
    # cell_size != 0 in the cast, a bad cull, a bad range: refused, nothing written
    for kw in (dict(cell_size=0.05), dict(cull=3), dict(t_min=2.0, t_max=1.0)):
        g = _guards(P)
        assert _cast_raw(sc, rays, P, *g, **kw)[0] == -1 and _untouched(g), kw
    # an output over the rays: refused, nothing written
    both = np.concatenate([rays.reshape(-1).view(np.uint32), np.full(8, GUARD, np.uint32)])
    snapshot = both.copy()
    g = _guards(P)
    assert _cast_raw(sc, both, P, g[0], g[1], both[6 * P - 1:])[0] == -1 and both.tobytes() == snapshot.tobytes() and _untouched(g[:2])
    # n_rays == 0
    rc, st = _cast_raw(sc, None, 0, None, None, None)
    assert rc == 0 and st.n_rays == 0 and st.n_hit == 0 and st.n_layers == 0
    # device arrays give the same bytes
    din, dry = smx.CUDABuffer(1, 3 * n_in, np.uint32), smx.CUDABuffer(1, 6 * P, np.uint32)
    sizes = (P + 4, P + 4, 2 * P + 4)
    outs = [smx.CUDABuffer(1, k, np.uint32) for k in sizes]
    din.Upload(tri.reshape(1, -1))
    dry.Upload(rays.reshape(1, -1).view(np.uint32))
    for b, k in zip(outs, sizes):
        b.Upload(np.full((1, k), GUARD, np.uint32))
    a = [b.ToCUDA().address for b in [din, dry] + outs]
    assert _build_raw(rec, sc, a[0], n_in, 0.0225, 1, on_device=1)[0] == 0
    rc, st = _cast_raw(sc, a[1], P, a[2], a[3], a[4], cull=1, on_device=1)
    back = [b.Download()[0] for b in outs]
    assert rc == 0 and back[0].tobytes() == hit.tobytes() and back[1].tobytes() == t.tobytes() and back[2].tobytes() == uv.tobytes()
    assert din.Download()[0].tobytes() == tri.tobytes() and dry.Download()[0].tobytes() == rays.tobytes()
    assert _cast_raw(sc, a[1], P, a[1] + 8, a[3], a[4], on_device=1)[0] == -1          # overlap on the device
    # a bad index in the build, on the device and on the host: refused, and the scene is left empty
    bad = tri.copy()
    bad[n_in // 3, 2] = n
    din.Upload(bad.reshape(1, -1))
    assert _build_raw(rec, sc, a[0], n_in, on_device=1)[0] == -1
    outs[0].Upload(np.full((1, P + 4), GUARD, np.uint32))
    assert _cast_raw(sc, a[1], P, a[2], a[3], a[4], on_device=1)[0] == -1 and np.all(outs[0].Download()[0] == GUARD)
    for b in [din, dry] + outs:
        b.close()
    assert _build_raw(rec, sc, tri, n_in)[0] == 0
    for where in (0, 3 * n_in - 1):
        bad = tri.copy()
        bad.reshape(-1)[where] = n
        g = _guards(P)
        assert _build_raw(rec, sc, bad, n_in)[0] == -1 and _cast_raw(sc, rays, P, *g)[0] == -1 and _untouched(g)
    # bad build parameters: refused, and the scene stays empty
    for cs, occ in ((-1.0, 0), (float("nan"), 0), (0.0, -2), (0.0, 8)):
        assert _build_raw(rec, sc, tri, n_in, cs, occ)[0] == -1
    # n_in == 0 is a valid build: every ray is "none"
    rc, bst = _build_raw(rec, sc, None, 0, 0.0, 4)
    assert rc == 0 and bst.n_in == 0 and bst.n_entries == 0 and bst.n_blocks_set == 0
    g = _guards(P)
    rc, st = _cast_raw(sc, rays, P, *g)
    assert rc == 0 and np.all(g[0][:P] == rr.INVALID) and np.all(np.isinf(g[1][:P].view(np.float32))) and np.all(np.isnan(g[2][:2 * P].view(np.float32)))
    assert st.n_hit == 0 and st.n_rays == P and st.n_bad_rays == wst["n_bad_rays"] and np.all(g[0][P:] == GUARD)
    assert L.smx_rayscene_destroy(sc) == 0 and L.smx_rayscene_destroy(None) == 0
    # device tensors through the Python calls
    import torch
    tt, tr = torch.from_numpy(tri.astype(np.int32)).cuda(), torch.from_numpy(rays.copy()).cuda()
    with rec.BuildRayScene(None, tt, 0.0, 0) as ts:
        th, tq, tuv, tst = ts.Cast(None, tr, t0, t1, cull=1, return_uv=True)
        torch.cuda.synchronize()
        assert th.cpu().numpy().view(np.uint32).tobytes() == wh.tobytes() and tq.cpu().numpy().tobytes() == wt.tobytes()
        assert tuv.cpu().numpy().tobytes() == wuv.tobytes() and tst["n_hit"] == wst["n_hit"]


def test_an_explicit_block_size_that_does_not_fit_is_refused(smx):
    """Two small triangles 120 m apart at the smallest cell: 61 440 cells per axis, 2^33 bits at k = 5, 2^30 at k = 6."""
    f = np.float32
    corner = np.array([[0, 0, 0], [0.001, 0, 0], [0, 0.001, 0]], f)
    pos = np.concatenate([corner - f(59.99), corner + f(59.99)])
    nrm = np.tile(np.array([0, 0, 1], f), (6, 1))
    r2 = np.full(6, 1e-4, f)
    tri = np.array([[0, 1, 2], [3, 4, 5]], np.uint32)
    g = sr.grid(pos, r2, tri, 2.0 ** -9)
    assert not sr.fits(g, 5) and sr.fits(g, 6) and sr.smallest(g) == 6
    rec = _rec_of(smx, (pos, nrm, r2), spare=10)
    rays = np.array([[-59.9897, -59.9897, -50.0, 0, 0, -1], [59.9903, 59.9903, 50.0, 0, 0, 1], [0, 0, 0, 1, -1, 0.5]], f)
    want = rr.answer(rr.brute(pos, r2, tri, rays, 0.0, 100.0), 0)
    assert want[3]["n_hit"] == 2
    for occ in (1, 6):
        with pytest.raises(smx.SmxError):
            rec.BuildRayScene(None, tri, 2.0 ** -9, occ)
    keep = rec.BuildRayScene(None, tri, 2.0 ** -9, -1)
    with pytest.raises(smx.SmxError):
        rec.BuildRayScene(None, tri, 2.0 ** -9, 3, scene=keep)                  # ... and it leaves the scene empty
    with pytest.raises(smx.SmxError):
        keep.Cast(None, rays, 0.0, 100.0)
    keep.close()
    for occ in (7, 0, -1):
        with rec.BuildRayScene(None, tri, 2.0 ** -9, occ) as sc:
            _check_build(sc.stats, g, 2.0 ** -9, occ, "far apart, occupancy %d" % occ)
            got = sc.Cast(None, rays, 0.0, 100.0, 0, return_uv=True)
            assert all(got[k].tobytes() == want[k].tobytes() for k in range(3))
            print("occupancy %d: k = %d, %d bytes, %d blocks set" % (occ, sc.stats["occupancy_log2"], sc.stats["occupancy_bytes"], sc.stats["n_blocks_set"]))
    rec.close()


def test_a_failed_allocation_writes_nothing_and_destroy_frees_everything(smx):
    L = _lib_of().load()
    start = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    rays = np.ascontiguousarray(rr.ray_sets()["inside-out"][0][:200])
    wh, wt, wuv, wst = rr.answer(rr.brute(m[0], m[2], tri, rays, 0.0, 10.0), 0)
    P, n_in = rays.shape[0], tri.shape[0]
    build_failed, cast_failed = [], []
    try:
        # the build: every allocation in line, each on a fresh scene and a fresh object
        for nth in range(40):
            sc = C.c_void_p()
            assert L.smx_rayscene_create(C.c_int32(-1), C.byref(sc)) == 0
            smx.DebugFailAllocation(nth)
            rc = _build_raw(rec, sc, tri, n_in, 0.0, 4)[0]
            smx.DebugFailAllocation(-1)
            if rc == 0:
                break
            build_failed.append(rc)
            g = _guards(P, 0)
            assert rc == -2 and _cast_raw(sc, rays, P, *g, t_max=10.0)[0] == -1 and _untouched(g), nth      # a failed build: an empty scene
            assert _build_raw(rec, sc, tri, n_in, 0.0, 4)[0] == 0                                             # the next call succeeds
            assert _cast_raw(sc, rays, P, *g, t_max=10.0)[0] == 0 and g[0].tobytes() == wh.tobytes() and g[1].tobytes() == wt.tobytes()
            assert L.smx_rayscene_destroy(sc) == 0
            rec.close()
            rec = _rec_of(smx, m)
        assert rc == 0 and 10 <= len(build_failed) < 40, "the build reached %d allocations" % len(build_failed)
        # the cast: every allocation in line, each on a fresh scene
        for nth in range(20):
            g = _guards(P, 0)
            smx.DebugFailAllocation(nth)
            rc = _cast_raw(sc, rays, P, *g, t_max=10.0)[0]
            smx.DebugFailAllocation(-1)
            if rc == 0:
                break
            cast_failed.append(rc)
            assert rc == -2 and _untouched(g), nth
            g = _guards(P, 0)
            assert _cast_raw(sc, rays, P, *g, t_max=10.0)[0] == 0 and g[2].tobytes() == wuv.tobytes()       # the next call succeeds
            assert L.smx_rayscene_destroy(sc) == 0
            sc = C.c_void_p()
            assert L.smx_rayscene_create(C.c_int32(-1), C.byref(sc)) == 0 and _build_raw(rec, sc, tri, n_in, 0.0, 4)[0] == 0
        assert rc == 0 and 6 <= len(cast_failed) < 20, "the cast reached %d allocations" % len(cast_failed)
        assert g[0].tobytes() == wh.tobytes() and g[1].tobytes() == wt.tobytes() and g[2].tobytes() == wuv.tobytes()
    finally:
        smx.DebugFailAllocation(-1)
    assert L.smx_rayscene_destroy(sc) == 0
    # a scene's memory is counted, and all of it goes with the scene (the object's workspace has its size by now)
    before = smx.DebugLiveAllocations()
    sc = C.c_void_p()
    assert L.smx_rayscene_create(C.c_int32(-1), C.byref(sc)) == 0
    rc, bst = _build_raw(rec, sc, tri, n_in, 0.0, 4)
    g = _guards(P, 0)
    assert rc == 0 and _cast_raw(sc, rays, P, *g, t_max=10.0)[0] == 0
    held = smx.DebugLiveAllocations()
    assert held[0] > before[0] and held[1] - before[1] >= bst.device_bytes
    assert L.smx_rayscene_destroy(sc) == 0
    assert smx.DebugLiveAllocations() == before
    rec.close()
    assert smx.DebugLiveAllocations() == start


def test_the_python_helpers_with_a_scene_equal_their_own_results(world):
    from surfelmeshing_amd import meshing, render
    rec, tri = world["rec"], world["tri"]
    with meshing.build_ray_scene(rec, tri) as sc:
        slots, visible, stats = meshing.vertex_visibility(rec, tri, rr.SEGMENT_CAMERA)
        s2, v2, st2 = meshing.vertex_visibility(rec, tri, rr.SEGMENT_CAMERA, scene=sc)
        assert s2.tobytes() == slots.tobytes() and v2.tobytes() == visible.tobytes() and all(st2[k] == stats[k] for k in CAST)
        pose = render.look_at([0.0, 0.0, 0.95], [0.3, 0.1, 1.5])
        W, H, fx, fy, cx, cy = 32, 24, 20.0, 20.0, 16.0, 12.0
        img = render.raycast_mesh_view(rec, tri, W, H, fx, fy, cx, cy, pose)
        img2 = render.raycast_mesh_view(rec, tri, W, H, fx, fy, cx, cy, pose, scene=sc)
        assert sorted(img) == sorted(img2) and all(np.asarray(img[k]).tobytes() == np.asarray(img2[k]).tobytes() for k in img if k != "stats")
        rays, t0, t1 = rr.ray_sets()["pinhole"]
        a = meshing.cast_rays(rec, tri, rays[:, :3], rays[:, 3:], t0, t1, return_uv=True)
        b = meshing.cast_rays(rec, tri, rays[:, :3], rays[:, 3:], t0, t1, return_uv=True, scene=sc)
        assert all(a[k].tobytes() == b[k].tobytes() for k in range(3))


def test_run_tum_casts_the_rays_of_several_frames_against_one_scene(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "8",
                        "--outlier_filtering_frame_count", "2", "--mesh", "--mesh_eval_rays", "--mesh_eval_rays_frames", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    one = re.search(r"surface error along the rays of frame (\d+): (\d+) of (\d+) rays hit the mesh \(([0-9.]+) %\): mean ([0-9.]+) mm, rms ([0-9.]+) mm", r.stdout)
    assert one, r.stdout[-1500:]
    lines = re.findall(r"scene rays of frame (\d+): (\d+) of (\d+) rays hit the mesh \(([0-9.]+) %\): mean ([0-9.]+) mm, rms ([0-9.]+) mm", r.stdout)
    assert len(lines) == 3 and len({ln[0] for ln in lines}) == 3, r.stdout[-1500:]
    assert lines[-1] == one.groups(), (lines[-1], one.groups())
    total = re.search(r"scene rays of 3 frames: (\d+) of (\d+) rays hit the mesh", r.stdout)
    assert total and int(total.group(1)) == sum(int(ln[1]) for ln in lines) and int(total.group(2)) == sum(int(ln[2]) for ln in lines)
    print("\n".join(" ".join(ln) for ln in lines))
