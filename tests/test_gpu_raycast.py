"""smx_recon_raycast_mesh on the device.  The contract (include/smx.h) is made of integers and of float32 expressions that numpy
reproduces bit for bit, and its answer is the minimum over ALL triangles, so everything here is compared for EQUALITY with the
brute-force model of tests/raycast_ref.py: hit, t, uv and every statistic (the grid's three counts whenever the cell size is
given; cell_size_used never; the three work counters only between two calls)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import components_ref as cr
import decimate_ref as dr_dec
import distance_ref as dr
import fill_ref as fr
import mesh_ref as mr
import raycast_ref as rr
from common import ROOT

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


def _check(got, want, m, tri, cell_size, what):
    """got / want: (hit, t, uv, stats)."""
    gst, wst = dict(got[3]), dict(want[3])
    used = gst.pop("cell_size_used")
    for k in rr.WORK_NAMES:
        assert gst.pop(k) >= 0
    if cell_size > 0:
        assert used == float(rr.cell_used(cell_size)), what
        wst.update(rr.structure(m[0], m[2], tri, cell_size))
    else:
        assert used >= float(rr.MIN_CELL), what
        for k in GRID:
            gst.pop(k)
    assert gst == wst, (what, gst, wst)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32 and got[2].dtype == np.float32
    for k, name in enumerate(("hit", "t", "uv")):
        assert got[k].tobytes() == want[k].tobytes(), (what, name, int(np.sum(got[k].view(np.uint32) != want[k].view(np.uint32))))


@pytest.mark.parametrize("name", list(rr.ray_sets()))
def test_every_ray_set_equals_the_model(world, name):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    (rays, t0, t1), model = rr.ray_sets()[name], rr.model_of(name)
    for cull in (0, 1, 2):
        want = rr.answer(model, cull)
        for cs in rr.CELL_SIZES:
            got = rec.RaycastMesh(None, tri, rays, t0, t1, cs, cull, return_uv=True)
            _check(got, want, m, tri, cs, "%s cell %g cull %d" % (name, cs, cull))
        print("%s cull %d: %d of %d hit (%d front), bad %d, dropped %d / %d / %d" % (
            name, cull, want[3]["n_hit"], want[3]["n_rays"], want[3]["n_front_hits"], want[3]["n_bad_rays"], want[3]["n_not_live"],
            want[3]["n_repeated"], want[3]["n_out_of_range"]))
    t = rec.debug_raycast_timings()
    assert set(t) == {"mark", "index", "cast", "stats"} and all(np.isfinite(v) and v >= 0 for v in t.values())


def _raw(rec, tri, n_in, rays, n_rays, hit, t, uv, t_min=0.0, t_max=2.0 ** 20, cell_size=0.0, cull=0, on_device=0, stats=True):
    """The C call itself; arrays: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    prm, st = _lib.RaycastParams(t_min, t_max, cell_size, cull), _lib.RaycastStats()
    rc = _lib.load().smx_recon_raycast_mesh(rec._h, None, C.byref(prm), ptr(tri), C.c_uint32(n_in), ptr(rays), C.c_uint32(n_rays),
                                            ptr(hit), ptr(t), ptr(uv), C.c_int32(on_device), C.byref(st) if stats else None)
    return rc, st


def _guards(P, extra=4):
    return np.full(P + extra, GUARD, np.uint32), np.full(P + extra, GUARD, np.uint32), np.full(2 * P + extra, GUARD, np.uint32)


def test_calling_rules_on_host_and_device_arrays(smx, world):
    from surfelmeshing_amd import api
    rec, tri, m = world["rec"], world["tri"], world["m"]
    name = "around the hand-made triangles"
    rays, t0, t1 = rr.ray_sets()[name]
    P, n_in, n = rays.shape[0], tri.shape[0], m[0].shape[0]
    wh, wt, wuv, wst = rr.answer(rr.model_of(name), 1)
    # host arrays pre-filled with a guard word; room to spare stays untouched
    hit, t, uv = _guards(P)
    rc, st = _raw(rec, tri, n_in, rays, P, hit, t, uv, cull=1)
    assert rc == 0 and hit[:P].tobytes() == wh.tobytes() and t[:P].tobytes() == wt.tobytes() and uv[:2 * P].tobytes() == wuv.tobytes()
    assert np.all(hit[P:] == GUARD) and np.all(t[P:] == GUARD) and np.all(uv[2 * P:] == GUARD)
    gst = api.raycast_stats_dict(st)
    assert {k: gst[k] for k in wst} == wst
    # uv = NULL and stats = NULL leave the other outputs as they are
    h2, t2, _ = _guards(P)
    rc, _ = _raw(rec, tri, n_in, rays, P, h2, t2, None, cull=1, stats=False)
    assert rc == 0 and h2.tobytes() == hit.tobytes() and t2.tobytes() == t.tobytes()
    # an index >= n, anywhere: refused, nothing written
    for where in (0, 3 * (n_in // 2) + 1, 3 * n_in - 1):
        bad = tri.copy()
        bad.reshape(-1)[where] = n
        g = _guards(P)
        assert _raw(rec, bad, n_in, rays, P, *g)[0] == -1 and all(np.all(a == GUARD) for a in g)
    # an output over an input: refused, nothing written
    both = np.concatenate([rays.reshape(-1).view(np.uint32), np.full(8, GUARD, np.uint32)])
    snapshot = both.copy()
    g = _guards(P)
    assert _raw(rec, tri, n_in, both, P, g[0], g[1], both[6 * P - 1:])[0] == -1 and both.tobytes() == snapshot.tobytes()
    # n_in == 0: every ray is "none"; n_rays == 0: only the triangles' statistics
    g = _guards(P)
    rc, st = _raw(rec, None, 0, rays, P, *g)
    assert rc == 0 and np.all(g[0][:P] == rr.INVALID) and np.all(np.isinf(g[1][:P].view(np.float32))) and np.all(np.isnan(g[2][:2 * P].view(np.float32)))
    assert st.n_hit == 0 and st.n_in == 0 and st.n_rays == P and st.n_bad_rays == wst["n_bad_rays"] and np.all(g[0][P:] == GUARD)
    rc, st = _raw(rec, tri, n_in, None, 0, None, None, None, cell_size=0.05)
    assert rc == 0 and st.n_rays == 0 and st.n_not_live == wst["n_not_live"] and st.n_repeated == 1 and st.n_out_of_range == 1
    assert {k: int(getattr(st, k)) for k in GRID} == rr.structure(m[0], m[2], tri, 0.05)
    # device arrays give the same bytes
    din, dry = smx.CUDABuffer(1, 3 * n_in, np.uint32), smx.CUDABuffer(1, 6 * P, np.uint32)
    sizes = (P + 4, P + 4, 2 * P + 4)
    outs = [smx.CUDABuffer(1, k, np.uint32) for k in sizes]
    din.Upload(tri.reshape(1, -1))
    dry.Upload(rays.reshape(1, -1).view(np.uint32))
    for b, k in zip(outs, sizes):
        b.Upload(np.full((1, k), GUARD, np.uint32))
    a = [b.ToCUDA().address for b in [din, dry] + outs]
    rc, st = _raw(rec, a[0], n_in, a[1], P, a[2], a[3], a[4], cull=1, on_device=1)
    back = [b.Download()[0] for b in outs]
    assert rc == 0 and back[0].tobytes() == hit.tobytes() and back[1].tobytes() == t.tobytes() and back[2].tobytes() == uv.tobytes()
    assert din.Download()[0].tobytes() == tri.tobytes() and dry.Download()[0].tobytes() == rays.tobytes()
    bad = tri.copy()
    bad[n_in // 3, 2] = n
    din.Upload(bad.reshape(1, -1))
    outs[0].Upload(np.full((1, P + 4), GUARD, np.uint32))
    assert _raw(rec, a[0], n_in, a[1], P, a[2], a[3], a[4], on_device=1)[0] == -1 and np.all(outs[0].Download()[0] == GUARD)
    assert _raw(rec, a[0], n_in, a[1], P, a[1] + 8, a[3], a[4], on_device=1)[0] == -1          # overlap on the device
    for b in [din, dry] + outs:
        b.close()
    # device tensors through the Python call
    import torch
    tt, tr = torch.from_numpy(tri.astype(np.int32)).cuda(), torch.from_numpy(rays.copy()).cuda()
    th, tq, tuv, tst = rec.RaycastMesh(None, tt, tr, t0, t1, cull=1, return_uv=True)
    torch.cuda.synchronize()
    assert th.cpu().numpy().view(np.uint32).tobytes() == wh.tobytes() and tq.cpu().numpy().tobytes() == wt.tobytes()
    assert tuv.cpu().numpy().tobytes() == wuv.tobytes() and tst["n_hit"] == wst["n_hit"]


def test_on_the_outputs_of_the_mesh_services(world):
    """One case each: Triangulate's, DecimateMesh's, MeshComponents' and FillHoles' array of the same map."""
    rec, m = world["rec"], world["m"]
    pos, nrm, r2 = m
    rays = np.concatenate([rr.ray_sets()["inside-out"][0][:200], rr.ray_sets()["pinhole"][0][200:400]])
    meshed, _ = rec.Triangulate(None)
    clean, _ = rec.MeshComponents(None, meshed, min_triangles=3)
    filled, _ = rec.FillHoles(None, clean)
    coarse, _ = rec.DecimateMesh(None, meshed, 0.1)
    assert clean.tobytes() == cr.components(pos, r2, meshed, min_triangles=3)[0].tobytes()
    assert filled.tobytes() == fr.fill(pos, nrm, r2, clean)[0].tobytes() and coarse.tobytes() == dr_dec.decimate(pos, r2, meshed, 0.1)[0].tobytes()
    for what, arr in (("triangulated", meshed), ("cleaned", clean), ("filled", filled), ("decimated", coarse)):
        want = rr.answer(rr.brute(pos, r2, arr, rays, 0.0, 100.0), 0)
        got = rec.RaycastMesh(None, arr, rays, 0.0, 100.0, 0.0, 0, return_uv=True)
        _check(got, want, m, arr, 0.0, what)
        print("%s: %d triangles, %d of %d rays hit" % (what, arr.shape[0], want[3]["n_hit"], rays.shape[0]))
        assert want[3]["n_hit"] > 100


def test_two_calls_give_the_same_bytes_and_a_smaller_call_reuses_the_workspace(smx, world):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    rays, t0, t1 = rr.ray_sets()["pinhole"]
    first = rec.RaycastMesh(None, tri, rays, t0, t1, 0.0, 0, return_uv=True)
    live = smx.DebugLiveAllocations()
    again = rec.RaycastMesh(None, tri, rays, t0, t1, 0.0, 0, return_uv=True)
    assert first[3] == again[3] and all(first[k].tobytes() == again[k].tobytes() for k in range(3))      # (the work counters included)
    assert first[3]["n_layers"] > 0 and first[3]["n_lookups"] > 0 and first[3]["n_pair_tests"] > 0
    small = rec.RaycastMesh(None, tri[:2000], rays[:100], t0, t1, 0.0, 0, return_uv=True)
    assert smx.DebugLiveAllocations() == live
    _check(small, rr.answer(rr.brute(m[0], m[2], tri[:2000], rays[:100], t0, t1), 0), m, tri[:2000], 0.0, "smaller")


def test_a_failed_allocation_writes_nothing_and_close_frees_everything(smx):
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    rays = np.ascontiguousarray(rr.ray_sets()["inside-out"][0][:200])
    wh, wt, wuv, wst = rr.answer(rr.brute(m[0], m[2], tri, rays, 0.0, 10.0), 0)
    P, n_in = rays.shape[0], tri.shape[0]
    failed = []
    try:
        for nth in range(40):
            g = _guards(P, 0)
            smx.DebugFailAllocation(nth)
            rc = _raw(rec, tri, n_in, rays, P, *g, t_max=10.0)[0]
            if rc == 0:
                break
            failed.append(rc)
            assert rc == -2 and all(np.all(a == GUARD) for a in g), nth        # the allocation error, nothing written
            smx.DebugFailAllocation(-1)
            got = rec.RaycastMesh(None, tri, rays, 0.0, 10.0, return_uv=True)     # the next call succeeds
            assert got[0].tobytes() == wh.tobytes() and got[1].tobytes() == wt.tobytes() and got[2].tobytes() == wuv.tobytes()
            rec.close()                       # a fresh object for the next allocation in line
            rec = _rec_of(smx, m)
    finally:
        smx.DebugFailAllocation(-1)
    # from the first allocation of the call (the counters) to its last (the cell table)
    assert rc == 0 and 15 <= len(failed) < 40, "the call reached %d allocations" % len(failed)
    assert g[0].tobytes() == wh.tobytes() and g[1].tobytes() == wt.tobytes() and g[2].tobytes() == wuv.tobytes()
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
    rays = rr.ray_sets()["inside-out"][0][:500]
    out = rec.RaycastMesh(None, tri, rays, 0.0, 10.0)
    assert out[2]["n_hit"] > 300
    assert rec.stats() == stats_before and rec.surfels_size() == n and rec.surfel_count() == n
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()
    assert rec.TransferChangedToCPU(None, 2).count == 0
    mesh_again, st2, us2 = rec.TriangulateUpdate(None, index=nn)
    assert us2["mode"] == 0 and us2["n_changed"] == 0 and mesh_again.tobytes() == tri.tobytes() and st2 == st
    full2, full_st2 = rec.Triangulate(None)
    assert full2.tobytes() == full.tobytes() and full_st2 == full_st
    nn.close()
    rec.close()


def test_a_view_from_inside_the_sphere_equals_the_model(world):
    """raycast_mesh_view from a camera inside the sphere, 5 cm from its surface: the camera plane cuts triangles, which the
    rasteriser loses."""
    from surfelmeshing_amd import meshing, render
    rec, tri, m = world["rec"], world["tri"], world["m"]
    pose = render.look_at([0.0, 0.0, 0.95], [0.3, 0.1, 1.5])
    W, H, fx, fy, cx, cy = 32, 24, 20.0, 20.0, 16.0, 12.0
    img = render.raycast_mesh_view(rec, tri, W, H, fx, fy, cx, cy, pose)
    o, d = meshing.camera_rays(fx, fy, cx, cy, W, H, pose)
    wh, wt, _, wst = rr.answer(rr.brute(m[0], m[2], tri, np.concatenate([o, d], axis=1), 0.0, 2.0 ** 20), 0)
    assert img["depth"].shape == (H, W) and img["depth"].dtype == np.float32 and img["index"].shape == (H, W) and img["index"].dtype == np.uint32
    assert img["index"].tobytes() == wh.tobytes() and img["depth"].tobytes() == np.where(wh != rr.INVALID, wt, np.float32(0)).astype(np.float32).tobytes()
    print("%d of %d pixels hit, nearest %.4f" % (wst["n_hit"], W * H, float(wt.min())))
    assert wst["n_hit"] > W * H // 2 and float(wt.min()) < 0.1


def test_vertex_visibility_equals_the_segments_set(world):
    from surfelmeshing_amd import meshing
    rec, tri = world["rec"], world["tri"]
    slots, visible, stats = meshing.vertex_visibility(rec, tri, rr.SEGMENT_CAMERA)
    used = np.unique(tri)
    assert slots.tobytes() == used.tobytes() and visible.dtype == bool and visible.shape == used.shape and stats["n_rays"] == used.size
    want = rr.answer(rr.model_of("segments"), 0)[0] == rr.INVALID
    got = visible[np.searchsorted(used, rr.segment_slots())]
    assert np.array_equal(got, want)
    print("%d of %d used vertices visible; of the segments set %d of %d" % (int(visible.sum()), used.size, int(want.sum()), want.size))
    assert 0 < int(want.sum()) < want.size


def test_run_tum_prints_the_ray_evaluation(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "8",
                        "--outlier_filtering_frame_count", "2", "--mesh", "--mesh_eval_rays"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"surface error along the rays of frame (\d+): (\d+) of (\d+) rays hit the mesh \(([0-9.]+) %\): mean ([0-9.]+) mm, rms ([0-9.]+) mm", r.stdout)
    assert m, r.stdout[-1500:]
    print(m.group(0))
    assert int(m.group(2)) > 0 and int(m.group(3)) > 0
