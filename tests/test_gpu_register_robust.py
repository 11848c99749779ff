"""smx_distscene_register_robust, smx_recon_build_distscene_rim and smx_recon_register_mesh on the device, against the exact
model of tests/register_robust_ref.py.  Every iteration's 33 sums -- the 31 of the plain call and the two new counts -- are
compared for EQUALITY (as uint64 bits) with the model evaluated at the pose the device recorded for that iteration; the status
has to agree, the solve within rtol 1e-9 / atol 1e-14, the final pose within 4 U max(1, |want|): the plain call's tolerances.
Every case of register_robust_ref.cases() runs against both scene builds."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import mesh_ref as mr
import register_ref as rr
import register_robust_ref as rb
import rim_ref as rf
import track_ref as tr

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
U = 2.0 ** -24          # float32 unit roundoff
GUARD = 0xA5


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


@pytest.fixture(scope="module")
def scenes(smx):
    """(mesh name, bound) -> a scene with a rim: the world at both builds; ("plain", bound): the world without a rim."""
    pos, nrm, r2, tri, info = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    out = {}
    for bound, cell in rb.BUILDS:
        out["world", bound] = rec.BuildDistanceScene(None, tri, bound, cell, rim=True)
        out["plain", bound] = rec.BuildDistanceScene(None, tri, bound, cell)
    rec.close()            # (a scene is a snapshot: the map may go)
    yield out
    for sc in out.values():
        sc.close()


def _params(p):
    from surfelmeshing_amd import meshing
    return meshing.register_params(**p.fields())


def _robust(r):
    from surfelmeshing_amd import meshing
    return meshing.register_robust_params(**r.fields())


def _sums33(scene):
    recs, counts = scene.RegisterIterations(), scene.RegisterRobustCounts()
    assert counts.shape == (len(recs), 2) and counts.dtype == np.uint32
    for r, c in zip(recs, counts):
        r["sums"] = np.concatenate([r["sums"], c.astype(np.float64)])
    return recs, counts


def _check(scene, mesh, pts, nrm, T_init, p, robust, bound, what, own=None):
    res = scene.Register(None, pts, nrm, T_init, _params(p), robust=_robust(robust))
    recs, counts = _sums33(scene)
    if own is not None and len(recs) == len(own["records"]) and all(g["Tf"].tobytes() == w["Tf_own"].tobytes() for g, w in zip(recs, own["records"])):
        want = own
    else:
        want = rb.exact_call(mesh, pts, nrm, T_init, p, robust, bound, recorded=recs)
    assert res["iterations_run"] == len(recs) == want["iterations_run"], (what, res["iterations_run"], len(recs), want["iterations_run"])
    for k, (g, w) in enumerate(zip(recs, want["records"])):
        assert (g["level"], g["stride"]) == (w["level"], w["stride"]), (what, k)
        assert np.allclose(g["Tf"].reshape(3, 4), w["Tf_own"], rtol=0, atol=4 * U * max(1.0, float(np.abs(w["Tf_own"]).max()))), (what, k)
        differ = g["sums"].view(np.uint64) != w["sums"].view(np.uint64)
        assert not np.any(differ), (what, k, np.flatnonzero(differ), g["sums"][differ], w["sums"][differ])
        assert counts[k].tolist() == [int(w["sums"][rb.S_RIM]), int(w["sums"][rb.S_WEIGHT])], (what, k)
        assert g["status"] == w["status"], (what, k, g["status"], w["status"])
        assert np.allclose(g["x"], w["x_ref"], rtol=1e-9, atol=1e-14), (what, k, g["x"], w["x_ref"])
    assert res["status"] == want["status"], (what, res["status"], want["status"])
    T = want["scene_T_points"].astype(np.float64)
    assert np.allclose(res["scene_T_points"], T, rtol=0, atol=4 * U * max(1.0, float(np.abs(T).max()))), (what, res["scene_T_points"], T)
    assert (res["inliers"], res["points_used"]) == (want["inliers"], want["points_used"]), what
    assert np.isclose(res["rms_residual"], want["rms_residual"], rtol=1e-6), what
    return res, recs, want


@pytest.mark.parametrize("bound", [b for b, _ in rb.BUILDS])
@pytest.mark.parametrize("name", list(rb.cases()))
def test_every_new_case_equals_the_model_bit_for_bit(smx, scenes, name, bound):
    c = rb.cases()[name]
    res, recs, want = _check(scenes[c["mesh"], bound], rr.mesh_of(c), c["points"], c["normals"], c["T_init"], c["params"], c["robust"], bound,
                             (name, bound), own=rb.model_call(name, bound) if "524289" not in name else None)
    print("%s bound %g: status %d after %d iterations, %d inliers of %d used" % (name, bound, res["status"], len(recs), res["inliers"], res["points_used"]))
    if res["status"] >= tr.TOO_FEW_INLIERS:       # nothing solved: T_init itself
        assert res["scene_T_points"].tobytes() == np.asarray(c["T_init"], np.float32).tobytes()


@pytest.mark.parametrize("variant", ["rim rejected", "rim + Tukey 16 / 8 / 4 mm"])
def test_the_patch_fixtures_device_chain_is_the_models(smx, variant):
    """The behaviour fixture (a patch cut out of a larger surface, the default schedule): the device follows the model's chain,
    whose distance from the true pose tests/test_register_robust_model.py asserts on the CPU."""
    f = rb.patch()
    mesh = f["mesh"]
    rec = _rec_of(smx, (mesh.pos, mesh.nrm, mesh.r2))
    which, robust = rb.PATCH_VARIANTS[variant]
    for bound in (0.02, 0.05):
        own, dt, drot = rb.patch_call(variant, bound)
        with rec.BuildDistanceScene(None, mesh.tri, bound, rim=True) as scene:
            res, recs, want = _check(scene, mesh, f[which], None, rr.IDENTITY, rr.Params(), robust, bound, (variant, bound), own=own)
        got_dt, got_dr = tr.pose_difference(res["scene_T_points"].astype(np.float64), f["T_true"])
        print("%s at %g: %d iterations; the model ends %.3g m from the truth, the device's float32 pose %.3g m" % (variant, bound, len(recs), dt, got_dt))
        assert res["status"] == own["status"] and len(recs) == own["iterations_run"]
    rec.close()


def _bits(res):
    return b"".join(np.asarray(res[k]).tobytes() for k in sorted(res))


def _records_bits(scene):
    return b"".join(r["sums"].tobytes() + r["x"].tobytes() + r["Tf"].tobytes() + bytes([r["level"], r["status"]]) for r in scene.RegisterIterations())


def test_the_scene_with_a_rim_holds_the_models_bytes_and_counts_them(smx, scenes):
    pos, nrm, r2, tri, _ = dr.world()
    want, wst = rf.rim(pos, r2, tri)
    for bound, _ in rb.BUILDS:
        with_rim, plain = scenes["world", bound], scenes["plain", bound]
        assert with_rim.has_rim and with_rim.rim_stats == wst and not plain.has_rim and plain.rim_stats is None
        extra = with_rim.stats["device_bytes"] - plain.stats["device_bytes"]
        assert tri.shape[0] <= extra <= tri.shape[0] + tri.shape[0] // 8 + 1024, extra
        assert {k: v for k, v in with_rim.stats.items() if k != "device_bytes"} == {k: v for k, v in plain.stats.items() if k != "device_bytes"}
    assert want.shape[0] == tri.shape[0] and wst["n_rim_triangles"] > 0


def test_kernel_0_and_rim_off_are_the_plain_call_byte_for_byte(smx, scenes):
    from surfelmeshing_amd import meshing
    c = rr.cases()["three levels on the world"]
    prm = _params(c["params"])
    for scene in (scenes["world", 0.02], scenes["plain", 0.02]):
        plain = scene.Register(None, c["points"], c["normals"], c["T_init"], prm)
        plain_records = _records_bits(scene)
        assert np.all(scene.RegisterRobustCounts() == 0)
        none = scene.Register(None, c["points"], c["normals"], c["T_init"], prm, robust=meshing.register_robust_params())
        assert _bits(none) == _bits(plain) and _records_bits(scene) == plain_records and np.all(scene.RegisterRobustCounts() == 0)
        # scales without a kernel are not looked at
        off = scene.Register(None, c["points"], c["normals"], c["T_init"], prm, robust=meshing.register_robust_params(kernel=0, scale=0.001))
        assert _bits(off) == _bits(plain) and _records_bits(scene) == plain_records
        # a kernel with scale 0 on every level weights nothing: the robust kernel, the same sums
        zero = scene.Register(None, c["points"], c["normals"], c["T_init"], prm, robust=meshing.register_robust_params(kernel="tukey", scale=0.0))
        assert _bits(zero) == _bits(plain) and _records_bits(scene) == plain_records and np.all(scene.RegisterRobustCounts() == 0)


def _lib_result():
    from surfelmeshing_amd import _lib
    out = _lib.RegisterResult()
    C.memset(C.byref(out), GUARD, C.sizeof(out))
    return out


def _untouched(out):
    return bytes(out) == bytes([GUARD]) * C.sizeof(out)


def _raw(scene, pts, nrm, T, prm, rp, out, on_device=0, result_on_device=0):
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else C.byref(a) if isinstance(a, C.Structure) else a.ctypes.data_as(C.c_void_p)
    T = np.ascontiguousarray(T, np.float32)
    return _lib.load().smx_distscene_register_robust(scene._h, None, C.byref(prm), ptr(rp), ptr(pts), ptr(nrm), C.c_uint32(0 if pts is None else pts.shape[0]),
                                                     C.c_int32(on_device), ptr(T), ptr(out), C.c_int32(result_on_device))


def test_refusals_write_nothing(smx, scenes):
    from surfelmeshing_amd import _lib, meshing
    c = rb.cases()["base set, rim"]
    prm, out = _params(c["params"]), _lib_result()
    pts, T = c["points"], c["T_init"]
    with_rim, plain = scenes["world", 0.02], scenes["plain", 0.02]
    good = meshing.register_robust_params(kernel="huber", scale=0.002, reject_rim=True)
    assert _raw(plain, pts, None, T, prm, good, out) == -1 and _untouched(out) and b"rim" in _lib.load().smx_last_error()
    with pytest.raises(ValueError):
        plain.Register(None, pts, None, T, prm, robust=good)
    for kernel, scale, rim in ((3, 0.002, 0), (-1, 0.002, 0), (1, -0.001, 0), (2, 17.0, 0), (1, float("nan"), 0), (2, 1e-7, 0), (0, 0.0, 2), (0, 0.0, -1)):
        rp = _lib.RegisterRobustParams(kernel, (C.c_float * 3)(scale, scale, scale), rim)
        assert _raw(with_rim, pts, None, T, prm, rp, out) == -1 and _untouched(out), (kernel, scale, rim)
    assert _raw(with_rim, pts, None, T, prm, None, out) == -1 and _untouched(out)
    with smx.DistanceScene() as empty:
        assert _raw(empty, pts, None, T, prm, good, out) == -1 and _untouched(out)
    # a bad scale on a level that is not used is not looked at
    rp = _lib.RegisterRobustParams(1, (C.c_float * 3)(0.002, -1.0, float("nan")), 1)
    assert _raw(with_rim, pts, None, T, prm, rp, out) == 0 and not _untouched(out)
    # a rebuild without a rim takes the rim away
    pos, nrm, r2, tri, _ = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    sc = rec.BuildDistanceScene(None, tri, 0.02, rim=True)
    assert sc.has_rim and _raw(sc, pts, None, T, prm, good, _lib_result()) == 0
    rec.BuildDistanceScene(None, tri, 0.02, scene=sc)
    out = _lib_result()
    assert not sc.has_rim and _raw(sc, pts, None, T, prm, good, out) == -1 and _untouched(out)
    # a refused rim build leaves the scene empty
    bad = tri.copy()
    bad[5, 1] = pos.shape[0] + 2000
    with pytest.raises(smx.SmxError):
        rec.BuildDistanceScene(None, bad, 0.02, scene=sc, rim=True)
    assert sc.stats is None and _raw(sc, pts, None, T, prm, meshing.register_robust_params(), out) == -1 and _untouched(out)
    sc.close()
    rec.close()


def test_two_calls_device_arrays_a_plain_call_and_a_query_in_between(smx, scenes):
    from surfelmeshing_amd import _lib
    scene = scenes["world", 0.02]
    c = rb.cases()["three levels, rim + Huber, a scale per level"]
    prm, rp = _params(c["params"]), _robust(c["robust"])
    first = scene.Register(None, c["points"], c["normals"], c["T_init"], prm, robust=rp)
    recs, counts = _sums33(scene)
    assert first["iterations_run"] == 6 and np.sum(counts[:, 0]) > 0 and np.sum(counts[:, 1]) > 0
    plain = scene.Register(None, c["points"], c["normals"], c["T_init"], prm)
    assert _bits(plain) != _bits(first) and np.all(scene.RegisterRobustCounts() == 0)
    qpts = dr.point_sets()["around the hand-made triangles"]
    got = scene.Query(None, qpts, 0.02, True, return_closest=True)
    want = dr.answer(dr.model_of("around the hand-made triangles"), 0.02, True)
    assert all(got[k].tobytes() == want[k].tobytes() for k in range(3))
    again = scene.Register(None, c["points"], c["normals"], c["T_init"], prm, robust=rp)
    recs2, counts2 = _sums33(scene)
    assert _bits(again) == _bits(first) and counts2.tobytes() == counts.tobytes()
    assert all(a["sums"].tobytes() == b["sums"].tobytes() and a["x"].tobytes() == b["x"].tobytes() and a["Tf"].tobytes() == b["Tf"].tobytes()
               for a, b in zip(recs2, recs))
    # device points and normals, the result left on the device, back to back with a plain registration: nothing waits in between
    n = c["points"].shape[0]
    size = C.sizeof(_lib.RegisterResult)
    dp, dn, dout = smx.CUDABuffer(1, 3 * n, np.float32), smx.CUDABuffer(1, 3 * n, np.float32), smx.CUDABuffer(1, 2 * size + 16, np.uint8)
    dp.Upload(c["points"].reshape(1, -1))
    dn.Upload(c["normals"].reshape(1, -1))
    dout.Upload(np.full((1, 2 * size + 16), GUARD, np.uint8))
    ap, an, ao = (b.ToCUDA().address for b in (dp, dn, dout))
    L = _lib.load()
    T = np.ascontiguousarray(c["T_init"], np.float32)

    def enqueue(robust, result_at):
        tail = (C.c_void_p(ap), C.c_void_p(an), C.c_uint32(n), C.c_int32(1), T.ctypes.data_as(C.c_void_p), C.c_void_p(result_at), C.c_int32(1))
        if robust:
            return L.smx_distscene_register_robust(scene._h, None, C.byref(prm), C.byref(rp), *tail)
        return L.smx_distscene_register(scene._h, None, C.byref(prm), *tail)
    assert enqueue(True, ao) == 0 and enqueue(False, ao + size) == 0 and enqueue(True, ao) == 0
    back = dout.Download()[0]
    r0 = smx.register_result_dict(_lib.RegisterResult.from_buffer_copy(back[:size].tobytes()))
    r1 = smx.register_result_dict(_lib.RegisterResult.from_buffer_copy(back[size:2 * size].tobytes()))
    assert _bits(r0) == _bits(first) and _bits(r1) == _bits(plain) and np.all(back[2 * size:] == GUARD)
    assert scene.RegisterRobustCounts().tobytes() == counts.tobytes()
    assert dp.Download()[0].tobytes() == c["points"].tobytes()          # the input is left alone
    for b in (dp, dn, dout):
        b.close()


def test_the_rim_is_a_snapshot_too(smx):
    pos, nrm, r2, tri, _ = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    c = rb.cases()["base set, rim + Tukey"]
    prm, rp = _params(c["params"]), _robust(c["robust"])
    scene = rec.BuildDistanceScene(None, tri, 0.02, rim=True)
    first = scene.Register(None, c["points"], c["normals"], c["T_init"], prm, robust=rp)
    recs, counts = _sums33(scene)
    want = rb.model_call("base set, rim + Tukey", 0.02)
    assert recs[0]["sums"].view(np.uint64).tobytes() == want["records"][0]["sums"].view(np.uint64).tobytes() and counts[0, 0] > 0

    def same(when):
        assert _bits(scene.Register(None, c["points"], c["normals"], c["T_init"], prm, robust=rp)) == _bits(first), when
        assert scene.RegisterRobustCounts().tobytes() == counts.tobytes(), when
    moved_r2 = r2.copy()
    moved_r2[::3] = -1.0
    rec.debug_upload_surfels(mr.rows_of_map(pos + np.array([0.004, -0.003, 0.002]), nrm, moved_r2), int(np.sum(moved_r2 < 0)))
    same("after an upload that kills slots")
    rec.MeshRim(None, tri[:100])                       # (the object's own rim workspace is not the scene's)
    same("after another rim call on the object")
    rec.Compact(None)
    same("after Compact")
    rec.close()
    same("after the reconstruction is gone")
    scene.close()


def test_a_failed_allocation_writes_nothing_and_leaks_nothing(smx):
    from surfelmeshing_amd import meshing
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    pts = np.ascontiguousarray((m[0][:400] * 1.002).astype(np.float32))
    nrm = np.ascontiguousarray(m[1][:400].astype(np.float32))
    prm = meshing.register_params(levels=[(2, 2), (1, 2)])
    rp = meshing.register_robust_params(kernel="tukey", scale=0.004, reject_rim=True)
    T = rr.IDENTITY
    with rec.BuildDistanceScene(None, tri, 0.02, rim=True) as scene:
        want = scene.Register(None, pts, nrm, T, prm, robust=rp)
    assert want["iterations_run"] >= 1 and want["points_used"] == 400
    failed = []
    try:
        for nth in range(40):           # every allocation of a call, on a fresh scene each time
            scene = rec.BuildDistanceScene(None, tri, 0.02, rim=True)
            out = _lib_result()
            smx.DebugFailAllocation(nth)
            rc = _raw(scene, pts, nrm, T, prm, rp, out)
            smx.DebugFailAllocation(-1)
            if rc == 0:
                break
            failed.append(rc)
            assert rc == -2 and _untouched(out), nth
            assert _bits(scene.Register(None, pts, nrm, T, prm, robust=rp)) == _bits(want), nth     # the next call succeeds
            scene.close()
        # the plain call's allocations (14 and more) and the two counts per workgroup
        assert rc == 0 and 15 <= len(failed) < 40, "the call reached %d allocations" % len(failed)
        assert _bits(smx.register_result_dict(out)) == _bits(want)
        scene.close()
        # the build: a failure in either half leaves the scene empty, and the next build succeeds
        with smx.DistanceScene() as sc:
            n_failed = 0
            for nth in range(60):
                smx.DebugFailAllocation(nth)
                try:
                    rec.BuildDistanceScene(None, tri, 0.02, scene=sc, rim=True)
                    ok = True
                except smx.SmxError:
                    ok = False
                smx.DebugFailAllocation(-1)
                if ok:
                    break
                n_failed += 1
                assert sc.stats is None and not sc.has_rim and _raw(sc, pts, nrm, T, prm, rp, _lib_result()) == -1, nth
            assert ok and n_failed >= 1 and sc.has_rim
            assert _bits(sc.Register(None, pts, nrm, T, prm, robust=rp)) == _bits(want)
    finally:
        smx.DebugFailAllocation(-1)
    rec.close()
    assert smx.DebugLiveAllocations() == base


def test_register_mesh_is_sample_mesh_then_register_robust(smx):
    from surfelmeshing_amd import meshing
    base = smx.DebugLiveAllocations()
    cp, cn, cr, ct = rr.corner()
    target = _rec_of(smx, (cp, cn, cr))
    scene = target.BuildDistanceScene(None, ct, 0.02, rim=True)
    target.close()
    # the source: the corner moved by the inverse of the known pose, every other triangle of it (all three planes are seen)
    T_true = rr.pose(*rr.CORNER_TRUE).astype(np.float64)
    inv = tr.se3_inv(T_true)
    src = _rec_of(smx, ((cp @ inv[:, :3].T + inv[:, 3]), cn @ inv[:, :3].T, cr))
    tri = np.ascontiguousarray(ct[::2])
    prm = meshing.register_params()
    for rp in (None, meshing.register_robust_params(kernel="tukey", scale=0.01, reject_rim=True)):
        got = src.RegisterMesh(None, scene, tri, 3000, seed=7, params=prm, robust=rp)
        mesh_records = _records_bits(scene)
        points, _, normals, _ = src.SampleMesh(None, tri, 3000, 7, return_normals=True)
        want = scene.Register(None, points, normals, None, prm, robust=rp if rp is not None else meshing.register_robust_params())
        assert _bits(got) == _bits(want) and mesh_records == _records_bits(scene)
        dt, dr_ = tr.pose_difference(got["scene_T_points"].astype(np.float64), T_true)
        print("register_mesh %s: status %d, %.3g rad and %.3g m from the known pose" % ("robust" if rp else "plain", got["status"], dr_, dt))
        # (the samples lie on the triangles up to their float32 rounding and the schedule stops at updates below 1e-5: the sanity
        # bound of the plain call's helper test; the arithmetic is pinned by the equalities above)
        assert got["status"] in (tr.OK, tr.CONVERGED) and dr_ < 1e-4 and dt < 1e-4
    assert meshing.register_mesh(src, scene, tri, 3000, seed=7, params=prm)["status"] in (tr.OK, tr.CONVERGED)
    with pytest.raises(ValueError):
        src.RegisterMesh(None, scene, tri, -1)
    scene.close()
    src.close()
    assert smx.DebugLiveAllocations() == base


ROBUST_LINE = r"robustly registered frame (\d+): status (\d) after (\d+) iterations, .*; last iteration: (\d+) on the rim, (\d+) weighted or rejected"


def test_run_tum_prints_the_plain_and_the_robust_line_of_every_frame(tmp_path):
    import os
    import re
    import subprocess
    import sys
    from common import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "6", "--mesh", "--mesh_eval", "0.05",
                        "--mesh_eval_register", "--mesh_eval_register_reject_rim", "--outlier_filtering_frame_count", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = re.findall(r"^registered frame (\d+): status (\d)", r.stdout, re.M)
    robust = re.findall(ROBUST_LINE, r.stdout)
    print(r.stdout[-1500:])
    assert [int(p[0]) for p in plain] == [int(q[0]) for q in robust] == [1, 2, 3, 4]
    assert re.search(r"^registered 4 frames:", r.stdout, re.M) and re.search(r"^robustly registered 4 frames:", r.stdout, re.M)
    # the ground-truth points reach beyond the reconstructed surface: some matches of every frame lie on its rim; no kernel, no weights
    assert all(int(q[3]) > 0 and int(q[4]) == 0 for q in robust)
