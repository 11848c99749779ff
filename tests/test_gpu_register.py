"""smx_distscene_register on the device, against the exact model of tests/register_ref.py.  Every iteration's 31 sums are
compared for EQUALITY (as uint64 bits) with the model evaluated at the pose the device recorded for that iteration; the status
has to agree, the solve within rtol 1e-9 / atol 1e-14, the final pose within 4 U max(1, |want|): the tracking tests' tolerances.
Every case of register_ref.cases() runs against both scene builds of register_ref.BUILDS."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distance_ref as dr
import mesh_ref as mr
import register_ref as rr
import track_ref as tr
from common import ROOT

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
U = 2.0 ** -24          # float32 unit roundoff


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


@pytest.fixture(scope="module")
def scenes(smx):
    """(mesh name, bound) -> a scene: the world, its hand-made triangles alone, and corner(), each at both builds."""
    pos, nrm, r2, tri, info = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    cp, cn, cr, ct = rr.corner()
    crec = _rec_of(smx, (cp, cn, cr))
    out = {}
    for bound, cell in rr.BUILDS:
        out["world", bound] = rec.BuildDistanceScene(None, tri, bound, cell)
        out["hand", bound] = rec.BuildDistanceScene(None, tri[info["hand_tri"]:], bound, cell)
        out["corner", bound] = crec.BuildDistanceScene(None, ct, bound, cell)
    rec.close()            # (a scene is a snapshot: the maps may go)
    crec.close()
    yield out
    for sc in out.values():
        sc.close()


def _params(smx, p):
    from surfelmeshing_amd import meshing
    return meshing.register_params(**p.fields())


def _check(smx, scene, mesh, pts, nrm, T_init, p, bound, what, own=None):
    """One call against the model at the recorded poses; returns (result, records, model).  own: the restatement's own chain,
    if the caller has it: where every recorded pose is that chain's to the bit, its sums are the model's at the recorded poses."""
    res = scene.Register(None, pts, nrm, T_init, _params(smx, p))
    recs = scene.RegisterIterations()
    if own is not None and len(recs) == len(own["records"]) and all(g["Tf"].tobytes() == w["Tf_own"].tobytes() for g, w in zip(recs, own["records"])):
        want = own
    else:
        want = rr.exact_call(mesh, pts, nrm, T_init, p, bound, recorded=recs)
    assert res["iterations_run"] == len(recs) == want["iterations_run"], (what, res["iterations_run"], len(recs), want["iterations_run"])
    for k, (g, w) in enumerate(zip(recs, want["records"])):
        assert (g["level"], g["stride"]) == (w["level"], w["stride"]), (what, k)
        # the pose the device handed this iteration is the chain's own, to the float
        assert np.allclose(g["Tf"].reshape(3, 4), w["Tf_own"], rtol=0, atol=4 * U * max(1.0, float(np.abs(w["Tf_own"]).max()))), (what, k)
        differ = g["sums"].view(np.uint64) != w["sums"].view(np.uint64)
        assert not np.any(differ), (what, k, np.flatnonzero(differ), g["sums"][differ], w["sums"][differ])
        assert g["status"] == w["status"], (what, k, g["status"], w["status"])
        assert np.allclose(g["x"], w["x_ref"], rtol=1e-9, atol=1e-14), (what, k, g["x"], w["x_ref"])
    assert res["status"] == want["status"], (what, res["status"], want["status"])
    T = want["scene_T_points"].astype(np.float64)
    assert np.allclose(res["scene_T_points"], T, rtol=0, atol=4 * U * max(1.0, float(np.abs(T).max()))), (what, res["scene_T_points"], T)
    assert (res["inliers"], res["points_used"]) == (want["inliers"], want["points_used"]), what
    assert np.isclose(res["rms_residual"], want["rms_residual"], rtol=1e-6) and res["information"].tobytes() == want["information"].tobytes(), what
    assert np.isclose(res["last_update_rotation"], want["last_update_rotation"], rtol=1e-5, atol=1e-12), what
    assert np.isclose(res["last_update_translation"], want["last_update_translation"], rtol=1e-5, atol=1e-12), what
    return res, recs, want


@pytest.mark.parametrize("bound", [b for b, _ in rr.BUILDS])
@pytest.mark.parametrize("name", list(rr.cases()))
def test_every_case_equals_the_model_bit_for_bit(smx, scenes, name, bound):
    c = rr.cases()[name]
    res, recs, want = _check(smx, scenes[c["mesh"], bound], rr.mesh_of(c), c["points"], c["normals"], c["T_init"], c["params"], bound, (name, bound))
    print("%s bound %g: status %d after %d iterations, %d inliers of %d used" % (name, bound, res["status"], len(recs), res["inliers"], res["points_used"]))
    if res["status"] >= tr.TOO_FEW_INLIERS:       # nothing solved: T_init itself
        assert res["scene_T_points"].tobytes() == np.asarray(c["T_init"], np.float32).tobytes()


# The model's own distance from the true pose after the default schedule, measured on the CPU (the restatement's own chain in
# double, no device in it; five iterations, every level CONVERGED): 1.6e-10 rad and 3.1e-10 m -- the samples lie on the
# triangles exactly, so what is left is their rounding to float32.  Asserted with a 4x margin -- on the CPU
# model against the truth, never on the device against itself; the device is held to the model by the tolerances above.
CORNER_MODEL_ROTATION, CORNER_MODEL_TRANSLATION = 1.6e-10, 3.1e-10


def test_corner_is_registered_to_the_known_pose(smx, scenes):
    pts, nrm, T_true = rr.corner_points()
    p = rr.Params()
    mesh = rr.corner_mesh()
    own = rr.exact_call(mesh, pts, nrm, rr.IDENTITY, p, 0.02)
    assert np.all(own["records"][0]["detail"]["where"] >= rr.COLLINEAR), "every sample is matched in the first iteration"
    dt, dr_ = tr.pose_difference(own["T"], T_true.astype(np.float64))
    print("the model against the truth: %.3g rad, %.3g m after %d iterations, status %d" % (dr_, dt, own["iterations_run"], own["status"]))
    assert own["status"] in (tr.OK, tr.CONVERGED)
    assert dr_ <= 4 * CORNER_MODEL_ROTATION and dt <= 4 * CORNER_MODEL_TRANSLATION, (dr_, dt)
    res, recs, want = _check(smx, scenes["corner", 0.02], mesh, pts, nrm, rr.IDENTITY, p, 0.02, "corner", own)
    assert res["status"] == own["status"] and len(recs) == own["iterations_run"]
    T = own["scene_T_points"].astype(np.float64)
    assert np.allclose(res["scene_T_points"], T, rtol=0, atol=4 * U * max(1.0, float(np.abs(T).max())))
    # the helper, without normals and from a device tensor: the same machinery, a pose as good
    import torch
    from surfelmeshing_amd import meshing
    out = meshing.register_points(scenes["corner", 0.02], torch.from_numpy(pts.copy()).cuda())
    dt2, dr2 = tr.pose_difference(out["scene_T_points"].astype(np.float64), T_true.astype(np.float64))
    assert out["status"] in (tr.OK, tr.CONVERGED) and dr2 < 1e-4 and dt2 < 1e-4, (dr2, dt2)


def _bits(res):
    return b"".join(np.asarray(res[k]).tobytes() for k in sorted(res))


def test_the_status_paths_return_T_init_bit_for_bit(smx, scenes):
    from surfelmeshing_amd import meshing
    world, corner = scenes["world", 0.02], scenes["corner", 0.02]
    T = rr.pose(np.deg2rad(0.2) * np.array([0.0, 0.0, 1.0]), [0.001, -0.0, 0.0])
    T[1, 3] = -0.0                                   # (bit for bit: the sign of a zero too)
    cp = rr.corner()[0]
    # a single plane: points over the hand-made triangles that lie in z = 0 (one grid of the corner would not do: its jitter
    # makes it no plane, and the solve holds it in place)
    flat = rr.shell_set()[0]
    res = world.Register(None, flat, None, T, meshing.register_params(levels=[(1, 3)], min_inliers=1))
    assert res["status"] == tr.DEGENERATE and res["iterations_run"] == 1 and res["inliers"] > 30, res
    assert res["scene_T_points"].tobytes() == T.tobytes()
    plane = np.ascontiguousarray(cp[:rr.CORNER_N ** 2] + np.array([0.0, 0.0, 0.002]), np.float32)
    # points a metre away: none matched
    res = corner.Register(None, plane + np.float32([0.0, 0.0, 1.0]), None, T, meshing.register_params(levels=[(1, 3)]))
    assert res["status"] == tr.DEGENERATE and res["iterations_run"] == 1 and (res["inliers"], res["points_used"]) == (0, plane.shape[0]), res
    assert res["scene_T_points"].tobytes() == T.tobytes()
    rec = corner.RegisterIterations()
    assert len(rec) == 1 and rec[0]["sums"][29] == plane.shape[0] and rec[0]["sums"][30] == 0 and np.all(rec[0]["x"] == 0)
    # min_inliers above the sample count
    pts = rr.corner_points()[0]
    res = corner.Register(None, pts, None, T, meshing.register_params(min_inliers=pts.shape[0] + 1))
    assert res["status"] == tr.TOO_FEW_INLIERS and res["iterations_run"] == 1 and res["scene_T_points"].tobytes() == T.tobytes(), res
    # no points at all
    res = world.Register(None, np.zeros((0, 3), np.float32), None, T)
    assert res["status"] == tr.TOO_FEW_INLIERS and res["points_used"] == 0 and res["scene_T_points"].tobytes() == T.tobytes()
    assert world.Register(None, np.zeros((0, 3), np.float32), None, T, meshing.register_params(min_inliers=0))["status"] == tr.DEGENERATE
    # a T_init that is not finite, a gate above the bound, an empty scene: refused, nothing written
    bad = T.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        corner.Register(None, pts, None, bad)
    out, prm = _lib_result(), meshing.register_params()
    assert _raw(corner, pts, None, bad, prm, out) == -1 and _untouched(out)
    assert _raw(corner, pts, None, T, meshing.register_params(levels=[(1, 2, 0.05)]), out) == -1 and _untouched(out)
    assert _raw(corner, None, None, T, prm, out, n=5) == -1 and _untouched(out)
    with smx.DistanceScene() as empty:
        assert _raw(empty, pts, None, T, prm, out) == -1 and _untouched(out)
    assert _raw(corner, pts, None, T, prm, out) == 0 and not _untouched(out)


GUARD = 0xA5


def _lib_result():
    from surfelmeshing_amd import _lib
    out = _lib.RegisterResult()
    C.memset(C.byref(out), GUARD, C.sizeof(out))
    return out


def _untouched(out):
    return bytes(out) == bytes([GUARD]) * C.sizeof(out)


def _raw(scene, pts, nrm, T, prm, out, n=None, on_device=0, result_on_device=0):
    """The C call itself; pts / nrm / out: numpy arrays, device addresses (int), ctypes structs or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else C.byref(a) if isinstance(a, C.Structure) else a.ctypes.data_as(C.c_void_p)
    T = np.ascontiguousarray(T, np.float32)
    count = n if n is not None else (0 if pts is None else pts.shape[0])
    return _lib.load().smx_distscene_register(scene._h, None, C.byref(prm), ptr(pts), ptr(nrm), C.c_uint32(count), C.c_int32(on_device), ptr(T), ptr(out),
                                              C.c_int32(result_on_device))


def test_two_calls_device_arrays_and_a_query_in_between_give_the_same_bytes(smx, scenes):
    import torch
    from surfelmeshing_amd import _lib
    scene = scenes["world", 0.02]
    c = rr.cases()["three levels on the world"]
    prm = _params(smx, c["params"])
    first = scene.Register(None, c["points"], c["normals"], c["T_init"], prm)
    recs = scene.RegisterIterations()
    assert first["iterations_run"] == 6 and first["status"] == tr.OK
    qpts = dr.point_sets()["around the hand-made triangles"]
    before = scene.Query(None, qpts, 0.02, True, return_closest=True)
    again = scene.Register(None, c["points"], c["normals"], c["T_init"], prm)
    assert _bits(again) == _bits(first)
    assert all(a["sums"].tobytes() == b["sums"].tobytes() and a["x"].tobytes() == b["x"].tobytes() and a["Tf"].tobytes() == b["Tf"].tobytes()
               for a, b in zip(scene.RegisterIterations(), recs))
    after = scene.Query(None, qpts, 0.02, True, return_closest=True)
    assert all(before[k].tobytes() == after[k].tobytes() for k in range(3)) and before[3] == after[3]
    want = dr.answer(dr.model_of("around the hand-made triangles"), 0.02, True)
    assert all(after[k].tobytes() == want[k].tobytes() for k in range(3))
    # device points and normals, the result left on the device: nothing waits; the same bytes
    tp, tn = torch.from_numpy(c["points"].copy()).cuda(), torch.from_numpy(c["normals"].copy()).cuda()
    out = torch.full((C.sizeof(_lib.RegisterResult) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    assert scene.Register(None, tp, tn, c["T_init"], prm, result_buffer=out.data_ptr()) is None
    assert scene.Register(None, tp, tn, c["T_init"], prm, result_buffer=out.data_ptr()) is None      # (back to back, the first still running)
    torch.cuda.synchronize()
    back = out.cpu().numpy()
    got = _lib.RegisterResult.from_buffer_copy(back[:C.sizeof(_lib.RegisterResult)].tobytes())
    assert _bits(smx.register_result_dict(got)) == _bits(first) and np.all(back[C.sizeof(_lib.RegisterResult):] == GUARD)
    assert tp.cpu().numpy().tobytes() == c["points"].tobytes() and tn.cpu().numpy().tobytes() == c["normals"].tobytes()
    assert _bits(scene.Register(None, tp, tn, c["T_init"], prm)) == _bits(first)
    t = scene.debug_register_timings()
    assert set(t) == {"call", "move", "query", "reduce", "solve"} and all(np.isfinite(v) and v >= 0 for v in t.values()) and t["call"] > 0 and t["query"] > 0
    assert t["call"] >= t["move"] + t["query"] + t["reduce"] + t["solve"]


def test_a_scene_is_a_snapshot_for_registration_too(smx):
    pos, nrm, r2, tri, _ = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    c = rr.cases()["three levels on the world"]
    prm = _params(smx, c["params"])
    scene = rec.BuildDistanceScene(None, tri, 0.02)
    first = scene.Register(None, c["points"], c["normals"], c["T_init"], prm)
    recs = scene.RegisterIterations()
    want = rr.model_call("three levels on the world", 0.02)
    assert first["status"] == want["status"] and len(recs) == want["iterations_run"]
    assert recs[0]["sums"].view(np.uint64).tobytes() == want["records"][0]["sums"].view(np.uint64).tobytes()
    moved_r2 = r2.copy()
    moved_r2[::3] = -1.0
    rec.debug_upload_surfels(mr.rows_of_map(pos + np.array([0.004, -0.003, 0.002]), nrm, moved_r2), int(np.sum(moved_r2 < 0)))
    assert _bits(scene.Register(None, c["points"], c["normals"], c["T_init"], prm)) == _bits(first), "after the upload"
    rec.Compact(None)
    assert _bits(scene.Register(None, c["points"], c["normals"], c["T_init"], prm)) == _bits(first), "after Compact"
    rec.close()
    assert _bits(scene.Register(None, c["points"], c["normals"], c["T_init"], prm)) == _bits(first), "after the reconstruction is gone"
    assert all(a["sums"].tobytes() == b["sums"].tobytes() for a, b in zip(scene.RegisterIterations(), recs))
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
    T = rr.IDENTITY
    with rec.BuildDistanceScene(None, tri, 0.02) as scene:
        want = scene.Register(None, pts, nrm, T, prm)
    assert want["iterations_run"] >= 1 and want["points_used"] == 400
    failed = []
    try:
        for nth in range(40):           # every allocation of a call, on a fresh scene each time
            scene = rec.BuildDistanceScene(None, tri, 0.02)
            live = smx.DebugLiveAllocations()
            out = _lib_result()
            smx.DebugFailAllocation(nth)
            rc = _raw(scene, pts, nrm, T, prm, out)
            smx.DebugFailAllocation(-1)
            if rc == 0:
                break
            failed.append(rc)
            assert rc == -2 and _untouched(out), nth
            assert smx.DebugLiveAllocations()[0] <= live[0] + nth, nth            # (what it got before the failure it keeps for the next call)
            assert _bits(scene.Register(None, pts, nrm, T, prm)) == _bits(want), nth     # the next call succeeds
            scene.close()
        # slabs and state, the query's counters, keys, two sort pairs and its workspace, four outputs of the query, two stagings
        assert rc == 0 and 14 <= len(failed) < 40, "the call reached %d allocations" % len(failed)
        assert _bits(smx.register_result_dict(out)) == _bits(want)
    finally:
        smx.DebugFailAllocation(-1)
    scene.close()
    rec.close()
    assert smx.DebugLiveAllocations() == base


LINE = r"registered frame (\d+): status (\d) after (\d+) iterations, ([0-9.]+) mrad and ([0-9.]+) mm from the identity; surface error ([0-9.]+) -> ([0-9.]+) mm mean, ([0-9.]+) -> ([0-9.]+) mm rms"


TOTAL = r"registered (\d+) frames: (\d+) solved, mean ([0-9.]+) mrad and ([0-9.]+) mm from the identity; surface error ([0-9.]+) -> ([0-9.]+) mm mean"


def _run_tum(tmp_path, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "6",
                        "--mesh", "--mesh_eval", "0.05", "--mesh_eval_register"] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines, total = re.findall(LINE, r.stdout), re.search(TOTAL, r.stdout)
    frames = re.search(r"ground truth of (\d+) frames to the mesh", r.stdout)
    assert total and frames, r.stdout[-2000:]
    assert int(total.group(1)) == len(lines) == int(frames.group(1)) and int(total.group(2)) == sum(int(ln[1]) <= 1 for ln in lines)
    return lines


def test_run_tum_registers_the_ground_truth_points_of_every_evaluated_frame(tmp_path):
    """One line per evaluated frame and a total.  With the tool's default outlier filter (a window of frames on either side) a
    recording of six frames leaves none to integrate: the flags alone print the total of no frames; with a window of two, frames
    1 .. 4 are integrated, evaluated and registered."""
    assert _run_tum(tmp_path, []) == []
    lines = _run_tum(tmp_path, ["--outlier_filtering_frame_count", "2"])
    assert [int(ln[0]) for ln in lines] == [1, 2, 3, 4], lines
    print("\n".join(" ".join(ln) for ln in lines))
    # true poses and a map of the same frames: what is left to recover is small, and the alignment, which minimises the squared
    # point-to-plane residuals, does not make the rms surface error worse by more than the change of the matched set can (a
    # quarter and 0.05 mm are allowed: a sanity check of the tool, the arithmetic is pinned above)
    for ln in lines:
        if int(ln[1]) <= 1:
            assert float(ln[3]) < 20.0 and float(ln[4]) < 20.0 and float(ln[8]) <= float(ln[7]) * 1.25 + 0.05, ln
