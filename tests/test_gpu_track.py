"""Camera tracking (smx_recon_track) on the GPU against the float64 restatement of tests/track_ref.py, on maps grown
from small_stream (2 degrees of yaw per frame) as in tests/test_gpu_render.py.

Bounds: the per-iteration sums are held to a bound derived in this file from the float32 operation count; whole calls
to 4 x the float32-vs-float64 difference of the restatement itself (measured on the CPU by tests/test_track_api.py) plus
the flagged-pixel term, capped at 5 % of the restatement's own distance to the ground truth; the 16-frame chain to 1.5 x
the restatement chain's running maximum.  Differences observed on an MI355X are recorded in DESIGN.md section 5c."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import track_exact as tx
import track_ref as tr
from common import ROOT, assert_surfels_match, run_both, small_stream
from test_gpu_parity import _compare_state, _pipes
from test_track_api import (CHAIN_FACTOR, CHAIN_FRAMES, CHAIN_RUNNING_MAX_ROTATION, CHAIN_RUNNING_MAX_TRANSLATION,
                            F32_VS_F64_MAX_ROTATION, F32_VS_F64_MAX_TRANSLATION, pose64)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24          # float32 unit roundoff


def _grown(smx, w=160, h=120, frames=range(4, 12), upload_to=32, **kw):
    s = small_stream(w, h, yaw_deg_per_frame=2.0, **kw)
    _, pg = _pipes(smx, s, 60000)
    for f in range(0, upload_to):
        pg.upload(f, *s.frame(f))
    for f in frames:
        pg.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    return s, pg, pg.reconstruction


@pytest.fixture(scope="module")
def grown(smx):
    return _grown(smx, obstacle_until=8)


def _params(smx, **kw):
    from surfelmeshing_amd._lib import TrackParams
    return TrackParams.defaults(**kw)


def _ref_params(p):
    return tr.Params(levels=[(s, n) for s, n in zip(p.level_stride, p.level_iterations) if n > 0],
                     max_distance=p.max_distance, max_normal_angle_deg=p.max_normal_angle_deg,
                     convergence_rotation=p.convergence_rotation, convergence_translation=p.convergence_translation,
                     min_inliers=p.min_inliers, min_inlier_fraction=p.min_inlier_fraction,
                     min_pivot_ratio=p.min_pivot_ratio, near_z=p.near_z, far_z=p.far_z,
                     disc_radius_factor=p.disc_radius_factor, max_splat_extent_in_pixels=p.max_splat_extent_in_pixels)


def _track(smx, s, pg, g, pred, params, want_model=True):
    """Preprocesses frame g without the cull and tracks it.  Returns (outcome, records, D, M, depth, normals)."""
    rec = pg.reconstruction
    pg.preprocess(g, [], None)
    md = smx.CUDABuffer(s.height, s.width, np.float32) if want_model else None
    mn = smx.CUDABuffer(s.height, s.width, np.float32, 4) if want_model else None
    out = rec.Track(pg.stream, s.depth_scaling, pg.depth_final, pg.normals, pred, params, md, mn)
    recs = rec.debug_track_iterations(pg.stream)
    depth, normals = pg.depth_final.Download(), pg.normals.Download().reshape(s.height, s.width, 2)
    if not want_model:
        return out, recs, None, None, depth, normals
    return out, recs, md.Download(), mn.Download().reshape(s.height, s.width, 4), depth, normals


def _replay(recs):
    """T_rel (float64) after the recorded iterations: exp(x) applied to the float-rounded pose of each solved one."""
    T = tr.IDENTITY.copy()
    for r in recs:
        if r["status"] < tr.TOO_FEW_INLIERS:
            T = tr.se3_mul(tr.se3_exp(r["x"]), T.astype(np.float32).astype(np.float64))
    return T


# ---- model images -----------------------------------------------------------------------------------------------------
def test_model_images_are_the_renders(smx, grown):
    from surfelmeshing_amd import render
    s, pg, rec = grown
    p = _params(smx)
    pred = s.pose(11)
    out, recs, D, M, _, _ = _track(smx, s, pg, 12, pred, p)
    got = render.render_view(rec, s.width, s.height, s.fx, s.fy, s.cx, s.cy, pred, stream=pg.stream, splat_mode="disc",
                             near_z=p.near_z, far_z=p.far_z, disc_radius_factor=p.disc_radius_factor,
                             max_splat_extent_in_pixels=p.max_splat_extent_in_pixels, outputs=("depth", "normal"))
    assert np.array_equal(D.view(np.uint32), got["depth"].view(np.uint32))
    assert np.array_equal(M.view(np.uint32), np.ascontiguousarray(got["normal"]).reshape(M.shape).view(np.uint32))
    assert (D > 0).mean() > 0.4 and out.ok


# ---- one iteration against the restatement ------------------------------------------------------------------------------
def _sum_bounds(inliers, flagged, B, max_distance):
    """Bound on |GPU - restatement| for the 28 float sums of one iteration, derived:
    per inlier, a rotational Jacobian entry (p x M) carries ~12 roundings on values <= B = max |p| (6 in a component of p,
    3 in the cross product, M exact): absolute error 12 U B; a translational entry is M itself, exact.  The residual
    M . (p - q) cancels, its absolute error stays ~30 U B.  A product adds one rounding.  With c = (B, B, B, 1, 1, 1):
      JtJ[a][b]:  (12 + 12 + 1) U c_a c_b            <= 32 U c_a c_b
      Jtr[a]:     12 U B max_distance + c_a 30 U B   <= 64 U B c_a
      sum r^2:    2 max_distance 30 U B + U r^2      <= 64 U B max_distance
    times the inlier count (the sums themselves are double on both sides); plus, for every pixel the restatement flags
    within the float32 margin of a floor or a gate, twice the largest term such a pixel can contribute (it may drop out,
    come in, or meet the neighbouring model pixel): c_a c_b, c_a max_distance, max_distance^2."""
    c = np.array([B, B, B, 1.0, 1.0, 1.0])
    out = np.zeros(28)
    e = 0
    for a in range(6):
        for b in range(a, 6):
            out[e] = inliers * 32 * U * c[a] * c[b] + 2 * flagged * c[a] * c[b]
            e += 1
    out[21:27] = inliers * 64 * U * B * c + 2 * flagged * c * max_distance
    out[27] = inliers * 64 * U * B * max_distance + 2 * flagged * max_distance ** 2
    return out


SIZES = [(160, 120), (200, 77), (320, 240)]


@pytest.fixture(scope="module", params=SIZES, ids=lambda z: "%dx%d" % z)
def sized(smx, request):
    w, h = request.param
    return _grown(smx, w, h, obstacle_until=8)


@pytest.mark.parametrize("stride", [1, 2, 4, 8])
def test_one_iteration_matches_the_restatement(smx, sized, stride):
    """From the identity (record 0) and from a perturbed T_rel (record 1: the pose the first iteration left) of a
    (stride, 1), (stride, 1) schedule, for predictions 1, 3 and 5 frames old.  Beside the bound: the sums are the exact
    model's (tests/track_exact.py) as float64 bits, evaluated on the model images the call returned."""
    s, pg, rec = sized
    intr = (s.fx, s.fy, s.cx, s.cy)
    pred = s.pose(11)
    worst = 0.0
    for g in (12, 14, 16):
        p = _params(smx, levels=[(stride, 1), (stride, 1)], min_inliers=10)   # (stride 4 from 5 frames back: ~90 inliers)
        rp = _ref_params(p)
        out, recs, D, M, depth, normals = _track(smx, s, pg, g, pred, p)
        assert len(recs) == 2 and [r["stride"] for r in recs] == [stride, stride] and [r["level"] for r in recs] == [0, 1]
        T1 = _replay(recs[:1])
        for k, (T, st) in enumerate(((tr.IDENTITY, stride), (T1, stride))):
            _, _, _, inl, pix, mg = tr.iteration(D, M, depth, normals, intr, T, st, rp.gates(), s.depth_scaling)
            got = recs[k]["sums"]
            # the condition under which the comparison means something: few pixels near a decision
            assert mg["flagged"] <= 0.01 * pix, (g, k, mg["flagged"], pix)
            assert got[tr.S_PIXELS] == pix
            assert abs(got[tr.S_ASSOCIATED] - mg["associated"]) <= mg["flagged"]
            assert abs(got[tr.S_INLIERS] - inl) <= mg["flagged"], (g, k, got[tr.S_INLIERS], inl, mg["flagged"])
            bound = _sum_bounds(inl, mg["flagged"], max(mg["p_max"], 1.0), rp.max_distance)
            diff = np.abs(got[:28] - mg["sums"][:28])
            ratio = float((diff / bound).max())
            worst = max(worst, ratio)
            print("one iteration %dx%d frame %d stride %d %s: inliers %d / %d (gpu %d), flagged %d, max |diff| / bound %.3g" % (
                s.width, s.height, g, st, "identity" if k == 0 else "perturbed", inl, pix, got[tr.S_INLIERS],
                mg["flagged"], ratio))
            assert np.all(diff <= bound), (g, k, int(np.argmax(diff / bound)), ratio)
            Tf = tr.IDENTITY if k == 0 else tx.next_pose(recs[0]["x"], tr.IDENTITY)
            exact, _ = tx.exact_sums(D, M, depth, normals, intr, Tf.astype(np.float32), st, rp.gates(), s.depth_scaling)
            assert np.array_equal(got.view(np.uint64), exact.view(np.uint64)), (g, k, np.nonzero(got != exact)[0])
        # the solution of the second record follows from its sums by the restatement's solve
        status, x, _ = tr.solve(recs[1]["sums"], T1, rp)
        assert status == recs[1]["status"] and np.allclose(x, recs[1]["x"], rtol=1e-9, atol=1e-14)


# ---- whole calls --------------------------------------------------------------------------------------------------------
def _call_bounds(ref, rp, err_t, err_r):
    flip = ref["flagged"] * rp.max_distance / max(ref["inliers"], 1)    # (metres; radians at a lever arm >= 1 m)
    return (min(4 * F32_VS_F64_MAX_TRANSLATION + flip, 0.05 * err_t), min(4 * F32_VS_F64_MAX_ROTATION + flip, 0.05 * err_r))


def test_whole_calls_match_the_restatement(smx, grown):
    s, pg, rec = grown
    intr = (s.fx, s.fy, s.cx, s.cy)
    pred = s.pose(11)
    p = _params(smx)
    rp = _ref_params(p)
    for g in (12, 14, 16):
        out, recs, D, M, depth, normals = _track(smx, s, pg, g, pred, p)
        ref = tr.track(D, M, depth, normals, intr, rp, s.depth_scaling)
        T_gpu = _replay(recs)
        dt, dr = tr.pose_difference(ref["T_rel"], T_gpu)
        err_t, err_r = tr.pose_difference(pose64(s, g), tr.se3_mul(pred, ref["T_rel"]))
        bt, br = _call_bounds(ref, rp, err_t, err_r)
        print("whole call frame %d: gpu status %d (%d iterations, %d inliers) ref status %d (%d, %d); |gpu - ref| %.3g m "
              "%.3g rad (bounds %.3g %.3g); ref to truth %.2f mm %.4f deg" % (
                  g, out.status, out.iterations_run, out.inliers, ref["status"], ref["iterations_run"], ref["inliers"],
                  dt, dr, bt, br, err_t * 1e3, np.degrees(err_r)))
        assert out.status == ref["status"] and out.iterations_run == ref["iterations_run"] == len(recs)
        assert dt <= bt and dr <= br, (g, dt, dr, bt, br)
        # the returned pose is the prediction times that T_rel, rounded to float
        want = tr.se3_mul(pred, T_gpu)
        assert np.allclose(out.global_T_frame, want, rtol=0, atol=4 * U * max(1.0, np.abs(want).max()))
        assert out.pixels_with_depth == ref["pixels"] and abs(out.inliers - ref["inliers"]) <= ref["flagged"]
        assert abs(out.rms_residual - ref["rms"]) <= 1e-3 * ref["rms"]
        info = np.zeros((6, 6))
        info[np.triu_indices(6)] = recs[-1]["sums"][:21]
        info = info + info.T - np.diag(np.diag(info))
        assert np.array_equal(out.information, info.astype(np.float32))


def test_the_schedule_is_honoured(smx, grown):
    """Ten iterations at stride 1 alone fail from a prediction 5 frames old where the three-level schedule succeeds (as
    in the restatement: tests/test_track_api.py)."""
    s, pg, rec = grown
    pred = s.pose(11)
    out3, _, _, _, _, _ = _track(smx, s, pg, 16, pred, _params(smx), want_model=False)
    out1, recs1, _, _, _, _ = _track(smx, s, pg, 16, pred, _params(smx, levels=[(1, 10)]), want_model=False)
    e3 = tr.pose_difference(pose64(s, 16), out3.global_T_frame)
    e1 = tr.pose_difference(pose64(s, 16), out1.global_T_frame)
    print("frame 16: three levels %.2f mm %.4f deg; stride 1 x 10: status %d, %.2f mm %.4f deg" % (
        e3[0] * 1e3, np.degrees(e3[1]), out1.status, e1[0] * 1e3, np.degrees(e1[1])))
    assert out3.ok and all(r["stride"] == 1 for r in recs1) and len(recs1) <= 10
    assert (not out1.ok) or e1[0] > 10 * e3[0] or e1[1] > 10 * e3[1]


# ---- statuses on inputs that branch -------------------------------------------------------------------------------------
def _map_snapshot(rec, pg):
    n = rec.surfels_size()
    return n, rec.surfel_count(), rec.debug_download_surfels(n), rec.stats()


def _assert_unchanged(before, rec, pg):
    n, live, rows, stats = before
    assert rec.surfels_size() == n and rec.surfel_count() == live
    assert np.array_equal(rec.debug_download_surfels(n).view(np.uint32), rows.view(np.uint32))
    assert rec.stats() == stats


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_frames_from_elsewhere_and_empty_frames_keep_the_prediction(smx):
    s, pg, rec = _grown(smx, upload_to=60, obstacle_until=8)
    rec.SetDeltaTracking(pg.stream, True)
    rec.TransferChangedToCPU(pg.stream, 11)
    before = _map_snapshot(rec, pg)
    pred = s.pose(11)
    for g in (41, 56):    # 60 and 90 degrees of yaw away
        out, recs, D, M, depth, normals = _track(smx, s, pg, g, pred, _params(smx))
        print("frame %d against the model at 11: %s, %d associated, %d inliers of %d" % (
            g, out.status_name, recs[0]["sums"][tr.S_ASSOCIATED], out.inliers, out.pixels_with_depth))
        assert out.status == smx.SMX_TRACK_TOO_FEW_INLIERS and not out.ok and out.iterations_run == 1 == len(recs)
        # the model IS under the frame (at the identity a pixel projects onto itself, so about the model's coverage, 0.54,
        # of the sampled pixels with depth is associated -- the first iteration samples at stride 4), and nothing passes
        assert recs[0]["stride"] == 4 and recs[0]["sums"][tr.S_PIXELS] == out.pixels_with_depth
        assert recs[0]["sums"][tr.S_ASSOCIATED] >= 0.4 * out.pixels_with_depth and out.inliers < 50
        assert np.array_equal(_bits(out.global_T_frame), _bits(pred))
        assert np.all(recs[0]["x"] == 0)
    zero = smx.CUDABuffer(s.height, s.width, np.uint16)
    zero.Clear(0, pg.stream)
    out = rec.Track(pg.stream, s.depth_scaling, zero, pg.normals, pred, _params(smx))
    assert out.status == smx.SMX_TRACK_TOO_FEW_INLIERS and out.pixels_with_depth == 0 and out.inliers == 0
    assert np.array_equal(_bits(out.global_T_frame), _bits(pred))
    _assert_unchanged(before, rec, pg)
    assert rec.TransferChangedToCPU(pg.stream, 12).count == 0      # no delta mark either


def test_empty_and_one_plane_maps_are_degenerate(smx):
    w, h, f = 160, 120, 131.25
    rec = smx.CUDASurfelReconstruction(60000, smx.PinholeCamera4f(w, h, f, f, 80.0, 60.0))
    depth = smx.CUDABuffer(h, w, np.uint16)
    depth.Clear(10000)                                             # a wall 2 m in front of the camera
    normals = smx.CUDABuffer(h, w, np.float32, 2)
    normals.Clear(0.0)                                             # n = (0, 0, -1)
    pred = np.array([[1, 0, 0, 0.25], [0, 1, 0, -0.5], [0, 0, 1, 0.125]], np.float32)
    out = rec.Track(None, 5000.0, depth, normals, pred, _params(smx))
    assert out.status == smx.SMX_TRACK_DEGENERATE and out.iterations_run == 1 and out.inliers == 0
    assert out.pixels_with_depth > 0 and np.array_equal(_bits(out.global_T_frame), _bits(pred))
    # one plane: a grid of discs on z = 2 (in the prediction's camera frame), 2 cm apart, 1.5 cm radius
    g = np.arange(-1.6, 1.6, 0.02)
    X, Y = np.meshgrid(g, g)
    k = X.size
    rows = np.zeros((25, k), np.float32)
    rows[0] = rows[3] = X.ravel() + pred[0, 3]
    rows[1] = rows[4] = Y.ravel() + pred[1, 3]
    rows[2] = rows[5] = 2.0 + pred[2, 3]
    rows[10] = -1.0
    rows[7] = 0.015 ** 2
    rows[19:23] = np.full((4, k), 0xFFFFFFFF, np.uint32).view(np.float32)
    rec.debug_upload_surfels(rows)
    before = (rec.surfels_size(), rec.debug_download_surfels(k))
    out = rec.Track(None, 5000.0, depth, normals, pred, _params(smx))
    recs = rec.debug_track_iterations()
    print("one plane: %s, %d inliers of %d" % (out.status_name, out.inliers, out.pixels_with_depth))
    assert out.status == smx.SMX_TRACK_DEGENERATE and out.iterations_run == 1
    assert out.inliers > 0.9 * out.pixels_with_depth and out.rms_residual < 1e-4
    assert np.array_equal(_bits(out.global_T_frame), _bits(pred)) and np.all(recs[0]["x"] == 0)
    assert rec.surfels_size() == before[0]
    assert np.array_equal(rec.debug_download_surfels(k).view(np.uint32), before[1].view(np.uint32))
    rec.close()


def test_argument_errors(smx, grown):
    from surfelmeshing_amd import _lib
    s, pg, rec = grown
    lib = _lib.load()
    pg.preprocess(12, [], None)
    d, n = pg.depth_final.ToCUDA(), pg.normals.ToCUDA()
    T = np.ascontiguousarray(s.pose(11), np.float32).reshape(12)
    Tp = T.ctypes.data_as(C.c_void_p)
    res = _lib.TrackResult()

    def call(p, depth=d, normals=n, md=None, mn=None):
        return lib.smx_recon_track(rec._h, None, C.c_float(s.depth_scaling), C.byref(depth), C.byref(normals), Tp,
                                   C.byref(p), C.byref(res), 0, md, mn)
    small = smx.CUDABuffer(s.height, s.width - 1, np.uint16).ToCUDA()
    f32img = smx.CUDABuffer(s.height, s.width, np.float32)
    assert call(_params(smx), depth=small) == -1
    assert call(_params(smx), normals=d) == -1                                  # (2-byte elements where 8 are needed)
    assert call(_params(smx), mn=C.byref(f32img.ToCUDA())) == -1                # (4-byte elements where 16 are needed)
    for levels in ([(3, 2)], [(1, 0)], [(1, 33)], [(16, 1)]):
        p = _params(smx)
        for k in range(3):
            p.level_stride[k], p.level_iterations[k] = levels[0] if k == 0 else (1, 0)
        assert call(p) == -1, levels
    for field, bad in (("max_distance", 0.0), ("max_normal_angle_deg", 0.0), ("near_z", 0.0), ("far_z", 0.01),
                       ("disc_radius_factor", 0.0), ("max_splat_extent_in_pixels", 0.0)):
        assert call(_params(smx, **{field: bad})) == -1, field
    assert call(_params(smx), md=C.byref(f32img.ToCUDA())) == 0
    assert res.status in (0, 1) and res.iterations_run == len(rec.debug_track_iterations())


# ---- reproducibility and ordering ---------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(smx, grown):
    s, pg, rec = grown
    a = _track(smx, s, pg, 14, s.pose(11), _params(smx))
    b = _track(smx, s, pg, 14, s.pose(11), _params(smx))
    assert np.array_equal(_bits(a[0].global_T_frame), _bits(b[0].global_T_frame))
    assert np.array_equal(_bits(a[0].information), _bits(b[0].information))
    assert len(a[1]) == len(b[1])
    for ra, rb in zip(a[1], b[1]):
        assert np.array_equal(ra["sums"].view(np.uint64), rb["sums"].view(np.uint64))
        assert np.array_equal(ra["x"].view(np.uint64), rb["x"].view(np.uint64)) and ra["status"] == rb["status"]


def test_track_between_integrate_calls_is_ordered_and_leaves_the_stream_alone(smx):
    """The same call between two Integrate calls of a running pipeline -- pipelining on and off, both hand-over modes --
    gives the same bits, and the Integrate results after it stay bit-equal to the oracle's."""
    results = {}
    for mode in ("handover1", "handover0", "no_overlap"):
        s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
        po, pg = _pipes(smx, s, 60000)
        rec = pg.reconstruction
        rec.set_handover_mode(0 if mode == "handover0" else 1)
        if mode == "no_overlap":
            rec.set_overlap(0)
        from surfelmeshing_amd.tracking import Tracker
        tracker = Tracker(pg)
        got = []

        def between(f):
            # straight behind Integrate(f), no synchronisation in between: the next frame against the map as it stands
            depth, normals = tracker.preprocess(f + 1)
            out = rec.Track(pg.stream, s.depth_scaling, depth, normals, s.pose(f), _params(smx))
            got.append((out.status, _bits(out.global_T_frame).copy(), out.inliers,
                        [r["sums"].view(np.uint64).copy() for r in rec.debug_track_iterations(pg.stream)]))
        run_both(po, pg, s, list(range(4, 16)), between)
        _compare_state(po, pg)
        assert all(st < tr.TOO_FEW_INLIERS for st, _, _, _ in got[2:])
        results[mode] = got
        tracker.close()
    for mode in ("handover0", "no_overlap"):
        for a, b in zip(results["handover1"], results[mode]):
            assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
            assert len(a[3]) == len(b[3]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


# ---- the chain ----------------------------------------------------------------------------------------------------------
def test_chain_of_tracked_and_integrated_frames_follows_the_ground_truth(smx):
    """16 frames (12 .. 27, 32 degrees of yaw), each tracked from the previous estimate and integrated at its tracked pose
    without the cull.  Error against the ground truth at every frame <= 1.5 x the restatement chain's running maximum."""
    s, pg, rec = _grown(smx, upload_to=max(CHAIN_FRAMES) + 1)
    last = s.pose(11)
    errs = []
    for g in CHAIN_FRAMES:
        pg.preprocess(g, [], None)
        out = rec.Track(pg.stream, s.depth_scaling, pg.depth_final, pg.normals, last, _params(smx))
        assert out.ok, (g, out)
        errs.append(tr.pose_difference(pose64(s, g), out.global_T_frame))
        pg.integrate(g, out.global_T_frame)
        last = out.global_T_frame
    print("gpu chain errors (mm): " + " ".join("%.2f" % (e[0] * 1e3) for e in errs))
    print("gpu chain errors (deg): " + " ".join("%.4f" % np.degrees(e[1]) for e in errs))
    for k, (et, er) in enumerate(errs):
        assert et <= CHAIN_FACTOR * CHAIN_RUNNING_MAX_TRANSLATION[k], (CHAIN_FRAMES[k], et)
        assert er <= CHAIN_FACTOR * CHAIN_RUNNING_MAX_ROTATION[k], (CHAIN_FRAMES[k], er)
    # so that the test cannot pass emptily: never updating the pose is at least ten times the bound away
    stay_t, stay_r = tr.pose_difference(pose64(s, CHAIN_FRAMES[-1]), pose64(s, 11))
    assert stay_r >= 10 * CHAIN_FACTOR * CHAIN_RUNNING_MAX_ROTATION[-1]


# ---- the tool -----------------------------------------------------------------------------------------------------------
def test_run_tum_tracks_a_synthetic_recording(tmp_path):
    traj = tmp_path / "tracked.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "40",
                        "--track", "--track_write_trajectory", str(traj)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout[-600:])
    m = re.search(r"ATE RMSE ([0-9.]+) m over (\d+) frames \(.*?: ([0-9.]+) m, ratio ([0-9.]+)\)", r.stdout)
    assert m, r.stdout[-1000:]
    ate, n, still = float(m.group(1)), int(m.group(2)), float(m.group(3))
    integrated = int(re.search(r"(\d+) frames integrated", r.stdout).group(1))
    lines = [ln for ln in open(traj).read().splitlines() if ln and not ln.startswith("#")]
    assert len(lines) == n == integrated and n >= 30
    assert all(len(ln.split()) == 8 for ln in lines)
    assert ate < 0.5 * still, (ate, still)
