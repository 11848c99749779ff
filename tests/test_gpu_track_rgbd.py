"""Tracking with colour (smx_recon_track_rgbd) on the GPU against the restatement of tests/track_rgbd_ref.py: the model
photometric image bit for bit, the 33 sums of one iteration within the bound derived in tests/track_ref.py /
tests/track_rgbd_ref.py, weight 0 bit-equal to smx_recon_track, the textured plane that geometry alone cannot hold, ordering
between Integrate calls, the 16-frame chain, argument errors.  Differences observed on an MI355X are recorded in DESIGN.md
section 5f."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import track_exact as tx
import track_ref as tr
import track_rgbd_ref as trr
from common import ROOT, run_both, small_stream
from test_gpu_parity import _compare_state, _pipes
from test_gpu_track import _bits, _grown, _replay, _sum_bounds
from test_track_api import CHAIN_FACTOR, CHAIN_FRAMES, pose64
from test_track_rgbd_api import (INTR, PLANE_F32_VS_F64_MAX_ROTATION, PLANE_F32_VS_F64_MAX_TRANSLATION, PLANE_PRED,
                                 PLANE_TWISTS, RGBD_CHAIN_RUNNING_MAX_ROTATION, RGBD_CHAIN_RUNNING_MAX_TRANSLATION,
                                 plane_frame, plane_rows)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SIZES = [(160, 120), (200, 77)]


def _params(**kw):
    from surfelmeshing_amd._lib import TrackRGBDParams
    return TrackRGBDParams.defaults(**kw)


def _ref_params(p):
    i = p.icp
    return trr.Params(levels=[(s, n) for s, n in zip(i.level_stride, i.level_iterations) if n > 0],
                      max_distance=i.max_distance, max_normal_angle_deg=i.max_normal_angle_deg,
                      convergence_rotation=i.convergence_rotation, convergence_translation=i.convergence_translation,
                      min_inliers=i.min_inliers, min_inlier_fraction=i.min_inlier_fraction,
                      min_pivot_ratio=i.min_pivot_ratio, near_z=i.near_z, far_z=i.far_z,
                      disc_radius_factor=i.disc_radius_factor, max_splat_extent_in_pixels=i.max_splat_extent_in_pixels,
                      photometric_weight=p.photometric_weight, max_intensity_difference=p.max_intensity_difference,
                      min_gradient=p.min_gradient, gradient_max_relative_depth_step=p.gradient_max_relative_depth_step)


@pytest.fixture(scope="module", params=SIZES, ids=lambda z: "%dx%d" % z)
def sized(smx, request):
    w, h = request.param
    return _grown(smx, w, h, obstacle_until=8)


@pytest.fixture(scope="module")
def grown(smx):
    return _grown(smx, obstacle_until=8)


def _track(smx, s, pg, g, pred, params, want_model=True):
    """Preprocesses frame g without the cull and tracks it with its colour image.  Returns (outcome, records, D, M, P,
    depth, normals, colour)."""
    rec = pg.reconstruction
    pg.preprocess(g, [], None)
    h, w = s.height, s.width
    md = smx.CUDABuffer(h, w, np.float32) if want_model else None
    mn = smx.CUDABuffer(h, w, np.float32, 4) if want_model else None
    mp = smx.CUDABuffer(h, w, np.float32, 4) if want_model else None
    out = rec.TrackRGBD(pg.stream, s.depth_scaling, pg.depth_final, pg.normals, pg.color[g], pred, params, md, mn, mp)
    recs = rec.debug_track_rgbd_iterations(pg.stream)
    depth, normals = pg.depth_final.Download(), pg.normals.Download().reshape(h, w, 2)
    color = pg.color[g].Download().reshape(h, w, 3)
    if not want_model:
        return out, recs, None, None, None, depth, normals, color
    return (out, recs, md.Download(), mn.Download().reshape(h, w, 4), mp.Download().reshape(h, w, 4), depth, normals, color)


# ---- 1. model images -----------------------------------------------------------------------------------------------------
def test_model_photo_is_the_restatement_of_the_gpus_own_renders(smx, sized):
    from surfelmeshing_amd import render
    s, pg, rec = sized
    p = _params()
    pred = s.pose(11)
    out, recs, D, M, P, _, _, _ = _track(smx, s, pg, 12, pred, p)
    got = render.render_view(rec, s.width, s.height, s.fx, s.fy, s.cx, s.cy, pred, stream=pg.stream, splat_mode="disc",
                             color="color", near_z=p.icp.near_z, far_z=p.icp.far_z,
                             disc_radius_factor=p.icp.disc_radius_factor,
                             max_splat_extent_in_pixels=p.icp.max_splat_extent_in_pixels, outputs=("depth", "color"))
    assert np.array_equal(D.view(np.uint32), got["depth"].view(np.uint32))
    Cm = np.ascontiguousarray(got["color"]).reshape(s.height, s.width, 4).view(np.uint32)[..., 0]
    assert np.array_equal((Cm >> 24) != 0, D > 0)
    want = trr.prepare(D, Cm, p.gradient_max_relative_depth_step)
    assert np.array_equal(P.view(np.uint32), want.view(np.uint32))
    valid = P[..., 3] != 0
    interior = np.zeros_like(valid)
    interior[1:-1, 1:-1] = True
    # empty pixels and depth steps: interior pixels WITH a depth that are not valid, and valid ones with a gradient
    assert (interior & (D > 0) & ~valid).sum() > 50 and (interior & (D == 0)).sum() > 50
    assert valid.sum() > 0.3 * valid.size and not valid[~interior].any()
    assert (np.hypot(P[..., 1], P[..., 2])[valid] >= p.min_gradient).sum() > 100
    assert out.ok and out.photometric_inliers > 0


# ---- 2. one iteration ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 4, 8])
def test_one_iteration_matches_the_restatement(smx, sized, stride):
    """From the identity (record 0) and from a perturbed T_rel (record 1) of a (stride, 1), (stride, 1) schedule, for
    predictions 1, 3 and 5 frames old: all 33 sums.  Beside the bound: the sums are the exact model's (tests/track_exact.py)
    as float64 bits, evaluated on the model images the call returned."""
    s, pg, rec = sized
    intr = (s.fx, s.fy, s.cx, s.cy)
    pred = s.pose(11)
    for g in (12, 14, 16):
        p = _params(levels=[(stride, 1), (stride, 1)], min_inliers=10)
        rp = _ref_params(p)
        out, recs, D, M, P, depth, normals, color = _track(smx, s, pg, g, pred, p)
        assert len(recs) == 2 and [r["stride"] for r in recs] == [stride, stride] and [r["level"] for r in recs] == [0, 1]
        T1 = _replay(recs[:1])
        for k, T in enumerate((tr.IDENTITY, T1)):
            want, mg = trr.iteration(D, M, P, depth, normals, color, intr, T, stride, rp, s.depth_scaling)
            ph, got = mg["photo"], recs[k]["sums"]
            pix, inl, fl = want[tr.S_PIXELS], want[tr.S_INLIERS], mg["flagged"]
            assert fl <= 0.01 * pix, (g, k, fl, pix)
            assert got[tr.S_PIXELS] == pix
            assert abs(got[tr.S_ASSOCIATED] - want[tr.S_ASSOCIATED]) <= fl and abs(got[tr.S_INLIERS] - inl) <= fl
            assert abs(got[trr.S_PHOTO_INLIERS] - ph["inliers"]) <= fl and ph["inliers"] > 0
            diff, bound = trr.compare_sums(got, want, mg, rp, _sum_bounds)
            ratio = float((diff / bound).max())
            print("rgbd one iteration %dx%d frame %d stride %d %s: inliers %d / %d, photometric %d (gpu %d), flagged %d, "
                  "max |diff| / bound %.3g" % (s.width, s.height, g, stride, "identity" if k == 0 else "perturbed", inl, pix,
                                                ph["inliers"], got[trr.S_PHOTO_INLIERS], fl, ratio))
            assert np.all(diff <= bound), (g, k, int(np.argmax(diff / bound)), ratio)
            Tf = tr.IDENTITY if k == 0 else tx.next_pose(recs[0]["x"], tr.IDENTITY)
            exact, _ = tx.exact_sums(D, M, depth, normals, intr, Tf.astype(np.float32), stride, rp.gates(), s.depth_scaling,
                                     (P, color, rp))
            assert np.array_equal(got.view(np.uint64), exact.view(np.uint64)), (g, k, np.nonzero(got != exact)[0])
        status, x, _ = trr.solve(recs[1]["sums"], T1, rp)
        assert status == recs[1]["status"] and np.allclose(x, recs[1]["x"], rtol=1e-9, atol=1e-14)


# ---- 3. weight 0 ---------------------------------------------------------------------------------------------------------
def test_weight_zero_is_track_bit_for_bit(smx, grown):
    s, pg, rec = grown
    pred = s.pose(11)
    for g in (12, 16):
        p = _params(photometric_weight=0.0)
        pg.preprocess(g, [], None)
        a = rec.Track(pg.stream, s.depth_scaling, pg.depth_final, pg.normals, pred, p.icp)
        ra = rec.debug_track_iterations(pg.stream)
        assert rec.debug_track_rgbd_iterations(pg.stream) == []          # (the last call was Track)
        sentinel = smx.CUDABuffer(s.height, s.width, np.float32, 4)
        sentinel.Clear(7.0, pg.stream)
        b = rec.TrackRGBD(pg.stream, s.depth_scaling, pg.depth_final, pg.normals, pg.color[g], pred, p, None, None, sentinel)
        rb = rec.debug_track_rgbd_iterations(pg.stream)
        assert a.ok and a.status == b.status and a.iterations_run == b.iterations_run == len(ra) == len(rb)
        assert (a.inliers, a.pixels_with_depth) == (b.inliers, b.pixels_with_depth)
        assert np.array_equal(_bits(a.global_T_frame), _bits(b.global_T_frame))
        assert np.array_equal(_bits(a.information), _bits(b.information))
        assert _bits(a.rms_residual) == _bits(b.rms_residual)
        assert b.photometric_inliers == 0 and b.rms_intensity_residual == 0
        for x, y in zip(ra, rb):
            assert np.array_equal(x["sums"].view(np.uint64), y["sums"][:31].view(np.uint64)) and np.all(y["sums"][31:] == 0)
            assert np.array_equal(x["x"].view(np.uint64), y["x"].view(np.uint64)) and x["status"] == y["status"]
        assert np.all(sentinel.Download() == 7.0)                         # (no prepare launch: P is not handed out)
        sentinel.close()


# ---- 4. the textured plane -----------------------------------------------------------------------------------------------
def _plane_rec(smx, flat=False):
    rec = smx.CUDASurfelReconstruction(60000, smx.PinholeCamera4f(160, 120, INTR[0], INTR[1], INTR[2], INTR[3]))
    rows = plane_rows(flat=flat)
    rec.debug_upload_surfels(rows)
    return rec, rows


def _plane_call(smx, rec, frame, params, want_model=False):
    T_true, depth, normals, color = frame
    d = smx.CUDABuffer(120, 160, np.uint16); d.Upload(depth)
    n = smx.CUDABuffer(120, 160, np.float32, 2); n.Upload(normals)
    c = smx.CUDABuffer(120, 160, np.uint8, 3); c.Upload(color)
    md, mn, mp = (smx.CUDABuffer(120, 160, np.float32), smx.CUDABuffer(120, 160, np.float32, 4),
                  smx.CUDABuffer(120, 160, np.float32, 4)) if want_model else (None, None, None)
    geo = rec.Track(None, 5000.0, d, n, PLANE_PRED, params.icp)
    out = rec.TrackRGBD(None, 5000.0, d, n, c, PLANE_PRED, params, md, mn, mp)
    recs = rec.debug_track_rgbd_iterations()
    imgs = (md.Download(), mn.Download().reshape(120, 160, 4), mp.Download().reshape(120, 160, 4)) if want_model else None
    for b in (d, n, c, md, mn, mp):
        if b is not None:
            b.close()
    return geo, out, recs, imgs


def test_textured_plane_is_tracked_where_geometry_is_degenerate(smx):
    rec, rows = _plane_rec(smx)
    rec.SetDeltaTracking(None, True)
    rec.TransferChangedToCPU(None, 0)
    before = rec.debug_download_surfels(rows.shape[1])
    p = _params()
    rp = _ref_params(p)
    for k, twist in enumerate(PLANE_TWISTS):
        frame = plane_frame(twist, seed=k)
        T_true, depth, normals, color = frame
        geo, out, recs, (D, M, P) = _plane_call(smx, rec, frame, p, want_model=True)
        assert geo.status == smx.SMX_TRACK_DEGENERATE and np.array_equal(_bits(geo.global_T_frame), _bits(PLANE_PRED))
        assert out.status in (smx.SMX_TRACK_OK, smx.SMX_TRACK_CONVERGED), out
        ref = trr.track(D, M, P, depth, normals, color, INTR, rp)
        T_gpu = _replay(recs)
        dt, dr = tr.pose_difference(ref["T_rel"], T_gpu)
        t0, r0 = tr.pose_difference(T_true, tr.IDENTITY)
        et, er = tr.pose_difference(T_true, ref["T_rel"])
        gt, gr = tr.pose_difference(T_true, T_gpu)
        # the rule of tests/test_gpu_track.py::_call_bounds with this scene's constants
        flip = ref["flagged"] * rp.max_distance / max(ref["inliers"], 1)
        bt = min(4 * PLANE_F32_VS_F64_MAX_TRANSLATION + flip, 0.05 * et)
        br = min(4 * PLANE_F32_VS_F64_MAX_ROTATION + flip, 0.05 * er)
        print("plane twist %d: gpu status %d (%d iterations, %d photometric inliers, rms %.4f) ref status %d (%d); |gpu - ref| "
              "%.3g m %.3g rad (bounds %.3g %.3g); start %.1f mm %.2f deg, gpu to truth %.3f mm %.4f deg" % (
                  k, out.status, out.iterations_run, out.photometric_inliers, out.rms_intensity_residual, ref["status"],
                  ref["iterations_run"], dt, dr, bt, br, t0 * 1e3, np.degrees(r0), gt * 1e3, np.degrees(gr)))
        assert out.status == ref["status"] and out.iterations_run == ref["iterations_run"] == len(recs)
        assert dt <= bt and dr <= br, (k, dt, dr, bt, br)
        assert gt <= t0 / 20 and gr <= r0 / 20, (k, gt, gr)
        want = tr.se3_mul(PLANE_PRED, T_gpu)
        assert np.allclose(out.global_T_frame, want, rtol=0, atol=4 * U * max(1.0, np.abs(want).max()))
        assert abs(out.photometric_inliers - ref["photometric_inliers"]) <= ref["flagged"]
        assert abs(out.rms_intensity_residual - ref["rms_intensity"]) <= 1e-3 * ref["rms_intensity"]
    assert np.array_equal(rec.debug_download_surfels(rows.shape[1]).view(np.uint32), before.view(np.uint32))
    assert rec.TransferChangedToCPU(None, 1).count == 0
    rec.close()


def test_flat_noisy_plane_stays_degenerate(smx):
    rec, rows = _plane_rec(smx, flat=True)
    geo, out, recs, _ = _plane_call(smx, rec, plane_frame(PLANE_TWISTS[1], flat=True, seed=1), _params())
    assert geo.status == smx.SMX_TRACK_DEGENERATE
    assert out.status == smx.SMX_TRACK_DEGENERATE and out.photometric_inliers == 0 and out.iterations_run == 1
    assert np.array_equal(_bits(out.global_T_frame), _bits(PLANE_PRED)) and np.all(recs[0]["x"] == 0)
    _, out, _, _ = _plane_call(smx, rec, plane_frame(PLANE_TWISTS[1], flat=True, seed=1), _params(min_gradient=0.0))
    assert out.status != smx.SMX_TRACK_DEGENERATE and out.photometric_inliers > 0     # (the gate is what decides)
    rec.close()


# ---- 5. reproducibility and ordering -------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(smx, grown):
    s, pg, rec = grown
    a = _track(smx, s, pg, 14, s.pose(11), _params())
    b = _track(smx, s, pg, 14, s.pose(11), _params())
    assert np.array_equal(_bits(a[0].global_T_frame), _bits(b[0].global_T_frame))
    assert np.array_equal(_bits(a[0].information), _bits(b[0].information))
    assert a[0].photometric_inliers == b[0].photometric_inliers
    assert _bits(a[0].rms_intensity_residual) == _bits(b[0].rms_intensity_residual)
    assert len(a[1]) == len(b[1]) and np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))
    for ra, rb in zip(a[1], b[1]):
        assert np.array_equal(ra["sums"].view(np.uint64), rb["sums"].view(np.uint64))
        assert np.array_equal(ra["x"].view(np.uint64), rb["x"].view(np.uint64)) and ra["status"] == rb["status"]


def test_track_rgbd_between_integrate_calls_is_ordered_and_leaves_the_stream_alone(smx):
    results = {}
    for mode in ("handover1", "handover0", "no_overlap"):
        s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
        po, pg = _pipes(smx, s, 60000)
        rec = pg.reconstruction
        rec.set_handover_mode(0 if mode == "handover0" else 1)
        if mode == "no_overlap":
            rec.set_overlap(0)
        from surfelmeshing_amd.tracking import Tracker
        tracker = Tracker(pg, _params(), rgbd=True)
        got = []

        def between(f):
            depth, normals = tracker.preprocess(f + 1)
            out = rec.TrackRGBD(pg.stream, s.depth_scaling, depth, normals, pg.color[f + 1], s.pose(f), _params())
            got.append((out.status, _bits(out.global_T_frame).copy(), out.photometric_inliers,
                        [r["sums"].view(np.uint64).copy() for r in rec.debug_track_rgbd_iterations(pg.stream)]))
        run_both(po, pg, s, list(range(4, 12)), between)
        _compare_state(po, pg)
        assert all(st < tr.TOO_FEW_INLIERS and n > 0 for st, _, n, _ in got[2:])
        results[mode] = got
        tracker.close()
    for mode in ("handover0", "no_overlap"):
        for a, b in zip(results["handover1"], results[mode]):
            assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
            assert len(a[3]) == len(b[3]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


# ---- 6. the chain --------------------------------------------------------------------------------------------------------
def test_chain_tracked_with_colour_follows_the_restatement_chain(smx):
    """Frames 12 .. 27, each tracked with colour from the previous estimate and integrated at its tracked pose.  Error
    against the ground truth at every frame <= CHAIN_FACTOR x the running maximum of the restatement's RGB-D chain."""
    s, pg, rec = _grown(smx, upload_to=max(CHAIN_FRAMES) + 1)
    last = s.pose(11)
    errs = []
    for g in CHAIN_FRAMES:
        pg.preprocess(g, [], None)
        out = rec.TrackRGBD(pg.stream, s.depth_scaling, pg.depth_final, pg.normals, pg.color[g], last, _params())
        assert out.ok, (g, out)
        errs.append(tr.pose_difference(pose64(s, g), out.global_T_frame))
        pg.integrate(g, out.global_T_frame)
        last = out.global_T_frame
    print("gpu rgbd chain errors (mm): " + " ".join("%.2f" % (e[0] * 1e3) for e in errs))
    print("gpu rgbd chain errors (deg): " + " ".join("%.4f" % np.degrees(e[1]) for e in errs))
    for k, (et, er) in enumerate(errs):
        assert et <= CHAIN_FACTOR * RGBD_CHAIN_RUNNING_MAX_TRANSLATION[k], (CHAIN_FRAMES[k], et)
        assert er <= CHAIN_FACTOR * RGBD_CHAIN_RUNNING_MAX_ROTATION[k], (CHAIN_FRAMES[k], er)
    stay_t, stay_r = tr.pose_difference(pose64(s, CHAIN_FRAMES[-1]), pose64(s, 11))
    assert stay_r >= 10 * CHAIN_FACTOR * RGBD_CHAIN_RUNNING_MAX_ROTATION[-1]


# ---- 7. argument errors, the tool ----------------------------------------------------------------------------------------
def test_argument_errors(smx, grown):
    from surfelmeshing_amd import _lib
    s, pg, rec = grown
    lib = _lib.load()
    pg.preprocess(12, [], None)
    d, n, c = pg.depth_final.ToCUDA(), pg.normals.ToCUDA(), pg.color[12].ToCUDA()
    T = np.ascontiguousarray(s.pose(11), np.float32).reshape(12)
    Tp = T.ctypes.data_as(C.c_void_p)
    res = _lib.TrackRGBDResult()

    def call(p, color=c, mp=None):
        return lib.smx_recon_track_rgbd(rec._h, None, C.c_float(s.depth_scaling), C.byref(d), C.byref(n), C.byref(color), Tp,
                                        C.byref(p), C.byref(res), 0, None, None, mp)
    small = smx.CUDABuffer(s.height, s.width - 1, np.uint8, 3).ToCUDA()
    grey = smx.CUDABuffer(s.height, s.width, np.uint8).ToCUDA()
    f32img = smx.CUDABuffer(s.height, s.width, np.float32)
    assert call(_params(), color=small) == -1
    assert call(_params(), color=grey) == -1                                   # (1-byte elements where 3 are needed)
    assert call(_params(), mp=C.byref(f32img.ToCUDA())) == -1                  # (4-byte elements where 16 are needed)
    for field, bad in (("photometric_weight", -0.1), ("max_intensity_difference", 0.0), ("min_gradient", -1.0),
                       ("gradient_max_relative_depth_step", 0.0), ("max_distance", 0.0)):
        assert call(_params(**{field: bad})) == -1, field
    assert b"invalid argument" in lib.smx_last_error()
    assert call(_params()) == 0
    assert res.icp.status in (0, 1) and res.icp.iterations_run == len(rec.debug_track_rgbd_iterations())


def test_run_tum_tracks_a_synthetic_recording_with_colour(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_tum.py"), str(tmp_path / "ds"), "--synthetic", "9",
                        "--track_rgbd"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout[-600:])
    assert int(re.search(r"tracked (\d+) frames", r.stdout).group(1)) >= 8
    assert re.search(r"ATE RMSE ([0-9.]+) m over (\d+) frames", r.stdout), r.stdout[-1000:]
