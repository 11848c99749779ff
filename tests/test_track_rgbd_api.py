"""Tracking with colour at the boundary (no GPU): the C-ABI symbols, the struct layouts against their ctypes mirrors, the
shim's TrackRGBD call compiling against libsmx.so, argument errors that need no device, and the numpy restatement of
tests/track_rgbd_ref.py -- weight 0 against tests/track_ref.py, on the textured plane geometry alone cannot hold, and on
the project's own data, which is where the bounds of tests/test_gpu_track_rgbd.py are measured (the constants below, each
with the measured value beside it)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import track_ref as tr
import track_rgbd_ref as trr
import viz_ref as vr
from common import ROOT, small_stream
from test_track_api import CHAIN_FRAMES, error_to_truth, oracle_map, pose64

NEW_SYMBOLS = ("smx_track_rgbd_params_default", "smx_recon_track_rgbd", "smx_recon_debug_track_rgbd_iterations")

# ---- measured on the CPU by the tests below ---------------------------------------------------------------------------
# test_textured_plane_is_held_by_colour: how far the float32 evaluation of the per-pixel part moves a whole call's answer on
# the textured plane, maximum over the three twists.  Measured: 5.9e-7 m, 1.16e-6 rad (both at the largest twist; the two
# others 2.6e-8 m, 3.1e-9 rad).  tests/test_gpu_track_rgbd.py holds the GPU to 4 x these (+ its flagged-pixel term).
PLANE_F32_VS_F64_MAX_TRANSLATION = 1e-6    # metres
PLANE_F32_VS_F64_MAX_ROTATION = 2e-6       # radians
# test_reference_single_calls_rgbd: the same on the oracle's map of small_stream for frame 12 against the model at frame
# 11's pose, the step of a frame loop.  Measured: 1.65e-7 m, 1.3e-8 rad without the obstacle, 1.41e-5 m, 4.41e-6 rad with it
# (all 19 iterations run and end OK, not CONVERGED: the last updates are still 1e-5).
F32_VS_F64_MAX_TRANSLATION = 2e-5
F32_VS_F64_MAX_ROTATION = 6e-6
# The same for frames 14 and 16 (a prediction 3 and 5 frames old), where the default weight ends far from the truth (that
# test's docstring): {frame: (metres, radians)}, the larger of the runs with and without the obstacle.  Measured: frame 14
# 4.5e-8 m / 9.9e-9 rad without and 1.83e-7 m / 3.7e-8 rad with the obstacle; frame 16 2.0e-7 m / 2.3e-8 rad without and
# 1.60e-4 m / 4.66e-5 rad with it (515 mm from the truth, 19 iterations that do not settle: two roundings of such a call
# part that far).  Kept so that a change of the restatement or of the algorithm at those frames is noticed.
FAR_F32_VS_F64_MAX = {14: (2.5e-7, 5e-8), 16: (2e-4, 6e-5)}
# ... and where those calls end, (metres, radians) from the ground truth, {(obstacle_until, frame): ...}; held to +-10 %.
FAR_ERROR_TO_TRUTH = {(-1, 14): (0.20347, 0.006806), (-1, 16): (0.44947, 0.013374),
                      (8, 14): (0.20756, 0.017520), (8, 16): (0.51502, 0.043099)}
# test_reference_chain_rgbd: running maximum of the restatement's RGB-D chain against the ground truth over frames 12 .. 27
# (the test's printout; the GPU chain must stay within CHAIN_FACTOR x these at every frame).
# Per-frame errors 1.41 1.78 1.83 3.06 6.69 10.0 13.2 17.3 20.8 22.3 26.4 29.3 31.3 33.6 35.3 37.1 mm and 0.012 .. 0.796
# degrees; the geometric chain of tests/test_track_api.py ends at 34.6 mm / 0.746 degrees: the first calls are better, the
# drift is the same.
RGBD_CHAIN_RUNNING_MAX_TRANSLATION = [1.414e-03, 1.780e-03, 1.828e-03, 3.064e-03, 6.686e-03, 1.001e-02, 1.315e-02, 1.728e-02,
                                      2.083e-02, 2.227e-02, 2.636e-02, 2.932e-02, 3.127e-02, 3.360e-02, 3.525e-02, 3.709e-02]
RGBD_CHAIN_RUNNING_MAX_ROTATION = [2.099e-04, 1.248e-03, 1.248e-03, 1.248e-03, 2.175e-03, 3.276e-03, 4.619e-03, 5.953e-03,
                                   7.399e-03, 8.006e-03, 9.512e-03, 1.062e-02, 1.163e-02, 1.264e-02, 1.325e-02, 1.390e-02]


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    from surfelmeshing_amd import _lib
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.EXPORTS and name in exported, name
    for name in ("smx_track_rgbd_params", "smx_track_rgbd_result", "smx_track_rgbd_iteration", "SMX_TRACK_RGBD_SUMS"):
        assert name in header, name


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    from surfelmeshing_amd import _lib
    structs = (("smx_track_rgbd_params", _lib.TrackRGBDParams), ("smx_track_rgbd_result", _lib.TrackRGBDResult),
               ("smx_track_rgbd_iteration", _lib.TrackRGBDIteration))
    body = ""
    for cname, mirror in structs:
        body += '  printf(" %%zu", sizeof(%s));\n' % cname
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in mirror._fields_)
    src = tmp_path / "track_rgbd_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx.h"\nint main(void) {\n' + body +
                   '  printf(" %d\\n", SMX_TRACK_RGBD_SUMS);\n  return 0;\n}\n')
    exe = tmp_path / "track_rgbd_probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = 0
    for cname, mirror in structs:
        n = len(mirror._fields_)
        assert vals[k] == ctypes.sizeof(mirror), cname
        assert vals[k + 1:k + 1 + n] == [getattr(mirror, f).offset for f, _ in mirror._fields_], cname
        k += 1 + n
    assert vals[k:] == [_lib.TRACK_RGBD_SUMS] == [trr.N_SUMS]


def test_default_parameters_are_as_stated():
    from surfelmeshing_amd._lib import TrackParams, TrackRGBDParams
    p, q = TrackRGBDParams.defaults(), trr.Params()
    assert bytes(p.icp) == bytes(TrackParams.defaults())
    assert (p.photometric_weight, p.max_intensity_difference, p.min_gradient, p.gradient_max_relative_depth_step) == tuple(
        float(np.float32(v)) for v in (0.1, 0.2, 0.02, 0.02))
    for name in ("photometric_weight", "max_intensity_difference", "min_gradient", "gradient_max_relative_depth_step"):
        assert getattr(p, name) == getattr(q, name), name
    for name in ("max_distance", "min_inliers", "min_pivot_ratio"):
        assert getattr(p.icp, name) == getattr(q, name), name
    p = TrackRGBDParams.defaults(levels=[(2, 3)], max_distance=0.05, photometric_weight=0.0)
    assert list(p.icp.level_iterations) == [3, 0, 0] and p.icp.max_distance == np.float32(0.05) and p.photometric_weight == 0


def test_argument_errors_need_no_device():
    from surfelmeshing_amd import _lib
    lib = _lib.load()
    assert lib.smx_track_rgbd_params_default(None) == -1
    p = _lib.TrackRGBDParams.defaults()
    res = _lib.TrackRGBDResult()
    d = _lib.BufferDesc()
    T = (ctypes.c_float * 12)()
    assert lib.smx_recon_track_rgbd(None, None, ctypes.c_float(5000.0), ctypes.byref(d), ctypes.byref(d), ctypes.byref(d), T,
                                    ctypes.byref(p), ctypes.byref(res), 0, None, None, None) == -1
    assert lib.smx_recon_track_rgbd(None, None, ctypes.c_float(5000.0), ctypes.byref(d), ctypes.byref(d), ctypes.byref(d), T,
                                    None, ctypes.byref(res), 0, None, None, None) == -1
    n = ctypes.c_int32(7)
    assert lib.smx_recon_debug_track_rgbd_iterations(None, None, None, 0, ctypes.byref(n)) == -1
    assert b"invalid argument" in lib.smx_last_error()


SHIM_SNIPPET = r'''
#include "smx_shim.hpp"
using namespace vis;
int track_frame(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, const CUDABuffer<u16>& depth,
                const CUDABuffer<float2>& normals, const CUDABuffer<Vec3u8>& color, const float* pred, float* pose_out) {
  smx_track_rgbd_params params;
  smx_track_rgbd_params_default(&params);
  params.photometric_weight = 0.05f;
  smx_track_rgbd_result result;
  reconstruction.TrackRGBD(stream, 5000.f, depth, normals, color, pred, params, &result);
  CUDABuffer<float> model_depth(48, 64);
  CUDABuffer<RenderNormal> model_normal(48, 64), model_photo(48, 64);
  reconstruction.TrackRGBD(stream, 5000.f, depth, normals, color, pred, params, &result, &model_depth, &model_normal,
                           &model_photo);
  for (int i = 0; i < 12; ++i) pose_out[i] = result.icp.global_T_frame[i];
  return result.icp.status >= SMX_TRACK_TOO_FEW_INLIERS ? -1 : (int)result.photometric_inliers;
}
int main() { return 0; }
'''


def test_shim_track_rgbd_call_compiles_and_links(tmp_path):
    from surfelmeshing_amd import _lib
    src = tmp_path / "tracker_rgbd.cc"
    src.write_text(SHIM_SNIPPET)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(tmp_path / "tracker_rgbd"), "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_tracking_module_takes_rgbd_without_a_device():
    import inspect
    from surfelmeshing_amd import api, tracking
    assert "rgbd" in inspect.signature(tracking.Tracker.__init__).parameters
    for name in ("TrackRGBD", "TrackRGBDAsync", "debug_track_rgbd_iterations"):
        assert hasattr(api.CUDASurfelReconstruction, name), name


# ---- the scene "textured plane" -----------------------------------------------------------------------------------------
W, H, F = 160, 120, 131.25
INTR = (F, F, 80.0, 60.0)
PLANE_PRED = np.array([[1, 0, 0, 0.25], [0, 1, 0, -0.5], [0, 0, 1, 0.125]], np.float32)
PLANE_TWISTS = ((0.003, -0.004, 0.01, 0.02, -0.015, 0.01), (0.01, -0.008, 0.02, 0.04, -0.03, 0.02),
                (0.02, 0.015, -0.035, 0.08, 0.05, -0.03))


def tex(X, Y):
    return (0.5 + 0.2 * np.sin(2 * np.pi * (X / 0.45 + 0.1)) * np.cos(2 * np.pi * Y / 0.6) +
            0.15 * np.sin(2 * np.pi * (0.7 * X + 0.7 * Y) / 0.3 + 1) + 0.1 * np.cos(2 * np.pi * (X - 2 * Y) / 0.8))


def _grey(X, Y, flat, rng):
    if flat:
        return (128 + rng.integers(-1, 2, size=np.shape(X))).astype(np.uint32)
    return np.rint(255 * tex(X, Y)).astype(np.uint32)


def plane_rows(pred=PLANE_PRED, flat=False):
    """Reference-order rows [25, 25600] of discs on a 2 cm grid at z = 2 m (+- 0.1 mm of jitter, so that no two discs tie
    in the z-test) in the frame of the camera `pred` (identity rotation), radius 1.5 cm, normal (0, 0, -1), grey texture
    (or flat grey with +-1 level of noise)."""
    g = np.arange(-1.6, 1.6, 0.02)
    X, Y = np.meshgrid(g, g)
    k = X.size
    rows = np.zeros((25, k), np.float32)
    rows[0] = rows[3] = X.ravel() + pred[0, 3]
    rows[1] = rows[4] = Y.ravel() + pred[1, 3]
    rows[2] = rows[5] = 2.0 + np.random.default_rng(9).uniform(-1e-4, 1e-4, k) + pred[2, 3]
    rows[10] = -1.0
    rows[7] = 0.015 ** 2
    rows[19:23] = np.full((4, k), 0xFFFFFFFF, np.uint32).view(np.float32)
    grey = _grey(X.ravel(), Y.ravel(), flat, np.random.default_rng(10))
    rows[24] = (grey | (grey << 8) | (grey << 16)).astype(np.uint32).view(np.float32)
    return rows


def plane_frame(twist, flat=False, seed=0, width=W, height=H, intr=INTR):
    """(T_true 3 x 4, depth uint16 [H, W], normals float32 [H, W, 2], colour uint8 [H, W, 3]) of the plane z = 2, ray-cast
    from the camera exp(twist) (prediction's camera <- frame camera)."""
    T = tr.se3_exp(twist)
    R, c = T[:, :3], T[:, 3]
    ys, xs = np.mgrid[0:height, 0:width]
    d = np.stack([(xs + 0.5 - intr[2]) / intr[0], (ys + 0.5 - intr[3]) / intr[1], np.ones((height, width))], axis=-1) @ R.T
    lam = (2.0 - c[2]) / d[..., 2]
    X = c + lam[..., None] * d
    rng = np.random.default_rng(100 + seed)
    depth = np.rint(5000.0 * (lam + rng.normal(0.0, 0.0012, lam.shape) * lam * lam)).astype(np.uint16)
    n = R.T @ np.array([0.0, 0.0, -1.0])
    normals = np.broadcast_to(n[:2].astype(np.float32), (height, width, 2)).copy()
    grey = _grey(X[..., 0], X[..., 1], flat, rng).astype(np.uint8)
    return T, depth, normals, np.ascontiguousarray(np.repeat(grey[..., None], 3, axis=-1))


_plane_models = {}


def plane_model(flat=False):
    """(rows, D, M, C, P) of the plane map at PLANE_PRED by tests/viz_ref.render, computed once."""
    if flat not in _plane_models:
        rows = plane_rows(flat=flat)
        _plane_models[flat] = (rows,) + trr.model_images(rows, rows.shape[1], vr.render, W, H, *INTR, PLANE_PRED)
    return _plane_models[flat]


def test_weight_zero_is_the_geometric_restatement():
    rows, D, M, Cm, P = plane_model()
    T_true, depth, normals, color = plane_frame(PLANE_TWISTS[0])
    # (a corner would be needed for an OK status; equality is what matters here, and it holds per iteration as well)
    p0 = trr.Params(photometric_weight=0.0)
    a = trr.track(D, M, P, depth, normals, color, INTR, p0)
    b = tr.track(D, M, depth, normals, INTR, tr.Params())
    assert a["status"] == b["status"] and a["iterations_run"] == b["iterations_run"]
    assert np.array_equal(a["T_rel"], b["T_rel"]) and a["photometric_inliers"] == 0
    for ra, rb in zip(a["records"], b["records"]):
        assert np.array_equal(ra["sums"][:31], rb["sums"]) and np.all(ra["sums"][31:] == 0)
    s, _ = trr.iteration(D, M, P, depth, normals, color, INTR, tr.se3_exp(PLANE_TWISTS[0]), 2, p0)
    g = tr.iteration(D, M, depth, normals, INTR, tr.se3_exp(PLANE_TWISTS[0]), 2, p0.gates())[5]["sums"]
    assert np.array_equal(s[:31], g)


def test_prepare_marks_borders_holes_and_depth_steps_invalid():
    D = np.full((6, 7), 2.0, np.float32)
    Cm = (np.arange(42, dtype=np.uint32).reshape(6, 7) * 3 + 20) * 0x010101 | 0xFF000000
    D[2, 3] = 0.0            # a hole: itself and its four neighbours
    D[4, 5] = 2.05           # a 2.5 % step: itself and (4, 4) / (3, 5); (5, 5), (4, 6) are border pixels anyway
    P = trr.prepare(D, Cm, 0.02)
    valid = P[..., 3] != 0
    want = np.zeros((6, 7), bool)
    want[1:-1, 1:-1] = True
    for y, x in ((2, 3), (1, 3), (3, 3), (2, 2), (2, 4), (4, 5), (4, 4), (3, 5)):
        want[y, x] = False
    assert np.array_equal(valid, want)
    assert np.all(P[~valid, 1:3] == 0)
    # grey levels rise by 3 per pixel along x and 21 per row: L = grey / 255 to rounding, gx = 3 / 255, gy = 21 / 255
    assert np.allclose(P[..., 0], (np.arange(42).reshape(6, 7) * 3 + 20) / 255.0, rtol=0, atol=3e-7)
    assert np.allclose(P[valid, 1], 3 / 255.0, atol=3e-7) and np.allclose(P[valid, 2], 21 / 255.0, atol=3e-7)
    assert P.dtype == np.float32


def test_textured_plane_is_held_by_colour():
    """Geometry alone is DEGENERATE on the plane; with the photometric term every twist ends within 1 / 20 of its start
    offset in translation and in rotation."""
    rows, D, M, Cm, P = plane_model()
    assert (D > 0).all() and (P[1:-1, 1:-1, 3] == 1).all()
    worst_t = worst_r = 0.0
    for k, twist in enumerate(PLANE_TWISTS):
        T_true, depth, normals, color = plane_frame(twist, seed=k)
        geo = tr.track(D, M, depth, normals, INTR, tr.Params())
        assert geo["status"] == tr.DEGENERATE and geo["iterations_run"] == 1
        out = trr.track(D, M, P, depth, normals, color, INTR, trr.Params())
        out32 = trr.track(D, M, P, depth, normals, color, INTR, trr.Params(), dtype=np.float32)
        t0, r0 = tr.pose_difference(T_true, tr.IDENTITY)
        t1, r1 = tr.pose_difference(T_true, out["T_rel"])
        dt, dr = tr.pose_difference(out["T_rel"], out32["T_rel"])
        print("plane twist %d: status %d, %d iterations, start %.1f mm %.2f deg, end %.3f mm %.4f deg, %d photometric "
              "inliers (rms %.4f) of %d pixels, flagged %d, |f32 - f64| %.3g m %.3g rad" % (
                  k, out["status"], out["iterations_run"], t0 * 1e3, np.degrees(r0), t1 * 1e3, np.degrees(r1),
                  out["photometric_inliers"], out["rms_intensity"], out["pixels"], out["flagged"], dt, dr))
        assert out["status"] in (tr.OK, tr.CONVERGED) and out32["status"] == out["status"]
        assert t1 <= t0 / 20 and r1 <= r0 / 20, (k, t0, t1, r0, r1)
        for r in out["records"]:
            assert r["flagged"] <= 0.01 * r["sums"][tr.S_PIXELS], (k, r["level"], r["flagged"])
        worst_t, worst_r = max(worst_t, dt), max(worst_r, dr)
    assert worst_t <= PLANE_F32_VS_F64_MAX_TRANSLATION and worst_r <= PLANE_F32_VS_F64_MAX_ROTATION, (worst_t, worst_r)


def test_flat_noisy_plane_is_degenerate_because_of_the_gradient_gate():
    rows, D, M, Cm, P = plane_model(flat=True)
    T_true, depth, normals, color = plane_frame(PLANE_TWISTS[1], flat=True, seed=1)
    assert np.ptp(color) == 2 and np.ptp(Cm & 255) == 2
    out = trr.track(D, M, P, depth, normals, color, INTR, trr.Params())
    assert out["status"] == tr.DEGENERATE and out["photometric_inliers"] == 0 and out["iterations_run"] == 1
    assert np.array_equal(out["T_rel"], tr.IDENTITY)
    # without the gate the noise gradients "solve": not DEGENERATE, and nowhere near the truth
    out = trr.track(D, M, P, depth, normals, color, INTR, trr.Params(min_gradient=0.0))
    t0, _ = tr.pose_difference(T_true, tr.IDENTITY)
    t1, _ = tr.pose_difference(T_true, out["T_rel"])
    print("flat plane without the gate: status %d, %.1f mm from the truth (start %.1f mm)" % (out["status"], t1 * 1e3, t0 * 1e3))
    assert out["status"] != tr.DEGENERATE and out["photometric_inliers"] > 0


# ---- the restatement on the project's own data ----------------------------------------------------------------------------
def frame_color(s, g):
    return np.ascontiguousarray(s.frame(g)[1], np.uint8).reshape(s.height, s.width, 3)


def reference_single_calls_rgbd(obstacle_until=-1):
    kw = {"obstacle_until": obstacle_until} if obstacle_until >= 0 else {}
    s = small_stream(yaw_deg_per_frame=2.0, **kw)
    po = oracle_map(s)
    rows, n = po.recon.surfels(), po.recon.surfels_size
    pred = s.pose(11)
    D, M, Cm, P = trr.model_images(rows, n, vr.render, s.width, s.height, s.fx, s.fy, s.cx, s.cy, pred)
    out = {}
    for g in (12, 14, 16):
        po.preprocess(g, [], None)
        depth, normals = np.asarray(po.depth_final), np.asarray(po.normals).reshape(s.height, s.width, 2)
        args = (D, M, P, depth, normals, frame_color(s, g), (s.fx, s.fy, s.cx, s.cy), trr.Params(), s.depth_scaling)
        a, b = trr.track(*args), trr.track(*args, dtype=np.float32)
        out[g] = (a, b, error_to_truth(s, g, pred, a["T_rel"]), float((P[..., 3] != 0).mean()))
    return s, out


@pytest.mark.parametrize("obstacle_until", [-1, 8])
def test_reference_single_calls_rgbd(orc, obstacle_until):
    """A prediction 1, 3 and 5 frames old on the room stream (2 degrees of yaw and 5 mm per frame), default parameters.
    Measured, distance to the ground truth: frame 12 ends at 1.41 mm / 0.012 deg (1.86 mm / 0.030 deg with the obstacle),
    where the geometric call ends at 6.84 / 7.12 mm.  From a prediction 3 and 5 frames old the default weight 0.1 does NOT
    track this stream: status OK, 203 mm / 0.39 deg and 449 mm / 0.77 deg (208 mm / 1.00 deg and 515 mm / 2.47 deg with the
    obstacle), where the geometric call ends at 6.4 and 3.2 mm.  At 6 and 10 degrees the room's texture is 14 and 23 pixels
    off, intensity residuals of 0.11 rms times the weight outweigh the 2 mm depth residuals, and without a pyramid the
    photometric term settles in a neighbouring minimum; with a weight of 0.03 the same calls end at 5.4 and 3.7 mm.  Only
    the one-frame call is therefore held to an accuracy here; the others must end with a good status in both roundings,
    where the record says they end (FAR_ERROR_TO_TRUTH), and their float32-vs-float64 differences are held to the
    recorded FAR_F32_VS_F64_MAX like the one-frame call's to F32_VS_F64_MAX_*."""
    s, out = reference_single_calls_rgbd(obstacle_until)
    worst_t = worst_r = 0.0
    for g, (a, b, (et, er), cov) in out.items():
        dt, dr = tr.pose_difference(a["T_rel"], b["T_rel"])
        print("rgbd single obstacle_until=%d frame %d: status %d/%d, %d iterations, error %.2f mm %.4f deg, inliers %d / %d, "
              "photometric %d (rms %.4f), valid P %.2f, flagged %d, |f32 - f64| %.3g m %.3g rad" % (
                  obstacle_until, g, a["status"], b["status"], a["iterations_run"], et * 1e3, np.degrees(er), a["inliers"],
                  a["pixels"], a["photometric_inliers"], a["rms_intensity"], cov, a["flagged"], dt, dr))
        assert a["status"] in (tr.OK, tr.CONVERGED) and b["status"] == a["status"]
        e0t, e0r = error_to_truth(s, g, s.pose(11), tr.IDENTITY)
        if g == 12:    # (one frame: the step a frame loop takes; better than the geometric call's 6.84 / 7.12 mm)
            assert et < 0.003 and er < np.deg2rad(0.05) and er < 0.1 * e0r, (g, et, er, e0t, e0r)
        assert a["photometric_inliers"] > 0
        for r in a["records"]:
            assert r["flagged"] <= 0.01 * r["sums"][tr.S_PIXELS], (g, r["level"], r["flagged"])
        if g == 12:
            worst_t, worst_r = max(worst_t, dt), max(worst_r, dr)
        else:
            assert dt <= FAR_F32_VS_F64_MAX[g][0] and dr <= FAR_F32_VS_F64_MAX[g][1], (g, dt, dr)
            wt, wr = FAR_ERROR_TO_TRUTH[(obstacle_until, g)]
            assert abs(et - wt) <= 0.1 * wt and abs(er - wr) <= 0.1 * wr, (g, et, er)
    assert worst_t <= F32_VS_F64_MAX_TRANSLATION and worst_r <= F32_VS_F64_MAX_ROTATION, (worst_t, worst_r)


def reference_chain_rgbd(frames=CHAIN_FRAMES):
    """tests/test_track_api.reference_chain with colour: per-frame (metres, radians) error against the ground truth."""
    s = small_stream(yaw_deg_per_frame=2.0)
    po = oracle_map(s, upload_to=max(frames) + 1)
    last = np.asarray(s.pose(11), np.float64)
    errs = []
    for g in frames:
        rows, n = po.recon.surfels(), po.recon.surfels_size
        pred = last.astype(np.float32)
        D, M, Cm, P = trr.model_images(rows, n, vr.render, s.width, s.height, s.fx, s.fy, s.cx, s.cy, pred)
        po.preprocess(g, [], None)
        depth, normals = np.asarray(po.depth_final), np.asarray(po.normals).reshape(s.height, s.width, 2)
        out = trr.track(D, M, P, depth, normals, frame_color(s, g), (s.fx, s.fy, s.cx, s.cy), trr.Params(), s.depth_scaling)
        assert out["status"] < tr.TOO_FEW_INLIERS, (g, out["status"])
        est = tr.se3_mul(pred, out["T_rel"]).astype(np.float32)
        errs.append(tr.pose_difference(pose64(s, g), est))
        po.integrate(g, est)
        last = est.astype(np.float64)
    return s, errs


def test_reference_chain_rgbd(orc):
    """The chain's drift comes from tracked poses being baked into the map; the photometric term neither cures nor
    worsens it.  The GPU chain is held to CHAIN_FACTOR x this chain's running maximum."""
    s, errs = reference_chain_rgbd()
    run_t = np.maximum.accumulate([e[0] for e in errs])
    run_r = np.maximum.accumulate([e[1] for e in errs])
    print("rgbd chain errors (mm): " + " ".join("%.2f" % (e[0] * 1e3) for e in errs))
    print("rgbd chain errors (deg): " + " ".join("%.4f" % np.degrees(e[1]) for e in errs))
    print("RGBD_CHAIN_RUNNING_MAX_TRANSLATION = [" + ", ".join("%.3e" % v for v in run_t) + "]")
    print("RGBD_CHAIN_RUNNING_MAX_ROTATION = [" + ", ".join("%.3e" % v for v in run_r) + "]")
    # (the constants are the printed values: four significant digits, rounded to nearest)
    assert np.all(run_t <= np.asarray(RGBD_CHAIN_RUNNING_MAX_TRANSLATION) * 1.001)
    assert np.all(run_r <= np.asarray(RGBD_CHAIN_RUNNING_MAX_ROTATION) * 1.001)
    assert np.all(run_t >= np.asarray(RGBD_CHAIN_RUNNING_MAX_TRANSLATION) * 0.9), "the recorded constants are stale"
