"""The tracking kernels' own functions on the host, walked in the launch's order.  Test infrastructure shared by
tests/test_track_kernel_host.py, tests/test_track_rgbd_kernel_host.py and tests/test_track_cases.py, as tests/ray_host.py is
for the ray kernels.

smx_track.hpp (part 1) holds the per-pixel work, the accumulation, the grid rule, the solve and the end of a call as plain
inline functions.  The program below compiles them for the host with the project's -ffp-contract=off and drives them with the
structure of the launch: track_grid(n) workgroups of kTrackBlock lanes, every lane its own accumulators over its grid-stride
samples, the cross-lane shifts of a wavefront (a lane whose partner lies beyond the wavefront gets its own value back, as the
device's shift does), one row of `part` per wavefront added in wavefront order, one slab per workgroup at the stride of the
kernel in a buffer that is never cleared (it starts as NaNs: a slab read that no workgroup of this launch wrote would show),
the slabs added in index order, track_solve_step and, behind the last launch, track_finish.  What the .hip file adds around
these functions -- the two loops and the skip test -- is restated here; everything else is the header's code."""
import ctypes as C
import os
import subprocess

import numpy as np

import track_ref as tr
import track_rgbd_ref as trr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PROGRAM = r'''
#define SMX_TRACK_HOST_ONLY 1
#include <string.h>
#include "smx_track.hpp"
using namespace smx;

struct Frame { const uint16_t* depth; const float2* normals; const unsigned char* color; const float* D; const float4* M; const float4* P; };

// One reduce launch as a single lane that visits every sample in index order (no cross-lane sum to make): the slab.
template <bool kPhoto>
static void reduce_one_lane(const TrackK& k, const TrackPhotoK& ph, int stride, const float* T, const Frame& f, double* slab) {
  double acc[28] = {0.0}, acc_ee = 0.0;
  uint32_t n_in = 0, n_px = 0, n_as = 0, n_ph = 0;
  for (int i = 0; i < k.sw * k.sh; ++i) {
    const int sy = i / k.sw, sx = i - sy * k.sw;
    const int x = stride / 2 + sx * stride, y = stride / 2 + sy * stride;
    const size_t at = (size_t)y * k.W + x;
    track_pixel<kPhoto>(k, ph, T, x, y, f.depth[at], f.normals + at, kPhoto ? f.color + 3 * at : nullptr, f.D, f.M, f.P, acc,
                        acc_ee, n_in, n_px, n_as, n_ph);
  }
  for (int e = 0; e < 28; ++e) slab[e] = acc[e];
  slab[kSumInliers] = n_in; slab[kSumPixels] = n_px; slab[kSumAssociated] = n_as;
  if (kPhoto) { slab[kSumEE] = acc_ee; slab[kSumPhotoInliers] = n_ph; }
}

// The device's shift towards lane 0 over one wavefront's values.
template <typename V>
static void shfl_down_add(V* v, int off) {
  V got[64];
  for (int l = 0; l < 64; ++l) got[l] = l + off < 64 ? v[l + off] : v[l];
  for (int l = 0; l < 64; ++l) v[l] += got[l];
}

// One reduce launch with the launch's structure.  Returns the grid.
template <bool kPhoto>
static int reduce_launch(const TrackK& k, const TrackPhotoK& ph, int stride, const float* T, const Frame& f, double* slabs) {
  constexpr int kStride = kPhoto ? kTrackRgbdSlabStride : kTrackSlabStride;
  constexpr int kSums = kPhoto ? SMX_TRACK_RGBD_SUMS : SMX_TRACK_SUMS;
  const int n = k.sw * k.sh;
  const int grid = track_grid(n);
  for (int b = 0; b < grid; ++b) {
    static double acc[kTrackBlock][28], acc_ee[kTrackBlock];
    static uint32_t n_in[kTrackBlock], n_px[kTrackBlock], n_as[kTrackBlock], n_ph[kTrackBlock];
    for (int t = 0; t < kTrackBlock; ++t) {
      for (int e = 0; e < 28; ++e) acc[t][e] = 0.0;
      acc_ee[t] = 0.0; n_in[t] = n_px[t] = n_as[t] = n_ph[t] = 0;
      for (long long i = (long long)b * kTrackBlock + t; i < n; i += (long long)grid * kTrackBlock) {
        const int sy = (int)(i / k.sw), sx = (int)(i - (long long)sy * k.sw);
        const int x = stride / 2 + sx * stride, y = stride / 2 + sy * stride;
        const size_t at = (size_t)y * k.W + x;
        track_pixel<kPhoto>(k, ph, T, x, y, f.depth[at], f.normals + at, kPhoto ? f.color + 3 * at : nullptr, f.D, f.M, f.P,
                            acc[t], acc_ee[t], n_in[t], n_px[t], n_as[t], n_ph[t]);
      }
    }
    double part[kTrackBlock / 64][kStride];
    for (int wave = 0; wave < kTrackBlock / 64; ++wave) {
      const int t0 = 64 * wave;
      for (int e = 0; e < 28; ++e) {
        double v[64];
        for (int l = 0; l < 64; ++l) v[l] = acc[t0 + l][e];
        for (int off = 32; off > 0; off >>= 1) shfl_down_add(v, off);
        part[wave][e] = v[0];
      }
      for (int off = 32; off > 0; off >>= 1) {
        if (kPhoto) { shfl_down_add(acc_ee + t0, off); shfl_down_add(n_ph + t0, off); }
        shfl_down_add(n_in + t0, off); shfl_down_add(n_px + t0, off); shfl_down_add(n_as + t0, off);
      }
      part[wave][kSumInliers] = (double)n_in[t0]; part[wave][kSumPixels] = (double)n_px[t0];
      part[wave][kSumAssociated] = (double)n_as[t0];
      if (kPhoto) { part[wave][kSumEE] = acc_ee[t0]; part[wave][kSumPhotoInliers] = (double)n_ph[t0]; }
    }
    for (int e = 0; e < kSums; ++e) {
      double v = part[0][e];
      for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][e];
      slabs[(size_t)b * kStride + e] = v;
    }
  }
  return grid;
}

// k_track_solve's sum over the slabs.
static void sum_slabs(const double* slabs, int n_slabs, int photo, double* S) {
  const int stride = photo ? kTrackRgbdSlabStride : kTrackSlabStride;
  for (int e = 0; e < SMX_TRACK_RGBD_SUMS; ++e) {
    double v = 0.0;
    if (e < SMX_TRACK_SUMS || photo)
      for (int b = 0; b < n_slabs; ++b) v += slabs[(size_t)b * stride + e];
    S[e] = v;
  }
}

static TrackK reduce_k(int stride, int W, int H, const float* fp) {
  TrackK k; k.W = W; k.H = H; k.sw = track_samples(W, stride); k.sh = track_samples(H, stride);
  k.fx = fp[0]; k.fy = fp[1]; k.cx = fp[2]; k.cy = fp[3]; k.depth_scaling = fp[4]; k.max_distance_sq = fp[5]; k.cos_max_angle = fp[6];
  return k;
}

extern "C" void host_reduce(int stride, int W, int H, float fx, float fy, float cx, float cy, float ds, float maxd2,
                            float cosang, float weight, float maxe, float ming2, const uint16_t* depth, const float* normals,
                            const unsigned char* color, const float* D, const float* M, const float* P, const float* Tf,
                            double* slab) {
  const float fp[7] = {fx, fy, cx, cy, ds, maxd2, cosang};
  const TrackK k = reduce_k(stride, W, H, fp);
  TrackPhotoK ph; ph.weight = weight; ph.max_intensity_difference = maxe; ph.min_gradient_sq = ming2;
  const Frame f = {depth, (const float2*)normals, color, D, (const float4*)M, (const float4*)P};
  if (weight != 0.0f) reduce_one_lane<true>(k, ph, stride, Tf, f, slab);
  else reduce_one_lane<false>(k, ph, stride, Tf, f, slab);
}
extern "C" void host_prepare(int W, int H, float step, const float* D, const uint32_t* Cm, float* P) {
  for (long long i = 0; i < (long long)W * H; ++i) ((float4*)P)[i] = track_photo_pixel(W, H, step, D, Cm, i);
}
extern "C" int host_grid(long long n) { return track_grid(n); }
extern "C" int host_samples(int size, int stride) { return track_samples(size, stride); }

// One launch in the launch's order: the sums as k_track_solve adds them.  slabs: kTrackMaxSlabs * kTrackRgbdSlabStride.
extern "C" int walk_reduce(int stride, int W, int H, const float* fp, const uint16_t* depth, const float* normals,
                           const unsigned char* color, const float* D, const float* M, const float* P, const float* Tf,
                           double* slabs, double* S) {
  const TrackK k = reduce_k(stride, W, H, fp);
  TrackPhotoK ph; ph.weight = fp[7]; ph.max_intensity_difference = fp[8]; ph.min_gradient_sq = fp[9];
  const Frame f = {depth, (const float2*)normals, color, D, (const float4*)M, (const float4*)P};
  const int photo = P != nullptr;
  const int grid = photo ? reduce_launch<true>(k, ph, stride, Tf, f, slabs) : reduce_launch<false>(k, ph, stride, Tf, f, slabs);
  sum_slabs(slabs, grid, photo, S);
  return grid;
}

// A whole call: ip = W, H, stride[3], iterations[3], min_inliers, photo; fp = fx, fy, cx, cy, depth_scaling,
// max_distance^2, cos_max_angle, weight, max_intensity_difference, min_gradient^2; dp = min_inlier_fraction, min_pivot_ratio,
// convergence_rotation, convergence_translation, pred[12].  Tf_start (12 floats or null) replaces the identity the call
// starts from.  Returns the iterations run.
extern "C" int walk_call(const int* ip, const float* fp, const double* dp, const uint16_t* depth, const float* normals,
                         const unsigned char* color, const float* D, const float* M, const float* P, const float* Tf_start,
                         double* slabs, smx_track_rgbd_iteration* recs, smx_track_rgbd_result* res, double* T_rel) {
  static TrackDev st;
  memset(&st, 0xff, sizeof(st));
  for (int k = 0; k < 12; ++k) {   // k_track_begin
    const double v = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
    st.T_rel[k] = v; st.T_prev[k] = v; st.Tf[k] = (float)v;
  }
  st.status = SMX_TRACK_OK; st.iterations_run = 0; st.converged_level = -1;
  if (Tf_start) for (int k = 0; k < 12; ++k) { st.Tf[k] = Tf_start[k]; st.T_rel[k] = Tf_start[k]; st.T_prev[k] = Tf_start[k]; }
  const int W = ip[0], H = ip[1], photo = ip[9];
  TrackPhotoK ph; ph.weight = fp[7]; ph.max_intensity_difference = fp[8]; ph.min_gradient_sq = fp[9];
  const Frame f = {depth, (const float2*)normals, color, D, (const float4*)M, (const float4*)P};
  int last_level = -1;
  for (int l = 0; l < kTrackLevels; ++l) if (ip[5 + l] > 0) last_level = l;
  for (int l = 0; l < kTrackLevels; ++l) {
    const int stride = ip[2 + l], iters = ip[5 + l];
    if (iters <= 0) continue;
    const TrackK k = reduce_k(stride, W, H, fp);
    TrackSolveK sk;
    sk.level = l; sk.stride = stride; sk.n_slabs = track_grid((long long)k.sw * k.sh); sk.final_launch = 0;
    sk.min_inliers = ip[8]; sk.photo = photo;
    sk.min_inlier_fraction = dp[0]; sk.min_pivot_ratio = dp[1]; sk.convergence_rotation = dp[2]; sk.convergence_translation = dp[3];
    for (int i = 0; i < 12; ++i) sk.pred[i] = dp[4 + i];
    for (int it = 0; it < iters; ++it) {
      const bool skip = st.status >= SMX_TRACK_TOO_FEW_INLIERS || st.converged_level == l;
      if (!skip) {
        float T[12];
        for (int i = 0; i < 12; ++i) T[i] = st.Tf[i];
        if (photo) reduce_launch<true>(k, ph, stride, T, f, slabs); else reduce_launch<false>(k, ph, stride, T, f, slabs);
        double S[SMX_TRACK_RGBD_SUMS];
        sum_slabs(slabs, sk.n_slabs, photo, S);
        track_solve_step(S, sk, &st);
      }
      if (l == last_level && it == iters - 1) { sk.final_launch = 1; track_finish(sk, &st); }
    }
  }
  for (int i = 0; i < st.iterations_run && i < kTrackRing; ++i) recs[i] = st.ring[i];
  *res = st.result;
  for (int i = 0; i < 12; ++i) T_rel[i] = st.T_rel[i];
  return st.iterations_run;
}

static TrackSolveK solve_k(int photo, int min_inliers, double pivot, double cr, double ct) {
  TrackSolveK k; k.level = 0; k.stride = 1; k.n_slabs = 1; k.final_launch = 1; k.min_inliers = min_inliers; k.photo = photo;
  k.min_inlier_fraction = 0; k.min_pivot_ratio = pivot; k.convergence_rotation = cr; k.convergence_translation = ct;
  for (int i = 0; i < 12; ++i) k.pred[i] = (i == 0 || i == 5 || i == 10) ? 1.0 : 0.0;
  return k;
}
extern "C" int host_solve(const double* S, int min_inliers, double pivot, double cr, double ct, const float* Tf_in,
                          double* x, double* Tout) {
  static TrackDev st;
  const TrackSolveK k = solve_k(0, min_inliers, pivot, cr, ct);
  for (int i = 0; i < 12; ++i) { st.Tf[i] = Tf_in[i]; st.T_rel[i] = Tf_in[i]; }
  const int s = track_solve_one(S, k, &st, x);
  for (int i = 0; i < 12; ++i) Tout[i] = st.T_rel[i];
  return s;
}
// Lane 0 of one k_track_solve launch with colour (the final one of a call) on one slab; returns the status, fills the
// record and the result.
extern "C" int host_solve_rgbd(const double* slab, int min_inliers, double pivot, double cr, double ct, const float* Tf_in,
                               smx_track_rgbd_iteration* rec, smx_track_rgbd_result* res) {
  static TrackDev st;
  st.status = 0; st.converged_level = -1; st.iterations_run = 0;
  for (int i = 0; i < 12; ++i) { st.Tf[i] = Tf_in[i]; st.T_rel[i] = Tf_in[i]; st.T_prev[i] = Tf_in[i]; }
  const TrackSolveK k = solve_k(1, min_inliers, pivot, cr, ct);
  double S[SMX_TRACK_RGBD_SUMS];
  for (int i = 0; i < SMX_TRACK_RGBD_SUMS; ++i) S[i] = 0.0 + slab[i];
  track_solve_step(S, k, &st);
  track_finish(k, &st);
  *rec = st.ring[0]; *res = st.result;
  return st.status;
}
'''


def host_library(tmp_path):
    src = tmp_path / "track_host.cpp"
    src.write_text(PROGRAM)
    lib = tmp_path / "libtrack_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", SRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(lib))
    L.host_grid.argtypes = [C.c_longlong]
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def host_reduce(L, s, stride, gates, Tf, depth, normals, D, M, photo=None):
    """The 40-double slab of one reduce launch walked by a single lane; photo = (weight, max_intensity_difference,
    min_gradient_sq, color, P) or None for the geometric kernel.  s: anything with width, height, fx, fy, cx, cy,
    depth_scaling."""
    weight, maxe, ming2, color, P = photo if photo is not None else (0.0, 0.0, 0.0, None, None)
    slab = np.zeros(40)
    L.host_reduce(stride, s.width, s.height, C.c_float(s.fx), C.c_float(s.fy), C.c_float(s.cx), C.c_float(s.cy),
                  C.c_float(s.depth_scaling), C.c_float(gates[0]), C.c_float(gates[1]), C.c_float(weight), C.c_float(maxe),
                  C.c_float(ming2), ptr(depth), ptr(normals), ptr(color), ptr(D), ptr(M), ptr(P), ptr(Tf), ptr(slab))
    return slab


def _floats(intrinsics, depth_scaling, params, photo):
    g2, ca = params.gates()
    ph = (params.photometric_weight, params.max_intensity_difference, params.min_gradient_sq()) if photo else (0.0, 0.0, 0.0)
    return np.array(list(intrinsics) + [depth_scaling, g2, ca] + list(ph), np.float32)


def _images(depth, normals, color, D, M, P):
    c = np.ascontiguousarray
    return (c(depth, np.uint16), c(normals, np.float32), c(color, np.uint8) if color is not None else None, c(D, np.float32),
            c(M, np.float32), c(P, np.float32) if P is not None else None)


def new_slabs():
    return np.full(256 * 40, np.nan)


def walk_reduce(L, D, M, depth, normals, intrinsics, Tf, stride, params, depth_scaling, photo=None, slabs=None):
    """(sums [31 or 33], grid) of one launch walked in the launch's order; photo = (P, colour) runs track_pixel<true>."""
    H, W = depth.shape
    P, color = photo if photo is not None else (None, None)
    img = _images(depth, normals, color, D, M, P)
    fp = _floats(intrinsics, depth_scaling, params, photo is not None)
    slabs = new_slabs() if slabs is None else slabs
    S = np.zeros(trr.N_SUMS)
    Tf = np.ascontiguousarray(Tf, np.float32)
    grid = L.walk_reduce(stride, W, H, ptr(fp), ptr(img[0]), ptr(img[1]), ptr(img[2]), ptr(img[3]), ptr(img[4]), ptr(img[5]),
                         ptr(Tf), ptr(slabs), ptr(S))
    return S[:trr.N_SUMS if photo is not None else tr.N_SUMS].copy(), grid


def walk_call(L, D, M, depth, normals, intrinsics, pred, params, depth_scaling, photo=None, Tf_start=None, slabs=None):
    """A whole call walked on the host.  Returns (records, result dict, T_rel [3, 4] float64); photo = (P, colour) with a
    track_rgbd_ref.Params whose weight is not 0."""
    from surfelmeshing_amd._lib import TrackRGBDIteration, TrackRGBDResult
    H, W = depth.shape
    with_photo = photo is not None and params.photometric_weight != 0
    P, color = photo if with_photo else (None, None)
    img = _images(depth, normals, color, D, M, P)
    levels = list(params.levels) + [(1, 0)] * (3 - len(params.levels))
    ip = np.array([W, H] + [s for s, _ in levels] + [n for _, n in levels] + [params.min_inliers, int(with_photo)], np.int32)
    fp = _floats(intrinsics, depth_scaling, params, with_photo)
    dp = np.array([params.min_inlier_fraction, params.min_pivot_ratio, params.convergence_rotation, params.convergence_translation]
                  + list(np.asarray(pred, np.float32).astype(np.float64).reshape(12)), np.float64)
    recs, res, T = (TrackRGBDIteration * 96)(), TrackRGBDResult(), np.zeros(12)
    slabs = new_slabs() if slabs is None else slabs
    start = np.ascontiguousarray(Tf_start, np.float32) if Tf_start is not None else None
    n = L.walk_call(ptr(ip), ptr(fp), ptr(dp), ptr(img[0]), ptr(img[1]), ptr(img[2]), ptr(img[3]), ptr(img[4]), ptr(img[5]),
                    ptr(start), ptr(slabs), recs, C.byref(res), ptr(T))
    records = [{"level": r.level, "stride": r.stride, "status": r.status, "sums": np.array(r.sums, np.float64),
                "x": np.array(r.x, np.float64)} for r in recs[:n]]
    return records, result_fields(res), T.reshape(3, 4)


def result_fields(res):
    """The fields of a smx_track_rgbd_result (or of an api.TrackRGBDOutcome / TrackOutcome) by the names of
    track_exact.exact_call."""
    icp = getattr(res, "icp", res)
    return {"status": int(icp.status), "iterations_run": int(icp.iterations_run),
            "global_T_frame": np.array(icp.global_T_frame, np.float32).reshape(3, 4), "inliers": int(icp.inliers),
            "pixels_with_depth": int(icp.pixels_with_depth), "rms_residual": np.float32(icp.rms_residual),
            "last_update_rotation": np.float32(icp.last_update_rotation),
            "last_update_translation": np.float32(icp.last_update_translation),
            "information": np.array(icp.information, np.float32).reshape(6, 6),
            "photometric_inliers": int(getattr(res, "photometric_inliers", 0)),
            "rms_intensity_residual": np.float32(getattr(res, "rms_intensity_residual", 0.0))}


RESULT_FIELDS = ("status", "iterations_run", "global_T_frame", "inliers", "pixels_with_depth", "rms_residual",
                 "last_update_rotation", "last_update_translation", "information", "photometric_inliers", "rms_intensity_residual")


def same_result(got, want):
    """The names of the fields of two result dicts that differ in a bit."""
    bad = []
    for k in RESULT_FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype == np.float32:
            a, b = np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
        if not np.array_equal(a, b):
            bad.append(k)
    return bad
