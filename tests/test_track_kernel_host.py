"""The arithmetic of smx_track.hip without a GPU: smx_track.hpp holds the per-pixel work, the accumulation order, the solve
and the exponential as plain inline functions, so this test compiles them for the host with the project's
-ffp-contract=off, drives them the way k_track_reduce / k_track_solve do (one lane that visits every sampled pixel in index
order, so the cross-lane sums have nothing to add) and compares them with the float64 restatement of tests/track_ref.py on
the oracle's map -- the same comparison tests/test_gpu_track.py makes on the device, with the same derived bound."""
import ctypes as C
import os
import subprocess

import numpy as np

import track_ref as tr
import viz_ref as vr
from common import ROOT, small_stream
from test_track_api import oracle_map

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")
U = 2.0 ** -24

HARNESS = r'''
#define SMX_TRACK_HOST_ONLY 1
#include "smx_track.hpp"
using namespace smx;

// One reduce launch as a single lane: slab = the 28 float sums, the three counts, sum e^2, the photometric inliers.  As
// track_enqueue, weight 0 (or no colour at all) runs the instantiation without the photometric term.
template <bool kPhoto>
static void reduce(const TrackK& k, const TrackPhotoK& ph, int stride, const float* T, const uint16_t* depth,
                   const float2* normals, const unsigned char* color, const float* D, const float4* M, const float4* P,
                   double* slab) {
  double acc[28] = {0.0}, acc_ee = 0.0;
  uint32_t n_in = 0, n_px = 0, n_as = 0, n_ph = 0;
  for (int i = 0; i < k.sw * k.sh; ++i) {
    const int sy = i / k.sw, sx = i - sy * k.sw;
    const int x = stride / 2 + sx * stride, y = stride / 2 + sy * stride;
    const size_t at = (size_t)y * k.W + x;
    track_pixel<kPhoto>(k, ph, T, x, y, depth[at], normals + at, kPhoto ? color + 3 * at : nullptr, D, M, P, acc, acc_ee,
                        n_in, n_px, n_as, n_ph);
  }
  for (int e = 0; e < 28; ++e) slab[e] = acc[e];
  slab[kSumInliers] = n_in; slab[kSumPixels] = n_px; slab[kSumAssociated] = n_as;
  if (kPhoto) { slab[kSumEE] = acc_ee; slab[kSumPhotoInliers] = n_ph; }
}
extern "C" void host_reduce(int stride, int W, int H, float fx, float fy, float cx, float cy, float ds, float maxd2,
                            float cosang, float weight, float maxe, float ming2, const uint16_t* depth, const float* normals,
                            const unsigned char* color, const float* D, const float* M, const float* P, const float* Tf,
                            double* slab) {
  TrackK k; k.W = W; k.H = H; k.sw = track_samples(W, stride); k.sh = track_samples(H, stride);
  k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy; k.depth_scaling = ds; k.max_distance_sq = maxd2; k.cos_max_angle = cosang;
  TrackPhotoK ph; ph.weight = weight; ph.max_intensity_difference = maxe; ph.min_gradient_sq = ming2;
  if (weight != 0.0f) reduce<true>(k, ph, stride, Tf, depth, (const float2*)normals, color, D, (const float4*)M, (const float4*)P, slab);
  else reduce<false>(k, ph, stride, Tf, depth, (const float2*)normals, nullptr, D, (const float4*)M, nullptr, slab);
}
extern "C" void host_prepare(int W, int H, float step, const float* D, const uint32_t* Cm, float* P) {
  for (long long i = 0; i < (long long)W * H; ++i) ((float4*)P)[i] = track_photo_pixel(W, H, step, D, Cm, i);
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


def _host_library(tmp_path):
    src = tmp_path / "track_host.cpp"
    src.write_text(HARNESS)
    lib = tmp_path / "libtrack_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", SRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


def host_reduce(L, s, stride, gates, Tf, depth, normals, D, M, photo=None):
    """The 40-double slab of one reduce launch on the host; photo = (weight, max_intensity_difference, min_gradient_sq,
    color, P) or None for the geometric kernel."""
    weight, maxe, ming2, color, P = photo if photo is not None else (0.0, 0.0, 0.0, None, None)
    slab = np.zeros(40)
    L.host_reduce(stride, s.width, s.height, C.c_float(s.fx), C.c_float(s.fy), C.c_float(s.cx), C.c_float(s.cy),
                  C.c_float(s.depth_scaling), C.c_float(gates[0]), C.c_float(gates[1]), C.c_float(weight), C.c_float(maxe),
                  C.c_float(ming2), _ptr(depth), _ptr(normals), _ptr(color) if color is not None else None, _ptr(D), _ptr(M),
                  _ptr(P) if P is not None else None, _ptr(Tf), _ptr(slab))
    return slab


def _sum_bounds(inliers, flagged, B, max_distance):
    """The bound of tests/test_gpu_track.py::_sum_bounds (derived there)."""
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


# Per stride: the inlier floor under which the comparison would mean little, the floor of photometric inliers (for
# tests/test_track_rgbd_kernel_host.py), and the min_inliers the solve is asked with.  Stride 8 leaves 20 x 15 samples of the
# 160x120 frame, a quarter of stride 4's, and the restatement finds 23 to 132 inliers among them: too few for the default
# min_inliers of 50, so stride 8 runs with the floors tests/test_gpu_track.py and tests/test_gpu_track_rgbd.py use for all
# their strides (min_inliers = 10, inliers >= min_inliers, photometric inliers > 0).
FLOORS = {1: (90, 20, 50), 2: (90, 20, 50), 4: (90, 20, 50), 8: (10, 0, 10)}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_kernel_arithmetic_on_the_host_matches_the_restatement(orc, tmp_path):
    L = _host_library(tmp_path)
    s = small_stream(yaw_deg_per_frame=2.0, obstacle_until=8)
    po = oracle_map(s)
    rows, n = po.recon.surfels(), po.recon.surfels_size
    D, M = tr.model_images(rows, n, vr.render, s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.pose(11))
    D, M = np.ascontiguousarray(D), np.ascontiguousarray(M)
    p = tr.Params()
    g2, ca = p.gates()
    intr = (s.fx, s.fy, s.cx, s.cy)
    for g in (12, 16):
        po.preprocess(g, [], None)
        depth = np.ascontiguousarray(po.depth_final, np.uint16)
        normals = np.ascontiguousarray(np.asarray(po.normals).reshape(s.height, s.width, 2), np.float32)
        T1 = tr.se3_exp([0.001, 0.027 * (g - 11), 0.0005, 0.003, -0.002, 0.004])
        for T in (tr.IDENTITY, T1):
            for stride in (1, 2, 4, 8):
                _, _, _, inl, pix, mg = tr.iteration(D, M, depth, normals, intr, T, stride, p.gates(), s.depth_scaling)
                Tf = np.ascontiguousarray(T, np.float32)
                slab = host_reduce(L, s, stride, (g2, ca), Tf, depth, normals, D, M)
                assert inl >= FLOORS[stride][0] and mg["flagged"] <= 0.01 * pix
                assert slab[tr.S_PIXELS] == pix
                assert abs(slab[tr.S_ASSOCIATED] - mg["associated"]) <= mg["flagged"]
                assert abs(slab[tr.S_INLIERS] - inl) <= mg["flagged"]
                bound = _sum_bounds(inl, mg["flagged"], max(mg["p_max"], 1.0), p.max_distance)
                assert np.all(np.abs(slab[:28] - mg["sums"][:28]) <= bound), (g, stride)
                # the solve: status, twist and new pose against the restatement's, from the same sums
                p.min_inliers = FLOORS[stride][2]
                status, x, Tn = tr.solve(mg["sums"], T, p)
                S = (C.c_double * 31)(*mg["sums"])
                xo, To = (C.c_double * 6)(), (C.c_double * 12)()
                got = L.host_solve(S, p.min_inliers, C.c_double(p.min_pivot_ratio), C.c_double(p.convergence_rotation),
                                   C.c_double(p.convergence_translation), _ptr(Tf), xo, To)
                assert got == status and status in (tr.OK, tr.CONVERGED)
                assert np.allclose(np.array(xo), x, rtol=1e-9, atol=1e-15)
                assert np.allclose(np.array(To).reshape(3, 4), Tn, rtol=0, atol=1e-14)
    # the statuses that need no image
    Tf = np.ascontiguousarray(tr.IDENTITY, np.float32)
    xo, To = (C.c_double * 6)(), (C.c_double * 12)()

    def status_of(sums):
        return L.host_solve((C.c_double * 31)(*sums), 50, C.c_double(1e-6), C.c_double(1e-5), C.c_double(1e-5), _ptr(Tf), xo, To)
    z = np.zeros(31)
    z[tr.S_PIXELS] = 100
    assert status_of(z) == tr.DEGENERATE            # pixels with depth, nothing associated: an empty render
    z[tr.S_ASSOCIATED] = 100
    assert status_of(z) == tr.TOO_FEW_INLIERS
    z[3] = np.nan
    assert status_of(z) == tr.NOT_FINITE
    assert np.all(np.array(xo) == 0)
