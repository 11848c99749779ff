"""The arithmetic of the kernels of smx_recon_track_rgbd without a GPU, in the manner of tests/test_track_kernel_host.py:
k_track_photo_prepare, the body of k_track_reduce_rgbd and k_track_solve_rgbd are plain C++, compiled here for the host
(one lane per workgroup, cross-lane shifts that add nothing, -ffp-contract=off).  The prepare output must equal the float32
restatement of tests/track_rgbd_ref.py bit for bit; the 33 sums stay within the bound derived there and in
tests/test_gpu_track.py -- the comparison tests/test_gpu_track_rgbd.py makes on the device."""
import ctypes as C
import os
import subprocess

import numpy as np

import track_ref as tr
import track_rgbd_ref as trr
import viz_ref as vr
from common import ROOT, small_stream
from test_track_api import oracle_map
from test_track_kernel_host import PRELUDE, _ptr, _sum_bounds
from test_track_rgbd_api import frame_color

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PRELUDE_RGBD = PRELUDE + r'''
struct uchar3 { unsigned char x, y, z; };
static inline float4 make_float4(float x, float y, float z, float w) { float4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
'''

HARNESS = r'''
extern "C" void host_prepare(int W, int H, float step, const float* D, const uint32_t* Cm, float* P) {
  threadIdx.x = 0;
  for (unsigned i = 0; i < (unsigned)(W * H); ++i) { blockIdx.x = i; k_track_photo_prepare(W, H, step, D, Cm, (float4*)P); }
  blockIdx.x = 0;
}
extern "C" void host_reduce_rgbd(int stride, int W, int H, float fx, float fy, float cx, float cy, float ds, float maxd2,
                                 float cosang, float weight, float maxe, float ming2, uint16_t* depth, float* normals,
                                 unsigned char* color, const float* D, const float* M, const float* P, const float* Tf,
                                 double* slab) {
  static TrackDev st; st.status = 0; st.converged_level = -1;
  for (int i = 0; i < 12; ++i) st.Tf[i] = Tf[i];
  TrackK k; k.W = W; k.H = H; const int s = stride;
  k.sw = W > s / 2 ? (W - s / 2 + s - 1) / s : 0; k.sh = H > s / 2 ? (H - s / 2 + s - 1) / s : 0;
  k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy; k.depth_scaling = ds; k.max_distance_sq = maxd2; k.cos_max_angle = cosang;
  TrackPhotoK ph; ph.weight = weight; ph.max_intensity_difference = maxe; ph.min_gradient_sq = ming2;
  Img<uint16_t> d{depth, H, W, (size_t)W * 2}; Img<float2> n{(float2*)normals, H, W, (size_t)W * 8};
  Img<uchar3> c{(uchar3*)color, H, W, (size_t)W * 3};
  for (unsigned j = 0; j < SMX_TRACK_RGBD_SUMS; ++j) {   // (as lane j the kernel stores entry j of what lane 0 left in LDS)
    threadIdx.x = j;
    if (s == 1) k_track_reduce_rgbd<1>(k, ph, d, n, c, D, (const float4*)M, (const float4*)P, &st, 0, slab);
    else if (s == 2) k_track_reduce_rgbd<2>(k, ph, d, n, c, D, (const float4*)M, (const float4*)P, &st, 0, slab);
    else if (s == 4) k_track_reduce_rgbd<4>(k, ph, d, n, c, D, (const float4*)M, (const float4*)P, &st, 0, slab);
    else k_track_reduce_rgbd<8>(k, ph, d, n, c, D, (const float4*)M, (const float4*)P, &st, 0, slab);
  }
  threadIdx.x = 0;
}
// One k_track_solve_rgbd launch (the final one of a call) on one slab; returns the status, fills the record and the result.
extern "C" int host_solve_rgbd(const double* slab, int min_inliers, double pivot, double cr, double ct, const float* Tf_in,
                               smx_track_rgbd_iteration* rec, smx_track_rgbd_result* res) {
  static TrackDev st; static TrackRgbdDev rst;
  st.status = 0; st.converged_level = -1; st.iterations_run = 0;
  for (int i = 0; i < 12; ++i) { st.Tf[i] = Tf_in[i]; st.T_rel[i] = Tf_in[i]; st.T_prev[i] = Tf_in[i]; }
  TrackSolveK k; k.level = 0; k.stride = 1; k.n_slabs = 1; k.final_launch = 1; k.min_inliers = min_inliers;
  k.min_inlier_fraction = 0; k.min_pivot_ratio = pivot; k.convergence_rotation = cr; k.convergence_translation = ct;
  for (int i = 0; i < 12; ++i) k.pred[i] = (i == 0 || i == 5 || i == 10) ? 1.0 : 0.0;
  for (int j = SMX_TRACK_RGBD_SUMS - 1; j >= 0; --j) { threadIdx.x = (unsigned)j; k_track_solve_rgbd(k, slab, &st, &rst, res); }
  *rec = rst.ring[0];
  return st.status;
}
'''


def _host_library(tmp_path):
    hip = open(os.path.join(SRC, "smx_track.hip")).read()
    hpp = open(os.path.join(SRC, "smx_track.hpp")).read()
    state = hpp[hpp.index("struct TrackDev {"):hpp.index("struct TrackBuffers")]
    state += hpp[hpp.index("constexpr int kTrackRgbdSlabStride"):hpp.index("struct TrackRgbdBuffers")]
    kernels = hip[hip.index("struct TrackK {"):hip.index("template <int STRIDE>\nvoid launch_reduce_rgbd")]
    kernels = kernels.replace("kTrackBlock / 64", "1")      # (one wavefront row of LDS)
    for name in ("k_track_photo_prepare", "k_track_reduce_rgbd", "k_track_solve_rgbd", "track_solve_one"):
        assert name in kernels, name
    src = tmp_path / "track_rgbd_host.cpp"
    src.write_text(PRELUDE_RGBD + state + kernels + HARNESS)
    lib = tmp_path / "libtrack_rgbd_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


def test_rgbd_kernel_arithmetic_on_the_host_matches_the_restatement(orc, tmp_path):
    from surfelmeshing_amd._lib import TrackRGBDIteration, TrackRGBDResult
    L = _host_library(tmp_path)
    s = small_stream(yaw_deg_per_frame=2.0, obstacle_until=8)
    po = oracle_map(s)
    rows, n = po.recon.surfels(), po.recon.surfels_size
    p = trr.Params()
    D, M, Cm, P = trr.model_images(rows, n, vr.render, s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.pose(11), p)
    D, M, Cm = np.ascontiguousarray(D), np.ascontiguousarray(M), np.ascontiguousarray(Cm)
    # the prepare kernel: bit for bit, on a map with empty pixels and depth steps
    got = np.full((s.height, s.width, 4), 7.0, np.float32)
    L.host_prepare(s.width, s.height, C.c_float(p.gradient_max_relative_depth_step), _ptr(D), _ptr(Cm), _ptr(got))
    assert np.array_equal(got.view(np.uint32), P.view(np.uint32))
    valid = P[..., 3] != 0
    assert (~valid[1:-1, 1:-1] & (D[1:-1, 1:-1] > 0)).sum() > 50 and valid.sum() > 0.3 * valid.size
    P = np.ascontiguousarray(P)
    g2, ca = p.gates()
    intr = (s.fx, s.fy, s.cx, s.cy)
    for g in (12, 16):
        po.preprocess(g, [], None)
        depth = np.ascontiguousarray(po.depth_final, np.uint16)
        normals = np.ascontiguousarray(np.asarray(po.normals).reshape(s.height, s.width, 2), np.float32)
        color = frame_color(s, g)
        T1 = tr.se3_exp([0.001, 0.027 * (g - 11), 0.0005, 0.003, -0.002, 0.004])
        for T in (tr.IDENTITY, T1):
            for stride in (1, 2, 4):
                Tf = np.ascontiguousarray(T, np.float32)

                def reduce(weight, photo):
                    slab = np.zeros(40)
                    L.host_reduce_rgbd(stride, s.width, s.height, C.c_float(s.fx), C.c_float(s.fy), C.c_float(s.cx),
                                       C.c_float(s.cy), C.c_float(s.depth_scaling), C.c_float(g2), C.c_float(ca),
                                       C.c_float(weight), C.c_float(p.max_intensity_difference),
                                       C.c_float(p.min_gradient_sq()), _ptr(depth), _ptr(normals), _ptr(color), _ptr(D),
                                       _ptr(M), _ptr(P) if photo else None, _ptr(Tf), _ptr(slab))
                    return slab
                want, mg = trr.iteration(D, M, P, depth, normals, color, intr, T, stride, p, s.depth_scaling)
                slab = reduce(p.photometric_weight, True)
                pix, fl = want[tr.S_PIXELS], mg["flagged"]
                assert fl <= 0.01 * pix and slab[tr.S_PIXELS] == pix and mg["photo"]["inliers"] > 20
                for e in (tr.S_ASSOCIATED, tr.S_INLIERS, trr.S_PHOTO_INLIERS):
                    assert abs(slab[e] - want[e]) <= fl, (g, stride, e)
                diff, bound = trr.compare_sums(slab, want, mg, p, _sum_bounds)
                assert np.all(diff <= bound), (g, stride, int(np.argmax(diff / bound)), float((diff / bound).max()))
                # the term is there: the same bound would not cover leaving it out
                geo = reduce(0.0, False)
                assert np.all(geo[31:33] == 0) and np.any(np.abs(geo[:28] - want[:28]) > bound[:28])
                # the solve: status, twist, record and result from the kernel's own sums against the restatement's solve
                status, x, Tn = trr.solve(slab[:33], T, p)
                rec, res = TrackRGBDIteration(), TrackRGBDResult()
                st = L.host_solve_rgbd(_ptr(slab), p.min_inliers, C.c_double(p.min_pivot_ratio),
                                       C.c_double(p.convergence_rotation), C.c_double(p.convergence_translation), _ptr(Tf),
                                       C.byref(rec), C.byref(res))
                assert st == status == rec.status == res.icp.status and status in (tr.OK, tr.CONVERGED)
                assert np.array_equal(np.array(rec.sums), slab[:33])
                assert np.allclose(np.array(rec.x), x, rtol=1e-9, atol=1e-15)
                assert np.allclose(np.array(res.icp.global_T_frame).reshape(3, 4), Tn, rtol=0, atol=1e-6)
                assert res.photometric_inliers == slab[32] and res.icp.inliers == slab[tr.S_INLIERS]
                assert abs(res.rms_intensity_residual - np.sqrt(slab[31] / slab[32])) < 1e-6
    # weight 0 (P == nullptr) leaves the geometric sums: the restatement's, within the geometric bound alone
    _, _, _, inl, pix, mg0 = tr.iteration(D, M, depth, normals, intr, T1, 4, p.gates(), s.depth_scaling)
    assert np.all(np.abs(geo[:28] - mg0["sums"][:28]) <= _sum_bounds(inl, mg0["flagged"], max(mg0["p_max"], 1.0), p.max_distance))
    # a non-finite photometric sum is NOT_FINITE before anything is solved
    bad = slab.copy()
    bad[31] = np.nan
    rec, res = TrackRGBDIteration(), TrackRGBDResult()
    assert L.host_solve_rgbd(_ptr(bad), 50, C.c_double(1e-6), C.c_double(1e-5), C.c_double(1e-5), _ptr(Tf), C.byref(rec),
                             C.byref(res)) == tr.NOT_FINITE
    assert np.all(np.array(rec.x) == 0) and res.icp.status == tr.NOT_FINITE
