"""The arithmetic of smx_track.hip without a GPU: the body of k_track_reduce and the solve / exponential code are plain
C++, so this test compiles them for the host (one lane per workgroup, cross-lane shifts that add nothing, the project's
-ffp-contract=off) and compares them with the float64 restatement of tests/track_ref.py on the oracle's map -- the same
comparison tests/test_gpu_track.py makes on the device, with the same derived bound."""
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

PRELUDE = r'''
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "smx.h"
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __shared__ static
#define __syncthreads()
#define __launch_bounds__(x)
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
struct Idx { unsigned x; };
static Idx blockIdx{0}, threadIdx{0}, gridDim{1};
template <typename T> static T __shfl_down(T, int, int) { return T(0); }   // (the other lanes hold nothing)
constexpr int kTrackRing = 96, kTrackBlock = 1, kTrackSlabStride = 32;   // (one lane visits every pixel)
enum { kSumRR = 27, kSumInliers = 28, kSumPixels = 29, kSumAssociated = 30 };
template <typename T> struct Img {
  T* address; int32_t height; int32_t width; size_t pitch;
  T& operator()(int y, int x) const {
    return *reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(address) + (size_t)y * pitch + (size_t)x * sizeof(T)); }
};
'''

HARNESS = r'''
extern "C" void host_reduce(int stride, int W, int H, float fx, float fy, float cx, float cy, float ds, float maxd2,
                            float cosang, uint16_t* depth, float* normals, const float* D, const float* M, const float* Tf,
                            double* slab) {
  static TrackDev st; st.status = 0; st.converged_level = -1;
  for (int i = 0; i < 12; ++i) st.Tf[i] = Tf[i];
  TrackK k; k.W = W; k.H = H; const int s = stride;
  k.sw = W > s / 2 ? (W - s / 2 + s - 1) / s : 0; k.sh = H > s / 2 ? (H - s / 2 + s - 1) / s : 0;
  k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy; k.depth_scaling = ds; k.max_distance_sq = maxd2; k.cos_max_angle = cosang;
  Img<uint16_t> d{depth, H, W, (size_t)W * 2}; Img<float2> n{(float2*)normals, H, W, (size_t)W * 8};
  // lane 0 visits every pixel and leaves the sums in the (static) LDS row; run as lane j, the kernel stores entry j
  for (unsigned j = 0; j < SMX_TRACK_SUMS; ++j) {
    threadIdx.x = j;
    if (s == 1) k_track_reduce<1>(k, d, n, D, (const float4*)M, &st, 0, slab);
    else if (s == 2) k_track_reduce<2>(k, d, n, D, (const float4*)M, &st, 0, slab);
    else if (s == 4) k_track_reduce<4>(k, d, n, D, (const float4*)M, &st, 0, slab);
    else k_track_reduce<8>(k, d, n, D, (const float4*)M, &st, 0, slab);
  }
}
extern "C" int host_solve(const double* S, int min_inliers, double pivot, double cr, double ct, const float* Tf_in,
                          double* x, double* Tout) {
  static TrackDev st; TrackSolveK k; k.min_inliers = min_inliers; k.min_inlier_fraction = 0; k.min_pivot_ratio = pivot;
  k.convergence_rotation = cr; k.convergence_translation = ct;
  for (int i = 0; i < 12; ++i) { st.Tf[i] = Tf_in[i]; st.T_rel[i] = Tf_in[i]; }
  const int s = track_solve_one(S, k, &st, x);
  for (int i = 0; i < 12; ++i) Tout[i] = st.T_rel[i];
  return s;
}
'''


def _host_library(tmp_path):
    hip = open(os.path.join(SRC, "smx_track.hip")).read()
    hpp = open(os.path.join(SRC, "smx_track.hpp")).read()
    state = hpp[hpp.index("struct TrackDev {"):hpp.index("struct TrackBuffers")]
    kernels = hip[hip.index("struct TrackK {"):hip.index("__global__ void __launch_bounds__(64)")]
    kernels = kernels.replace("kTrackBlock / 64", "1")      # (one wavefront row of LDS)
    assert "k_track_reduce" in kernels and "track_solve_one" in kernels and "se3_exp" in kernels
    src = tmp_path / "track_host.cpp"
    src.write_text(PRELUDE + state + kernels + HARNESS)
    lib = tmp_path / "libtrack_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


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
            for stride in (1, 2, 4):
                _, _, _, inl, pix, mg = tr.iteration(D, M, depth, normals, intr, T, stride, p.gates(), s.depth_scaling)
                slab = np.zeros(32)
                Tf = np.ascontiguousarray(T, np.float32)
                L.host_reduce(stride, s.width, s.height, C.c_float(s.fx), C.c_float(s.fy), C.c_float(s.cx),
                              C.c_float(s.cy), C.c_float(s.depth_scaling), C.c_float(g2), C.c_float(ca), _ptr(depth),
                              _ptr(normals), _ptr(D), _ptr(M), _ptr(Tf), _ptr(slab))
                assert inl >= 90 and mg["flagged"] <= 0.01 * pix
                assert slab[tr.S_PIXELS] == pix
                assert abs(slab[tr.S_ASSOCIATED] - mg["associated"]) <= mg["flagged"]
                assert abs(slab[tr.S_INLIERS] - inl) <= mg["flagged"]
                bound = _sum_bounds(inl, mg["flagged"], max(mg["p_max"], 1.0), p.max_distance)
                assert np.all(np.abs(slab[:28] - mg["sums"][:28]) <= bound), (g, stride)
                # the solve: status, twist and new pose against the restatement's, from the same sums
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
