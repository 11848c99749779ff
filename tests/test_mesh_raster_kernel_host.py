"""The arithmetic of smx_mesh_raster.hip without a GPU: smx_mesh_raster.hpp holds vertex set-up, triangle set-up with its
verdict and box, coverage, depth and key, the tile test and the resolve's normal and colour as plain inline functions, so this
test compiles them for the host with the project's -ffp-contract=off and walks the three passes of the kernels one "lane"
after the other -- triangles, then the list of large ones in 8 x 8 tiles, then pixels -- in ascending and in descending order.
Images and counters have to equal the model of tests/mesh_raster_ref.py byte for byte, as on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_raster_ref as rr
import mesh_ref as mr
import viz_ref as vr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

HARNESS = r'''
#define SMX_MESH_RASTER_HOST_ONLY 1
#include "smx_mesh_raster.hpp"
#include <vector>
using namespace smx;

struct Map { int n; const float* S; const float* N; };   // S: [n][4] smooth x y z -, N: [n][4] normal x y z, RadiusSquared

static MrVertex corner(const MrCam& cam, const Map& m, uint32_t i) { return mr_vertex(cam, m.S[4 * (size_t)i], m.S[4 * (size_t)i + 1], m.S[4 * (size_t)i + 2]); }

static int setup(const MrCam& cam, const Map& m, const uint32_t* tri, uint32_t t, MrTri* T) {
  const uint32_t a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
  if (a >= (uint32_t)m.n || b >= (uint32_t)m.n || c >= (uint32_t)m.n) return kMrOutOfRange;
  for (uint32_t i : {a, b, c})
    if (!mr_live(m.S[4 * (size_t)i], m.S[4 * (size_t)i + 1], m.S[4 * (size_t)i + 2], m.N[4 * (size_t)i + 3])) return kMrNotLive;
  return mr_setup(cam, corner(cam, m, a), corner(cam, m, b), corner(cam, m, c), T);
}

static void zmin(std::vector<unsigned long long>& z, size_t at, unsigned long long key) { if (key < z[at]) z[at] = key; }

// global_T_camera [12] float, intr: fx fy cx cy near far (float); col: the vis_color word of every slot.
// counters: the kMrWords of the device.  reverse != 0 walks every pass's lanes downwards.
extern "C" void host_render_mesh(int n, const float* S, const float* N, const uint32_t* col, const uint32_t* tri, int n_tri,
                                 const float* pose, const float* intr, int W, int H, int cull, int mode, int reverse,
                                 float* depth, uint32_t* index, float* normal, uint32_t* color, uint32_t* counters) {
  MrCam cam;
  mr_invert_pose(pose, cam.L);
  cam.fx = intr[0]; cam.fy = intr[1]; cam.cx = intr[2]; cam.cy = intr[3]; cam.near_z = intr[4]; cam.far_z = intr[5];
  cam.W = W; cam.H = H; cam.cull_back_faces = cull; cam.normal_mode = mode;
  const Map m{n, S, N};
  for (int k = 0; k < kMrWords; ++k) counters[k] = 0;
  std::vector<unsigned long long> z((size_t)W * H, ~0ull);
  std::vector<uint32_t> list;
  auto lane = [&](int i, int count) { return reverse ? count - 1 - i : i; };
  // k_mrast_small
  for (int l = 0; l < n_tri; ++l) {
    const uint32_t t = (uint32_t)lane(l, n_tri);
    MrTri T;
    const int verdict = setup(cam, m, tri, t, &T);
    if (verdict <= kMrCulled) ++counters[verdict];
    if (verdict == kMrDrawn || verdict == kMrLarge) ++counters[kMrDrawn];
    if (verdict == kMrLarge) { ++counters[kMrLarge]; list.push_back(t); }
    if (verdict != kMrDrawn) continue;
    for (int y = T.y0; y <= T.y1; ++y)
      for (int x = T.x0; x <= T.x1; ++x) {
        const MrW w = mr_weights(T, x, y);
        if (mr_covered(T, w)) zmin(z, (size_t)y * W + x, mr_key(mr_persp(T, w).Z, t));
      }
  }
  counters[kMrListLen] = (uint32_t)list.size();
  // k_mrast_large
  for (size_t j = 0; j < list.size(); ++j) {
    const uint32_t t = list[j];
    MrTri T;
    if (setup(cam, m, tri, t, &T) != kMrLarge) { counters[kMrListLen] = 0xDEAD; continue; }
    for (int ty = T.y0 & ~7; ty <= T.y1; ty += 8)
      for (int tx = T.x0 & ~7; tx <= T.x1; tx += 8) {
        const int ax = tx > T.x0 ? tx : T.x0, bx = tx + 7 < T.x1 ? tx + 7 : T.x1, ay = ty > T.y0 ? ty : T.y0, by = ty + 7 < T.y1 ? ty + 7 : T.y1;
        if (mr_tile_outside(T, ax, ay, bx, by)) continue;
        for (int l = 0; l < 64; ++l) {
          const int x = tx + (lane(l, 64) & 7), y = ty + (lane(l, 64) >> 3);
          if (x < ax || x > bx || y < ay || y > by) continue;
          const MrW w = mr_weights(T, x, y);
          if (mr_covered(T, w)) zmin(z, (size_t)y * W + x, mr_key(mr_persp(T, w).Z, t));
        }
      }
  }
  // k_mrast_resolve
  for (int l = 0; l < W * H; ++l) {
    const int at = lane(l, W * H), x = at % W, y = at / W;
    const unsigned long long key = z[at];
    depth[at] = 0.0f; index[at] = 0xFFFFFFFFu; color[at] = 0u;
    for (int k = 0; k < 4; ++k) normal[4 * (size_t)at + k] = 0.0f;
    if (key == ~0ull) continue;
    ++counters[kMrCovered];
    const uint32_t t = (uint32_t)key, bits = (uint32_t)(key >> 32);
    __builtin_memcpy(&depth[at], &bits, 4);
    index[at] = t;
    const uint32_t a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
    const MrVertex va = corner(cam, m, a), vb = corner(cam, m, b), vc = corner(cam, m, c);
    MrTri T;
    (void)mr_setup(cam, va, vb, vc, &T);
    const MrPersp p = mr_persp(T, mr_weights(T, x, y));
    if (mode == SMX_MESH_NORMAL_FACE) {
      mr_normal_face(va, vb, vc, &normal[4 * (size_t)at]);
    } else {
      const float *na = N + 4 * (size_t)a, *nb = N + 4 * (size_t)b, *nc = N + 4 * (size_t)c;
      mr_normal_vertex(p, mr_rotate(cam, na[0], na[1], na[2]), mr_rotate(cam, nb[0], nb[1], nb[2]), mr_rotate(cam, nc[0], nc[1], nc[2]),
                       &normal[4 * (size_t)at]);
    }
    color[at] = mr_color(p, col[a], col[b], col[c]);
  }
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_raster_host")
    src = d / "mesh_raster_host.cpp"
    src.write_text(HARNESS)
    lib = d / "libmesh_raster_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", SRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_render(L, rows, n, tri, width, height, fx, fy, cx, cy, global_T_camera, near_z=0.05, far_z=1000.0, cull_back_faces=False,
                normal_mode=0, color_flags=0, frame_index=0, window=0, reverse=0):
    S, N = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    S[:, :3], N[:, :3], N[:, 3] = rows[3:6, :n].T, rows[8:11, :n].T, rows[7, :n]
    col = np.ascontiguousarray(vr.vis_color(rows, np.arange(n), color_flags, frame_index, window), np.uint32)
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    pose = np.ascontiguousarray(global_T_camera, np.float32).reshape(12)
    intr = np.array([fx, fy, cx, cy, near_z, far_z], np.float32)
    W, H = width, height
    depth, index = np.empty((H, W), np.float32), np.empty((H, W), np.uint32)
    normal, color, cnt = np.empty((H, W, 4), np.float32), np.empty((H, W), np.uint32), np.zeros(12, np.uint32)
    L.host_render_mesh(n, _ptr(S), _ptr(N), _ptr(col), _ptr(t), t.shape[0], _ptr(pose), _ptr(intr), W, H, int(cull_back_faces),
                       normal_mode, reverse, _ptr(depth), _ptr(index), _ptr(normal), _ptr(color), _ptr(cnt))
    st = dict(zip(rr.STAT_KEYS, [t.shape[0]] + [int(v) for v in cnt[:8]]))
    assert int(cnt[8]) == st["n_large"]                  # the list's length
    return {"depth": depth, "index": index, "normal": normal, "color": color.view(np.uint8).reshape(H, W, 4), "stats": st}


def _compare(L, rows, tri, cam, what, **opts):
    n = rows.shape[1]
    want = rr.render_mesh(rows, n, tri, **cam, **opts)
    for reverse in (0, 1):
        got = host_render(L, rows, n, tri, reverse=reverse, **cam, **opts)
        print("%s %s, lanes %s: %s" % (what, opts, "downwards" if reverse else "upwards", got["stats"]))
        assert got["stats"] == want["stats"]
        for k in ("depth", "index", "normal", "color"):
            assert got[k].tobytes() == want[k].tobytes(), k
    return want


CAM = dict(width=160, height=120, fx=131.25, fy=131.25, cx=80.0, cy=60.0)


@pytest.fixture(scope="module")
def sphere():
    m = mr.sphere_map()
    return rr.rows_with_colors(*m), mr.triangulate(*m)[0]


def test_sphere_from_outside_on_the_host(host, sphere):
    rows, tri = sphere
    cam = dict(CAM, global_T_camera=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -3]], np.float32))
    out = _compare(host, rows, tri, cam, "sphere from outside")
    assert out["stats"]["n_covered_pixels"] > 0.25 * 160 * 120 and out["stats"]["n_large"] == 0
    _compare(host, rows, tri, cam, "sphere from outside", cull_back_faces=True, normal_mode=rr.NORMAL_FACE, color_flags=4)
    # a stale array: a tenth of the slots merged, and indices out of range
    stale = rows.copy()
    stale[7, ::10] = -1.0
    bad = tri.copy()
    bad[::7, 1] = rows.shape[1] + 5
    st = _compare(host, stale, bad, cam, "stale")["stats"]
    assert st["n_not_live"] > 0 and st["n_out_of_range"] > 0


def test_sphere_from_inside_on_the_host(host, sphere):
    rows, tri = sphere
    cam = dict(CAM, global_T_camera=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.9]], np.float32))
    # the hull instead of the mesher's output, so that nothing shows through a hole: the image is covered entirely
    from scipy.spatial import ConvexHull
    hull = ConvexHull(rows[3:6].T.astype(np.float64)).simplices.astype(np.uint32)
    for mode in (rr.NORMAL_VERTEX, rr.NORMAL_FACE):
        st = _compare(host, rows, hull, cam, "sphere from inside", normal_mode=mode)["stats"]
        assert st["n_large"] > 0 and st["n_covered_pixels"] == 160 * 120
    st = _compare(host, rows, tri, cam, "sphere from inside, the mesher's triangles")["stats"]
    assert st["n_large"] > 0 and st["n_clipped"] > 0


@pytest.mark.parametrize("reverse", [False, True])
def test_grid_on_the_host(host, reverse):
    rows, tri, cam = rr.grid_case(reverse)
    out = _compare(host, rows, tri, cam, "grid")
    assert out["stats"]["n_covered_pixels"] == 1600
    _compare(host, rows, tri, cam, "grid", cull_back_faces=True)
