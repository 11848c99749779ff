// smx_mesh_raster.hpp -- rasterisation of a triangle array over the surfel map (smx_recon_render_mesh).
//
// The arithmetic of the contract (include/smx.h) as plain inline functions: vertex set-up, triangle set-up with its verdict
// and pixel box, coverage with the tie rule, perspective-correct depth and the z-buffer key, the resolve's normal and colour.
// smx_mesh_raster.hip calls them from its three kernels; a test compiles this header alone for the host
// (SMX_MESH_RASTER_HOST_ONLY) and walks the same passes.  Every floating-point quantity is a double expression evaluated as
// written (no contraction: -ffp-contract=off); everything that decides coverage is an integer.
#pragma once

#include <stdint.h>

#if defined(SMX_MESH_RASTER_HOST_ONLY)
#include <math.h>
#include "smx.h"
#define SMX_MR_FN static inline
#else
#include "smx_common.hpp"
#define SMX_MR_FN __host__ __device__ __forceinline__
#endif

namespace smx {

// Verdict of the triangle set-up, in the order of the contract's steps 1-6.  kMrEmptyBox is counted nowhere.
enum : int { kMrOutOfRange = 0, kMrNotLive, kMrClipped, kMrDegenerate, kMrCulled, kMrDrawn, kMrLarge, kMrCovered, kMrListLen,
             kMrWords = 12, kMrEmptyBox = kMrWords };

struct MrCam {
  double L[12];   // camera_T_global (inverted on the host in double precision, as in smx_recon_render)
  double fx, fy, cx, cy, near_z, far_z;
  int W, H, cull_back_faces, normal_mode;
};

// camera_T_global of global_T_camera = [R | t]: R^T, -(R^T t), the translation summed left to right in double
SMX_MR_FN void mr_invert_pose(const float* m, double* L) {
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) L[4 * i + k] = m[4 * k + i];
    L[4 * i + 3] = -(L[4 * i + 0] * m[3] + L[4 * i + 1] * m[7] + L[4 * i + 2] * m[11]);
  }
}

SMX_MR_FN bool mr_finite(float v) { return v - v == 0.0f; }
// Live as in smx_recon_triangulate: not merged, and a finite smooth position.
SMX_MR_FN bool mr_live(float x, float y, float z, float radius_squared) {
  return !(radius_squared < 0.0f) && mr_finite(x) && mr_finite(y) && mr_finite(z);
}

// A corner in camera space and snapped to 1/256 pixel.  |X|, |Y| <= 2^28 when ok, so differences of two fit 32 bits and
// every product of two differences stays below 2^59.
struct MrVertex { double x, y, z; int32_t X, Y; bool ok; };

SMX_MR_FN MrVertex mr_vertex(const MrCam& c, float spx, float spy, float spz) {
  const double px = spx, py = spy, pz = spz;
  const double* L = c.L;
  MrVertex v;
  v.x = L[0] * px + L[1] * py + L[2] * pz + L[3];
  v.y = L[4] * px + L[5] * py + L[6] * pz + L[7];
  v.z = L[8] * px + L[9] * py + L[10] * pz + L[11];
  v.X = 0; v.Y = 0;
  v.ok = c.near_z < v.z && v.z < c.far_z;
  if (v.ok) {
    const double u = c.fx * v.x / v.z + c.cx, w = c.fy * v.y / v.z + c.cy;
    v.ok = fabs(u) < 1048576.0 && fabs(w) < 1048576.0;
    if (v.ok) {
      v.X = (int32_t)(long long)floor(u * 256.0 + 0.5);
      v.Y = (int32_t)(long long)floor(w * 256.0 + 0.5);
    }
  }
  return v;
}

// What the pixel loops need of a triangle that is drawn: the snapped corners, the signed doubled area (in 1/256 pixel
// units squared), the corners' depths and the pixel box [x0, x1] x [y0, y1] (clamped to the image, not empty).
struct MrTri {
  int32_t Xa, Ya, Xb, Yb, Xc, Yc;
  long long A;
  double za, zb, zc;
  int x0, x1, y0, y1;
};

SMX_MR_FN int32_t mr_min3(int32_t a, int32_t b, int32_t c) { const int32_t m = a < b ? a : b; return m < c ? m : c; }
SMX_MR_FN int32_t mr_max3(int32_t a, int32_t b, int32_t c) { const int32_t m = a > b ? a : b; return m > c ? m : c; }

// Steps 3-6 of the contract for three live corners; returns kMrClipped, kMrDegenerate, kMrCulled, kMrEmptyBox, kMrDrawn or
// kMrLarge (drawn, and its box holds more than SMX_MESH_RENDER_LARGE_PIXELS pixels).
SMX_MR_FN int mr_setup(const MrCam& c, const MrVertex& a, const MrVertex& b, const MrVertex& d, MrTri* t) {
  if (!(a.ok && b.ok && d.ok)) return kMrClipped;
  t->Xa = a.X; t->Ya = a.Y; t->Xb = b.X; t->Yb = b.Y; t->Xc = d.X; t->Yc = d.Y;
  t->za = a.z; t->zb = b.z; t->zc = d.z;
  t->A = (long long)(b.X - a.X) * (long long)(d.Y - a.Y) - (long long)(b.Y - a.Y) * (long long)(d.X - a.X);
  if (t->A == 0) return kMrDegenerate;
  if (c.cull_back_faces && t->A > 0) return kMrCulled;
  // pixels whose centre 256 x + 128 lies in [min X, max X]: x0 = ceil((min X - 128) / 256), x1 = floor((max X - 128) / 256)
  // (an arithmetic shift rounds towards minus infinity)
  const int x0 = (mr_min3(a.X, b.X, d.X) + 127) >> 8, x1 = (mr_max3(a.X, b.X, d.X) - 128) >> 8;
  const int y0 = (mr_min3(a.Y, b.Y, d.Y) + 127) >> 8, y1 = (mr_max3(a.Y, b.Y, d.Y) - 128) >> 8;
  t->x0 = x0 > 0 ? x0 : 0; t->x1 = x1 < c.W - 1 ? x1 : c.W - 1;
  t->y0 = y0 > 0 ? y0 : 0; t->y1 = y1 < c.H - 1 ? y1 : c.H - 1;
  if (t->x0 > t->x1 || t->y0 > t->y1) return kMrEmptyBox;
  return (t->x1 - t->x0 + 1) * (t->y1 - t->y0 + 1) > SMX_MESH_RENDER_LARGE_PIXELS ? kMrLarge : kMrDrawn;
}

// s E(p, q, P) for the centre P of pixel (x, y), s = sign(A): positive on the triangle's side of the edge p -> q.
SMX_MR_FN long long mr_edge(int32_t Xp, int32_t Yp, int32_t Xq, int32_t Yq, int x, int y, bool flip) {
  const long long e = (long long)(Xq - Xp) * (long long)(256 * y + 128 - Yp) - (long long)(Yq - Yp) * (long long)(256 * x + 128 - Xp);
  return flip ? -e : e;
}
// The tie rule for a centre exactly on the edge p -> q: with d = s (q - p), d.y < 0 || (d.y == 0 && d.x > 0).
SMX_MR_FN bool mr_edge_owns(int32_t Xp, int32_t Yp, int32_t Xq, int32_t Yq, bool flip) {
  const int32_t dx = flip ? Xp - Xq : Xq - Xp, dy = flip ? Yp - Yq : Yq - Yp;
  return dy < 0 || (dy == 0 && dx > 0);
}

struct MrW { long long w0, w1, w2; };

SMX_MR_FN MrW mr_weights(const MrTri& t, int x, int y) {
  const bool flip = t.A < 0;
  MrW w;
  w.w0 = mr_edge(t.Xb, t.Yb, t.Xc, t.Yc, x, y, flip);
  w.w1 = mr_edge(t.Xc, t.Yc, t.Xa, t.Ya, x, y, flip);
  w.w2 = mr_edge(t.Xa, t.Ya, t.Xb, t.Yb, x, y, flip);
  return w;
}

SMX_MR_FN bool mr_covered(const MrTri& t, const MrW& w) {
  const bool flip = t.A < 0;
  if (w.w0 < 0 || w.w1 < 0 || w.w2 < 0) return false;
  return (w.w0 > 0 || mr_edge_owns(t.Xb, t.Yb, t.Xc, t.Yc, flip)) && (w.w1 > 0 || mr_edge_owns(t.Xc, t.Yc, t.Xa, t.Ya, flip)) &&
         (w.w2 > 0 || mr_edge_owns(t.Xa, t.Ya, t.Xb, t.Yb, flip));
}

// The largest of s E(p, q, .) over the centres of the pixels [x0, x1] x [y0, y1]: the function is affine, so it is reached
// at one of the four corner pixels.
SMX_MR_FN long long mr_edge_max(int32_t Xp, int32_t Yp, int32_t Xq, int32_t Yq, int x0, int y0, int x1, int y1, bool flip) {
  const long long e00 = mr_edge(Xp, Yp, Xq, Yq, x0, y0, flip), e10 = mr_edge(Xp, Yp, Xq, Yq, x1, y0, flip);
  const long long e01 = mr_edge(Xp, Yp, Xq, Yq, x0, y1, flip), e11 = mr_edge(Xp, Yp, Xq, Yq, x1, y1, flip);
  const long long m0 = e00 > e10 ? e00 : e10, m1 = e01 > e11 ? e01 : e11;
  return m0 > m1 ? m0 : m1;
}
// No pixel of the rectangle can be covered: it lies outside one edge altogether.
SMX_MR_FN bool mr_tile_outside(const MrTri& t, int x0, int y0, int x1, int y1) {
  const bool flip = t.A < 0;
  return mr_edge_max(t.Xb, t.Yb, t.Xc, t.Yc, x0, y0, x1, y1, flip) < 0 || mr_edge_max(t.Xc, t.Yc, t.Xa, t.Ya, x0, y0, x1, y1, flip) < 0 ||
         mr_edge_max(t.Xa, t.Ya, t.Xb, t.Yb, x0, y0, x1, y1, flip) < 0;
}

// l_k / z_k for the three corners (their sum is 1 / Z) and Z itself.
struct MrPersp { double q0, q1, q2, Z; };

SMX_MR_FN MrPersp mr_persp(const MrTri& t, const MrW& w) {
  const double area = (double)(t.A < 0 ? -t.A : t.A);
  const double l0 = (double)w.w0 / area, l1 = (double)w.w1 / area, l2 = (double)w.w2 / area;
  MrPersp p;
  p.q0 = l0 / t.za; p.q1 = l1 / t.zb; p.q2 = l2 / t.zc;
  const double invz = (p.q0 + p.q1) + p.q2;
  p.Z = 1.0 / invz;
  return p;
}

// (float_bits(depth) << 32) | t: the depth is positive, so its bit pattern orders as its value does
SMX_MR_FN unsigned long long mr_key(double Z, uint32_t t) {
  const float d = (float)Z;
  uint32_t bits;
  __builtin_memcpy(&bits, &d, sizeof(bits));
  return ((unsigned long long)bits << 32) | t;
}

struct MrVec { double x, y, z; };

// a normal rotated into the camera frame by L's rotation, each component summed left to right
SMX_MR_FN MrVec mr_rotate(const MrCam& c, float nx, float ny, float nz) {
  const double x = nx, y = ny, z = nz;
  const double* L = c.L;
  return MrVec{L[0] * x + L[1] * y + L[2] * z, L[4] * x + L[5] * y + L[6] * z, L[8] * x + L[9] * y + L[10] * z};
}

// N / sqrt((NxNx + NyNy) + NzNz) rounded to float, zeros if the squared length is not positive (or NaN)
SMX_MR_FN void mr_normalise(const MrVec& N, float out[3]) {
  const double len2 = (N.x * N.x + N.y * N.y) + N.z * N.z;
  out[0] = out[1] = out[2] = 0.0f;
  if (!(len2 > 0.0)) return;
  const double len = sqrt(len2);
  out[0] = (float)(N.x / len); out[1] = (float)(N.y / len); out[2] = (float)(N.z / len);
}

// SMX_MESH_NORMAL_VERTEX: the corners' camera-frame normals weighted by m_k = (l_k / z_k) Z
SMX_MR_FN void mr_normal_vertex(const MrPersp& p, const MrVec& na, const MrVec& nb, const MrVec& nc, float out[3]) {
  const double m0 = p.q0 * p.Z, m1 = p.q1 * p.Z, m2 = p.q2 * p.Z;
  mr_normalise(MrVec{(m0 * na.x + m1 * nb.x) + m2 * nc.x, (m0 * na.y + m1 * nb.y) + m2 * nc.y, (m0 * na.z + m1 * nb.z) + m2 * nc.z}, out);
}

// SMX_MESH_NORMAL_FACE: g = (b - a) x (c - a) on the camera-space corners, negated if (g . a) > 0 so that it faces the camera
SMX_MR_FN void mr_normal_face(const MrVertex& a, const MrVertex& b, const MrVertex& c, float out[3]) {
  const double ex = b.x - a.x, ey = b.y - a.y, ez = b.z - a.z, fx = c.x - a.x, fy = c.y - a.y, fz = c.z - a.z;
  MrVec g{ey * fz - ez * fy, ez * fx - ex * fz, ex * fy - ey * fx};
  if ((g.x * a.x + g.y * a.y) + g.z * a.z > 0.0) { g.x = -g.x; g.y = -g.y; g.z = -g.z; }
  mr_normalise(g, out);
}

// One colour channel: the corners' bytes weighted by m_k, rounded half up, saturated at 255.
SMX_MR_FN uint32_t mr_channel(const MrPersp& p, uint32_t ca, uint32_t cb, uint32_t cc) {
  const double m0 = p.q0 * p.Z, m1 = p.q1 * p.Z, m2 = p.q2 * p.Z;
  const double v = floor(((m0 * (double)ca + m1 * (double)cb) + m2 * (double)cc) + 0.5);
  return v < 255.0 ? (uint32_t)v : 255u;
}
// The colour word: channels in bytes 0-2 of the corners' vis_color words, alpha 255.
SMX_MR_FN uint32_t mr_color(const MrPersp& p, uint32_t wa, uint32_t wb, uint32_t wc) {
  uint32_t out = 0xFF000000u;
  for (int k = 0; k < 3; ++k)
    out |= mr_channel(p, (wa >> (8 * k)) & 255u, (wb >> (8 * k)) & 255u, (wc >> (8 * k)) & 255u) << (8 * k);
  return out;
}

}  // namespace smx
