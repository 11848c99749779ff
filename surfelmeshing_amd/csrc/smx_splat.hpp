// smx_splat.hpp -- the splat render of the surfel map (smx_recon_render; the tracking calls render their model
// images with it).
//
// The arithmetic of the contract (include/smx.h) as plain inline functions: the view with its widened fields, a slot's depth
// test, projection and guard, its extent in both modes, its pixel rectangle and the clip, the z-buffer key, a disc's per-pixel
// test, the key's decode and the normal's rotation.  k_render_splat and k_render_resolve (smx_recon_map.hip) call them, the
// loops stay there; a test compiles this header alone for the host (SMX_SPLAT_HOST_ONLY) and walks the same passes.  Every
// quantity that decides coverage or depth is a double expression evaluated as written (no contraction: -ffp-contract=off).
#pragma once

#include <stdint.h>

#if defined(SMX_SPLAT_HOST_ONLY)
#include <math.h>
#include "smx.h"
#if !defined(SMX_MESH_RASTER_HOST_ONLY)
#define SMX_MESH_RASTER_HOST_ONLY 1
#endif
#define SMX_SPLAT_FN static inline
#else
#include "smx_common.hpp"
#define SMX_SPLAT_FN __host__ __device__ __forceinline__
#endif
#include "smx_mesh_raster.hpp"   // mr_invert_pose

namespace smx {

struct SplatCam {
  double L[12];   // camera_T_global (inverted on the host in double precision)
  float Lf[12];   // ... inverted in float: the rotation part is exact (a transpose), used for the normal image
  double fx, fy, cx, cy, near_z, far_z;
  double half_extent;   // square mode
  double disc_factor, max_extent, f_max;   // disc mode (f_max = max(fx, fy))
  int W, H, mode;
};

// The view of a call: every float field widened to double as it is (near_z = 0.05f is not 0.05), L by mr_invert_pose, Lf as
// R^T, -(R^T t) in float, summed left to right (se3_inverse of smx_common.hpp).
SMX_SPLAT_FN void sp_make_cam(const smx_render_params& p, SplatCam* c) {
  mr_invert_pose(p.global_T_camera, c->L);
  const float* m = p.global_T_camera;
  for (int i = 0; i < 3; ++i) {
    c->Lf[4 * i + 0] = m[0 + i]; c->Lf[4 * i + 1] = m[4 + i]; c->Lf[4 * i + 2] = m[8 + i];
    c->Lf[4 * i + 3] = -(c->Lf[4 * i + 0] * m[3] + c->Lf[4 * i + 1] * m[7] + c->Lf[4 * i + 2] * m[11]);
  }
  c->fx = p.fx; c->fy = p.fy; c->cx = p.cx; c->cy = p.cy; c->near_z = p.near_z; c->far_z = p.far_z;
  c->half_extent = p.splat_half_extent_in_pixels;
  c->disc_factor = p.disc_radius_factor; c->max_extent = p.max_splat_extent_in_pixels;
  c->f_max = p.fx > p.fy ? p.fx : p.fy;
  c->W = p.width; c->H = p.height; c->mode = p.splat_mode;
}

// Not merged: RadiusSquared >= 0 (a NaN is not drawn either)
SMX_SPLAT_FN bool sp_live(float radius_squared) { return radius_squared >= 0.0f; }

// A slot in camera space and on the image plane; e is its half extent in pixels, rho its disc's radius (disc mode), and
// [x0, x1] x [y0, y1] its pixel rectangle clipped to the image (empty where x0 > x1 or y0 > y1).
struct SplatSlot {
  double cx, cy, cz, u, v, e, rho;
  int x0, x1, y0, y1;
};

// The camera-space depth of the smooth position, summed left to right, and the open depth range.
SMX_SPLAT_FN double sp_depth(const SplatCam& c, float spx, float spy, float spz) {
  const double px = spx, py = spy, pz = spz;
  const double* L = c.L;
  return L[8] * px + L[9] * py + L[10] * pz + L[11];
}
SMX_SPLAT_FN bool sp_in_range(const SplatCam& c, double cz) { return cz > c.near_z && cz < c.far_z; }

// The rest of the camera-space position and the projection.  False far outside any image (or at a NaN): the guard keeps the
// conversions of sp_rect defined.
SMX_SPLAT_FN bool sp_project(const SplatCam& c, float spx, float spy, float spz, double cz, SplatSlot* s) {
  const double px = spx, py = spy, pz = spz;
  const double* L = c.L;
  s->cz = cz;
  s->cx = L[0] * px + L[1] * py + L[2] * pz + L[3];
  s->cy = L[4] * px + L[5] * py + L[6] * pz + L[7];
  s->u = c.fx * s->cx / cz + c.cx;
  s->v = c.fy * s->cy / cz + c.cy;
  return fabs(s->u) < 1e8 && fabs(s->v) < 1e8;
}

// Square mode: the call's half extent.  Disc mode: the disc's bounding square, max_extent where the disc reaches the near plane.
SMX_SPLAT_FN void sp_extent(const SplatCam& c, float radius_squared, SplatSlot* s) {
  s->e = c.half_extent;
  s->rho = 0.0;
  if (c.mode == SMX_SPLAT_DISC) {
    s->rho = c.disc_factor * sqrt((double)radius_squared);
    const double dz = s->cz - s->rho;
    s->e = dz <= c.near_z ? c.max_extent : fmin(c.max_extent, 2.0 * c.f_max * s->rho / dz);
  }
}

// pixels whose centre x + 1/2 lies within e of u: u - e - 1/2 <= x <= u + e - 1/2 (square mode, h = 0: floor(u)), clipped
SMX_SPLAT_FN void sp_rect(const SplatCam& c, SplatSlot* s) {
  const double u = s->u, v = s->v, e = s->e;
  const bool point = c.mode == SMX_SPLAT_SQUARE && e == 0.0;
  const double x0f = point ? floor(u) : ceil(u - e - 0.5), x1f = point ? floor(u) : floor(u + e - 0.5);
  const double y0f = point ? floor(v) : ceil(v - e - 0.5), y1f = point ? floor(v) : floor(v + e - 0.5);
  s->x0 = (int)fmax(x0f, 0.0); s->x1 = (int)fmin(x1f, (double)(c.W - 1));
  s->y0 = (int)fmax(y0f, 0.0); s->y1 = (int)fmin(y1f, (double)(c.H - 1));
}

// (float_bits(depth) << 32) | slot: the depth is positive, so its bit pattern orders as its value does; the smaller key wins
SMX_SPLAT_FN unsigned long long sp_key(double depth, uint32_t slot) {
  const float d = (float)depth;
  uint32_t bits;
  __builtin_memcpy(&bits, &d, sizeof(bits));
  return ((unsigned long long)bits << 32) | slot;
}

// A disc's plane in camera space: the normal rotated by L, each component summed left to right, and n . c.
struct SplatDisc { double nx, ny, nz, n_dot_c, rho2; };

SMX_SPLAT_FN SplatDisc sp_disc(const SplatCam& c, const SplatSlot& s, float snx, float sny, float snz) {
  const double* L = c.L;
  SplatDisc d;
  d.nx = L[0] * snx + L[1] * sny + L[2] * snz;
  d.ny = L[4] * snx + L[5] * sny + L[6] * snz;
  d.nz = L[8] * snx + L[9] * sny + L[10] * snz;
  d.n_dot_c = d.nx * s.cx + d.ny * s.cy + d.nz * s.cz;
  d.rho2 = s.rho * s.rho;
  return d;
}

// The ray through the centre of pixel column x / row y, at z = 1.
SMX_SPLAT_FN double sp_ray_x(const SplatCam& c, int x) { return ((double)x + 0.5 - c.cx) / c.fx; }
SMX_SPLAT_FN double sp_ray_y(const SplatCam& c, int y) { return ((double)y + 0.5 - c.cy) / c.fy; }

// Does the ray (dx, dy, 1) meet the disc?  The four steps of a pixel, in the kernel's order: n . d and the edge-on test (no
// hit), the depth t of the ray's point on the disc's plane, the near plane (no hit at or behind it), and the distance of
// that point to the centre (a hit within rho, the border included).
SMX_SPLAT_FN double sp_n_dot_d(const SplatDisc& d, double dx, double dy) { return d.nx * dx + d.ny * dy + d.nz; }
SMX_SPLAT_FN bool sp_edge_on(double n_dot_d) { return fabs(n_dot_d) < 1e-4; }
SMX_SPLAT_FN double sp_plane_depth(const SplatDisc& d, double n_dot_d) { return d.n_dot_c / n_dot_d; }
SMX_SPLAT_FN bool sp_in_front(const SplatCam& c, double t) { return t > c.near_z; }
SMX_SPLAT_FN bool sp_within_disc(const SplatSlot& s, const SplatDisc& d, double t, double dx, double dy) {
  const double ex = t * dx - s.cx, ey = t * dy - s.cy, ez = t - s.cz;
  return ex * ex + ey * ey + ez * ez <= d.rho2;
}

// The resolve's decode of a z-buffer word.
SMX_SPLAT_FN bool sp_key_empty(unsigned long long key) { return key == ~0ull; }
SMX_SPLAT_FN uint32_t sp_key_slot(unsigned long long key) { return sp_key_empty(key) ? 0xFFFFFFFFu : (uint32_t)key; }
SMX_SPLAT_FN float sp_key_depth(unsigned long long key) {
  const uint32_t bits = sp_key_empty(key) ? 0u : (uint32_t)(key >> 32);
  float d;
  __builtin_memcpy(&d, &bits, sizeof(d));
  return d;
}

// The normal image: the slot's normal rotated by Lf in float, each component summed left to right.
SMX_SPLAT_FN void sp_rotate_normal(const float* Lf, float x, float y, float z, float out[3]) {
  out[0] = Lf[0] * x + Lf[1] * y + Lf[2] * z;
  out[1] = Lf[4] * x + Lf[5] * y + Lf[6] * z;
  out[2] = Lf[8] * x + Lf[9] * y + Lf[10] * z;
}

}  // namespace smx
