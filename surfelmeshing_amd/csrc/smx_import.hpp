// smx_import.hpp -- importing a point cloud as surfels (smx_recon_import_points).
//
// Part 1: the arithmetic of the definition in include/smx.h as plain inline functions: the BAD rule, the nine sums of a
// neighbourhood, the covariance, the cyclic Jacobi iteration with compile-time pairs, the choice of the normal, its
// orientation, the radius and the class of a point.  The kernels call these; a test compiles this part alone for the host
// (SMX_IMPORT_HOST_ONLY) and walks the fit in lane order.
// Part 2: the workspace the object keeps for the call (kernels and glue: smx_import.hip).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(SMX_IMPORT_HOST_ONLY)
#define SMX_IMPORT_FN static inline
#else
#include "smx_common.hpp"
#define SMX_IMPORT_FN __host__ __device__ __forceinline__
#endif

#ifndef SMX_IMPORT_JACOBI_SWEEPS
#define SMX_IMPORT_JACOBI_SWEEPS 6
#endif

namespace smx {

// the class byte of a point, in the order of the definition's step 9
enum : uint32_t { kImportBad = 0, kImportSparse = 1, kImportDegenerate = 2, kImportRough = 3, kImportOk = 4 };
constexpr uint32_t kImportNone = 0xFFFFFFFFu;

struct ImVec { float x, y, z; };

SMX_IMPORT_FN bool im_finite(float v) { return v - v == 0.0f; }
SMX_IMPORT_FN bool im_vec_finite(const ImVec& v) { return im_finite(v.x) && im_finite(v.y) && im_finite(v.z); }

// ---- the nine sums, in list order: d = p_j - p_i in float32, sums and products in double ----
struct ImSums { double s0, s1, s2, q00, q01, q02, q11, q12, q22; };
SMX_IMPORT_FN ImSums im_sums_zero() { return ImSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }
SMX_IMPORT_FN void im_sums_add(ImSums& a, const ImVec& pi, const ImVec& pj) {
  const float fx = pj.x - pi.x, fy = pj.y - pi.y, fz = pj.z - pi.z;
  const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
  a.s0 += dx; a.s1 += dy; a.s2 += dz;
  a.q00 += dx * dx; a.q01 += dx * dy; a.q02 += dx * dz;
  a.q11 += dy * dy; a.q12 += dy * dz; a.q22 += dz * dz;
}

// ---- the symmetric 3 x 3 matrix as its upper triangle: a[im_sym(i, j)], i <= j ----
SMX_IMPORT_FN constexpr int im_sym(int i, int j) { return i > j ? im_sym(j, i) : i == 0 ? j : i == 1 ? 2 + j : 5; }

SMX_IMPORT_FN void im_covariance(const ImSums& s, int m, double* a) {
  const double inv = 1.0 / (double)m;
  const double m0 = s.s0 * inv, m1 = s.s1 * inv, m2 = s.s2 * inv;
  a[0] = s.q00 * inv - m0 * m0; a[1] = s.q01 * inv - m0 * m1; a[2] = s.q02 * inv - m0 * m2;
  a[3] = s.q11 * inv - m1 * m1; a[4] = s.q12 * inv - m1 * m2; a[5] = s.q22 * inv - m2 * m2;
}

// One rotation of the pair (P, Q), R the third index; v[3 * row + column].  With a_pq == 0 nothing happens.  The two-row
// formulas, as the definition states them:
//   a_pp' = a_pp - t a_pq     a_qq' = a_qq + t a_pq     a_pq' = 0
//   a_rp' = c a_rp - sn a_rq  a_rq' = sn a_rp + c a_rq
//   v_ip' = c v_ip - sn v_iq  v_iq' = sn v_ip + c v_iq   for the rows i = 0, 1, 2
// Every index is a compile-time constant, so a and v are nine plus six scalars to the compiler.
template <int P, int Q>
SMX_IMPORT_FN void im_rotate(double* a, double* v) {
  constexpr int R = 3 - P - Q;
  const double apq = a[im_sym(P, Q)];
  if (apq == 0.0) return;
  const double app = a[im_sym(P, P)], aqq = a[im_sym(Q, Q)];
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta infinite: t = 0)
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double sn = t * c;
  a[im_sym(P, P)] = app - t * apq;
  a[im_sym(Q, Q)] = aqq + t * apq;
  a[im_sym(P, Q)] = 0.0;
  const double arp = a[im_sym(R, P)], arq = a[im_sym(R, Q)];
  a[im_sym(R, P)] = c * arp - sn * arq;
  a[im_sym(R, Q)] = sn * arp + c * arq;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 3; ++i) {
    const double vip = v[3 * i + P], viq = v[3 * i + Q];
    v[3 * i + P] = c * vip - sn * viq;
    v[3 * i + Q] = sn * vip + c * viq;
  }
}

// SMX_IMPORT_JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2); then the smallest diagonal entry (ties: the lowest column) is
// lam[0] and its column of V the normal; lam[1], lam[2] are the other two diagonal entries in ascending column order.
SMX_IMPORT_FN void im_eigen(double* a, double* lam, double* nrm) {
  double v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < SMX_IMPORT_JACOBI_SWEEPS; ++sweep) {
    im_rotate<0, 1>(a, v);
    im_rotate<0, 2>(a, v);
    im_rotate<1, 2>(a, v);
  }
  const double d0 = a[0], d1 = a[3], d2 = a[5];
  int col = 0;
  double low = d0;
  if (d1 < low) { col = 1; low = d1; }
  if (d2 < low) { col = 2; low = d2; }
  lam[0] = low;
  lam[1] = col == 0 ? d1 : d0;
  lam[2] = col == 2 ? d1 : d2;
  nrm[0] = col == 0 ? v[0] : col == 1 ? v[1] : v[2];
  nrm[1] = col == 0 ? v[3] : col == 1 ? v[4] : v[5];
  nrm[2] = col == 0 ? v[6] : col == 1 ? v[7] : v[8];
}

// ---- what the fit needs of smx_import_params, and what it leaves of a point ----
struct ImFitParams {
  int32_t k, min_neighbors, radius_rank, orient;   // orient: 0 none, 1 view point, 2 origins
  float max_surface_variation, radius_scale_squared;
  ImVec view_point;
};
struct ImFit { uint32_t cls; ImVec n; float radius_squared; };

SMX_IMPORT_FN int im_radius_entry(int radius_rank, int m) { return radius_rank < m - 1 ? radius_rank : m - 1; }

// The point's class before the sums are formed (steps 3 and 8): kImportOk = go on.  radius_d2 = d2[im_radius_entry(..)].
SMX_IMPORT_FN uint32_t im_class_early(int m, float radius_d2, const ImFitParams& prm, float* radius_squared) {
  *radius_squared = 0.0f;
  if (m < prm.min_neighbors) return kImportSparse;
  *radius_squared = prm.radius_scale_squared * radius_d2;
  if (!(*radius_squared > 0.0f)) return kImportDegenerate;
  return kImportOk;
}

// Steps 4 to 7 from the sums of the point's m entries; o = the view point or the point's origin (unused with orient 0).
SMX_IMPORT_FN ImFit im_fit(const ImSums& sums, int m, const ImVec& p, const ImVec& o, float radius_squared, const ImFitParams& prm) {
  ImFit f;
  f.cls = kImportOk; f.radius_squared = radius_squared; f.n = ImVec{0.0f, 0.0f, 0.0f};
  double a[6], lam[3], nd[3];
  im_covariance(sums, m, a);
  im_eigen(a, lam, nd);
  float nx = (float)nd[0], ny = (float)nd[1], nz = (float)nd[2];
  const float len2 = (nx * nx + ny * ny) + nz * nz;
  const float len = sqrtf(len2);
  nx = nx / len; ny = ny / len; nz = nz / len;
  if (!(len2 > 0.0f) || !(im_finite(nx) && im_finite(ny) && im_finite(nz))) { f.cls = kImportDegenerate; return f; }
  if (lam[0] > (double)prm.max_surface_variation * ((lam[0] + lam[1]) + lam[2])) { f.cls = kImportRough; return f; }
  if (prm.orient != 0) {
    const float vx = o.x - p.x, vy = o.y - p.y, vz = o.z - p.z;
    if ((nx * vx + ny * vy) + nz * vz < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
  }
  f.n = ImVec{nx, ny, nz};
  return f;
}

#if !defined(SMX_IMPORT_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of the device counters (ctr)
enum : int { kImBad = 0, kImSparse, kImDegenerate, kImRough, kImSaturated, kImImported, kImWords };

// The workspace of smx_recon_import_points, owned by the object: sized by the cloud and by n * k, grown when a larger one
// comes, freed with the object.  rows = the three rows the index is built over [3][npad] (NaN for a BAD point); rec = the
// packed records (x, y, z, colour bits); fit = (normal, RadiusSquared); slot = point_to_slot; cls = the class bytes;
// seg = the per-segment counts / offsets of the imported points; idx, d2, cnt = the answer of the self query; in_* =
// staging of host inputs.
struct ImportWork {
  DevBuf<float> rows;
  DevBuf<float4> rec, fit;
  DevBuf<uint32_t> slot, seg, ctr, idx;
  DevBuf<uint8_t> cls;
  DevBuf<float> d2;
  DevBuf<int32_t> cnt;
  DevBuf<float> in_points, in_origins;
  DevBuf<uint32_t> in_colors;
  PhaseStamps<SMX_IMPORT_PHASES> stamps;
};
#endif

}  // namespace smx
