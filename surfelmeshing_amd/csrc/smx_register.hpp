// smx_register.hpp -- point-to-plane registration of a point set to a kept distance scene (smx_distscene_register).
//
// Part 1: what only the registration needs, as plain inline functions: the move of a point by the pose an iteration linearised
// at, the row of a matched sample (the winner's plane normal, the two gates, r and J) and a sample's share of the counts.  The
// association is the scene's own query (smx_distance.hpp / smx_distscene.hpp), the sum order, the solve and the end of a call
// are the tracker's (smx_track.hpp).  The kernels call these; a test compiles this part alone for the host
// (SMX_REGISTER_HOST_ONLY) and walks the same passes in the launch's order.
// Part 2: the device state of a call (kernels and glue: smx_register.hip; the workspace itself is a member of the scene,
// smx_distscene.hpp).
#pragma once

#include <stdint.h>

#if defined(SMX_REGISTER_HOST_ONLY)
#if !defined(SMX_DISTSCENE_HOST_ONLY)
#define SMX_DISTSCENE_HOST_ONLY 1
#endif
#if !defined(SMX_TRACK_HOST_ONLY)
#define SMX_TRACK_HOST_ONLY 1
#endif
#endif
#include "smx_distscene.hpp"
#include "smx_track.hpp"
#define SMX_REG_FN SMX_DIST_FN

namespace smx {

constexpr int kRegMaxStride = 65536;
enum : int { kRegCollinear = 0, kRegNormalGate = 1, kRegInlier = 2 };   // where a matched sample ends

// ---- the move: p' = R p + t and m = R n from the 12 floats the iteration reads, summed left to right ----------------------
SMX_REG_FN TgVec reg_move(const float* T, const TgVec& p) {
  return TgVec{((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3], ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7],
               ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11]};
}
SMX_REG_FN TgVec reg_rotate(const float* T, const TgVec& n) {
  return TgVec{(T[0] * n.x + T[1] * n.y) + T[2] * n.z, (T[4] * n.x + T[5] * n.y) + T[6] * n.z, (T[8] * n.x + T[9] * n.y) + T[10] * n.z};
}
// samples of a level: point j * stride for j < ceil(n / stride)
SMX_REG_FN uint32_t reg_samples(uint32_t n_points, uint32_t stride) { return (uint32_t)(((unsigned long long)n_points + stride - 1) / stride); }

// ---- the row of a sample the query matched: p' (moved), Q (the query's closest point), the winner's corners -------------------
// N = the unit normal of (A, B, C) as they wind (Triangulate winds counter-clockwise about the surfel normals: no flip); a
// winner without an area ends as kRegCollinear.  With a normal m = R n the sample needs m . N >= cos_max.  r = N . (p' - Q),
// J = (p' x N, N): rotation first, a left twist in the scene's frame.  J and r are written for kRegInlier only.
SMX_REG_FN int reg_row(const TgVec& P, const TgVec& Q, const TgVec& A, const TgVec& B, const TgVec& C, bool with_normal, const TgVec& m,
                       float cos_max, float* J, float* r) {
  const TgVec g = tg_cross(tg_sub(B, A), tg_sub(C, A));
  const float len2 = tg_dot(g, g);
  if (!(len2 > 0.0f)) return kRegCollinear;
  const float len = sqrtf(len2);
  const TgVec N{g.x / len, g.y / len, g.z / len};
  if (with_normal && !(tg_dot(m, N) >= cos_max)) return kRegNormalGate;
  *r = tg_dot(N, tg_sub(P, Q));
  const TgVec c = tg_cross(P, N);
  J[0] = c.x; J[1] = c.y; J[2] = c.z; J[3] = N.x; J[4] = N.y; J[5] = N.z;
  return kRegInlier;
}

// One sample into a lane's sums: acc [28] as track_accumulate keeps them, the three counts.  t = the query's nearest for p'
// (kInvalid: not matched within the gate), Q its closest point, (A, B, C) the corners the winner's first record holds; they
// and m are looked at only where the text above says so.
SMX_REG_FN void reg_sample(const TgVec& P, uint32_t t, const TgVec& Q, const TgVec& A, const TgVec& B, const TgVec& C, bool with_normal,
                           const TgVec& m, float cos_max, double* acc, uint32_t& n_in, uint32_t& n_ok, uint32_t& n_matched) {
  if (!tg_point_ok(P)) return;
  ++n_ok;
  if (t == 0xFFFFFFFFu) return;
  ++n_matched;
  float J[6], r;
  if (reg_row(P, Q, A, B, C, with_normal, m, cos_max, J, &r) != kRegInlier) return;
  ++n_in;
  track_accumulate(acc, acc[kSumRR], J, r, r);
}

// ---- the robust row (smx_distscene_register_robust) -----------------------------------------------------------
enum : int { kRegKernelNone = 0, kRegKernelHuber = 1, kRegKernelTukey = 2 };
// "The closest point of p' lies on the rim": the region of dist_closest on the winner's first-record corners -- the computation
// the query's Q came from -- picks the bit of the triangle's rim byte (smx_rim.hpp; the interior, region 6, has none).
SMX_REG_FN bool reg_rim_hit(uint32_t rim_byte, const TgVec& P, const TgVec& A, const TgVec& B, const TgVec& C) {
  uint32_t region;
  (void)dist_closest(P, A, B, C, &region);
  return ((rim_byte >> region) & 1u) != 0;
}
// The weight of a row with residual r at scale c > 0, as the factor s on J and r (the weight is s * s); a = |r|.
//   Huber: a <= c leaves the row as it is (s = 1, not applied); else s = sqrtf(c / a) and the sample is counted as down-weighted.
//   Tukey: !(a < c) rejects the sample (counted); else u = a / c, s = 1 - u u, always applied.
// kept = the sample stays an inlier, apply = multiply the row by s, counted = the sample adds 1 to sum [32].
struct RegWeight { float s; int kept, apply, counted; };
SMX_REG_FN RegWeight reg_weight(int kernel, float c, float r) {
  const float a = fabsf(r);
  if (kernel == kRegKernelHuber) {
    if (a <= c) return RegWeight{1.0f, 1, 0, 0};
    return RegWeight{sqrtf(c / a), 1, 1, 1};
  }
  if (kernel == kRegKernelTukey) {
    if (!(a < c)) return RegWeight{1.0f, 0, 0, 1};
    const float u = a / c;
    return RegWeight{1.0f - u * u, 1, 1, 0};
  }
  return RegWeight{1.0f, 1, 0, 0};
}
// reg_sample with the two new decisions, in this order per sample: BAD -> not matched -> collinear winner -> rim -> normal gate
// -> weight -> inlier.  c == 0 (or kernel 0): no weights.  The weighted row is (s J, s r) with e = r, so sum [27] stays the
// geometric sum of r * r.  n_rim and n_weight are the sums [31] and [32].
SMX_REG_FN void reg_sample_robust(const TgVec& P, uint32_t t, const TgVec& Q, const TgVec& A, const TgVec& B, const TgVec& C, bool with_normal,
                                  const TgVec& m, float cos_max, uint32_t rim_byte, bool reject_rim, int kernel, float c, double* acc,
                                  uint32_t& n_in, uint32_t& n_ok, uint32_t& n_matched, uint32_t& n_rim, uint32_t& n_weight) {
  if (!tg_point_ok(P)) return;
  ++n_ok;
  if (t == 0xFFFFFFFFu) return;
  ++n_matched;
  const TgVec g = tg_cross(tg_sub(B, A), tg_sub(C, A));
  if (!(tg_dot(g, g) > 0.0f)) return;
  if (reject_rim && reg_rim_hit(rim_byte, P, A, B, C)) { ++n_rim; return; }
  float J[6], r;
  if (reg_row(P, Q, A, B, C, with_normal, m, cos_max, J, &r) != kRegInlier) return;
  const RegWeight w = (kernel == kRegKernelNone || c == 0.0f) ? RegWeight{1.0f, 1, 0, 0} : reg_weight(kernel, c, r);
  if (w.counted) ++n_weight;
  if (!w.kept) return;
  ++n_in;
  float rw = r;
  if (w.apply) {
    for (int k = 0; k < 6; ++k) J[k] = w.s * J[k];
    rw = w.s * r;
  }
  track_accumulate(acc, acc[kSumRR], J, rw, r);
}

#if !defined(SMX_REGISTER_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// The device state of a call: the tracker's (T_rel = scene <- points, the ring of records) with what a registration adds: the
// pose every recorded iteration read, and the result in the call's own layout.  Written by k_reg_begin and by lane 0 of
// k_reg_solve only.
struct RegDev {
  TrackDev t;
  float ring_Tf[kTrackRing][12];
  smx_register_result result;
  uint32_t ring_counts[kTrackRing][2];     // sums [31] and [32] of every recorded iteration of a robust call (behind what the plain kernels address)
};

struct RegPose { float m[12]; };
// what the robust reduce kernel needs besides the plain one's arguments
struct RegRobustK { const uint8_t* rim; int reject_rim, kernel; float c; };
#endif

}  // namespace smx
