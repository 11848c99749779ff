// smx_global.hpp -- registration without a start pose: a lattice of candidate poses, the integer score of a pose, the choice of
// the starts (smx_register_pose_lattice, smx_distscene_score_poses, smx_distscene_register_global).
//
// Everything of the contract that is not a launch, as plain inline functions: the lattice in double with + - * / only, a sample's
// share of a pose's score words, the order of the poses.  smx_global.hip calls them from its kernels and its glue; a test compiles
// this file alone for the host (SMX_GLOBAL_HOST_ONLY).  The move, the rim test and the BAD rule are the registration's
// (smx_register.hpp), the distance word is smx_recon_compare_meshes' (smx_sample.hpp).
#pragma once

#include <stdint.h>

#if defined(SMX_GLOBAL_HOST_ONLY)
#if !defined(SMX_REGISTER_HOST_ONLY)
#define SMX_REGISTER_HOST_ONLY 1
#endif
#if !defined(SMX_SAMPLE_HOST_ONLY)
#define SMX_SAMPLE_HOST_ONLY 1
#endif
#endif
#include "smx_register.hpp"
#include "smx_sample.hpp"
#define SMX_GLOB_FN SMX_DIST_FN

namespace smx {

constexpr int kGlobMaxK = 8;
constexpr uint32_t kGlobMaxPoses = 1u << 20, kGlobMaxSamples = 1u << 16;
constexpr int kGlobMaxStarts = 64;
constexpr int kGlobBlock = 256;        // lanes of both kernels
constexpr int kGlobBatch = 4;          // samples of a lane whose gathers are in flight together (the rim variant)

// ---- the lattice ---------------------------------------------------------------------------------------------------------
// N_k = ((2k+1)^4 - (2k-1)^4) / 2: the points of the cube's surface, one of each +- pair
inline uint32_t glob_lattice_rotations(int k) {
  const long long a = 2LL * k + 1, b = 2LL * k - 1;
  return (uint32_t)((a * a * a * a - b * b * b * b) / 2);
}
// (w, x, y, z) in [-k, k]^4 belongs to the lattice: the largest absolute component is k, the first non-zero one is positive
inline bool glob_lattice_has(int k, int w, int x, int y, int z) {
  const int q[4] = {w, x, y, z};
  int largest = 0, first = 0;
  for (int i = 0; i < 4; ++i) {
    const int a = q[i] < 0 ? -q[i] : q[i];
    if (a > largest) largest = a;
    if (first == 0) first = q[i];
  }
  return largest == k && first > 0;
}
// R of an integer quaternion: every entry one exact integer numerator divided once by n
inline void glob_lattice_matrix(int w, int x, int y, int z, double* R /* [9] */) {
  const double n = (double)(w * w + x * x + y * y + z * z);
  R[0] = (double)(w * w + x * x - y * y - z * z) / n; R[1] = (double)(2 * (x * y - w * z)) / n; R[2] = (double)(2 * (x * z + w * y)) / n;
  R[3] = (double)(2 * (x * y + w * z)) / n; R[4] = (double)(w * w - x * x + y * y - z * z) / n; R[5] = (double)(2 * (y * z - w * x)) / n;
  R[6] = (double)(2 * (x * z - w * y)) / n; R[7] = (double)(2 * (y * z + w * x)) / n; R[8] = (double)(w * w - x * x - y * y + z * z) / n;
}
// The pose of rotation R about `centre` onto `anchor`, each value rounded once to float32.
inline void glob_lattice_pose(const double* R, const double* centre, const double* anchor, float* pose /* [12] */) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose[4 * i + j] = (float)R[3 * i + j];
    pose[4 * i + 3] = (float)(anchor[i] - ((R[3 * i] * centre[0] + R[3 * i + 1] * centre[1]) + R[3 * i + 2] * centre[2]));
  }
}
// All of them in the contract's order: pose index = rotation index * A + anchor index.  poses holds N_k * A of them.
inline void glob_lattice(int k, const double* centre, const double* anchors, uint32_t A, float* poses) {
  size_t at = 0;
  for (int w = 0; w <= k; ++w)               // (ascending (w, x, y, z); a negative w never comes first)
    for (int x = -k; x <= k; ++x)
      for (int y = -k; y <= k; ++y)
        for (int z = -k; z <= k; ++z) {
          if (!glob_lattice_has(k, w, x, y, z)) continue;
          double R[9];
          glob_lattice_matrix(w, x, y, z, R);
          for (uint32_t a = 0; a < A; ++a, ++at) glob_lattice_pose(R, centre, anchors + 3 * (size_t)a, poses + 12 * at);
        }
}

// ---- the score of a pose ---------------------------------------------------------------------------------------------------
// One sample into a lane's words.  P = the moved sample, t and distance = the query's answer for it at gate q (t == 0xFFFFFFFF:
// not matched), q_word = cmp_dq(q).  on_rim: glob_on_rim below, false without reject_rim.
SMX_GLOB_FN void glob_sample(const TgVec& P, uint32_t t, float distance, uint32_t q_word, bool on_rim, unsigned long long& cost, uint32_t& n_ok,
                             uint32_t& n_matched, uint32_t& n_rim) {
  const bool ok = tg_point_ok(P);
  if (ok) ++n_ok;
  if (!ok || t == 0xFFFFFFFFu) { cost += q_word; return; }
  ++n_matched;
  if (on_rim) { ++n_rim; cost += q_word; return; }
  cost += cmp_dq(distance);
}
// The rim decision of smx_distscene_register_robust for a matched sample, in that call's order: a winner without an area is
// never on the rim; otherwise the region of dist_closest on the winner's first-record corners picks the bit.
SMX_GLOB_FN bool glob_on_rim(uint32_t rim_byte, const TgVec& P, const TgVec& A, const TgVec& B, const TgVec& C) {
  const TgVec g = tg_cross(tg_sub(B, A), tg_sub(C, A));
  if (!(tg_dot(g, g) > 0.0f)) return false;
  return reg_rim_hit(rim_byte, P, A, B, C);
}

// ---- the choice -------------------------------------------------------------------------------------------------------------
// (cost, index) ascending: the smaller cost first, of equal costs the smaller index
inline bool glob_before(unsigned long long cost_a, uint32_t index_a, unsigned long long cost_b, uint32_t index_b) {
  return cost_a < cost_b || (cost_a == cost_b && index_a < index_b);
}
// The first M = min(n_starts, P) poses in that order into order[M]; returns M.  cost(i) = the cost of pose i.
template <class Cost>
inline uint32_t glob_select(const Cost& cost, uint32_t P, uint32_t n_starts, uint32_t* order) {
  const uint32_t M = n_starts < P ? n_starts : P;
  uint32_t held = 0;
  for (uint32_t i = 0; i < P; ++i) {       // (an insertion into at most 64 kept places)
    const unsigned long long c = cost(i);
    if (held == M && !glob_before(c, i, cost(order[M - 1]), order[M - 1])) continue;
    uint32_t at = held < M ? held++ : M - 1;
    while (at > 0 && glob_before(c, i, cost(order[at - 1]), order[at - 1])) { order[at] = order[at - 1]; --at; }
    order[at] = i;
  }
  return M;
}
// found: the winner's status is OK (0) or CONVERGED (1) and enough of its samples that are not BAD are matched
inline bool glob_found(int status, uint32_t n_matched, uint32_t n_ok, float min_matched_fraction) {
  return (status == 0 || status == 1) && (float)n_matched >= min_matched_fraction * (float)n_ok;
}

}  // namespace smx
