// smx_merge.hpp -- merging another session's map into this one (smx_recon_merge_map).
//
// Part 1: the arithmetic of the definition in include/smx.h as plain inline functions: the move of a source slot, the BAD
// rule, the normal test and the walk over a candidate list, the link rule of an appended slot and one step of the blend.  The
// kernels call these; a test compiles this part alone for the host (SMX_MERGE_HOST_ONLY) and walks select, append and blend
// in lane order.
// Part 2: the workspace the destination object keeps for the call (kernels and glue: smx_merge.hip).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(SMX_MERGE_HOST_ONLY)
#define SMX_MERGE_FN static inline
#else
#include "smx_common.hpp"
#define SMX_MERGE_FN __host__ __device__ __forceinline__
#endif

namespace smx {

enum : uint32_t { kMergeDead = 0, kMergeBad = 1, kMergeMatched = 2, kMergeAppend = 3 };   // the class byte of a source slot
constexpr uint32_t kMergeNone = 0xFFFFFFFFu;

struct MgVec { float x, y, z; };

// ---- the move: p' = R p + t and n' = R n from the 12 floats of dst_T_src, summed left to right (smx_register.hpp: reg_move) ----
SMX_MERGE_FN MgVec mg_move(const float* T, const MgVec& p) {
  return MgVec{((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3], ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7],
               ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11]};
}
SMX_MERGE_FN MgVec mg_rotate(const float* T, const MgVec& n) {
  return MgVec{(T[0] * n.x + T[1] * n.y) + T[2] * n.z, (T[4] * n.x + T[5] * n.y) + T[6] * n.z, (T[8] * n.x + T[9] * n.y) + T[10] * n.z};
}
SMX_MERGE_FN bool mg_finite(float v) { return v - v == 0.0f; }
SMX_MERGE_FN bool mg_vec_finite(const MgVec& v) { return mg_finite(v.x) && mg_finite(v.y) && mg_finite(v.z); }
SMX_MERGE_FN bool mg_live(float radius_squared) { return !(radius_squared < 0.0f); }

// What k_merge_move leaves of a source slot: the moved words, the class so far (dead, BAD, or kMergeAppend = "to be matched")
// and the ball of its query (-1: none).
struct MgMoved { MgVec P, S, N; uint32_t cls; float r2; };
SMX_MERGE_FN MgMoved mg_move_slot(const float* T, const MgVec& p, const MgVec& s, const MgVec& n, float radius_squared, float factor_sq) {
  MgMoved m;
  m.P = mg_move(T, p); m.S = mg_move(T, s); m.N = mg_rotate(T, n);
  m.cls = kMergeAppend; m.r2 = -1.0f;
  if (!mg_live(radius_squared)) { m.cls = kMergeDead; return m; }
  if (!(mg_vec_finite(m.P) && mg_vec_finite(m.S) && mg_vec_finite(m.N))) { m.cls = kMergeBad; return m; }
  m.r2 = factor_sq * radius_squared;
  return m;
}

// ---- the match: the first of the slot's `count` candidates whose normal passes ----
SMX_MERGE_FN bool mg_compatible(const MgVec& n, const MgVec& Nd, float cos_max) { return (n.x * Nd.x + n.y * Nd.y) + n.z * Nd.z >= cos_max; }
// normal_of(d) = the normal of dst slot d as it stood.  Returns m(i) or kMergeNone; *saturated = unmatched with a full list.
template <class NormalOf>
SMX_MERGE_FN uint32_t mg_select(const MgVec& n, const uint32_t* cand, int count, int k, float cos_max, NormalOf normal_of, bool* saturated) {
  *saturated = false;
  for (int j = 0; j < count; ++j)
    if (mg_compatible(n, normal_of(cand[j]), cos_max)) return cand[j];
  *saturated = count == k;
  return kMergeNone;
}

// ---- a link of an appended slot: through the map if it points at an appended source slot, else gone ----
// cls_of(l), new_of(l) for l < n_src.  *dropped is raised for a link that was valid in src and is not any more.
template <class ClsOf, class NewOf>
SMX_MERGE_FN uint32_t mg_link(uint32_t l, uint32_t n_src, ClsOf cls_of, NewOf new_of, uint32_t* dropped) {
  if (l == kMergeNone) return kMergeNone;
  if (l < n_src && cls_of(l) == kMergeAppend) return new_of(l);
  ++*dropped;
  return kMergeNone;
}

// ---- one source into the running blend of a dst slot ----
struct MgBlend { MgVec P, S, N; float c, r; };
SMX_MERGE_FN void mg_blend_step(MgBlend& d, const MgVec& P, const MgVec& S, const MgVec& n, float w, float radius_squared, float cap) {
  const float W = d.c + w;
  if (!(W > 0.0f)) return;
  const float a = d.c / W, b = w / W;
  d.P = MgVec{(a * d.P.x) + (b * P.x), (a * d.P.y) + (b * P.y), (a * d.P.z) + (b * P.z)};
  d.S = MgVec{(a * d.S.x) + (b * S.x), (a * d.S.y) + (b * S.y), (a * d.S.z) + (b * S.z)};
  const MgVec M{(a * d.N.x) + (b * n.x), (a * d.N.y) + (b * n.y), (a * d.N.z) + (b * n.z)};
  const float len2 = (M.x * M.x + M.y * M.y) + M.z * M.z;
  if (len2 > 0.0f) {
    const float len = sqrtf(len2);
    d.N = MgVec{M.x / len, M.y / len, M.z / len};
  }
  d.r = fminf(d.r, radius_squared);
  d.c = fminf(W, cap);
}

#if !defined(SMX_MERGE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of the device counters (ctr)
enum : int { kMgLive = 0, kMgBad, kMgMatched, kMgSaturated, kMgAppended, kMgPairs, kMgBlended, kMgDropped, kMgWords };
constexpr uint32_t kMergeChunkDefault = 1u << 22;

// The workspace of smx_recon_merge_map, owned by the destination: sized by the source's slot count, grown when a larger
// source comes, freed with the object.  q = the query rows [4][n]; moved = the records P', S', (n', RadiusSquared) [3][n];
// match = m(i), then src_to_dst; cls = the class bytes; seg = the per-segment counts / offsets of the appended and of the
// matched slots [2][segments]; idx, d2, cnt = the answer of one query chunk; keys, vals, hist = the blend's (d, i) pairs.
struct MergeWork {
  DevBuf<float> q;
  DevBuf<float4> moved;
  DevBuf<uint32_t> match, seg, ctr, idx;
  DevBuf<uint8_t> cls;
  DevBuf<float> d2;
  DevBuf<int32_t> cnt;
  DevBuf<unsigned long long> keys[2];
  DevBuf<uint32_t> vals[2], hist;
  uint32_t chunk = 0;          // smx_recon_debug_set_merge_chunk (0: kMergeChunkDefault)
  PhaseStamps<SMX_MERGE_PHASES> stamps;
};
#endif

}  // namespace smx
