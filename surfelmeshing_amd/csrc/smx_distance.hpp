// smx_distance.hpp -- the distance from points to a triangle array over the map (smx_recon_mesh_distance).
//
// Part 1: the distance arithmetic of the contract as plain inline functions (the closest point of Ericson's regions with its
// squared distance, key and sign, the histogram bin, the neighbour cells, the walk of a cell's records, the query of one
// point).  smx_distance.hip calls them from its kernels; a test compiles this part alone for the host
// (SMX_DISTANCE_HOST_ONLY) and walks the same passes with plain words.  The classes of step 1, the cell functions, the cell
// table and the packed records are the triangle grid's (smx_trigrid.hpp).
// Part 2: the counter words, the workspace the object keeps for the call, and what the query of a kept index (smx_distscene.hpp)
// needs of this file (kernels and glue: smx_distance.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_DISTANCE_HOST_ONLY) && !defined(SMX_TRIGRID_HOST_ONLY)
#define SMX_TRIGRID_HOST_ONLY 1
#endif
#include "smx_trigrid.hpp"    // the vector type, step 1's classes, the cell functions, the box, the cell table
#define SMX_DIST_FN SMX_TG_FN

namespace smx {

constexpr uint32_t kDistBins = 32;                          // SMX_DIST_BINS
constexpr float kDistMargin = 1.125f;                       // c >= kDistMargin * max_distance (why that is enough)
enum : uint32_t { kDistRegionA = 0, kDistRegionB, kDistRegionAB, kDistRegionC, kDistRegionAC, kDistRegionBC, kDistRegionInside };

// ---- step 3: the closest point of P on (A, B, C), Ericson's regions in the contract's order ------------------------------
SMX_DIST_FN TgVec dist_closest(const TgVec& P, const TgVec& A, const TgVec& B, const TgVec& C, uint32_t* region) {
  const TgVec ab = tg_sub(B, A), ac = tg_sub(C, A), ap = tg_sub(P, A);
  const float d1 = tg_dot(ab, ap), d2 = tg_dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) { *region = kDistRegionA; return A; }
  const TgVec bp = tg_sub(P, B);
  const float d3 = tg_dot(ab, bp), d4 = tg_dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) { *region = kDistRegionB; return B; }
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    const float v = d1 / (d1 - d3);
    *region = kDistRegionAB;
    return tg_add(A, tg_scale(v, ab));
  }
  const TgVec cp = tg_sub(P, C);
  const float d5 = tg_dot(ab, cp), d6 = tg_dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) { *region = kDistRegionC; return C; }
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    const float w = d2 / (d2 - d6);
    *region = kDistRegionAC;
    return tg_add(A, tg_scale(w, ac));
  }
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
    const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    *region = kDistRegionBC;
    return tg_add(B, tg_scale(w, tg_sub(C, B)));
  }
  const float s = (va + vb) + vc;
  float v = vb / s, w = vc / s;
  // exact arithmetic arrives here with va, vb, vc > 0; float32 may not, so v and w are held to the triangle (a NaN stays one)
  v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  const float lim = 1.0f - v;
  w = w < 0.0f ? 0.0f : (w > lim ? lim : w);
  *region = kDistRegionInside;
  return tg_add(tg_add(A, tg_scale(v, ab)), tg_scale(w, ac));
}
SMX_DIST_FN float dist_dist2(const TgVec& P, const TgVec& Q) { const TgVec e = tg_sub(P, Q); return tg_dot(e, e); }
// The key of triangle t for P: (float_bits(dist2) << 32) | t if it is a candidate, kTgNone otherwise (NaN never is).
SMX_DIST_FN unsigned long long dist_key(const TgVec& P, const TgVec& A, const TgVec& B, const TgVec& C, uint32_t t, float max2) {
  uint32_t region;
  const float d2 = dist_dist2(P, dist_closest(P, A, B, C, &region));
  return d2 <= max2 ? dec_value_word(d2, t) : kTgNone;
}
SMX_DIST_FN bool dist_negative(const TgVec& P, const TgVec& Q, const TgVec& A, const TgVec& B, const TgVec& C) {
  return tg_dot(tg_sub(P, Q), tg_cross(tg_sub(B, A), tg_sub(C, A))) < 0.0f;
}
SMX_DIST_FN uint32_t dist_bin(float abs_distance, float max_distance) {
  const uint32_t b = (uint32_t)((abs_distance * 32.0f) / max_distance);
  return b < kDistBins - 1 ? b : kDistBins - 1;
}

SMX_DIST_FN float dist_cell_size(float cell_size, float max_distance) { return tg_cell_size(cell_size, kDistMargin * max_distance); }

// ---- the query of one point ----------------------------------------------------------------------------------------------
// Recs: void load(j, &A, &B, &C, &t) = record j of a packed array.  The smallest key over records [first, end).
template <class Recs>
SMX_DIST_FN unsigned long long dist_walk(const Recs& recs, uint32_t first, uint32_t end, const TgVec& P, float max2, unsigned long long best,
                                         uint32_t stride = 1) {
  for (uint32_t j = first; j < end; j += stride) {
    TgVec A, B, C;
    uint32_t t;
    recs.load(j, &A, &B, &C, &t);
    const unsigned long long key = dist_key(P, A, B, C, t, max2);
    best = key < best ? key : best;
  }
  return best;
}
// The 27 cells around P's own, then the wide list.  A triangle met through two cells gives the same key twice.  This is one
// point's view of the query: k_dist_query makes the same look-ups once per cell and walks the same records from LDS, its lanes
// sharing a point's records by `stride`; the host walk calls it as it stands.
// neighbour k (0 <= k < 27) of the cell (cx, cy, cz), x fastest
SMX_DIST_FN unsigned long long dist_neighbour_key(int32_t cx, int32_t cy, int32_t cz, uint32_t k) {
  return dec_cell_key(cx + (int32_t)(k % 3) - 1, cy + (int32_t)((k / 3) % 3) - 1, cz + (int32_t)(k / 9) - 1);
}
template <class Tab, class Recs>
SMX_DIST_FN unsigned long long dist_query(const Tab& tab, uint32_t mask, const Recs& cell_recs, const Recs& wide_recs, uint32_t n_wide,
                                          const TgVec& P, float cell, float max2) {
  unsigned long long best = kTgNone;
  const int32_t cx = tg_cell(P.x, cell), cy = tg_cell(P.y, cell), cz = tg_cell(P.z, cell);
  for (uint32_t k = 0; k < 27; ++k) {
    uint32_t first, end;
    if (tg_table_find(tab, mask, dist_neighbour_key(cx, cy, cz, k), &first, &end)) best = dist_walk(cell_recs, first, end, P, max2, best);
  }
  return dist_walk(wide_recs, 0, n_wide, P, max2, best);
}

#if !defined(SMX_DISTANCE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of the device counters behind the grid's.  k_dist_stats adds to the three counts and to the histogram from every
// wavefront: they sit in different 64-byte blocks, as atomics on one block queue behind each other.
enum : int { kDistMatched = kTgWords, kDistBadPoints, kDistMaxBits, kDistHist = (kDistMaxBits / 16 + 1) * 16, kDistWords = kDistHist + kDistBins };
static_assert(kDistMaxBits < kDistHist && kDistHist % 16 == 0, "the counts, then the histogram in blocks of its own");

constexpr int kDistBlock = 256;                              // points per workgroup of the query's kernels

// The workspace, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so nothing
// reads a block that goes.
struct DistanceWork {
  TgWork grid;                             // the build's; keys / vals hold max(n_entries, n_points): the entries first, then the points
  DevBuf<float> recs, wide_recs;          // [n_entries] / [n_wide] TgRec, the first in the sorted order
  DevBuf<unsigned long long> table;        // [table entries][2] TgCell
  DevBuf<unsigned long long> best;         // [n_points] the winning key of every point
  DevBuf<uint32_t> in;                     // staging when the caller's arrays are host memory
  DevBuf<float> pts, out_distance, out_closest;
  DevBuf<uint32_t> out_nearest;
  DevBuf<uint32_t> counters;               // [kDistWords]
  PhaseStamps<SMX_DIST_PHASES> stamps;     // of the last call; a refused call publishes the phases it completed
};

// ---- the query of a kept index (smx_distscene) -------------------------------------------------------------------
// What a scene's query needs besides the index: the points' sort, the winning keys, the staging, its own counter words.
struct DistQueryWork {
  DevBuf<unsigned long long> keys[2];      // [n_points] the points' cell keys, sorted
  DevBuf<uint32_t> vals[2];
  DevBuf<uint32_t> hist;                   // the sort's workspace
  DevBuf<unsigned long long> best;         // [n_points] the winning key of every point
  DevBuf<float> pts, out_distance, out_closest;      // staging when the caller's arrays are host memory
  DevBuf<uint32_t> out_nearest;
  DevBuf<uint32_t> counters;               // [kDistWords]; only the words from kTgWords on are used
  unsigned long long bytes() const;
};
// A view of the index a scene keeps.  cnt = the build's device counters (c at [kTgCellBits]).
struct DistSceneIndex {
  const TgCell* table; uint32_t mask;
  const TgRec *recs, *wide_recs; uint32_t n_wide;
  const uint32_t* first_rec;
  const uint32_t* cnt;
};
// k_dist_point_keys -> the sort -> k_dscene_query -> k_dist_stats on st, synchronous: the query and stats phases of
// smx_recon_mesh_distance with the winner's corners read from the records (smx_distance.hip).  Every allocation lies before the
// first write to an output.  Fills the point words of *stats (may be null): n_bad_points, n_matched, max_dist2_bits, histogram.
int dist_scene_query(DistQueryWork& w, const DistSceneIndex& ix, const smx_distance_params* p, const float* points, uint32_t n_points,
                     uint32_t* nearest, float* distance, float* closest, bool on_device, hipStream_t st, PhaseStamps<2>& stamps,
                     smx_distance_stats* stats);
// Its enqueue-only half, which smx_distscene_register runs once per iteration: dist_scene_reserve holds every allocation (the
// counters, the winning keys, the points' sort) for n_points points, in the order the query always had; dist_scene_enqueue
// then launches k_dist_point_keys -> the sort -> k_dscene_query on st for device arrays and looks at nothing on the host.
int dist_scene_reserve(DistQueryWork& w, uint32_t n_points);
int dist_scene_enqueue(const DistQueryWork& w, const DistSceneIndex& ix, const float* dpts, uint32_t n_points, float max_distance,
                       int signed_distance, uint32_t* d_nearest, float* d_distance, float* d_closest, hipStream_t st);
#endif

}  // namespace smx
