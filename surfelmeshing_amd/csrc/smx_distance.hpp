// smx_distance.hpp -- the distance from points to a triangle array over the map (smx_recon_mesh_distance).
//
// Part 1: the arithmetic and the cell functions of the contract as plain inline functions (step 1's classes, the closest point
// of Ericson's regions with its squared distance and sign, the cell of a coordinate, the box of a triangle and its entry count,
// the cell table's insert and look-up templated on how an entry is read, claimed and bumped, the walk of a cell's records, the
// histogram bin).  smx_distance.hip calls them from its kernels; a test compiles this part alone for the host
// (SMX_DISTANCE_HOST_ONLY) and walks the same passes with plain words.
// Part 2: the device-side records and the workspace the object keeps for the call (kernels and glue: smx_distance.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_DISTANCE_HOST_ONLY)
#if !defined(SMX_DECIMATE_HOST_ONLY)
#define SMX_DECIMATE_HOST_ONLY 1
#endif
#define SMX_DIST_FN static inline
#else
#include "smx_common.hpp"
#define SMX_DIST_FN __host__ __device__ __forceinline__
#endif
#include "smx_decimate.hpp"   // dec_live, dec_finite, dec_hash, dec_table_size, dec_cell_key, dec_value_word

namespace smx {

constexpr float kDistMaxCoord = 64.0f;                      // SMX_DIST_MAX_COORD
constexpr uint32_t kDistWideCells = 64;                     // SMX_DIST_WIDE_CELLS
constexpr uint32_t kDistBins = 32;                          // SMX_DIST_BINS
constexpr float kDistMargin = 1.125f;                       // c >= kDistMargin * max_distance (why that is enough)
constexpr unsigned long long kDistNone = ~0ull;             // the key of "no candidate"
constexpr unsigned long long kDistEmpty = 0ull;             // a table entry's key word is the cell key + 1: zeroed memory is empty
constexpr uint32_t kDistWide = 0x80000000u;                 // the mark word of a triangle on the wide list (else: its entry count)
enum : uint32_t { kDistInR = 0, kDistDropNotLive = 1, kDistDropRepeated = 2, kDistDropRange = 3 };
enum : uint32_t { kDistRegionA = 0, kDistRegionB, kDistRegionAB, kDistRegionC, kDistRegionAC, kDistRegionBC, kDistRegionInside };

struct DistVec { float x, y, z; };
SMX_DIST_FN DistVec dist_sub(const DistVec& a, const DistVec& b) { return DistVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
SMX_DIST_FN DistVec dist_add(const DistVec& a, const DistVec& b) { return DistVec{a.x + b.x, a.y + b.y, a.z + b.z}; }
SMX_DIST_FN DistVec dist_scale(float s, const DistVec& a) { return DistVec{s * a.x, s * a.y, s * a.z}; }
SMX_DIST_FN float dist_dot(const DistVec& u, const DistVec& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
SMX_DIST_FN DistVec dist_cross(const DistVec& u, const DistVec& v) {
  return DistVec{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

// ---- step 1 and step 2 ---------------------------------------------------------------------------------------------------
SMX_DIST_FN bool dist_coord_ok(float v) { return dec_finite(v) && !(v > kDistMaxCoord) && !(v < -kDistMaxCoord); }
SMX_DIST_FN bool dist_point_ok(const DistVec& p) { return dist_coord_ok(p.x) && dist_coord_ok(p.y) && dist_coord_ok(p.z); }
// The class of a triangle whose three indices are in range; live0..2 = dec_live of its corners.
SMX_DIST_FN uint32_t dist_classify(uint32_t i0, uint32_t i1, uint32_t i2, bool live0, bool live1, bool live2, const DistVec& a,
                                   const DistVec& b, const DistVec& c) {
  if (!(live0 && live1 && live2)) return kDistDropNotLive;
  if (i0 == i1 || i1 == i2 || i0 == i2) return kDistDropRepeated;
  if (!(dist_point_ok(a) && dist_point_ok(b) && dist_point_ok(c))) return kDistDropRange;
  return kDistInR;
}

// ---- step 3: the closest point of P on (A, B, C), Ericson's regions in the contract's order ------------------------------
SMX_DIST_FN DistVec dist_closest(const DistVec& P, const DistVec& A, const DistVec& B, const DistVec& C, uint32_t* region) {
  const DistVec ab = dist_sub(B, A), ac = dist_sub(C, A), ap = dist_sub(P, A);
  const float d1 = dist_dot(ab, ap), d2 = dist_dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) { *region = kDistRegionA; return A; }
  const DistVec bp = dist_sub(P, B);
  const float d3 = dist_dot(ab, bp), d4 = dist_dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) { *region = kDistRegionB; return B; }
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    const float v = d1 / (d1 - d3);
    *region = kDistRegionAB;
    return dist_add(A, dist_scale(v, ab));
  }
  const DistVec cp = dist_sub(P, C);
  const float d5 = dist_dot(ab, cp), d6 = dist_dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) { *region = kDistRegionC; return C; }
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    const float w = d2 / (d2 - d6);
    *region = kDistRegionAC;
    return dist_add(A, dist_scale(w, ac));
  }
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
    const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    *region = kDistRegionBC;
    return dist_add(B, dist_scale(w, dist_sub(C, B)));
  }
  const float s = (va + vb) + vc;
  float v = vb / s, w = vc / s;
  // exact arithmetic arrives here with va, vb, vc > 0; float32 may not, so v and w are held to the triangle (a NaN stays one)
  v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  const float lim = 1.0f - v;
  w = w < 0.0f ? 0.0f : (w > lim ? lim : w);
  *region = kDistRegionInside;
  return dist_add(dist_add(A, dist_scale(v, ab)), dist_scale(w, ac));
}
SMX_DIST_FN float dist_dist2(const DistVec& P, const DistVec& Q) { const DistVec e = dist_sub(P, Q); return dist_dot(e, e); }
// The key of triangle t for P: (float_bits(dist2) << 32) | t if it is a candidate, kDistNone otherwise (NaN never is).
SMX_DIST_FN unsigned long long dist_key(const DistVec& P, const DistVec& A, const DistVec& B, const DistVec& C, uint32_t t, float max2) {
  uint32_t region;
  const float d2 = dist_dist2(P, dist_closest(P, A, B, C, &region));
  return d2 <= max2 ? dec_value_word(d2, t) : kDistNone;
}
SMX_DIST_FN float dist_key_dist2(unsigned long long key) {
  const uint32_t bits = (uint32_t)(key >> 32);
  float d2;
  __builtin_memcpy(&d2, &bits, sizeof(d2));
  return d2;
}
SMX_DIST_FN bool dist_negative(const DistVec& P, const DistVec& Q, const DistVec& A, const DistVec& B, const DistVec& C) {
  return dist_dot(dist_sub(P, Q), dist_cross(dist_sub(B, A), dist_sub(C, A))) < 0.0f;
}
SMX_DIST_FN uint32_t dist_bin(float abs_distance, float max_distance) {
  const uint32_t b = (uint32_t)((abs_distance * 32.0f) / max_distance);
  return b < kDistBins - 1 ? b : kDistBins - 1;
}

// ---- the grid ------------------------------------------------------------------------------------------------------------
SMX_DIST_FN float dist_cell_size(float cell_size, float max_distance) {
  const float least = kDistMargin * max_distance;
  return cell_size > least ? cell_size : least;
}
// |x| <= 64 and c >= 1.125e-3: |x / c| < 2^16, so the cell fits the 21 bits of dec_cell_key with room for the +-1 of a query
SMX_DIST_FN int32_t dist_cell(float x, float c) { return (int32_t)floorf(x / c); }
SMX_DIST_FN float dist_min3(float a, float b, float c) { const float m = a < b ? a : b; return m < c ? m : c; }
SMX_DIST_FN float dist_max3(float a, float b, float c) { const float m = a > b ? a : b; return m > c ? m : c; }
// the largest of the three extents of the triangle's box (cell_size == 0 takes their mean over R)
SMX_DIST_FN float dist_extent(const DistVec& a, const DistVec& b, const DistVec& c) {
  return dist_max3(dist_max3(a.x, b.x, c.x) - dist_min3(a.x, b.x, c.x), dist_max3(a.y, b.y, c.y) - dist_min3(a.y, b.y, c.y),
                   dist_max3(a.z, b.z, c.z) - dist_min3(a.z, b.z, c.z));
}
struct DistBox { int32_t lo[3], hi[3]; };
SMX_DIST_FN DistBox dist_box(const DistVec& a, const DistVec& b, const DistVec& c, float cell) {
  DistBox box;
  box.lo[0] = dist_cell(dist_min3(a.x, b.x, c.x), cell); box.hi[0] = dist_cell(dist_max3(a.x, b.x, c.x), cell);
  box.lo[1] = dist_cell(dist_min3(a.y, b.y, c.y), cell); box.hi[1] = dist_cell(dist_max3(a.y, b.y, c.y), cell);
  box.lo[2] = dist_cell(dist_min3(a.z, b.z, c.z), cell); box.hi[2] = dist_cell(dist_max3(a.z, b.z, c.z), cell);
  return box;
}
// The mark word of a triangle of R: the number of cells of its box, or kDistWide above kDistWideCells.
SMX_DIST_FN uint32_t dist_mark(const DistBox& box) {
  unsigned long long cells = 1;
  for (int k = 0; k < 3; ++k) {
    const unsigned long long d = (unsigned long long)(box.hi[k] - box.lo[k]) + 1ull;    // (at most 2^17 + 1 each)
    cells = cells * d > 0xFFFFFFFFull ? 0xFFFFFFFFull : cells * d;
  }
  return cells > kDistWideCells ? kDistWide : (uint32_t)cells;
}
// Cell number j (0 <= j < the mark word) of the box, x fastest.
SMX_DIST_FN unsigned long long dist_box_key(const DistBox& box, uint32_t j) {
  const uint32_t nx = (uint32_t)(box.hi[0] - box.lo[0]) + 1u, ny = (uint32_t)(box.hi[1] - box.lo[1]) + 1u;
  return dec_cell_key(box.lo[0] + (int32_t)(j % nx), box.lo[1] + (int32_t)((j / nx) % ny), box.lo[2] + (int32_t)(j / (nx * ny)));
}

// ---- the cell table: 16-byte entries (cell key + 1, first | end << 32 of the cell's run in the sorted entries) --------------
// Tab: unsigned long long key(h), unsigned long long value(h) (plain reads), unsigned long long claim(h, expected, desired)
// (compare-and-swap on the key word, returns the old word), void bump(h, inc) (add to the value word).  The table has at least
// twice as many entries as there are cells.  The head of a run adds its position, the tail its position + 1 in the upper half.
template <class Tab>
SMX_DIST_FN void dist_table_add(Tab& t, uint32_t mask, unsigned long long cell_key, unsigned long long inc) {
  uint32_t h = dec_hash(cell_key, mask);
  for (;;) {
    const unsigned long long prev = t.claim(h, kDistEmpty, cell_key + 1);
    if (prev == kDistEmpty || prev == cell_key + 1) break;
    h = (h + 1) & mask;
  }
  t.bump(h, inc);
}
// entry j of the sorted (key, t) pairs: what it adds to the table, if anything
template <class Tab>
SMX_DIST_FN bool dist_table_entry(Tab& t, uint32_t mask, const unsigned long long* keys, uint32_t n_entries, uint32_t j) {
  const unsigned long long k = keys[j];
  const bool head = j == 0 || keys[j - 1] != k, tail = j + 1 == n_entries || keys[j + 1] != k;
  if (head || tail) dist_table_add(t, mask, k, (head ? (unsigned long long)j : 0ull) + (tail ? (unsigned long long)(j + 1) << 32 : 0ull));
  return head;
}
// The run [first, end) of a cell; false if the cell is empty.  (after the inserts: plain reads)
template <class Tab>
SMX_DIST_FN bool dist_table_find(const Tab& t, uint32_t mask, unsigned long long cell_key, uint32_t* first, uint32_t* end) {
  for (uint32_t h = dec_hash(cell_key, mask);; h = (h + 1) & mask) {
    const unsigned long long k = t.key(h);
    if (k == cell_key + 1) {
      const unsigned long long v = t.value(h);
      *first = (uint32_t)v; *end = (uint32_t)(v >> 32);
      return true;
    }
    if (k == kDistEmpty) return false;
  }
}

// ---- the query of one point ----------------------------------------------------------------------------------------------
// Recs: void load(j, &A, &B, &C, &t) = record j of a packed array.  The smallest key over records [first, end).
template <class Recs>
SMX_DIST_FN unsigned long long dist_walk(const Recs& recs, uint32_t first, uint32_t end, const DistVec& P, float max2, unsigned long long best,
                                         uint32_t stride = 1) {
  for (uint32_t j = first; j < end; j += stride) {
    DistVec A, B, C;
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
                                          const DistVec& P, float cell, float max2) {
  unsigned long long best = kDistNone;
  const int32_t cx = dist_cell(P.x, cell), cy = dist_cell(P.y, cell), cz = dist_cell(P.z, cell);
  for (uint32_t k = 0; k < 27; ++k) {
    uint32_t first, end;
    if (dist_table_find(tab, mask, dist_neighbour_key(cx, cy, cz, k), &first, &end)) best = dist_walk(cell_recs, first, end, P, max2, best);
  }
  return dist_walk(wide_recs, 0, n_wide, P, max2, best);
}

#if !defined(SMX_DISTANCE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of the device counters: [kDistCellBits] = c as its bits, [kDistExtentLo / Hi] = the sum of the extents in 2^-20 m,
// [kDistEntries64Lo / Hi] = the entries as a 64-bit sum (the scan's 32-bit total must not have wrapped)
enum : int { kDistNotLive = 0, kDistRepeated, kDistRange, kDistInRCount, kDistNWide, kDistEntries, kDistCells, kDistBadPoints, kDistMatched,
             kDistMaxBits, kDistError, kDistCellBits, kDistExtentLo, kDistExtentHi, kDistEntries64Lo, kDistEntries64Hi, kDistHist = 16, kDistWords = kDistHist + 32 };

struct DistRec { float4 a, b, c; };                          // corners in input order; a.w = the bits of t
struct DistCell { unsigned long long key, value; };          // one 16-byte entry of the cell table
static_assert(sizeof(DistRec) == 48 && sizeof(DistCell) == 16, "packed records");

// The map as in mesh_triangulate: smooth position (x, y, z, -) of slot i at smooth[i * smooth_stride], (normal, RadiusSquared)
// at normal[i * normal_stride].
struct DistMap {
  const float4* smooth; size_t smooth_stride;
  const float4* normal; size_t normal_stride;
  uint32_t n;
};

constexpr int kDistBlock = 256;                              // triangles (or entries, or points) per workgroup of every kernel

// The workspace, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so nothing
// reads a block that goes.
struct DistanceWork {
  DevBuf<uint32_t> mark;                   // [n_in] entry count of the triangle, kDistWide, or 0 (not in R)
  DevBuf<uint32_t> blocks;                 // entries per workgroup, then their offsets
  DevBuf<uint32_t> wide_t;                 // [n_wide] the wide list, in arrival order (the minimum does not depend on it)
  DevBuf<unsigned long long> keys[2];      // [max(n_entries, n_points)] the sort's records: the entries first, then the points
  DevBuf<uint32_t> vals[2];
  DevBuf<uint32_t> hist;                   // the sort's workspace
  DevBuf<float> recs, wide_recs;           // [n_entries] / [n_wide] DistRec, the first in the sorted order
  DevBuf<unsigned long long> table;        // [table entries][2] DistCell
  DevBuf<unsigned long long> best;         // [n_points] the winning key of every point
  DevBuf<uint32_t> in;                     // staging when the caller's arrays are host memory
  DevBuf<float> pts, out_distance, out_closest;
  DevBuf<uint32_t> out_nearest;
  DevBuf<uint32_t> counters;               // [kDistWords]
  PhaseStamps<SMX_DIST_PHASES> stamps;     // of the last call; a refused call publishes the phases it completed
};
#endif

}  // namespace smx
