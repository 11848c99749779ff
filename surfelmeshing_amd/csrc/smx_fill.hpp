// smx_fill.hpp -- small holes of the device mesh closed by fans (smx_recon_fill_holes).
//
// Part 1: the arithmetic and the table operations of the contract as plain inline functions (the edge key and its counter
// increment, insert and look-up in the open-addressing edge table templated on how an entry is read, claimed and bumped, the
// classification of an entry, the bounded walk along next, cost, apex key, the fan's triangle test).  smx_fill.hip calls them
// from its kernels; a test compiles this part alone for the host (SMX_FILL_HOST_ONLY) and walks the same passes with plain words.
// Part 2: the device-side records and the workspace the object keeps for the call (kernels and glue: smx_fill.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_FILL_HOST_ONLY)
#if !defined(SMX_MESH_HOST_ONLY)
#define SMX_MESH_HOST_ONLY 1
#endif
#if !defined(SMX_DECIMATE_HOST_ONLY)
#define SMX_DECIMATE_HOST_ONLY 1
#endif
#define SMX_FILL_FN static inline
#else
#include "smx_common.hpp"
#define SMX_FILL_FN __host__ __device__ __forceinline__
#endif
#include "smx_decimate.hpp"   // dec_live, dec_hash, dec_table_size, dec_value_word, DecTri, dec_canonical, dec_key_ab
#include "smx_mesh.hpp"       // MeshVec, mesh_triangle_filter

namespace smx {

constexpr uint32_t kFillMaxHoleEdges = 32;                  // SMX_FILL_MAX_HOLE_EDGES: one lane of a half wavefront per loop vertex
constexpr unsigned long long kFillEmpty = 0ull;             // an entry's key word is the pair's key + 1: zeroed memory is an empty table
constexpr uint32_t kFillInterior = 0, kFillBoundaryUp = 1, kFillBoundaryDown = 2, kFillNonManifold = 3;

// ---- the edge table: 16-byte entries (key + 1, g << 32 | f), open addressing, linear probing -----------------------------
SMX_FILL_FN unsigned long long fill_edge_key(uint32_t u, uint32_t v) {
  const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
  return ((unsigned long long)lo << 32) | hi;
}
// what the half-edge u -> v adds to its pair's value word: f counts min -> max (and u -> u), g counts max -> min
SMX_FILL_FN unsigned long long fill_edge_inc(uint32_t u, uint32_t v) { return u <= v ? 1ull : 1ull << 32; }

// Tab: unsigned long long key(h) (a plain read), unsigned long long claim(h, expected, desired) (compare-and-swap on the key
// word, returns the old word), void bump(h, inc) (add to the value word).  The table has at least twice as many entries as
// half-edges are inserted, so an empty entry ends every chain.  Returns true iff this insert claimed the entry.
template <class Tab>
SMX_FILL_FN bool fill_insert(Tab& t, uint32_t mask, uint32_t u, uint32_t v) {
  const unsigned long long key = fill_edge_key(u, v);
  uint32_t h = dec_hash(key, mask);
  bool claimed = false;
  for (;;) {
    const unsigned long long prev = t.claim(h, kFillEmpty, key + 1);
    if (prev == kFillEmpty) claimed = true;
    if (prev == kFillEmpty || prev == key + 1) break;
    h = (h + 1) & mask;
  }
  t.bump(h, fill_edge_inc(u, v));
  return claimed;
}
// Is {u, v} a pair of R?  (after the inserts: plain reads)
template <class Tab>
SMX_FILL_FN bool fill_has_edge(const Tab& t, uint32_t mask, uint32_t u, uint32_t v) {
  const unsigned long long key = fill_edge_key(u, v);
  for (uint32_t h = dec_hash(key, mask);; h = (h + 1) & mask) {
    const unsigned long long k = t.key(h);
    if (k == key + 1) return true;
    if (k == kFillEmpty) return false;
  }
}
SMX_FILL_FN uint32_t fill_classify(unsigned long long value) {
  const uint32_t f = (uint32_t)value, g = (uint32_t)(value >> 32);
  if (f == 1 && g == 1) return kFillInterior;
  if (f == 1 && g == 0) return kFillBoundaryUp;      // the triangle's half-edge is lo -> hi: the gap is hi -> lo
  if (f == 0 && g == 1) return kFillBoundaryDown;    // ... hi -> lo: the gap is lo -> hi
  return kFillNonManifold;
}

// ---- loops ---------------------------------------------------------------------------------------------------------------
// deg[2 w] = out(w), deg[2 w + 1] = in(w); next[w] is read only where out(w) == 1, i.e. where exactly one lane stored it.
SMX_FILL_FN bool fill_simple(const uint32_t* deg, uint32_t w) { return deg[2 * (size_t)w] == 1 && deg[2 * (size_t)w + 1] == 1; }
// The length of the loop w owns, 0 if it owns none of at most max_edges edges: the walk stops at a vertex that is not simple
// and at a slot below w (then the loop, if it is one, belongs to a smaller slot), after max_edges steps at the latest.
SMX_FILL_FN uint32_t fill_walk(const uint32_t* deg, const uint32_t* next, uint32_t w, uint32_t max_edges) {
  if (!fill_simple(deg, w)) return 0;
  uint32_t cur = next[w], steps = 1;
  while (cur != w) {
    if (steps == max_edges || cur < w || !fill_simple(deg, cur)) return 0;
    cur = next[cur];
    ++steps;
  }
  return steps;
}

// ---- the fan -------------------------------------------------------------------------------------------------------------
// (d_x d_x + d_y d_y) + d_z d_z with d = other - at; no contraction (-ffp-contract=off)
SMX_FILL_FN float fill_d2(const MeshVec& at, const MeshVec& other) {
  const float dx = other.x - at.x, dy = other.y - at.y, dz = other.z - at.z;
  return (dx * dx + dy * dy) + dz * dz;
}
// Vecs: MeshVec operator[](uint32_t j) = the position of w_j.  cost(i): the squared lengths of the fan's diagonals from w_i.
template <class Vecs>
SMX_FILL_FN float fill_cost(const Vecs& pos, uint32_t L, uint32_t i) {
  float c = 0.0f;
  for (uint32_t k = 2; k + 2 <= L; ++k) c += fill_d2(pos[i], pos[(i + k) % L]);
  return c;
}
// Fan triangle k (1 <= k <= L - 2) from apex i: true iff the triangle filter gives 1 for (w_i, w_{i+k}, w_{i+k+1}).
template <class Vecs>
SMX_FILL_FN bool fill_fan_ok(const Vecs& pos, const Vecs& nrm, uint32_t L, uint32_t i, uint32_t k, float cos_min_angle, float cos_max_angle) {
  const uint32_t a = (i + k) % L, b = (i + k + 1) % L;
  return mesh_triangle_filter(pos[i], pos[a], pos[b], nrm[i], nrm[a], nrm[b], cos_min_angle, cos_max_angle) == 1;
}

#if !defined(SMX_FILL_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
enum : int { kFillNotLive = 0, kFillEdges, kFillBoundary, kFillNonManifoldEdges, kFillPinched, kFillListed, kFillFilled,
             kFillDiagonal, kFillFilter, kFillNew, kFillKept, kFillError, kFillWords = 12 };

struct FillEdge { unsigned long long key, value; };         // one 16-byte entry of the edge table
static_assert(sizeof(FillEdge) == 16, "one 16-byte entry per pair");
static_assert(sizeof(smx_mesh_hole) == 12, "smx_mesh_hole is 12 bytes");

// The map as in mesh_triangulate: smooth position (x, y, z, -) of slot i at smooth[i * smooth_stride], (normal, RadiusSquared)
// at normal[i * normal_stride].
struct FillMap {
  const float4* smooth; size_t smooth_stride;
  const float4* normal; size_t normal_stride;
  uint32_t n;
};

constexpr int kFillBlock = 256;                             // triangles (or slots, or entries) per workgroup; 8 loops in the fill kernel

// The workspace, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so nothing
// reads a block that goes.
struct FillWork {
  DevBuf<unsigned long long> table;        // [entries][2] FillEdge
  DevBuf<uint32_t> keep;                   // [n_in] 1 = the triangle is in R
  DevBuf<uint32_t> deg;                    // [n][2] out, in
  DevBuf<uint32_t> next;                   // [n]
  DevBuf<uint32_t> len;                    // [n] the length of the listed loop the slot owns, else 0
  DevBuf<uint32_t> tblocks, vblocks;       // triangles of R / owners per workgroup, then their offsets
  DevBuf<uint32_t> holes;                  // [n_listed] smx_mesh_hole
  DevBuf<uint32_t> fresh;                  // [n_new] DecTri, in the order the loops' groups arrived (the sort removes it)
  DevBuf<unsigned long long> keys[2];      // [n_new] the sort's records
  DevBuf<uint32_t> vals[2];
  DevBuf<uint32_t> hist;                   // the sort's workspace
  DevBuf<uint32_t> in, out;                // staging when the caller's arrays are host memory
  DevBuf<uint32_t> counters;               // [kFillWords]
  PhaseStamps<SMX_FILL_PHASES> stamps;     // of the last call; a refused call publishes the phases it completed
};
#endif

}  // namespace smx
