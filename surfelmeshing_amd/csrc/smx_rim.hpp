// smx_rim.hpp -- the rim of a triangle array over the map: which corners and edges of a triangle lie on the boundary of the
// surface the array shows (smx_recon_mesh_rim).
//
// Part 1: the integer rules of the contract as plain inline functions (the number of triangles on an edge from its entry of
// smx_fill.hpp's edge table, the look-up of an edge of R, the once-only mark of a non-manifold entry, the bits an edge and a
// corner add to the byte, the word and the bit of a slot in the rim-vertex bitmap).  The table's entry, key and insert are
// smx_fill.hpp's.  smx_rim.hip calls these from its kernels; a test compiles this part alone for the host (SMX_RIM_HOST_ONLY)
// and walks the same passes with plain words.
// Part 2: the counter words and the workspace the object keeps for the call (kernels and glue: smx_rim.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_RIM_HOST_ONLY)
#if !defined(SMX_FILL_HOST_ONLY)
#define SMX_FILL_HOST_ONLY 1
#endif
#if !defined(SMX_TRIGRID_HOST_ONLY)
#define SMX_TRIGRID_HOST_ONLY 1
#endif
#endif
#include "smx_fill.hpp"       // fill_edge_key, fill_insert, kFillEmpty: the edge table
#include "smx_trigrid.hpp"    // tg_classify: R is the triangle set of smx_recon_mesh_distance
#define SMX_RIM_FN SMX_TG_FN

namespace smx {

// The byte of a triangle: bit k = region k of smx_distance.hpp (A, B, AB, C, AC, BC); region 6, inside, has no bit.
constexpr uint32_t kRimBitA = 1u << 0, kRimBitB = 1u << 1, kRimBitAB = 1u << 2, kRimBitC = 1u << 3, kRimBitAC = 1u << 4, kRimBitBC = 1u << 5;
constexpr uint32_t kRimInR = 1u << 7;                       // between the passes only: the triangle is in R
// An entry's value word is f | g << 32 with f and g below 2^31 (at most 3 * 2^28 half-edges): bit 63 is free.  The first lane
// that finds an entry with three triangles or more sets it, and is the one that counts the entry.
constexpr unsigned long long kRimSeen = 1ull << 63;

// c(u, v): the half-edges of R on the pair, whatever their direction
SMX_RIM_FN uint32_t rim_count(unsigned long long value) { return (uint32_t)value + (uint32_t)((value & ~kRimSeen) >> 32); }
// The entry of {u, v}, a pair of R.  (after the inserts: plain reads; the pair is there, so the chain ends)
// Tab: unsigned long long key(h), value(h) (plain reads), unsigned long long mark(h, bits) (or into the value word, returns the
// old word), and smx_fill.hpp's claim and bump.
template <class Tab>
SMX_RIM_FN uint32_t rim_find(const Tab& t, uint32_t mask, uint32_t u, uint32_t v) {
  const unsigned long long key = fill_edge_key(u, v);
  uint32_t h = dec_hash(key, mask);
  while (t.key(h) != key + 1) h = (h + 1) & mask;
  return h;
}
// c of the pair; *first_nonmanifold = this lane is the first to see that the pair has three triangles or more
template <class Tab>
SMX_RIM_FN uint32_t rim_edge(Tab& t, uint32_t mask, uint32_t u, uint32_t v, bool* first_nonmanifold) {
  const uint32_t h = rim_find(t, mask, u, v);
  const uint32_t c = rim_count(t.value(h));
  *first_nonmanifold = c >= 3 && (t.mark(h, kRimSeen) & kRimSeen) == 0;
  return c;
}
// the edge bits of a triangle (A, B, C) from the counts of its three pairs
SMX_RIM_FN uint32_t rim_edge_bits(uint32_t c_ab, uint32_t c_bc, uint32_t c_ca) {
  return (c_ab == 1 ? kRimBitAB : 0u) | (c_ca == 1 ? kRimBitAC : 0u) | (c_bc == 1 ? kRimBitBC : 0u);
}
// which of its own corners the triangle's rim edges end in: bit 0 = A, bit 1 = B, bit 2 = C
SMX_RIM_FN uint32_t rim_corner_marks(uint32_t edge_bits) {
  return ((edge_bits & (kRimBitAB | kRimBitAC)) ? 1u : 0u) | ((edge_bits & (kRimBitAB | kRimBitBC)) ? 2u : 0u) |
         ((edge_bits & (kRimBitAC | kRimBitBC)) ? 4u : 0u);
}
// the rim-vertex bitmap: one bit per slot
SMX_RIM_FN uint32_t rim_word(uint32_t slot) { return slot >> 5; }
SMX_RIM_FN uint32_t rim_bit(uint32_t slot) { return 1u << (slot & 31u); }
SMX_RIM_FN bool rim_vertex(const uint32_t* bitmap, uint32_t slot) { return (bitmap[rim_word(slot)] & rim_bit(slot)) != 0; }
// the byte: the edge bits, and a corner's bit where the slot ends a rim edge of ANY triangle of R
SMX_RIM_FN uint32_t rim_byte(uint32_t edge_bits, bool a, bool b, bool c) {
  return edge_bits | (a ? kRimBitA : 0u) | (b ? kRimBitB : 0u) | (c ? kRimBitC : 0u);
}
// "the closest point lies on the rim": region as dist_closest reports it
SMX_RIM_FN bool rim_hit(uint32_t byte, uint32_t region) { return ((byte >> region) & 1u) != 0; }

#if !defined(SMX_RIM_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
enum : int { kRimNotLive = 0, kRimRepeated, kRimRange, kRimError, kRimEdges, kRimRimEdges, kRimNonManifold, kRimVertices, kRimTriangles,
             kRimWords = 16 };

constexpr int kRimBlock = 256;                               // triangles per workgroup of every kernel

// The workspace, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so nothing
// reads a block that goes.
struct RimWork {
  DevBuf<uint32_t> counters;               // [kRimWords]
  DevBuf<unsigned long long> table;        // [entries][2] FillEdge
  DevBuf<uint32_t> bitmap;                 // [ceil(n / 32)] the rim vertices
  DevBuf<uint8_t> bytes;                   // [n_in] kRimInR after the first pass, the edge bits after the second, the byte after the third
  DevBuf<uint32_t> in;                     // staging when the caller's array is host memory
};
// The three passes of smx_recon_mesh_rim on st, synchronous: every allocation, the launches, the one read of the counters.  n =
// the map's slots.  *d_rim = the bytes in the object's workspace (device memory, until its next call); *stats is written on
// success only.  SMX_ERR_INVALID_ARGUMENT with the error text set on an index >= n.  (smx_rim.hip)
int rim_run(smx_recon r, hipStream_t st, const uint32_t* triangles, uint32_t n_in, bool on_device, uint32_t n, const uint8_t** d_rim,
            smx_rim_stats* stats);
#endif

}  // namespace smx
