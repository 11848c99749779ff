// smx_decimate.hpp -- decimation of the device mesh by vertex clustering (smx_recon_decimate_mesh).
//
// Part 1: the arithmetic of the contract as plain inline functions (cell coordinate with its range check, cell key, centre,
// squared distance to the centre, the 64-bit value word, the canonical rotation of a triple).  smx_decimate.hip calls them
// from its kernels; a test compiles this part alone for the host (SMX_DECIMATE_HOST_ONLY) and walks the same passes.
// Part 2: the device-side records and the workspace the object keeps for the call (kernels and glue: smx_decimate.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_DECIMATE_HOST_ONLY)
#include <math.h>
#define SMX_DEC_FN static inline
#else
#include "smx_common.hpp"
#define SMX_DEC_FN __host__ __device__ __forceinline__
#endif

namespace smx {

constexpr int32_t kDecCellLimit = 1 << 20;                  // cell coordinates lie in [-2^20, 2^20): 21 bits each
constexpr unsigned long long kDecEmpty = ~0ull;             // no key has bit 63 set, and no value word is all ones
constexpr uint32_t kDecNoSlot = 0xFFFFFFFFu;                // vertex_map of a slot outside U; "no triangle" in the tables

// Live as in smx_recon_triangulate: not merged, and a finite smooth position.
SMX_DEC_FN bool dec_finite(float v) { return v - v == 0.0f; }
SMX_DEC_FN bool dec_live(float x, float y, float z, float radius_squared) {
  return !(radius_squared < 0.0f) && dec_finite(x) && dec_finite(y) && dec_finite(z);
}

// c = (int32)floorf(x * inv) with inv = 1.0f / cell_size formed once on the host; false if c is outside the 21 bits.
SMX_DEC_FN bool dec_cell_coord(float x, float inv, int32_t* c) {
  const float f = floorf(x * inv);
  if (!(f >= -1048576.0f && f < 1048576.0f)) return false;
  *c = (int32_t)f;
  return true;
}

SMX_DEC_FN unsigned long long dec_cell_key(int32_t cx, int32_t cy, int32_t cz) {
  return ((unsigned long long)(uint32_t)(cx + kDecCellLimit) << 42) | ((unsigned long long)(uint32_t)(cy + kDecCellLimit) << 21) |
         (unsigned long long)(uint32_t)(cz + kDecCellLimit);
}

SMX_DEC_FN float dec_cell_centre(int32_t c, float cell_size) { return ((float)c + 0.5f) * cell_size; }

// (d_x d_x + d_y d_y) + d_z d_z with d = position - centre of its cell; no contraction (-ffp-contract=off)
SMX_DEC_FN float dec_d2(float x, float y, float z, int32_t cx, int32_t cy, int32_t cz, float cell_size) {
  const float dx = x - dec_cell_centre(cx, cell_size), dy = y - dec_cell_centre(cy, cell_size), dz = z - dec_cell_centre(cz, cell_size);
  return (dx * dx + dy * dy) + dz * dz;
}

// The word whose minimum over a cell names its representative: d2 is a non-negative float, so its bit pattern orders as
// its value does, and a tie goes to the lower slot.
SMX_DEC_FN unsigned long long dec_value_word(float d2, uint32_t slot) {
  uint32_t bits;
  __builtin_memcpy(&bits, &d2, sizeof(bits));
  return ((unsigned long long)bits << 32) | slot;
}
SMX_DEC_FN uint32_t dec_word_slot(unsigned long long word) { return (uint32_t)word; }

// Start of a probe chain in a table of mask + 1 entries (a power of two): murmur3's 64-bit finaliser.
SMX_DEC_FN uint32_t dec_hash(unsigned long long k, uint32_t mask) {
  k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull; k ^= k >> 33;
  return (uint32_t)k & mask;
}

struct DecTri { uint32_t p, a, b; };

// (r0, r1, r2) rotated so that its smallest index comes first; the winding is kept.  Corners are pairwise different.
SMX_DEC_FN DecTri dec_canonical(uint32_t r0, uint32_t r1, uint32_t r2) {
  if (r0 < r1 && r0 < r2) return DecTri{r0, r1, r2};
  if (r1 < r2) return DecTri{r1, r2, r0};
  return DecTri{r2, r0, r1};
}
SMX_DEC_FN bool dec_collapsed(uint32_t r0, uint32_t r1, uint32_t r2) { return r0 == r1 || r1 == r2 || r0 == r2; }
// The same set of three corners, in either winding (both canonical: p is the smallest of each).
SMX_DEC_FN bool dec_same_corners(const DecTri& s, const DecTri& t) {
  return s.p == t.p && ((s.a == t.a && s.b == t.b) || (s.a == t.b && s.b == t.a));
}
SMX_DEC_FN uint32_t dec_tri_hash(const DecTri& t, uint32_t mask) {
  const uint32_t lo = t.a < t.b ? t.a : t.b, hi = t.a < t.b ? t.b : t.a;
  return dec_hash(((unsigned long long)t.p << 42) ^ ((unsigned long long)lo << 21) ^ (unsigned long long)hi ^
                  ((unsigned long long)hi << 50), mask);
}

// Sort keys of the output order (p, a, b): `bits` = bit length of the largest slot index, at most 32.
SMX_DEC_FN unsigned long long dec_key_ab(const DecTri& t, int bits) { return ((unsigned long long)t.a << bits) | t.b; }

// Table sizes: a power of two of at least twice the entries, so that linear probing ends at an empty entry.
SMX_DEC_FN uint32_t dec_table_size(uint32_t entries) {
  uint32_t s = 64;
  while (s < 0x80000000u && (unsigned long long)s < 2ull * entries) s <<= 1;
  return s;
}

#if !defined(SMX_DECIMATE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
enum : int { kDecNotLive = 0, kDecUsed, kDecCells, kDecCollapsed, kDecAlive, kDecTotal, kDecError, kDecWords = 8 };
enum : uint32_t { kDecErrIndex = 1u, kDecErrRange = 2u };   // bits of the device error word

struct DecCell { unsigned long long key, word; };           // one 16-byte entry of the cell table

// The map as in mesh_triangulate: smooth position (x, y, z, -) of slot i at smooth[i * smooth_stride], (normal, RadiusSquared)
// at normal[i * normal_stride].
struct DecMap {
  const float4* smooth; size_t smooth_stride;
  const float4* normal; size_t normal_stride;
  uint32_t n;
};

constexpr int kDecBlock = 256;                              // triangles (or slots) per workgroup of every kernel

// The workspace, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so nothing
// reads a block that goes.
struct DecimateWork {
  DevBuf<uint32_t> vmap;                   // [n] the vertex map
  DevBuf<unsigned long long> cells;        // [cell table entries][2]: key, value word (DecCell)
  DevBuf<uint32_t> canon, own;             // [n_in][3] canonical triples (DecTri); [n_in] each triangle's entry of
  DevBuf<uint32_t> dup;                    // the table of triangle indices
  DevBuf<uint32_t> blocks;                 // survivors per workgroup, then their offsets
  DevBuf<unsigned long long> keys[2];      // [T_out] the sort's records
  DevBuf<uint32_t> vals[2];
  DevBuf<uint32_t> hist;                   // the sort's workspace
  DevBuf<uint32_t> in, out;                // staging when the caller's arrays are host memory
  DevBuf<uint32_t> counters;               // [kDecWords]
  PhaseStamps<SMX_DECIMATE_PHASES> stamps; // of the last call; a refused call publishes the phases it completed
};
#endif

}  // namespace smx
