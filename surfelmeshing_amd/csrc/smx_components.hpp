// smx_components.hpp -- connected components of the device mesh (smx_recon_mesh_components).
//
// Part 1: the arithmetic of the contract as plain inline functions (the order key of a float and its inverse, diag2, the
// pass predicate, the rank record) and the lock-free union-find (cc_find / cc_unite), templated on how a word of `parent`
// is loaded, compare-and-swapped and min'd.  smx_components.hip calls them from its kernels with agent-scope atomics; a
// test compiles this part alone for the host (SMX_COMPONENTS_HOST_ONLY) and walks the same passes with plain words.
// Part 2: the device-side records and the workspace the object keeps for the call (kernels and glue: smx_components.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_COMPONENTS_HOST_ONLY)
#define SMX_CC_FN static inline
#else
#include "smx_common.hpp"
#define SMX_CC_FN __host__ __device__ __forceinline__
#endif

namespace smx {

constexpr uint32_t kCcNoSlot = 0xFFFFFFFFu;                 // parent / label of a slot outside U; component of a dropped triangle
constexpr unsigned long long kCcNoRecord = ~0ull;           // rank record of a component that does not pass (sorts last)

// Live as in smx_recon_triangulate: not merged, and a finite smooth position.
SMX_CC_FN bool cc_finite(float v) { return v - v == 0.0f; }
SMX_CC_FN bool cc_live(float x, float y, float z, float radius_squared) {
  return !(radius_squared < 0.0f) && cc_finite(x) && cc_finite(y) && cc_finite(z);
}

// k(f): unsigned integers that order as the floats do, -0 below +0; a bijection on the bit patterns, so the box keeps the
// bytes of the winning input.
SMX_CC_FN uint32_t cc_key(float f) {
  uint32_t bits;
  __builtin_memcpy(&bits, &f, sizeof(bits));
  return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
SMX_CC_FN float cc_unkey(uint32_t k) {
  const uint32_t bits = (k >> 31) ? (k ^ 0x80000000u) : ~k;
  float f;
  __builtin_memcpy(&f, &bits, sizeof(f));
  return f;
}

// (d_x d_x + d_y d_y) + d_z d_z with d = hi - lo; no contraction (-ffp-contract=off)
SMX_CC_FN float cc_diag2(const float lo[3], const float hi[3]) {
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return (dx * dx + dy * dy) + dz * dz;
}
SMX_CC_FN bool cc_passes(uint32_t n_triangles, float diag2, uint32_t min_triangles, float min_diagonal) {
  return n_triangles >= min_triangles && diag2 >= min_diagonal * min_diagonal;
}
// Ascending records = (n_triangles descending, label ascending).  n_triangles >= 1, so no record equals kCcNoRecord.
SMX_CC_FN unsigned long long cc_rank_record(uint32_t n_triangles, uint32_t label) {
  return ((unsigned long long)(0xFFFFFFFFu - n_triangles) << 32) | label;
}

// ---- lock-free union-find over parent[] --------------------------------------------------------------------------------
// Mem: uint32_t load(i), uint32_t cas(i, expected, desired) (returns the old word), void min(i, v) on word i of parent.
// Invariants:
//   * parent[x] <= x always, and parent[x] == x iff x is a root.  So a tree's root is its smallest slot, and once every
//     edge is united the root of a component is the component's smallest slot, whatever the schedule was.
//   * A word changes by CAS only while it is a root (expected == the word's own index), and then to a smaller index: a
//     slot that has stopped being a root never becomes one again.
//   * Halving writes only to non-roots, and only an ancestor of the slot (min: the word only decreases; an ancestor is
//     smaller).  Whatever value a lane reads from parent[x], fresh or overtaken, is x or an ancestor of x.
//   * Every read goes through Mem::load (on the device a relaxed agent-scope atomic load, never a cached register).
//   * No lane waits for another: a failed CAS means another lane has hooked that root, i.e. the number of roots went
//     down.  Divergent lanes of a wavefront therefore cannot hang each other, and the loops need no bound.
template <class Mem>
SMX_CC_FN uint32_t cc_find(Mem& m, uint32_t x) {
  for (;;) {
    const uint32_t p = m.load(x);
    if (p == x) return x;
    const uint32_t g = m.load(p);
    if (g == p) return p;
    m.min(x, g);          // (x is not a root: p != x; g is an ancestor of p, hence of x)
    x = g;
  }
}

template <class Mem>
SMX_CC_FN void cc_unite(Mem& m, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_find(m, a);
    b = cc_find(m, b);
    if (a == b) return;
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    if (m.cas(hi, hi, lo) == hi) return;      // the larger root goes under the smaller, if it still is a root
    a = hi; b = lo;                           // (someone else hooked it: find again from where we stand)
  }
}

#if !defined(SMX_COMPONENTS_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
enum : int { kCcNotLive = 0, kCcUsed, kCcComponents, kCcKept, kCcLargest, kCcTotal, kCcError, kCcWords = 8 };

// The accumulators of one component while it is measured: counts, then the box as keys (lo starts at all ones, hi at 0).
struct CcAcc { uint32_t n_vertices, n_triangles, lo[3], hi[3]; };
static_assert(sizeof(CcAcc) == 32, "one 32-byte row per component");
static_assert(sizeof(smx_mesh_component) == 40, "smx_mesh_component is 40 bytes");

// The map as in mesh_triangulate: smooth position (x, y, z, -) of slot i at smooth[i * smooth_stride], (normal, RadiusSquared)
// at normal[i * normal_stride].
struct CcMap {
  const float4* smooth; size_t smooth_stride;
  const float4* normal; size_t normal_stride;
  uint32_t n;
};

constexpr int kCcBlock = 256;                               // triangles (or slots, or components) per workgroup of every kernel

// The workspace, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so nothing
// reads a block that goes.
struct ComponentsWork {
  DevBuf<uint32_t> parent;                 // [n] the union-find forest; after the flatten pass the dense number of every root
  DevBuf<uint32_t> label;                  // [n] the contract's vertex_labels
  DevBuf<uint32_t> tcomp;                  // [n_in] 0 / kCcNoSlot after the mark pass, then the dense component of the triangle
  DevBuf<uint32_t> blocks;                 // roots, later surviving triangles, per workgroup; then their offsets
  DevBuf<uint32_t> acc;                    // [n_components] CcAcc
  DevBuf<uint32_t> table;                  // [n_components] smx_mesh_component
  DevBuf<unsigned long long> keys[2];      // [n_components] the rank records (keep_largest)
  DevBuf<uint32_t> vals[2];
  DevBuf<uint32_t> hist;                   // the sort's workspace
  DevBuf<uint32_t> in, out;                // staging when the caller's arrays are host memory
  DevBuf<uint32_t> counters;               // [kCcWords]
  PhaseStamps<SMX_COMPONENTS_PHASES> stamps; // of the last call; a refused call publishes the phases it completed
};
#endif

}  // namespace smx
