// smx_rayscene.hpp -- a ray-casting scene: the index of smx_recon_raycast_mesh kept between casts (smx_rayscene).
//
// Part 1: what only a kept scene needs of the occupancy bit grid, as plain inline functions: which block sizes fit, the grid of a
// box, the bit an entry of the sorted cell keys sets.  The grid's index function, the look-up it filters and the traversal are
// smx_raycast.hpp's.  smx_rayscene.hip calls them from its kernels; a test compiles this part alone for the host
// (SMX_RAYSCENE_HOST_ONLY) and walks the same passes with plain words.
// Part 2: what the scene object holds (kernels and glue: smx_rayscene.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_RAYSCENE_HOST_ONLY)
#if !defined(SMX_RAYCAST_HOST_ONLY)
#define SMX_RAYCAST_HOST_ONLY 1
#endif
#endif
#include "smx_raycast.hpp"

namespace smx {

constexpr int kSceneMaxLog2 = 6;                             // a block has at most 2^6 cells per axis
constexpr unsigned long long kSceneMaxBits = 1ull << 31;     // 256 MiB of bits: the Infinity Cache

// ---- the occupancy bit grid ----------------------------------------------------------------------------------------------
// RayGrid (smx_raycast.hpp) over the occupied cell box [lo, hi]: a block is 2^k cells per axis.
SMX_RAY_FN uint32_t scene_blocks(int32_t lo, int32_t hi, int k) { return ((uint32_t)(hi - lo) >> k) + 1u; }
// The bits a grid of block size 2^k over the box has (0 for an empty box); at most 2^17 blocks per axis, so no overflow.
SMX_RAY_FN unsigned long long scene_grid_bits(const int32_t* lo, const int32_t* hi, int k) {
  if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) return 0ull;
  return (unsigned long long)scene_blocks(lo[0], hi[0], k) * scene_blocks(lo[1], hi[1], k) * scene_blocks(lo[2], hi[2], k);
}
SMX_RAY_FN bool scene_grid_fits(const int32_t* lo, const int32_t* hi, int k) { return scene_grid_bits(lo, hi, k) <= kSceneMaxBits; }
// The smallest k in 0 .. kSceneMaxLog2 that fits, or -1.
SMX_RAY_FN int scene_grid_smallest(const int32_t* lo, const int32_t* hi) {
  for (int k = 0; k <= kSceneMaxLog2; ++k)
    if (scene_grid_fits(lo, hi, k)) return k;
  return -1;
}
SMX_RAY_FN RayGrid scene_grid_make(const int32_t* lo, const int32_t* hi, int k) {
  RayGrid g;
  const bool empty = lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2];
  for (int a = 0; a < 3; ++a) { g.lo[a] = empty ? 0 : lo[a]; g.nb[a] = (empty || k < 0) ? 0u : scene_blocks(lo[a], hi[a], k); }
  g.k = k;
  return g;
}
// the cell of a cell key (dec_cell_key's inverse)
SMX_RAY_FN void scene_key_cell(unsigned long long key, int32_t* x, int32_t* y, int32_t* z) {
  *x = (int32_t)((key >> 42) & 0x1FFFFFu) - kDecCellLimit; *y = (int32_t)((key >> 21) & 0x1FFFFFu) - kDecCellLimit;
  *z = (int32_t)(key & 0x1FFFFFu) - kDecCellLimit;
}
// Entry j of the sorted cell keys: the head of a run is the one lane of its cell; *bit = the bit it sets.
SMX_RAY_FN bool scene_entry_bit(const RayGrid& g, const unsigned long long* keys, uint32_t j, unsigned long long* bit) {
  const unsigned long long key = keys[j];
  if (j != 0 && keys[j - 1] == key) return false;
  int32_t x, y, z;
  scene_key_cell(key, &x, &y, &z);
  return ray_grid_bit(g, x, y, z, bit);
}

#if !defined(SMX_RAYSCENE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of the build's counters behind the grid's (kept as the build left them)
enum : int { kSceneBlocksSet = kTgWords, kSceneBuildWords = 32 };      // the set bits of the occupancy grid; device_bytes counts 32 words
static_assert(kSceneBlocksSet < kSceneBuildWords, "the build's counters");
#endif

}  // namespace smx

#if !defined(SMX_RAYSCENE_HOST_ONLY)
// A snapshot: after a build a cast reads nothing but these.
struct smx_rayscene_s {
  int device = 0;
  bool built = false;
  // the build's
  smx::DevBuf<float> recs, wide_recs;              // [n_entries] / [n_wide] TgRec
  smx::DevBuf<unsigned long long> table;           // [mask + 1][2] TgCell
  smx::DevBuf<uint32_t> bits;                      // the occupancy grid, 32 bits a word
  smx::DevBuf<uint32_t> counters;                  // [kSceneBuildWords] as the build left them: c, the occupied box
  uint32_t h[smx::kSceneBuildWords] = {};          // ... and on the host
  uint32_t mask = 0, n_entries = 0, n_wide = 0;
  smx::RayGrid grid{{0, 0, 0}, {0, 0, 0}, -1};
  smx::RayCastWork cast;                           // a cast's
  smx::PhaseStamps<3> build_stamps;                // mark, index, occupancy of the last build
  smx::PhaseStamps<2> cast_stamps;                 // cast, stats of the last cast
};
#endif
