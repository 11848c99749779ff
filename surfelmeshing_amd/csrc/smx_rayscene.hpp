// smx_rayscene.hpp -- a ray-casting scene: the index of smx_recon_raycast_mesh kept between casts (smx_rayscene).
//
// Part 1: the occupancy bit grid's index arithmetic, the look-up it filters, the walk that keeps the winner's (u, v, det), and
// one ray's view of the cast, as plain inline functions beside ray_cast_one (smx_raycast.hpp), which stays as it is.
// smx_rayscene.hip calls them from its kernels; a test compiles this part alone for the host (SMX_RAYSCENE_HOST_ONLY) and walks
// the same passes with plain words.
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
// It spans the occupied cell box [lo, hi]; a block is 2^k cells per axis.  k < 0: no grid.  nb = 0 on every axis: the box is
// empty, and so is the grid.
struct SceneGrid { int32_t lo[3]; uint32_t nb[3]; int32_t k; };
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
SMX_RAY_FN SceneGrid scene_grid_make(const int32_t* lo, const int32_t* hi, int k) {
  SceneGrid g;
  const bool empty = lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2];
  for (int a = 0; a < 3; ++a) { g.lo[a] = empty ? 0 : lo[a]; g.nb[a] = (empty || k < 0) ? 0u : scene_blocks(lo[a], hi[a], k); }
  g.k = k;
  return g;
}
// The bit number of the block of cell (x, y, z); false for a cell outside the box (the traversal asks about none: ray_axes and
// ray_span clamp to the occupied box).
SMX_RAY_FN bool scene_bit_of(const SceneGrid& g, int32_t x, int32_t y, int32_t z, unsigned long long* bit) {
  const uint32_t bx = (uint32_t)(x - g.lo[0]) >> g.k, by = (uint32_t)(y - g.lo[1]) >> g.k, bz = (uint32_t)(z - g.lo[2]) >> g.k;
  if (x < g.lo[0] || y < g.lo[1] || z < g.lo[2] || bx >= g.nb[0] || by >= g.nb[1] || bz >= g.nb[2]) return false;
  *bit = ((unsigned long long)bz * g.nb[1] + by) * g.nb[0] + bx;
  return true;
}
// the cell of a cell key (dec_cell_key's inverse)
SMX_RAY_FN void scene_key_cell(unsigned long long key, int32_t* x, int32_t* y, int32_t* z) {
  *x = (int32_t)((key >> 42) & 0x1FFFFFu) - kDecCellLimit; *y = (int32_t)((key >> 21) & 0x1FFFFFu) - kDecCellLimit;
  *z = (int32_t)(key & 0x1FFFFFu) - kDecCellLimit;
}
// Entry j of the sorted cell keys: the head of a run is the one lane of its cell; *bit = the bit it sets.
SMX_RAY_FN bool scene_entry_bit(const SceneGrid& g, const unsigned long long* keys, uint32_t j, unsigned long long* bit) {
  const unsigned long long key = keys[j];
  if (j != 0 && keys[j - 1] == key) return false;
  int32_t x, y, z;
  scene_key_cell(key, &x, &y, &z);
  return scene_bit_of(g, x, y, z, bit);
}

// ---- the cast ------------------------------------------------------------------------------------------------------------
// cell number j of layer m's rectangle, b fastest: the cell ray_rect_key makes its key of
SMX_RAY_FN void scene_rect_cell(const RayAxes& r, const RayRect& q, uint32_t m, uint32_t j, int32_t* x, int32_t* y, int32_t* z) {
  const uint32_t nb = (uint32_t)(q.b1 - q.b0) + 1u;
  const int32_t a = r.first + r.sgn * (int32_t)m, b = q.b0 + (int32_t)(j % nb), c = q.c0 + (int32_t)(j / nb);
  if (r.axis == 0) { *x = a; *y = b; *z = c; } else if (r.axis == 1) { *x = b; *y = a; *z = c; } else { *x = b; *y = c; *z = a; }
}
struct SceneWork { uint32_t layers, bit_tests, lookups, misses, tests; };
// The look-up of one cell with the grid in front of it: a clear bit is "no run", a set bit goes on to the table.
// Bits: bool test(unsigned long long bit).
template <class Bits, class Tab>
SMX_RAY_FN bool scene_find(const SceneGrid& g, const Bits& bits, const Tab& tab, uint32_t mask, int32_t x, int32_t y, int32_t z, uint32_t* first,
                           uint32_t* end, SceneWork* w) {
  if (g.k >= 0) {
    unsigned long long bit;
    ++w->bit_tests;
    if (!scene_bit_of(g, x, y, z, &bit) || !bits.test(bit)) return false;
  }
  ++w->lookups;
  const bool found = tg_table_find(tab, mask, dec_cell_key(x, y, z), first, end);
  if (!found) ++w->misses;
  return found;
}
// ray_walk that remembers what the lane's own smallest key came with: a cast reads no map, so the winner's (u, v) and the sign
// of det are taken from the lane that computed the winning key.  Any lane with that key computed it from the same three corners
// by the same expressions.
struct SceneKeep { unsigned long long own; float u, v, det; };
template <class Recs>
SMX_RAY_FN unsigned long long scene_walk(const Recs& recs, uint32_t first, uint32_t end, uint32_t stride, const TgVec& O, const TgVec& D,
                                         float t_min, float t_max, int cull, unsigned long long best, SceneKeep* keep, uint32_t* tests) {
  for (uint32_t j = first; j < end; j += stride) {
    TgVec A, B, C;
    uint32_t i;
    RayHit h{0.0f, 0.0f, 0.0f, 0.0f};
    recs.load(j, &A, &B, &C, &i);
    const unsigned long long key = ray_key(O, D, A, B, C, i, t_min, t_max, cull, &h);
    if (key < best) { best = key; keep->own = key; keep->u = h.u; keep->v = h.v; keep->det = h.det; }
    ++*tests;
  }
  return best;
}
// One ray's view of k_scene_cast: ray_cast_one with scene_find for its look-up.  Seen: void operator()(cell key) for every
// cell looked up in the table.
template <class Bits, class Tab, class Recs, class Seen>
SMX_RAY_FN unsigned long long scene_cast_one(const SceneGrid& g, const Bits& bits, const Tab& tab, uint32_t mask, const Recs& cell_recs,
                                             const Recs& wide_recs, uint32_t n_wide, const RayAxes& r, const TgVec& O, const TgVec& D, float cell,
                                             float t_min, float t_max, int cull, bool early_exit, Seen& seen, SceneKeep* keep, SceneWork* work) {
  unsigned long long best = scene_walk(wide_recs, 0, n_wide, 1, O, D, t_min, t_max, cull, kTgNone, keep, &work->tests);
  for (uint32_t m = 0; m < r.n_layers; ++m) {
    if (early_exit && ray_done(r, cell, best, m)) break;
    const RayRect q = ray_layer_rect(r, cell, t_min, t_max, m);
    const uint32_t cells = ray_rect_cells(q);
    ++work->layers;
    for (uint32_t j = 0; j < cells; ++j) {
      int32_t x, y, z;
      uint32_t first, end;
      scene_rect_cell(r, q, m, j, &x, &y, &z);
      const uint32_t before = work->lookups;
      const bool found = scene_find(g, bits, tab, mask, x, y, z, &first, &end, work);
      if (work->lookups != before) seen(dec_cell_key(x, y, z));
      if (found) best = scene_walk(cell_recs, first, end, 1, O, D, t_min, t_max, cull, best, keep, &work->tests);
    }
  }
  return best;
}

#if !defined(SMX_RAYSCENE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of the build's counters behind the grid's (kept as the build left them), and the words of a cast's counters
enum : int { kSceneBlocksSet = kTgWords, kSceneBuildWords = 32 };      // the set bits of the occupancy grid; device_bytes counts 32 words
static_assert(kSceneBlocksSet < kSceneBuildWords, "the build's counters");
enum : int { kSceneBadRays = 0, kSceneHits, kSceneFrontHits, kSceneMaxTBits, kSceneLayersLo, kSceneLayersHi, kSceneBitTestsLo, kSceneBitTestsHi,
             kSceneLookupsLo, kSceneLookupsHi, kSceneMissesLo, kSceneMissesHi, kSceneTestsLo, kSceneTestsHi, kSceneWords = 16 };
enum : uint32_t { kSceneWorkWords = 8 };                    // per ray: layers, bit tests, look-ups, misses, pair tests, flags, -, -

struct SceneBits {
  const uint32_t* w;
  __device__ __forceinline__ bool test(unsigned long long bit) const { return (w[bit >> 5] >> (uint32_t)(bit & 31u)) & 1u; }
};
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
  smx::SceneGrid grid{{0, 0, 0}, {0, 0, 0}, -1};
  // a cast's
  smx::DevBuf<unsigned long long> best;            // [n_rays] the winning key of every ray
  smx::DevBuf<uint32_t> work;                      // [n_rays][kSceneWorkWords]
  smx::DevBuf<float> rays, out_t, out_uv;          // staging when the caller's arrays are host memory
  smx::DevBuf<uint32_t> out_hit;
  smx::DevBuf<uint32_t> cast_counters;             // [kSceneWords]
  smx::PhaseStamps<3> build_stamps;                // mark, index, occupancy of the last build
  smx::PhaseStamps<2> cast_stamps;                 // cast, stats of the last cast
};
#endif
