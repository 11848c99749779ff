"""What the host tests of the triangle grid's users share (a plain module, no fixtures): GRID_BUILD, the grid build of
smx_trigrid.hip as C++ text that a stand-alone program includes after the header under test; build(), which compiles such a
program; RAY_PROGRAM, the one program of tests/test_raycast_kernel_host.py and tests/test_rayscene_kernel_host.py, and
host_scene(), which runs it.

RAY_PROGRAM compiles part 1 of smx_rayscene.hpp (and with it smx_raycast.hpp) for the host with the project's
-ffp-contract=off, builds the index one "lane" after the other in a given order, then the occupancy bit grid for each setting
asked for (-1: none, which is the index smx_recon_raycast_mesh casts), and walks every ray with ray_cast_one, the function
whose look-ups and record walks k_ray_cast makes."""
import os
import subprocess

import numpy as np

import raycast_ref as rr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

# Needs TgVec, tg_classify, tg_extent, tg_mark, tg_box_key, tg_table_entry and dec_* of smx_trigrid.hpp before it.
GRID_BUILD = r'''
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
using namespace smx;

struct Entry { unsigned long long key, value; };
struct Tab {                         // one lane at a time: the operations on plain words
  Entry* e;
  unsigned long long key(uint32_t h) const { return e[h].key; }
  unsigned long long value(uint32_t h) const { return e[h].value; }
  unsigned long long claim(uint32_t h, unsigned long long expected, unsigned long long desired) const {
    const unsigned long long old = e[h].key;
    if (old == expected) e[h].key = desired;
    return old;
  }
  void bump(uint32_t h, unsigned long long inc) const { e[h].value += inc; }
};
struct Rec { TgVec a, b, c; uint32_t t; };
struct Recs {
  const Rec* r;
  void load(uint32_t j, TgVec* A, TgVec* B, TgVec* C, uint32_t* t) const { *A = r[j].a; *B = r[j].b; *C = r[j].c; *t = r[j].t; }
};

static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  std::iota(l.begin(), l.end(), 0u);
  if (order == 1) std::reverse(l.begin(), l.end());
  if (order > 1) { std::mt19937 g(order); std::shuffle(l.begin(), l.end(), g); }
  return l;
}

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

// What mark and index leave behind.
struct HostGrid {
  uint32_t n_not_live = 0, n_repeated = 0, n_range = 0, n_cells = 0, E = 0, mask = 0;
  float cell = 0.0f;
  std::vector<uint32_t> mark;                  // per triangle: its entries, kTgWide, or 0 (not in R)
  std::vector<TgBox> boxes;                    // per triangle of R
  std::vector<uint32_t> wide_t;                // in arrival order
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};      // the fold of the entered boxes
  std::vector<unsigned long long> skeys;       // the sorted cell keys
  std::vector<Rec> recs, wide_recs;
  std::vector<Entry> table;
  Tab tab() { return Tab{table.data()}; }
};

// tg_enqueue_mark and tg_enqueue_index a lane at a time, the lanes of every pass in `order`.  S: [n][4] position and
// RadiusSquared.  cell_of: float(the given or mean cell size) = c; box: TgBox(a, b, c, cell), exact or inflated.  Returns 0,
// or -1 (an index out of range).
template <class CellOf, class Box>
static int host_tg_build(uint32_t n, const float* S, const uint32_t* tri, uint32_t n_in, float cell_size, uint32_t order, CellOf cell_of, Box box,
                         HostGrid* g) {
  auto pos = [&](uint32_t i) { return TgVec{S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2]}; };
  auto live = [&](uint32_t i) { return dec_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], S[4 * (size_t)i + 3]); };
  // k_tg_classify, k_tg_cell
  g->mark.assign(n_in, 0);
  g->boxes.assign(n_in, TgBox{});
  unsigned long long extent = 0;
  uint32_t in_r = 0;
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= n || i1 >= n || i2 >= n) return -1;
    const TgVec a = pos(i0), b = pos(i1), c = pos(i2);
    const uint32_t cls = tg_classify(i0, i1, i2, live(i0), live(i1), live(i2), a, b, c);
    if (cls == kTgDropNotLive) ++g->n_not_live;
    if (cls == kTgDropRepeated) ++g->n_repeated;
    if (cls == kTgDropRange) ++g->n_range;
    if (cls == kTgInR) { g->mark[t] = 1; ++in_r; extent += (unsigned long long)(tg_extent(a, b, c) * 1048576.0f); }
  }
  float given = cell_size;
  if (!(cell_size > 0.0f)) given = in_r != 0 ? (float)((double)extent / (double)in_r * (1.0 / 1048576.0)) : 0.0f;
  g->cell = cell_of(given);
  // k_tg_mark: the wide list in arrival order; the occupied box; the scan
  for (uint32_t t : lanes(n_in, order)) {
    if (g->mark[t] == 0) continue;
    const TgBox b = box(pos(tri[3 * (size_t)t]), pos(tri[3 * (size_t)t + 1]), pos(tri[3 * (size_t)t + 2]), g->cell);
    g->boxes[t] = b;
    g->mark[t] = tg_mark(b);
    if (g->mark[t] == kTgWide) { g->wide_t.push_back(t); continue; }
    for (int k = 0; k < 3; ++k) { g->lo[k] = std::min(g->lo[k], b.lo[k]); g->hi[k] = std::max(g->hi[k], b.hi[k]); }
  }
  std::vector<uint32_t> off(n_in + 1, 0);
  for (uint32_t t = 0; t < n_in; ++t) off[t + 1] = off[t] + (g->mark[t] == kTgWide ? 0u : g->mark[t]);
  const uint32_t E = g->E = off[n_in];
  // k_tg_entries, the stable sort, k_tg_records
  std::vector<unsigned long long> keys(E);
  std::vector<uint32_t> vals(E);
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t count = g->mark[t] == kTgWide ? 0u : g->mark[t];
    for (uint32_t j = 0; j < count; ++j) { keys[off[t] + j] = tg_box_key(g->boxes[t], j); vals[off[t] + j] = t; }
  }
  std::vector<uint32_t> perm(E);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
  g->skeys.resize(E); g->recs.resize(E); g->wide_recs.resize(g->wide_t.size());
  auto rec_of = [&](uint32_t t) { return Rec{pos(tri[3 * (size_t)t]), pos(tri[3 * (size_t)t + 1]), pos(tri[3 * (size_t)t + 2]), t}; };
  for (uint32_t j = 0; j < E; ++j) { g->skeys[j] = keys[perm[j]]; g->recs[j] = rec_of(vals[perm[j]]); }
  for (size_t j = 0; j < g->wide_t.size(); ++j) g->wide_recs[j] = rec_of(g->wide_t[j]);
  // k_tg_table
  const uint32_t entries = dec_table_size(E);
  g->mask = entries - 1;
  g->table.assign(entries, Entry{kTgEmpty, 0});
  Tab tab = g->tab();
  for (uint32_t j : lanes(E, order)) g->n_cells += tg_table_entry(tab, g->mask, g->skeys.data(), E, j) ? 1u : 0u;
  return 0;
}
'''

RAY_PROGRAM = r'''
#define SMX_RAYSCENE_HOST_ONLY 1
#include "smx_rayscene.hpp"
''' + GRID_BUILD + r'''
#include <set>
#include <unordered_set>

struct Bits {
  const std::vector<uint32_t>* w;
  bool test(unsigned long long bit) const { return ((*w).at(bit >> 5) >> (bit & 31u)) & 1u; }
};
struct Unseen { void operator()(unsigned long long) const {} };
struct SeenSet { std::unordered_set<unsigned long long>* s; void operator()(unsigned long long k) const { s->insert(k); } };

enum { N_IN = 0, N_NOT_LIVE, N_REPEATED, N_RANGE, N_RAYS, N_BAD, N_HIT, N_FRONT, MAX_BITS, N_WIDE, N_ENTRIES, N_CELLS, CELL,
       K_USED, BLOCKS_SET, GRID_BITS, BITS_WRONG, RELATIONS_WRONG, PAIRS_MISSED, EXIT_DIFFERS, LAYERS, BIT_TESTS, LOOKUPS, MISSES, TESTS,
       FOUND, BASE_LOOKUPS, LAYERS_FULL, LOOKUPS_FULL, KEPT_DIFFERS, WORDS };

static uint32_t word_of(float f) { uint32_t w; __builtin_memcpy(&w, &f, 4); return w; }

// occupancy: -1 none, 0 the smallest block that fits, 1 + k.  pairs: (ray, triangle) candidates of the model, ascending by ray.
// Returns 0, -1 (an index out of range) or -3 (the block size does not fit).
static int host_scene(uint32_t n, const float* S, const uint32_t* tri, uint32_t n_in, const float* rays, uint32_t n_rays, float t_min, float t_max,
                      float cell_size, int cull, int occupancy, uint32_t order, const uint32_t* pairs, uint32_t n_pairs, uint32_t* hit, float* t_out,
                      float* uv, uint32_t* stats) {
  for (int k = 0; k < WORDS; ++k) stats[k] = 0;
  stats[N_IN] = n_in; stats[N_RAYS] = n_rays;
  auto pos = [&](uint32_t i) { return TgVec{S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2]}; };
  // ---- mark and index, as smx_recon_raycast_mesh and a scene's build share them
  HostGrid g;
  if (host_tg_build(n, S, tri, n_in, cell_size, order, ray_cell_size, ray_box, &g) != 0) return -1;
  const float cell = g.cell;
  const int32_t* lo = g.lo;
  const int32_t* hi = g.hi;
  const uint32_t E = g.E, mask = g.mask, n_wide = (uint32_t)g.wide_t.size();
  const Tab tab = g.tab();
  const std::vector<unsigned long long>& skeys = g.skeys;
  stats[N_NOT_LIVE] = g.n_not_live; stats[N_REPEATED] = g.n_repeated; stats[N_RANGE] = g.n_range;
  stats[N_WIDE] = n_wide; stats[N_ENTRIES] = E; stats[N_CELLS] = g.n_cells; stats[CELL] = word_of(cell);
  // ---- the occupancy grid: k_scene_occupancy a lane at a time, k_scene_popcount
  int k = -1;
  if (occupancy > 0) { k = occupancy - 1; if (!scene_grid_fits(lo, hi, k)) return -3; }
  if (occupancy == 0 && E != 0) k = scene_grid_smallest(lo, hi);
  const RayGrid grid = scene_grid_make(lo, hi, k), no_grid = scene_grid_make(lo, hi, -1);
  const unsigned long long n_bits = k < 0 ? 0ull : scene_grid_bits(lo, hi, k);
  std::vector<uint32_t> words((size_t)((n_bits + 31) >> 5), 0u);
  stats[K_USED] = (uint32_t)k; stats[GRID_BITS] = (uint32_t)n_bits;
  if (k >= 0) {
    std::set<unsigned long long> blocks;
    for (uint32_t j : lanes(E, order)) {
      unsigned long long bit = 0;
      if (!scene_entry_bit(grid, skeys.data(), j, &bit)) continue;
      if (bit >= n_bits) { ++stats[BITS_WRONG]; continue; }
      words[bit >> 5] |= 1u << (bit & 31u);
      blocks.insert(bit);
    }
    for (uint32_t w : words) stats[BLOCKS_SET] += (uint32_t)__builtin_popcount(w);
    if (stats[BLOCKS_SET] != blocks.size()) ++stats[BITS_WRONG];
    if (k == 0 && stats[BLOCKS_SET] != stats[N_CELLS]) ++stats[BITS_WRONG];               // no bit without a cell with entries
    const Bits probe{&words};
    for (uint32_t j = 0; j < E; ++j) {                                                      // every entry's cell has its block's bit
      int32_t x, y, z;
      unsigned long long bit = 0;
      scene_key_cell(skeys[j], &x, &y, &z);
      if (dec_cell_key(x, y, z) != skeys[j] || !ray_grid_bit(grid, x, y, z, &bit) || !probe.test(bit)) ++stats[BITS_WRONG];
      if (((uint32_t)(x - lo[0]) >> k) + (((uint32_t)(y - lo[1]) >> k) + (unsigned long long)((uint32_t)(z - lo[2]) >> k) * grid.nb[1]) * grid.nb[0] != bit)
        ++stats[BITS_WRONG];
    }
  }
  // ---- k_ray_cast, k_ray_stats; beside them the same walk without a grid (k = -1) on the same index
  const Recs cell_recs{g.recs.data()}, wrecs{g.wide_recs.data()};
  const Bits bits{&words};
  uint32_t at_pair = 0;
  for (uint32_t p = 0; p < n_rays; ++p) {
    const float* r = rays + 6 * (size_t)p;
    const TgVec O{r[0], r[1], r[2]}, D{r[3], r[4], r[5]};
    unsigned long long key = kTgNone;
    RayKeep keep{kTgNone, 0.0f, 0.0f, 0.0f};
    if (ray_bad(O, D)) {
      ++stats[N_BAD];
    } else {
      RayWork work{0, 0, 0, 0, 0}, full{0, 0, 0, 0, 0}, base{0, 0, 0, 0, 0}, base_full{0, 0, 0, 0, 0};
      RayKeep keep_full{kTgNone, 0.0f, 0.0f, 0.0f}, keep_base{kTgNone, 0.0f, 0.0f, 0.0f}, keep_base_full{kTgNone, 0.0f, 0.0f, 0.0f};
      RayAxes ax = ray_axes(O, D, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], cell, t_min, t_max);
      if (E == 0) ax.n_layers = 0;
      Unseen unseen;
      key = ray_cast_one(grid, bits, tab, mask, cell_recs, wrecs, n_wide, ax, O, D, cell, t_min, t_max, cull, true, unseen, &keep, &work);
      const unsigned long long plain = ray_cast_one(no_grid, bits, tab, mask, cell_recs, wrecs, n_wide, ax, O, D, cell, t_min, t_max, cull, true, unseen,
                                                    &keep_base, &base);
      std::unordered_set<unsigned long long> cells;
      SeenSet seen{&cells};
      const unsigned long long all = ray_cast_one(grid, bits, tab, mask, cell_recs, wrecs, n_wide, ax, O, D, cell, t_min, t_max, cull, false, seen,
                                                  &keep_full, &full);
      const unsigned long long plain_all = ray_cast_one(no_grid, bits, tab, mask, cell_recs, wrecs, n_wide, ax, O, D, cell, t_min, t_max, cull, false,
                                                        unseen, &keep_base_full, &base_full);
      if (all != key || plain != key || plain_all != key) ++stats[EXIT_DIFFERS];
      if (key != kTgNone && (keep.own != key || keep_full.own != key || keep.u != keep_full.u || keep.v != keep_full.v)) ++stats[EXIT_DIFFERS];
      // the contract's relations, with the exit on and off
      const RayWork* sw[2] = {&work, &full};
      const RayWork* bw[2] = {&base, &base_full};
      for (int e = 0; e < 2; ++e) {
        bool ok = sw[e]->layers == bw[e]->layers && sw[e]->tests == bw[e]->tests && sw[e]->misses <= sw[e]->lookups && bw[e]->bit_tests == 0;
        if (k < 0) ok = ok && sw[e]->bit_tests == 0 && sw[e]->lookups == bw[e]->lookups;
        else ok = ok && sw[e]->bit_tests == bw[e]->lookups && sw[e]->lookups <= bw[e]->lookups && (k != 0 || sw[e]->misses == 0);
        if (!ok) ++stats[RELATIONS_WRONG];
      }
      stats[LAYERS] += work.layers; stats[BIT_TESTS] += work.bit_tests; stats[LOOKUPS] += work.lookups; stats[MISSES] += work.misses;
      stats[TESTS] += work.tests; stats[FOUND] += work.lookups - work.misses; stats[BASE_LOOKUPS] += base.lookups;
      stats[LAYERS_FULL] += full.layers; stats[LOOKUPS_FULL] += full.lookups;
      for (; at_pair < n_pairs && pairs[2 * (size_t)at_pair] == p; ++at_pair) {
        const uint32_t i = pairs[2 * (size_t)at_pair + 1];
        bool found = g.mark[i] == kTgWide;
        if (!found && g.mark[i] != 0)
          for (uint32_t j = 0; j < g.mark[i] && !found; ++j) found = cells.count(tg_box_key(g.boxes[i], j)) != 0;
        if (!found) ++stats[PAIRS_MISSED];
      }
    }
    for (; at_pair < n_pairs && pairs[2 * (size_t)at_pair] == p; ++at_pair) ++stats[PAIRS_MISSED];      // (a candidate of a BAD ray)
    uint32_t i = 0xFFFFFFFFu;
    float t = INFINITY, u = NAN, v = NAN;
    if (key != kTgNone) {                       // as lane 0 of k_ray_cast: from what the walk kept, no read of the map
      i = (uint32_t)key;
      t = tg_key_float(key); u = keep.u; v = keep.v;
      ++stats[N_HIT];
      if (keep.det > 0.0f) ++stats[N_FRONT];
      stats[MAX_BITS] = std::max(stats[MAX_BITS], (uint32_t)(key >> 32));
      // what the kernel does not recompute: from the map positions of the winning triangle the same key, and bit for bit the
      // u and v and the sign of det that the walk kept
      RayHit h{0, 0, 0, 0};
      const unsigned long long again = ray_key(O, D, pos(tri[3 * (size_t)i]), pos(tri[3 * (size_t)i + 1]), pos(tri[3 * (size_t)i + 2]), i, t_min, t_max, cull, &h);
      if (again != key) ++stats[EXIT_DIFFERS];
      if (word_of(h.u) != word_of(keep.u) || word_of(h.v) != word_of(keep.v) || (h.det > 0.0f) != (keep.det > 0.0f) || (h.det < 0.0f) != (keep.det < 0.0f))
        ++stats[KEPT_DIFFERS];
    }
    hit[p] = i; t_out[p] = t; uv[2 * (size_t)p] = u; uv[2 * (size_t)p + 1] = v;
  }
  stats[PAIRS_MISSED] += n_pairs - at_pair;
  return 0;
}

// case file: u32 n, n_in, n_rays, cull, n_pairs, n_orders, n_settings; f32 t_min, t_max, cell_size; u32 orders[]; i32 settings[];
//            f32 S[n][4]; u32 tri[n_in][3]; f32 rays[n_rays][6]; u32 pairs[n_pairs][2]
// result file, per order and setting: i32 rc; u32 stats[WORDS]; u32 hit[n_rays]; f32 t[n_rays]; f32 uv[n_rays][2]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[7];
  float prm[3];
  if (!get(f, head, 7) || !get(f, prm, 3)) return 2;
  std::vector<uint32_t> orders(head[5]), tri(3 * (size_t)head[1]), pairs(2 * (size_t)head[4]);
  std::vector<int32_t> settings(head[6]);
  std::vector<float> S(4 * (size_t)head[0]), rays(6 * (size_t)head[2]);
  if (!get(f, orders.data(), orders.size()) || !get(f, settings.data(), settings.size()) || !get(f, S.data(), S.size()) ||
      !get(f, tri.data(), tri.size()) || !get(f, rays.data(), rays.size()) || !get(f, pairs.data(), pairs.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order : orders)
    for (int32_t occupancy : settings) {
      std::vector<uint32_t> hit(head[2], 0xA5A5A5A5u);
      std::vector<float> t(head[2], 0.0f), uv(2 * (size_t)head[2], 0.0f);
      uint32_t stats[WORDS];
      const int32_t rc = host_scene(head[0], S.data(), tri.data(), head[1], rays.data(), head[2], prm[0], prm[1], prm[2], (int)head[3], occupancy, order,
                                    pairs.data(), head[4], hit.data(), t.data(), uv.data(), stats);
      put(o, &rc, 1); put(o, stats, (size_t)WORDS);
      put(o, hit.data(), hit.size()); put(o, t.data(), t.size()); put(o, uv.data(), uv.size());
    }
  fclose(o);
  return 0;
}
'''

ORDERS = (0, 7)      # forwards, shuffled with seed 7
WORDS = 30
EXTRA = ("k", "n_blocks_set", "grid_bits", "bits_wrong", "relations_wrong", "pairs_missed", "exit_differs", "layers", "bit_tests", "lookups",
         "misses", "tests", "found", "base_lookups", "layers_full", "lookups_full", "kept_differs")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


# smx_raycast.hpp by itself: the traversal compiles for the host without the scene's header
ALONE = '''
#include <cmath>
#define SMX_RAYCAST_HOST_ONLY 1
#include "smx_raycast.hpp"
int main() { return smx::ray_bad(smx::TgVec{0.0f, 0.0f, 0.0f}, smx::TgVec{0.0f, 0.0f, 1.0f}) ? 1 : 0; }
'''


def build(d, program, flags, name):
    """Compiles `program` (C++ text with its own main) in directory d with the host compiler; the path of the executable."""
    src = d / (name + ".cpp")
    src.write_text(program)
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def host_scene(exe, work, pos, r2, tri, rays, t_min, t_max, cell_size, cull, pairs, settings):
    """[(order, occupancy, rc, hit, t, uv, stats, extra)] for every order of ORDERS and every occupancy setting."""
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3], S[:, 3] = pos, r2
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    ry = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    P = ry.shape[0]
    pr = np.zeros((0, 2), np.uint32) if pairs is None else np.ascontiguousarray(pairs, np.uint32)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, t.shape[0], P, int(cull), pr.shape[0], len(ORDERS), len(settings)], np.uint32).tobytes())
        f.write(np.array([t_min, t_max, cell_size], np.float32).tobytes())
        f.write(np.array(ORDERS, np.uint32).tobytes() + np.array(settings, np.int32).tobytes() + S.tobytes() + t.tobytes() + ry.tobytes() + pr.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint32), 0, []
    for order in ORDERS:
        for occ in settings:
            rc = int(raw[at:at + 1].view(np.int32)[0])
            w = raw[at + 1:at + 1 + WORDS]
            st = dict(zip(rr.STAT_NAMES, (int(v) for v in w[:9])))
            st.update(n_wide=int(w[9]), n_entries=int(w[10]), n_cells=int(w[11]), cell_size_used=float(w[12:13].view(np.float32)[0]))
            extra = dict(zip(EXTRA, (int(v) for v in w[13:])))
            extra["k"] = int(w[13:14].view(np.int32)[0])
            at += 1 + WORDS
            hit, tt = raw[at:at + P].copy(), raw[at + P:at + 2 * P].copy().view(np.float32)
            uv = raw[at + 2 * P:at + 4 * P].copy().view(np.float32).reshape(-1, 2)
            at += 4 * P
            runs.append((order, occ, rc, hit, tt, uv, st, extra))
    assert at == raw.size
    return runs
