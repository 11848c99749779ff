"""The occupancy bit grid and the filtered walk of smx_rayscene.hip without a GPU: smx_rayscene.hpp holds the grid's index
arithmetic, the look-up with the bit test in front of it, the walk that keeps the winner's (u, v, det) and one ray's view of the
cast as inline functions beside ray_cast_one.  This test compiles them for the host with the project's -ffp-contract=off into a
stand-alone program (its own main: it reads a case file and writes a result file).  The program builds the index as
tests/test_raycast_kernel_host.py does and the bit grid one "lane" after the other -- forwards and in a seeded shuffled order --
and walks every ray with scene_cast_one, for the occupancy settings none, the smallest block that fits, k = 0 and k = 3.  Every
output byte and statistic has to equal the brute-force model of tests/raycast_ref.py; the work counters have to stand in the
contract's relations to a walk of ray_cast_one in the same program; every cell with entries has its block's bit set, at k = 0 no
other bit is set, and the set bits number the distinct blocks; with the early exit off every candidate pair of the model is wide
or lies in a cell whose table entry was looked up.  The same program is also built with -fsanitize=address,undefined and run
directly."""
import os
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import raycast_ref as rr
import rayscene_ref as sr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PROGRAM = r'''
#define SMX_RAYSCENE_HOST_ONLY 1
#include "smx_rayscene.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include <set>
#include <unordered_set>
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
struct Bits {
  const std::vector<uint32_t>* w;
  bool test(unsigned long long bit) const { return ((*w).at(bit >> 5) >> (bit & 31u)) & 1u; }
};
struct Unseen { void operator()(unsigned long long) const {} };
struct SeenSet { std::unordered_set<unsigned long long>* s; void operator()(unsigned long long k) const { s->insert(k); } };

static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  std::iota(l.begin(), l.end(), 0u);
  if (order == 1) std::reverse(l.begin(), l.end());
  if (order > 1) { std::mt19937 g(order); std::shuffle(l.begin(), l.end(), g); }
  return l;
}

enum { N_IN = 0, N_NOT_LIVE, N_REPEATED, N_RANGE, N_RAYS, N_BAD, N_HIT, N_FRONT, MAX_BITS, N_WIDE, N_ENTRIES, N_CELLS, CELL,
       K_USED, BLOCKS_SET, GRID_BITS, BITS_WRONG, RELATIONS_WRONG, PAIRS_MISSED, EXIT_DIFFERS, LAYERS, BIT_TESTS, LOOKUPS, MISSES, TESTS,
       FOUND, BASE_LOOKUPS, WORDS };

// occupancy: -1 none, 0 the smallest block that fits, 1 + k.  Returns 0, -1 (an index out of range) or -3 (the block size does not fit).
static int host_scene(uint32_t n, const float* S, const uint32_t* tri, uint32_t n_in, const float* rays, uint32_t n_rays, float t_min, float t_max,
                      float cell_size, int cull, int occupancy, uint32_t order, const uint32_t* pairs, uint32_t n_pairs, uint32_t* hit, float* t_out,
                      float* uv, uint32_t* stats) {
  for (int k = 0; k < WORDS; ++k) stats[k] = 0;
  stats[N_IN] = n_in; stats[N_RAYS] = n_rays;
  auto pos = [&](uint32_t i) { return TgVec{S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2]}; };
  auto live = [&](uint32_t i) { return dec_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], S[4 * (size_t)i + 3]); };
  // ---- mark and index, as the build shares them with smx_recon_raycast_mesh
  std::vector<uint32_t> mark(n_in, 0);
  unsigned long long extent = 0;
  uint32_t in_r = 0;
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= n || i1 >= n || i2 >= n) return -1;
    const TgVec a = pos(i0), b = pos(i1), c = pos(i2);
    const uint32_t cls = tg_classify(i0, i1, i2, live(i0), live(i1), live(i2), a, b, c);
    if (cls == kTgDropNotLive) ++stats[N_NOT_LIVE];
    if (cls == kTgDropRepeated) ++stats[N_REPEATED];
    if (cls == kTgDropRange) ++stats[N_RANGE];
    if (cls == kTgInR) { mark[t] = 1; ++in_r; extent += (unsigned long long)(tg_extent(a, b, c) * 1048576.0f); }
  }
  float given = cell_size;
  if (!(cell_size > 0.0f)) given = in_r != 0 ? (float)((double)extent / (double)in_r * (1.0 / 1048576.0)) : 0.0f;
  const float cell = ray_cell_size(given);
  __builtin_memcpy(&stats[CELL], &cell, 4);
  std::vector<uint32_t> wide_t;
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  auto box_of = [&](uint32_t t) { return ray_box(pos(tri[3 * (size_t)t]), pos(tri[3 * (size_t)t + 1]), pos(tri[3 * (size_t)t + 2]), cell); };
  for (uint32_t t : lanes(n_in, order)) {
    if (mark[t] == 0) continue;
    const TgBox box = box_of(t);
    mark[t] = tg_mark(box);
    if (mark[t] == kTgWide) { wide_t.push_back(t); continue; }
    for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], box.lo[k]); hi[k] = std::max(hi[k], box.hi[k]); }
  }
  std::vector<uint32_t> off(n_in + 1, 0);
  for (uint32_t t = 0; t < n_in; ++t) off[t + 1] = off[t] + (mark[t] == kTgWide ? 0u : mark[t]);
  const uint32_t E = off[n_in];
  stats[N_WIDE] = (uint32_t)wide_t.size(); stats[N_ENTRIES] = E;
  std::vector<unsigned long long> keys(E);
  std::vector<uint32_t> vals(E);
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t count = mark[t] == kTgWide ? 0u : mark[t];
    if (count == 0) continue;
    const TgBox box = box_of(t);
    for (uint32_t j = 0; j < count; ++j) { keys[off[t] + j] = tg_box_key(box, j); vals[off[t] + j] = t; }
  }
  std::vector<uint32_t> perm(E);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
  std::vector<unsigned long long> skeys(E);
  std::vector<Rec> recs(E), wide_recs(wide_t.size());
  auto rec_of = [&](uint32_t t) { return Rec{pos(tri[3 * (size_t)t]), pos(tri[3 * (size_t)t + 1]), pos(tri[3 * (size_t)t + 2]), t}; };
  for (uint32_t j = 0; j < E; ++j) { skeys[j] = keys[perm[j]]; recs[j] = rec_of(vals[perm[j]]); }
  for (size_t j = 0; j < wide_t.size(); ++j) wide_recs[j] = rec_of(wide_t[j]);
  const uint32_t entries = dec_table_size(E), mask = entries - 1;
  std::vector<Entry> table(entries, Entry{kTgEmpty, 0});
  Tab tab{table.data()};
  for (uint32_t j : lanes(E, order)) stats[N_CELLS] += tg_table_entry(tab, mask, skeys.data(), E, j) ? 1u : 0u;
  // ---- the occupancy grid: k_scene_occupancy a lane at a time, k_scene_popcount
  int k = -1;
  if (occupancy > 0) { k = occupancy - 1; if (!scene_grid_fits(lo, hi, k)) return -3; }
  if (occupancy == 0 && E != 0) k = scene_grid_smallest(lo, hi);
  const SceneGrid grid = scene_grid_make(lo, hi, k);
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
      if (dec_cell_key(x, y, z) != skeys[j] || !scene_bit_of(grid, x, y, z, &bit) || !probe.test(bit)) ++stats[BITS_WRONG];
      if (((uint32_t)(x - lo[0]) >> k) + (((uint32_t)(y - lo[1]) >> k) + (unsigned long long)((uint32_t)(z - lo[2]) >> k) * grid.nb[1]) * grid.nb[0] != bit)
        ++stats[BITS_WRONG];
    }
  }
  // ---- k_scene_cast, k_scene_stats; beside them ray_cast_one on the same index
  const Recs cell_recs{recs.data()}, wrecs{wide_recs.data()};
  const Bits bits{&words};
  uint32_t at_pair = 0;
  for (uint32_t p = 0; p < n_rays; ++p) {
    const float* r = rays + 6 * (size_t)p;
    const TgVec O{r[0], r[1], r[2]}, D{r[3], r[4], r[5]};
    unsigned long long key = kTgNone;
    SceneKeep keep{kTgNone, 0.0f, 0.0f, 0.0f};
    if (ray_bad(O, D)) {
      ++stats[N_BAD];
    } else {
      SceneWork work{0, 0, 0, 0, 0}, full{0, 0, 0, 0, 0};
      RayWork base{0, 0, 0}, base_full{0, 0, 0};
      SceneKeep keep_full{kTgNone, 0.0f, 0.0f, 0.0f};
      RayAxes ax = ray_axes(O, D, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], cell, t_min, t_max);
      if (E == 0) ax.n_layers = 0;
      Unseen unseen;
      key = scene_cast_one(grid, bits, tab, mask, cell_recs, wrecs, (uint32_t)wide_t.size(), ax, O, D, cell, t_min, t_max, cull, true, unseen, &keep, &work);
      const unsigned long long plain = ray_cast_one(tab, mask, cell_recs, wrecs, (uint32_t)wide_t.size(), ax, O, D, cell, t_min, t_max, cull, true, unseen, &base);
      std::unordered_set<unsigned long long> cells;
      SeenSet seen{&cells};
      const unsigned long long all = scene_cast_one(grid, bits, tab, mask, cell_recs, wrecs, (uint32_t)wide_t.size(), ax, O, D, cell, t_min, t_max, cull, false,
                                                    seen, &keep_full, &full);
      const unsigned long long plain_all = ray_cast_one(tab, mask, cell_recs, wrecs, (uint32_t)wide_t.size(), ax, O, D, cell, t_min, t_max, cull, false,
                                                        unseen, &base_full);
      if (all != key || plain != key || plain_all != key) ++stats[EXIT_DIFFERS];
      if (key != kTgNone && (keep.own != key || keep_full.own != key || keep.u != keep_full.u || keep.v != keep_full.v)) ++stats[EXIT_DIFFERS];
      // the contract's relations, with the exit on and off
      const SceneWork* sw[2] = {&work, &full};
      const RayWork* bw[2] = {&base, &base_full};
      for (int e = 0; e < 2; ++e) {
        bool ok = sw[e]->layers == bw[e]->layers && sw[e]->tests == bw[e]->tests && sw[e]->misses <= sw[e]->lookups;
        if (k < 0) ok = ok && sw[e]->bit_tests == 0 && sw[e]->lookups == bw[e]->lookups;
        else ok = ok && sw[e]->bit_tests == bw[e]->lookups && sw[e]->lookups <= bw[e]->lookups && (k != 0 || sw[e]->misses == 0);
        if (!ok) ++stats[RELATIONS_WRONG];
      }
      stats[LAYERS] += work.layers; stats[BIT_TESTS] += work.bit_tests; stats[LOOKUPS] += work.lookups; stats[MISSES] += work.misses;
      stats[TESTS] += work.tests; stats[FOUND] += work.lookups - work.misses; stats[BASE_LOOKUPS] += base.lookups;
      for (; at_pair < n_pairs && pairs[2 * (size_t)at_pair] == p; ++at_pair) {
        const uint32_t i = pairs[2 * (size_t)at_pair + 1];
        bool found = mark[i] == kTgWide;
        if (!found && mark[i] != 0) {
          const TgBox box = box_of(i);
          for (uint32_t j = 0; j < mark[i] && !found; ++j) found = cells.count(tg_box_key(box, j)) != 0;
        }
        if (!found) ++stats[PAIRS_MISSED];
      }
    }
    for (; at_pair < n_pairs && pairs[2 * (size_t)at_pair] == p; ++at_pair) ++stats[PAIRS_MISSED];      // (a candidate of a BAD ray)
    uint32_t i = 0xFFFFFFFFu;
    float t = INFINITY, u = NAN, v = NAN;
    if (key != kTgNone) {                       // as lane 0 of k_scene_cast: from what the walk kept, no read of the map
      i = (uint32_t)key;
      t = tg_key_float(key); u = keep.u; v = keep.v;
      ++stats[N_HIT];
      if (keep.det > 0.0f) ++stats[N_FRONT];
      stats[MAX_BITS] = std::max(stats[MAX_BITS], (uint32_t)(key >> 32));
    }
    hit[p] = i; t_out[p] = t; uv[2 * (size_t)p] = u; uv[2 * (size_t)p + 1] = v;
  }
  stats[PAIRS_MISSED] += n_pairs - at_pair;
  return 0;
}

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

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
WORDS = 27
EXTRA = ("k", "n_blocks_set", "grid_bits", "bits_wrong", "relations_wrong", "pairs_missed", "exit_differs", "layers", "bit_tests", "lookups",
         "misses", "tests", "found", "base_lookups")


def _build(d, flags, name):
    src = d / "rayscene_host.cpp"
    src.write_text(PROGRAM)
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("rayscene_host")


@pytest.fixture(scope="module")
def program(work):
    return _build(work, [], "rayscene_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return _build(work, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "rayscene_host_san")


def host_scene(exe, work, pos, r2, tri, rays, t_min, t_max, cell_size=0.0, cull=0, pairs=None, settings=sr.SETTINGS):
    """[(order, occupancy, rc, hit, t, uv, stats, extra)] for every order and setting."""
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


def _compare(exe, work, world, model, rays, t0, t1, what, cell_size, cull, seen_k=None):
    pos, nrm, r2, tri, _ = world
    wh, wt, wuv, wst = rr.answer(model, cull)
    if cell_size > 0:
        wst.update(rr.structure(pos, r2, tri, cell_size))
    p = model["pairs"]
    pairs = p[np.argsort(p[:, 0], kind="stable")]
    found = set()
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(exe, work, pos, r2, tri, rays, t0, t1, cell_size, cull, pairs):
        tag = (what, cell_size, cull, order, occ)
        assert rc == 0, tag
        used = st.pop("cell_size_used")
        g = sr.grid(pos, r2, tri, used)
        if cell_size > 0:
            assert used == float(rr.cell_used(cell_size))
        else:
            assert used >= float(rr.MIN_CELL)
            for k in ("n_wide", "n_entries", "n_cells"):
                st.pop(k)
        assert st == wst, (tag, st, wst)
        k = extra["k"]
        assert k == (-1 if occ == -1 else sr.smallest(g) if occ == 0 else occ - 1), tag
        if k >= 0:
            assert extra["n_blocks_set"] == sr.blocks_set(g, k) and extra["grid_bits"] == sr.bits(g, k), (tag, extra)
        for name in ("bits_wrong", "relations_wrong", "pairs_missed", "exit_differs"):
            assert extra[name] == 0, (tag, extra)
        assert extra["bit_tests"] == (extra["base_lookups"] if k >= 0 else 0) and extra["found"] == extra["lookups"] - extra["misses"], (tag, extra)
        found.add(extra["found"])
        for got, want in ((hit, wh), (tt, wt), (uv, wuv)):
            assert got.tobytes() == want.tobytes(), tag
        if order == ORDERS[0]:
            if seen_k is not None:
                seen_k.add(k)
            print("%s cell %g cull %d occupancy %d: k = %d, %d blocks set; %d bit tests, %d look-ups (%d without a grid), %d misses" % (
                what, cell_size, cull, occ, k, extra["n_blocks_set"], extra["bit_tests"], extra["lookups"], extra["base_lookups"], extra["misses"]))
    assert len(found) == 1, (what, cell_size, cull, found)       # look-ups that found a run: the same for every setting


def test_every_ray_set_on_the_host(program, work):
    world = dr.world()
    seen_k = set()
    for k, (name, (rays, t0, t1)) in enumerate(rr.ray_sets().items()):
        m = rr.model_of(name)
        for j, cs in enumerate(rr.CELL_SIZES):
            _compare(program, work, world, m, rays, t0, t1, name, cs, (k + j) % 3, seen_k)
    assert 0 in seen_k and any(k > 0 for k in seen_k) and -1 in seen_k, seen_k


def test_every_cull_mode_on_the_host(program, work):
    world = dr.world()
    for name in ("around the hand-made triangles", "inside-out"):
        rays, t0, t1 = rr.ray_sets()[name]
        for cull in (0, 1, 2):
            _compare(program, work, world, rr.model_of(name), rays, t0, t1, name, 0.0225, cull)


def test_a_block_size_that_does_not_fit_an_index_out_of_range_and_empty_inputs(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    rays, t0, t1 = rr.ray_sets()["BAD and limits"]
    bad = tri.copy()
    bad[77, 2] = pos.shape[0]
    assert [r[2] for r in host_scene(program, work, pos, r2, bad, rays, t0, t1)] == [-1] * (len(ORDERS) * len(sr.SETTINGS))
    none = np.zeros((0, 3), np.uint32)
    n_bad = int(rr.bad_rays(rays).sum())
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(program, work, pos, r2, none, rays, t0, t1):
        assert rc == 0 and np.all(hit == rr.INVALID) and np.all(np.isinf(tt)) and np.all(np.isnan(uv))
        assert st["n_hit"] == 0 and st["n_bad_rays"] == n_bad and st["n_entries"] == 0 and extra["n_blocks_set"] == 0 and extra["bit_tests"] == 0
        assert extra["k"] == (occ - 1 if occ > 0 else -1)
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(program, work, pos, r2, tri, np.zeros((0, 6), np.float32), 0.0, 1.0, 0.2):
        assert rc == 0 and hit.size == 0 and st["n_rays"] == 0 and st["n_entries"] == rr.structure(pos, r2, tri, 0.2)["n_entries"]
    # two small triangles 120 m apart at the smallest cell: 2^33 bits at k = 5 (refused), below 2^31 at k = 6, which is the smallest that fits
    f = np.float32
    corner = np.array([[0, 0, 0], [0.001, 0, 0], [0, 0.001, 0]], f)
    far = np.concatenate([corner - f(59.99), corner + f(59.99)])
    far_r2, far_tri = np.full(6, 1e-4, f), np.array([[0, 1, 2], [3, 4, 5]], np.uint32)
    far_rays = np.array([[-59.9897, -59.9897, -50.0, 0, 0, -1], [59.9903, 59.9903, 50.0, 0, 0, 1], [0, 0, 0, 1, -1, 0.5]], f)
    want = rr.answer(rr.brute(far, far_r2, far_tri, far_rays, 0.0, 100.0), 0)
    assert want[3]["n_hit"] == 2
    g = sr.grid(far, far_r2, far_tri, 2.0 ** -9)
    assert not sr.fits(g, 5) and sr.fits(g, 6)
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(program, work, far, far_r2, far_tri, far_rays, 0.0, 100.0, 2.0 ** -9, 0, None, (1, 6, 7, 0, -1)):
        assert rc == (-3 if occ in (1, 6) else 0), (occ, rc)
        if rc == 0:
            assert extra["k"] == (6 if occ in (7, 0) else -1) and extra["bits_wrong"] == 0 and extra["relations_wrong"] == 0
            assert hit.tobytes() == want[0].tobytes() and tt.tobytes() == want[1].tobytes() and uv.tobytes() == want[2].tobytes()
            if extra["k"] == 6:
                assert extra["n_blocks_set"] == sr.blocks_set(g, 6) == 2 and extra["grid_bits"] == sr.bits(g, 6)


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    world = dr.world()
    for name, cs, cull in (("around the hand-made triangles", 0.0, 0), ("BAD and limits", 2.0 ** -9, 0), ("BAD and limits", 0.2, 1),
                           ("axis rays", 0.0225, 2), ("t_min = t_max", 0.2, 0)):
        rays, t0, t1 = rr.ray_sets()[name]
        _compare(sanitized, work, world, rr.model_of(name), rays, t0, t1, name + ", sanitized", cs, cull)
