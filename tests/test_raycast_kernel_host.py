"""The arithmetic, the index and the traversal of smx_raycast.hip without a GPU: smx_raycast.hpp holds the BAD test of a ray, the
candidate test of step 3 with its key, the inflated box of a triangle, the dominant axis and its layers, the t interval and the
cell rectangle of a layer, the exit test and the walk of one ray as inline functions (the classes, the cell table and its
operations come from smx_distance.hpp).  This test compiles them for the host with the project's -ffp-contract=off into a
stand-alone program (its own main: it reads a case file and writes a result file) and walks mark, index, cast and stats one
"lane" after the other -- forwards and in a seeded shuffled order -- with plain words behind the table operations.  Every output
byte and every statistic has to equal the brute-force model of tests/raycast_ref.py, as on the device, for every ray set and
every cell size.  With the early exit off the program also checks, for EVERY candidate (ray, triangle) pair of the model and
not only the winners, that the triangle is on the wide list or entered in a cell the walk looked up.  The same program is also
built with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import raycast_ref as rr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PROGRAM = r'''
#define SMX_RAYCAST_HOST_ONLY 1
#include "smx_raycast.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
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
       PAIRS_MISSED, EXIT_DIFFERS, LAYERS, LOOKUPS, LAYERS_FULL, LOOKUPS_FULL, WORDS };

// Returns 0, or -1 (an index out of range).  pairs: (ray, triangle) candidates of the model, ascending by ray.
static int host_raycast(uint32_t n, const float* S, const uint32_t* tri, uint32_t n_in, const float* rays, uint32_t n_rays, float t_min, float t_max,
                        float cell_size, int cull, uint32_t order, const uint32_t* pairs, uint32_t n_pairs, uint32_t* hit, float* t_out, float* uv,
                        uint32_t* stats) {
  for (int k = 0; k < WORDS; ++k) stats[k] = 0;
  stats[N_IN] = n_in; stats[N_RAYS] = n_rays;
  auto pos = [&](uint32_t i) { return TgVec{S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2]}; };
  auto live = [&](uint32_t i) { return dec_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], S[4 * (size_t)i + 3]); };
  // k_ray_classify, k_ray_cell
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
  // k_ray_mark: the wide list in arrival order; the occupied box; the scan
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
  // k_ray_entries, the stable sort, k_ray_records
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
  // k_ray_table
  const uint32_t entries = dec_table_size(E), mask = entries - 1;
  std::vector<Entry> table(entries, Entry{kTgEmpty, 0});
  Tab tab{table.data()};
  for (uint32_t j : lanes(E, order)) stats[N_CELLS] += tg_table_entry(tab, mask, skeys.data(), E, j) ? 1u : 0u;
  // k_ray_cast, k_ray_stats
  const Recs cell_recs{recs.data()}, wrecs{wide_recs.data()};
  uint32_t at_pair = 0;
  for (uint32_t p = 0; p < n_rays; ++p) {
    const float* r = rays + 6 * (size_t)p;
    const TgVec O{r[0], r[1], r[2]}, D{r[3], r[4], r[5]};
    unsigned long long key = kTgNone;
    if (ray_bad(O, D)) {
      ++stats[N_BAD];
    } else {
      RayWork work{0, 0, 0}, full{0, 0, 0};
      RayAxes ax = ray_axes(O, D, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], cell, t_min, t_max);
      if (E == 0) ax.n_layers = 0;
      Unseen unseen;
      key = ray_cast_one(tab, mask, cell_recs, wrecs, (uint32_t)wide_t.size(), ax, O, D, cell, t_min, t_max, cull, true, unseen, &work);
      std::unordered_set<unsigned long long> cells;
      SeenSet seen{&cells};
      const unsigned long long all = ray_cast_one(tab, mask, cell_recs, wrecs, (uint32_t)wide_t.size(), ax, O, D, cell, t_min, t_max, cull, false, seen, &full);
      if (all != key) ++stats[EXIT_DIFFERS];
      stats[LAYERS] += work.layers; stats[LOOKUPS] += work.lookups; stats[LAYERS_FULL] += full.layers; stats[LOOKUPS_FULL] += full.lookups;
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
    if (key != kTgNone) {
      i = (uint32_t)key;
      RayHit h{0, 0, 0, 0};
      const unsigned long long again = ray_key(O, D, pos(tri[3 * (size_t)i]), pos(tri[3 * (size_t)i + 1]), pos(tri[3 * (size_t)i + 2]), i, t_min, t_max, cull, &h);
      if (again != key) ++stats[EXIT_DIFFERS];
      t = tg_key_float(key); u = h.u; v = h.v;
      ++stats[N_HIT];
      if (h.det > 0.0f) ++stats[N_FRONT];
      stats[MAX_BITS] = std::max(stats[MAX_BITS], (uint32_t)(key >> 32));
    }
    hit[p] = i; t_out[p] = t; uv[2 * (size_t)p] = u; uv[2 * (size_t)p + 1] = v;
  }
  stats[PAIRS_MISSED] += n_pairs - at_pair;
  return 0;
}

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

// case file: u32 n, n_in, n_rays, cull, n_pairs, n_orders; f32 t_min, t_max, cell_size; u32 orders[]; f32 S[n][4]; u32 tri[n_in][3];
//            f32 rays[n_rays][6]; u32 pairs[n_pairs][2]
// result file, per order: i32 rc; u32 stats[WORDS]; u32 hit[n_rays]; f32 t[n_rays]; f32 uv[n_rays][2]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[6];
  float prm[3];
  if (!get(f, head, 6) || !get(f, prm, 3)) return 2;
  std::vector<uint32_t> orders(head[5]), tri(3 * (size_t)head[1]), pairs(2 * (size_t)head[4]);
  std::vector<float> S(4 * (size_t)head[0]), rays(6 * (size_t)head[2]);
  if (!get(f, orders.data(), orders.size()) || !get(f, S.data(), S.size()) || !get(f, tri.data(), tri.size()) || !get(f, rays.data(), rays.size()) ||
      !get(f, pairs.data(), pairs.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order : orders) {
    std::vector<uint32_t> hit(head[2], 0xA5A5A5A5u);
    std::vector<float> t(head[2], 0.0f), uv(2 * (size_t)head[2], 0.0f);
    uint32_t stats[WORDS];
    const int32_t rc = host_raycast(head[0], S.data(), tri.data(), head[1], rays.data(), head[2], prm[0], prm[1], prm[2], (int)head[3], order,
                                    pairs.data(), head[4], hit.data(), t.data(), uv.data(), stats);
    put(o, &rc, 1); put(o, stats, (size_t)WORDS);
    put(o, hit.data(), hit.size()); put(o, t.data(), t.size()); put(o, uv.data(), uv.size());
  }
  fclose(o);
  return 0;
}
'''

ORDERS = (0, 7)      # forwards, shuffled with seed 7
WORDS = 19


def _build(d, flags, name):
    src = d / "raycast_host.cpp"
    src.write_text(PROGRAM)
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("raycast_host")


@pytest.fixture(scope="module")
def program(work):
    return _build(work, [], "raycast_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return _build(work, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "raycast_host_san")


def host_raycast(exe, work, pos, r2, tri, rays, t_min, t_max, cell_size=0.0, cull=0, pairs=None):
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3], S[:, 3] = pos, r2
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    ry = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    P = ry.shape[0]
    pr = np.zeros((0, 2), np.uint32) if pairs is None else np.ascontiguousarray(pairs, np.uint32)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, t.shape[0], P, int(cull), pr.shape[0], len(ORDERS)], np.uint32).tobytes())
        f.write(np.array([t_min, t_max, cell_size], np.float32).tobytes())
        f.write(np.array(ORDERS, np.uint32).tobytes() + S.tobytes() + t.tobytes() + ry.tobytes() + pr.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint32), 0, []
    for _ in ORDERS:
        rc = int(raw[at:at + 1].view(np.int32)[0])
        w = raw[at + 1:at + 1 + WORDS]
        st = dict(zip(rr.STAT_NAMES, (int(v) for v in w[:9])))
        st.update(n_wide=int(w[9]), n_entries=int(w[10]), n_cells=int(w[11]), cell_size_used=float(w[12:13].view(np.float32)[0]))
        extra = dict(pairs_missed=int(w[13]), exit_differs=int(w[14]), layers=int(w[15]), lookups=int(w[16]), layers_full=int(w[17]),
                     lookups_full=int(w[18]))
        at += 1 + WORDS
        hit, tt = raw[at:at + P].copy(), raw[at + P:at + 2 * P].copy().view(np.float32)
        uv = raw[at + 2 * P:at + 4 * P].copy().view(np.float32).reshape(-1, 2)
        at += 4 * P
        runs.append((rc, hit, tt, uv, st, extra))
    assert at == raw.size
    return runs


def _pairs_for(model, cull):
    """The candidate pairs of the model under `cull`, ascending by ray.  (The side of a pair is not kept, so cull 1 / 2 check the
    pairs of cull 0: a superset, which the walk with the exit off has to cover just the same.)"""
    p = model["pairs"]
    return p[np.argsort(p[:, 0], kind="stable")]


def _compare(exe, work, world, model, rays, t0, t1, what, cell_size, cull):
    pos, nrm, r2, tri, _ = world
    wh, wt, wuv, wst = rr.answer(model, cull)
    if cell_size > 0:
        wst.update(rr.structure(pos, r2, tri, cell_size))
    pairs = _pairs_for(model, cull)
    differing = 0
    for order, (rc, hit, tt, uv, st, extra) in zip(ORDERS, host_raycast(exe, work, pos, r2, tri, rays, t0, t1, cell_size, cull, pairs)):
        assert rc == 0
        used = st.pop("cell_size_used")
        if cell_size > 0:
            assert used == float(rr.cell_used(cell_size))
        else:
            assert used >= float(rr.MIN_CELL)
            for k in ("n_wide", "n_entries", "n_cells"):
                st.pop(k)
        assert st == wst, (what, order, st, wst)
        assert extra["pairs_missed"] == 0 and extra["exit_differs"] == 0, (what, order, extra)
        differing += sum(int(a.tobytes() != b.tobytes()) for a, b in ((hit, wh), (tt, wt), (uv, wuv)))
    print("%s cell %g cull %d: %d hit, %d candidate pairs all met, %.2f cells per layer (%d layers, %d with the exit off), %d differing arrays"
          % (what, cell_size, cull, wst["n_hit"], pairs.shape[0], extra["lookups_full"] / max(1, extra["layers_full"]), extra["layers"],
             extra["layers_full"], differing))
    assert differing == 0, what


def test_every_ray_set_on_the_host(program, work):
    world = dr.world()
    for k, (name, (rays, t0, t1)) in enumerate(rr.ray_sets().items()):
        m = rr.model_of(name)
        for j, cs in enumerate(rr.CELL_SIZES):
            _compare(program, work, world, m, rays, t0, t1, name, cs, (k + j) % 3)


def test_every_cull_mode_on_the_host(program, work):
    world = dr.world()
    for name in ("around the hand-made triangles", "inside-out"):
        rays, t0, t1 = rr.ray_sets()[name]
        for cull in (0, 1, 2):
            _compare(program, work, world, rr.model_of(name), rays, t0, t1, name, 0.0225, cull)


def test_an_index_out_of_range_and_empty_inputs_on_the_host(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    rays, t0, t1 = rr.ray_sets()["BAD and limits"]
    bad = tri.copy()
    bad[77, 2] = pos.shape[0]
    assert [r[0] for r in host_raycast(program, work, pos, r2, bad, rays, t0, t1)] == [-1, -1]
    none = np.zeros((0, 3), np.uint32)
    n_bad = int(rr.bad_rays(rays).sum())
    for rc, hit, tt, uv, st, extra in host_raycast(program, work, pos, r2, none, rays, t0, t1):
        assert rc == 0 and np.all(hit == rr.INVALID) and np.all(np.isinf(tt)) and np.all(np.isnan(uv))
        assert st["n_hit"] == 0 and st["n_bad_rays"] == n_bad and st["n_entries"] == 0
    for rc, hit, tt, uv, st, extra in host_raycast(program, work, pos, r2, tri, np.zeros((0, 6), np.float32), 0.0, 1.0, 0.2):
        assert rc == 0 and hit.size == 0 and st["n_rays"] == 0 and st["n_entries"] == rr.structure(pos, r2, tri, 0.2)["n_entries"]


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    world = dr.world()
    for name, cs, cull in (("around the hand-made triangles", 0.0, 0), ("BAD and limits", 2.0 ** -9, 0), ("BAD and limits", 0.2, 1),
                           ("axis rays", 0.0225, 2), ("t_min = t_max", 0.2, 0)):
        rays, t0, t1 = rr.ray_sets()[name]
        _compare(sanitized, work, world, rr.model_of(name), rays, t0, t1, name + ", sanitized", cs, cull)
