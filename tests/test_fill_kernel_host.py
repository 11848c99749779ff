"""The arithmetic and the table operations of smx_fill.hip without a GPU: smx_fill.hpp holds the edge key, insert and look-up
in the open-addressing table (templated on how an entry is read, claimed and bumped), the classification of an entry, the
bounded walk along next, cost, the apex key and the fan's triangle test as inline functions.  This test compiles them for
the host with the project's -ffp-contract=off into a stand-alone program (its own main: it reads a case file and writes a
result file) and walks the passes of the kernels one "lane" after the other -- forwards, backwards and in a seeded shuffled
order -- with plain words behind the table operations.  Every byte has to equal the model of tests/fill_ref.py, as on the
device.  The same program is also built with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import numpy as np
import pytest

import fill_cases as fc
import fill_ref as fr
import mesh_ref as mr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PROGRAM = r'''
#define SMX_FILL_HOST_ONLY 1
#include "smx_fill.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
using namespace smx;

struct Entry { unsigned long long key, value; };
struct Tab {                         // one lane at a time: the three operations on plain words
  Entry* e;
  unsigned long long key(uint32_t h) const { return e[h].key; }
  unsigned long long claim(uint32_t h, unsigned long long expected, unsigned long long desired) const {
    const unsigned long long old = e[h].key;
    if (old == expected) e[h].key = desired;
    return old;
  }
  void bump(uint32_t h, unsigned long long inc) const { e[h].value += inc; }
};
struct Vecs {
  const float* p;                    // [.][4]
  MeshVec operator[](uint32_t j) const { return MeshVec{p[4 * j], p[4 * j + 1], p[4 * j + 2]}; }
};
struct Hole { uint32_t label, n_edges, status; };

static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  std::iota(l.begin(), l.end(), 0u);
  if (order == 1) std::reverse(l.begin(), l.end());
  if (order > 1) { std::mt19937 g(order); std::shuffle(l.begin(), l.end(), g); }
  return l;
}

// stats: the twelve words of smx_fill_stats.  Returns 0, or -1 (an index out of range).
static int host_fill(uint32_t n, const float* S, const float* N, const uint32_t* tri, uint32_t n_in, uint32_t max_edges, float min_deg,
                     float max_deg, uint32_t order, std::vector<uint32_t>& out, uint32_t& kept, std::vector<Hole>& holes, uint32_t* stats) {
  for (int k = 0; k < 12; ++k) stats[k] = 0;
  stats[0] = n_in;
  const uint32_t entries = dec_table_size(3 * n_in), mask = entries - 1;
  std::vector<Entry> table(entries, Entry{kFillEmpty, 0});
  std::vector<uint32_t> keep(n_in, 0), deg(2 * (size_t)n, 0), next(n, 0xDEADBEEFu), len(n, 0);
  Tab tab{table.data()};
  auto live = [&](uint32_t i) { return dec_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], N[4 * (size_t)i + 3]); };
  // k_fill_edges
  uint32_t claimed = 0;
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    if (i0 >= n || i1 >= n || i2 >= n) return -1;
    if (live(i0) && live(i1) && live(i2)) {
      keep[t] = 1;
      claimed += fill_insert(tab, mask, i0, i1) + fill_insert(tab, mask, i1, i2) + fill_insert(tab, mask, i2, i0);
    } else {
      ++stats[1];
    }
  }
  // k_fill_classify
  for (uint32_t h : lanes(entries, order)) {
    const Entry e = table[h];
    if (e.key == kFillEmpty) continue;
    ++stats[2];
    const uint32_t lo = (uint32_t)((e.key - 1) >> 32), hi = (uint32_t)(e.key - 1);
    const uint32_t c = fill_classify(e.value);
    if (c == kFillNonManifold) ++stats[4];
    if (c == kFillBoundaryUp || c == kFillBoundaryDown) {
      ++stats[3];
      const uint32_t from = c == kFillBoundaryUp ? hi : lo, to = c == kFillBoundaryUp ? lo : hi;
      ++deg[2 * (size_t)from]; ++deg[2 * (size_t)to + 1];
      next[from] = to;                 // (the last lane to pass wins: only where out > 1, which nobody reads)
    }
  }
  if (claimed != stats[2]) return -2;
  // k_fill_walk, the scan, k_fill_list
  for (uint32_t i : lanes(n, order)) {
    const uint32_t o = deg[2 * (size_t)i], in = deg[2 * (size_t)i + 1];
    if ((o | in) != 0 && !(o == 1 && in == 1)) ++stats[5];
    const uint32_t L = fill_walk(deg.data(), next.data(), i, max_edges);
    len[i] = L < 3 ? 0 : L;
  }
  holes.clear();
  for (uint32_t i = 0; i < n; ++i) if (len[i] != 0) holes.push_back(Hole{i, len[i], 0});
  stats[6] = (uint32_t)holes.size();
  // k_fill_loops: the groups arrive in lane order, the lanes of a group likewise
  const double rad = 3.14159265358979323846 / 180.0;
  const float cmin = (float)std::cos((double)min_deg * rad), cmax = (float)std::cos((double)max_deg * rad);
  std::vector<DecTri> fresh;
  for (uint32_t g : lanes((uint32_t)holes.size(), order)) {
    Hole& row = holes[g];
    const uint32_t L = row.n_edges;
    uint32_t w[kFillMaxHoleEdges];
    float sp[kFillMaxHoleEdges * 4], sn[kFillMaxHoleEdges * 4];
    for (uint32_t j = 0; j < L; ++j) {
      uint32_t v = row.label;
      for (uint32_t s = 0; s < j; ++s) v = next[v];
      w[j] = v;
      for (int q = 0; q < 4; ++q) { sp[4 * j + q] = S[4 * (size_t)v + q]; sn[4 * j + q] = N[4 * (size_t)v + q]; }
    }
    const Vecs pos{sp}, nrm{sn};
    unsigned long long best = ~0ull;
    uint32_t ia = 0;
    for (uint32_t j : lanes(L, order)) {
      const unsigned long long key = dec_value_word(fill_cost(pos, L, j), w[j]);
      if (key < best) { best = key; ia = j; }
    }
    bool diagonal = false, rejected = false;
    for (uint32_t k : lanes(L, order)) {
      if (!(k >= 1 && k + 2 <= L)) continue;
      if (k >= 2) diagonal = diagonal || fill_has_edge(tab, mask, w[ia], w[(ia + k) % L]);
      rejected = rejected || !fill_fan_ok(pos, nrm, L, ia, k, cmin, cmax);
    }
    row.status = diagonal ? 2u : rejected ? 3u : 1u;
    ++stats[6 + row.status];
    if (row.status == 1)
      for (uint32_t k = 1; k + 2 <= L; ++k) fresh.push_back(dec_canonical(w[ia], w[(ia + k) % L], w[(ia + k + 1) % L]));
  }
  // the two stable sorts, by (a, b) and then by p
  std::stable_sort(fresh.begin(), fresh.end(), [](const DecTri& x, const DecTri& y) { return dec_key_ab(x, 32) < dec_key_ab(y, 32); });
  std::stable_sort(fresh.begin(), fresh.end(), [](const DecTri& x, const DecTri& y) { return x.p < y.p; });
  // k_fill_write, k_fill_emit
  out.clear();
  for (uint32_t t = 0; t < n_in; ++t) if (keep[t]) for (int c = 0; c < 3; ++c) out.push_back(tri[3 * t + c]);
  kept = (uint32_t)(out.size() / 3);
  for (const DecTri& c : fresh) { out.push_back(c.p); out.push_back(c.a); out.push_back(c.b); }
  stats[10] = (uint32_t)fresh.size();
  stats[11] = (uint32_t)(out.size() / 3);
  return 0;
}

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

// case file: u32 n, n_in, max_edges, n_orders; f32 min_deg, max_deg; u32 orders[n_orders]; f32 S[n][4], N[n][4]; u32 tri[n_in][3]
// result file, per order: i32 rc; u32 T, kept, H; u32 stats[12]; u32 out[T][3]; Hole holes[H]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[4];
  float ang[2];
  if (!get(f, head, 4) || !get(f, ang, 2)) return 2;
  std::vector<uint32_t> orders(head[3]), tri(3 * (size_t)head[1]);
  std::vector<float> S(4 * (size_t)head[0]), N(4 * (size_t)head[0]);
  if (!get(f, orders.data(), orders.size()) || !get(f, S.data(), S.size()) || !get(f, N.data(), N.size()) || !get(f, tri.data(), tri.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order : orders) {
    std::vector<uint32_t> out;
    std::vector<Hole> holes;
    uint32_t kept = 0, stats[12];
    const int32_t rc = host_fill(head[0], S.data(), N.data(), tri.data(), head[1], head[2], ang[0], ang[1], order, out, kept, holes, stats);
    const uint32_t sizes[3] = {rc == 0 ? (uint32_t)(out.size() / 3) : 0u, rc == 0 ? kept : 0u, rc == 0 ? (uint32_t)holes.size() : 0u};
    put(o, &rc, 1); put(o, sizes, 3); put(o, stats, 12);
    if (rc == 0) { put(o, out.data(), out.size()); put(o, holes.data(), holes.size()); }
  }
  fclose(o);
  return 0;
}
'''

ORDERS = (0, 1, 7)      # forwards, backwards, shuffled with seed 7


def _build(d, flags, name):
    src = d / "fill_host.cpp"
    src.write_text(PROGRAM)
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("fill_host")


@pytest.fixture(scope="module")
def program(work):
    return _build(work, [], "fill_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return _build(work, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "fill_host_san")


def host_fill(exe, work, pos, nrm, r2, tri, max_hole_edges=8, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0):
    n = pos.shape[0]
    S, N = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    S[:, :3], N[:, :3], N[:, 3] = pos, nrm, r2
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, t.shape[0], max_hole_edges, len(ORDERS)], np.uint32).tobytes())
        f.write(np.array([min_triangle_angle_deg, max_triangle_angle_deg], np.float32).tobytes())
        f.write(np.array(ORDERS, np.uint32).tobytes() + S.tobytes() + N.tobytes() + t.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint32), 0, []
    for _ in ORDERS:
        rc, T, kept, H = int(raw[at:at + 1].view(np.int32)[0]), int(raw[at + 1]), int(raw[at + 2]), int(raw[at + 3])
        st = dict(zip(fr.STAT_NAMES, (int(v) for v in raw[at + 4:at + 16])))
        at += 16
        out = raw[at:at + 3 * T].reshape(-1, 3).copy()
        at += 3 * T
        holes = raw[at:at + 3 * H].copy().view(fr.HOLE_DTYPE)
        at += 3 * H
        runs.append((rc, out, kept, holes, st))
    assert at == raw.size
    return runs


def _compare(exe, work, pos, nrm, r2, tri, what, **p):
    want, wkept, wholes, wst = fr.fill(pos, nrm, r2, tri, **p)
    differing = 0
    for order, (rc, out, kept, holes, st) in zip(ORDERS, host_fill(exe, work, pos, nrm, r2, tri, **p)):
        assert rc == 0 and st == wst and kept == wkept, (what, order, st, wst)
        differing += int(out.tobytes() != want.tobytes()) + int(holes.tobytes() != wholes.tobytes())
    print("%s %s: %s, %d differing" % (what, p, wst, differing))
    assert differing == 0, what
    return wst


PARAMETER_SETS = (dict(), dict(min_triangle_angle_deg=1.0, max_triangle_angle_deg=179.0), dict(max_hole_edges=4))


def test_hand_cases_on_the_host(program, work):
    for name, pos, nrm, r2, tri, expect in fc.cases():
        st = _compare(program, work, pos, nrm, r2, tri, name)
        for k, v in expect.items():
            assert st[k] == v, (name, k)
    pos, nrm, r2, tri = fc.plane()
    by_name = {c[0]: c[4] for c in fc.cases()}
    for L, cap, listed in ((8, 8, 1), (9, 8, 0), (32, 32, 1), (33, 32, 0)):
        st = _compare(program, work, pos, nrm, r2, by_name["hole of %d edges" % L], "hole of %d edges" % L, max_hole_edges=cap,
                      min_triangle_angle_deg=1.0, max_triangle_angle_deg=179.0)
        assert st["n_listed_loops"] == listed
    bad = by_name["one triangle deleted"].copy()
    bad[7, 1] = pos.shape[0]
    assert [r[0] for r in host_fill(program, work, pos, nrm, r2, bad)] == [-1, -1, -1]
    st = _compare(program, work, pos, nrm, r2, np.zeros((0, 3), np.uint32), "empty")
    assert st["n_triangles"] == 0 and st["n_edges"] == 0


def test_sphere_and_holed_plane_on_the_host(program, work):
    pos, nrm, r2 = mr.sphere_map()
    tri = mr.triangulate(pos, nrm, r2)[0]
    for p in PARAMETER_SETS:
        st = _compare(program, work, pos, nrm, r2, tri, "sphere", **p)
        assert st["n_listed_loops"] >= 80 and st["n_filled_loops"] >= 30
    hp = fc.holed_plane()
    for p in PARAMETER_SETS + (dict(max_hole_edges=32),):
        st = _compare(program, work, *hp, "holed plane", **p)
        assert st["n_rejected_diagonal"] == 1 and st["n_rejected_filter"] >= 2 and st["n_filled_loops"] >= 1


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    hp = fc.holed_plane()
    _compare(sanitized, work, *hp, "holed plane, sanitized", max_hole_edges=32)
    pos, nrm, r2 = mr.sphere_map()
    _compare(sanitized, work, pos, nrm, r2, mr.triangulate(pos, nrm, r2)[0], "sphere, sanitized")
