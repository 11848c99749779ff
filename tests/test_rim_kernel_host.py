"""The integer rules of smx_rim.hip without a GPU: smx_rim.hpp holds the count of a pair, the look-up of an edge of R, the
once-only mark of a non-manifold entry, the edge bits, the corner marks, the bitmap's word and bit and the byte as inline
functions; the table's key and insert are smx_fill.hpp's.  This test compiles them for the host with the project's
-ffp-contract=off into a stand-alone program (its own main: it reads a case file and writes a result file) and walks the three
passes of the kernels one "lane" after the other -- forwards, backwards and in a seeded shuffled order -- with plain words
behind the table operations.  Every byte and every statistic has to equal the model of tests/rim_ref.py, as on the device.  The
same program is also built with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import rim_ref as rf
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PROGRAM = r'''
#define SMX_RIM_HOST_ONLY 1
#include "smx_rim.hpp"
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
using namespace smx;

struct Entry { unsigned long long key, value; };
struct Tab {                         // one lane at a time: the operations on plain words
  Entry* e;
  uint32_t mask;
  uint32_t* wraps;                   // census: probe chains that went from the last entry to entry 0
  unsigned long long key(uint32_t h) const { return e[h].key; }
  unsigned long long value(uint32_t h) const { return e[h].value; }
  unsigned long long claim(uint32_t h, unsigned long long expected, unsigned long long desired) const {
    const unsigned long long old = e[h].key;
    if (old == expected) e[h].key = desired;
    else if (old != desired && h == mask) ++*wraps;
    return old;
  }
  void bump(uint32_t h, unsigned long long inc) const { e[h].value += inc; }
  unsigned long long mark(uint32_t h, unsigned long long bits) const { const unsigned long long old = e[h].value; e[h].value = old | bits; return old; }
};

static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  std::iota(l.begin(), l.end(), 0u);
  if (order == 1) std::reverse(l.begin(), l.end());
  if (order > 1) { std::mt19937 g(order); std::shuffle(l.begin(), l.end(), g); }
  return l;
}

// stats: the nine words of smx_rim_stats, then the census (wrapped chains, entries of the table).  Returns 0, or -1 (an index
// out of range: nothing is written).
static int host_rim(uint32_t n, const float* S, const float* N, const uint32_t* tri, uint32_t n_in, uint32_t order, std::vector<uint8_t>& out,
                    uint32_t* stats) {
  for (int k = 0; k < 11; ++k) stats[k] = 0;
  stats[0] = n_in;
  const uint32_t entries = dec_table_size(3 * n_in), mask = entries - 1;
  stats[10] = entries;
  std::vector<Entry> table(entries, Entry{kFillEmpty, 0});
  std::vector<uint32_t> bitmap((size_t)n / 32 + 1, 0);
  std::vector<uint8_t> bytes(n_in, 0);
  Tab tab{table.data(), mask, &stats[9]};
  auto vec = [&](uint32_t i) { return TgVec{S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2]}; };
  auto live = [&](uint32_t i) { return dec_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], N[4 * (size_t)i + 3]); };
  // k_rim_edges
  bool bad_index = false;
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= n || i1 >= n || i2 >= n) { bad_index = true; continue; }
    const uint32_t cls = tg_classify(i0, i1, i2, live(i0), live(i1), live(i2), vec(i0), vec(i1), vec(i2));
    if (cls == kTgDropNotLive) ++stats[1];
    if (cls == kTgDropRepeated) ++stats[2];
    if (cls == kTgDropRange) ++stats[3];
    if (cls != kTgInR) continue;
    bytes[t] = (uint8_t)kRimInR;
    stats[4] += (fill_insert(tab, mask, i0, i1) ? 1u : 0u) + (fill_insert(tab, mask, i1, i2) ? 1u : 0u) + (fill_insert(tab, mask, i2, i0) ? 1u : 0u);
  }
  if (bad_index) return -1;
  // k_rim_vertices
  for (uint32_t t : lanes(n_in, order)) {
    if (bytes[t] == 0) continue;
    const uint32_t i[3] = {tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2]};
    bool first[3];
    const uint32_t c_ab = rim_edge(tab, mask, i[0], i[1], &first[0]), c_bc = rim_edge(tab, mask, i[1], i[2], &first[1]),
                   c_ca = rim_edge(tab, mask, i[2], i[0], &first[2]);
    const uint32_t edge_bits = rim_edge_bits(c_ab, c_bc, c_ca);
    bytes[t] = (uint8_t)(kRimInR | edge_bits);
    const uint32_t marks = rim_corner_marks(edge_bits);
    stats[5] += (uint32_t)__builtin_popcount(edge_bits);
    stats[6] += (first[0] ? 1u : 0u) + (first[1] ? 1u : 0u) + (first[2] ? 1u : 0u);
    for (int k = 0; k < 3; ++k) {
      if (!((marks >> k) & 1u)) continue;
      uint32_t& word = bitmap[rim_word(i[k])];
      if (!(word & rim_bit(i[k]))) ++stats[7];
      word |= rim_bit(i[k]);
    }
  }
  // k_rim_bytes
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t held = bytes[t];
    if (held == 0) continue;
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    const uint32_t byte = rim_byte(held & ~kRimInR, rim_vertex(bitmap.data(), i0), rim_vertex(bitmap.data(), i1), rim_vertex(bitmap.data(), i2));
    bytes[t] = (uint8_t)byte;
    if (byte != 0) ++stats[8];
  }
  out = bytes;
  return 0;
}

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

// case file: u32 n, n_in, n_orders; u32 orders[n_orders]; f32 S[n][4], N[n][4]; u32 tri[n_in][3]
// result file, per order: i32 rc; u32 stats[11]; u8 bytes[n_in] if rc == 0.  Then u8 hits[64][7] = rim_hit(byte, region).
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[3];
  if (!get(f, head, 3)) return 2;
  std::vector<uint32_t> orders(head[2]), tri(3 * (size_t)head[1]);
  std::vector<float> S(4 * (size_t)head[0]), N(4 * (size_t)head[0]);
  if (!get(f, orders.data(), orders.size()) || !get(f, S.data(), S.size()) || !get(f, N.data(), N.size()) || !get(f, tri.data(), tri.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order : orders) {
    std::vector<uint8_t> out;
    uint32_t stats[11];
    const int32_t rc = host_rim(head[0], S.data(), N.data(), tri.data(), head[1], order, out, stats);
    put(o, &rc, 1); put(o, stats, 11);
    if (rc == 0) put(o, out.data(), out.size());
  }
  for (uint32_t byte = 0; byte < 64; ++byte)
    for (uint32_t region = 0; region < 7; ++region) { const uint8_t h = rim_hit(byte, region) ? 1 : 0; put(o, &h, 1); }
  fclose(o);
  return 0;
}
'''

ORDERS = (0, 1, 7)      # forwards, backwards, shuffled with seed 7


def _build(d, flags, name):
    src = d / "rim_host.cpp"
    src.write_text(PROGRAM)
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("rim_host")


@pytest.fixture(scope="module")
def program(work):
    return _build(work, [], "rim_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return _build(work, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "rim_host_san")


def host_rim(exe, work, pos, r2, tri):
    """[(rc, bytes, stats, census)] per order, and the table of rim_hit."""
    n = pos.shape[0]
    S, N = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    with np.errstate(over="ignore"):
        S[:, :3], N[:, 3] = pos, r2
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, t.shape[0], len(ORDERS)], np.uint32).tobytes())
        f.write(np.array(ORDERS, np.uint32).tobytes() + S.tobytes() + N.tobytes() + t.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint8), 0, []
    for _ in ORDERS:
        rc = int(raw[at:at + 4].view(np.int32)[0])
        words = raw[at + 4:at + 48].view(np.uint32)
        at += 48
        out = None
        if rc == 0:
            out = raw[at:at + t.shape[0]].copy()
            at += t.shape[0]
        runs.append((rc, out, dict(zip(rf.STAT_NAMES, (int(v) for v in words[:9]))), dict(wraps=int(words[9]), entries=int(words[10]))))
    hits = raw[at:at + 64 * 7].reshape(64, 7)
    assert at + 64 * 7 == raw.size
    return runs, hits


def _compare(exe, work, pos, r2, tri, what):
    want, wst = rf.rim(pos, r2, tri)
    runs, _ = host_rim(exe, work, pos, r2, tri)
    for order, (rc, out, st, census) in zip(ORDERS, runs):
        assert rc == 0 and st == wst, (what, order, st, wst)
        assert out.tobytes() == want.tobytes(), (what, order)
    print("%s: %s, %s" % (what, wst, runs[0][3]))
    return wst, runs[0][3]


def test_every_case_on_the_host(program, work):
    for name, pos, r2, tri, _, _ in rf.cases():
        _, census = _compare(program, work, pos, r2, tri, name)
        if name.startswith("pairs that hash"):
            assert census["wraps"] >= 1 and census["entries"] == 64
    pos, r2 = rf.grid_map()
    wst, _ = _compare(program, work, pos, r2, np.zeros((0, 3), np.uint32), "empty")
    assert all(v == 0 for v in wst.values())


def test_an_index_out_of_range_is_refused_on_the_host(program, work):
    for pos, r2, tri in rf.refused():
        runs, _ = host_rim(program, work, pos, r2, tri)
        assert [r[0] for r in runs] == [-1, -1, -1] and all(r[1] is None for r in runs)
        with pytest.raises(ValueError):
            rf.rim(pos, r2, tri)


def test_the_world_of_the_distance_tests_on_the_host(program, work):
    """The noisy sphere, the holed plane and the hand-made triangles (a dead slot, a repeated index, a corner at 65 m, the same
    triangle twice and once more with the other winding): about 10 000 triangles, tables of 65 536 entries."""
    pos, _, r2, tri, _ = dr.world()
    wst, census = _compare(program, work, pos, r2, tri, "world")
    assert wst["n_not_live"] > 0 and wst["n_repeated"] == 1 and wst["n_out_of_range"] == 1 and wst["n_nonmanifold_edges"] >= 1
    assert wst["n_rim_edges"] > 100 and census["entries"] == 65536


def test_rim_hit_is_the_bit_of_the_region(program, work):
    pos, r2 = rf.grid_map()
    _, hits = host_rim(program, work, pos, r2, np.zeros((0, 3), np.uint32))
    for byte in range(64):
        for region in range(7):
            assert bool(hits[byte, region]) == rf.hit(byte, region) == bool((byte >> region) & 1)
        assert not hits[byte, 6]


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    for name, pos, r2, tri, _, _ in rf.cases():
        _compare(sanitized, work, pos, r2, tri, name + ", sanitized")
    pos, _, r2, tri, _ = dr.world()
    _compare(sanitized, work, pos, r2, tri, "world, sanitized")
    for pos, r2, tri in rf.refused()[:1]:
        assert [r[0] for r in host_rim(sanitized, work, pos, r2, tri)[0]] == [-1, -1, -1]
