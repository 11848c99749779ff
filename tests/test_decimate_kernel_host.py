"""The arithmetic of smx_decimate.hip without a GPU: smx_decimate.hpp holds the cell coordinate, key, centre, d2, value
word, hashes and the canonical rotation as plain inline functions, so this test compiles them for the host with the
project's -ffp-contract=off and walks the passes of the kernels one "lane" after the other -- the same two open-addressing
tables, with a compare-and-swap and a minimum that one lane at a time makes trivial -- in forward and in reverse lane
order.  The output has to equal the model of tests/decimate_ref.py exactly, as on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decimate_ref as dr
import mesh_ref as mr
from common import ROOT, small_pre

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

HARNESS = r'''
#define SMX_DECIMATE_HOST_ONLY 1
#include "smx_decimate.hpp"
#include <algorithm>
#include <vector>
using namespace smx;

struct Cell { unsigned long long key, word; };

// returns T_out, or -1 (an index out of range) / -2 (a cell coordinate out of range); counters: not live, used, cells,
// collapsed, alive.  S: [n][4] smooth x y z -, r2: [n].  reverse != 0 walks every pass's lanes downwards.
extern "C" int host_decimate(int n, const float* S, const float* r2, const uint32_t* tri, int n_in, float cell_size, int reverse,
                             uint32_t* out, uint32_t* vmap, uint32_t* counters) {
  for (int k = 0; k < 5; ++k) counters[k] = 0;
  const float inv = 1.0f / cell_size;
  auto lane = [&](int i, int count) { return reverse ? count - 1 - i : i; };
  auto live = [&](uint32_t i) { return dec_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], r2[i]); };
  for (int i = 0; i < n; ++i) vmap[i] = kDecNoSlot;
  // k_dec_mark
  for (int l = 0; l < n_in; ++l) {
    const int t = lane(l, n_in);
    const uint32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    if (i0 >= (uint32_t)n || i1 >= (uint32_t)n || i2 >= (uint32_t)n) return -1;
    if (live(i0) && live(i1) && live(i2)) { vmap[i0] = 0; vmap[i1] = 0; vmap[i2] = 0; } else ++counters[0];
  }
  // k_dec_insert
  const uint32_t cells = dec_table_size((uint32_t)std::min<unsigned long long>((unsigned long long)n, 3ull * n_in));
  std::vector<Cell> table(cells, Cell{kDecEmpty, kDecEmpty});
  for (int l = 0; l < n; ++l) {
    const int i = lane(l, n);
    if (vmap[i] == kDecNoSlot) continue;
    ++counters[1];
    const float* s = S + 4 * (size_t)i;
    int32_t cx, cy, cz;
    if (!(dec_cell_coord(s[0], inv, &cx) && dec_cell_coord(s[1], inv, &cy) && dec_cell_coord(s[2], inv, &cz))) return -2;
    const unsigned long long key = dec_cell_key(cx, cy, cz), word = dec_value_word(dec_d2(s[0], s[1], s[2], cx, cy, cz, cell_size), (uint32_t)i);
    uint32_t h = dec_hash(key, cells - 1);
    for (;;) {
      if (table[h].key == kDecEmpty) { table[h].key = key; ++counters[2]; break; }
      if (table[h].key == key) break;
      h = (h + 1) & (cells - 1);
    }
    table[h].word = std::min(table[h].word, word);
    vmap[i] = h;
  }
  // k_dec_lookup
  for (int i = 0; i < n; ++i) if (vmap[i] != kDecNoSlot) vmap[i] = dec_word_slot(table[vmap[i]].word);
  // k_dec_remap
  std::vector<DecTri> canon((size_t)n_in);
  for (int t = 0; t < n_in; ++t) {
    const uint32_t a = vmap[tri[3 * t]], b = vmap[tri[3 * t + 1]], c = vmap[tri[3 * t + 2]];
    canon[t] = DecTri{kDecNoSlot, kDecNoSlot, kDecNoSlot};
    if (a == kDecNoSlot || b == kDecNoSlot || c == kDecNoSlot) continue;
    if (dec_collapsed(a, b, c)) { ++counters[3]; continue; }
    ++counters[4];
    canon[t] = dec_canonical(a, b, c);
  }
  // k_dec_dups
  const uint32_t dsize = dec_table_size((uint32_t)n_in);
  std::vector<uint32_t> dup(dsize, kDecNoSlot), own((size_t)n_in, kDecNoSlot);
  for (int l = 0; l < n_in; ++l) {
    const uint32_t t = (uint32_t)lane(l, n_in);
    if (canon[t].p == kDecNoSlot) continue;
    uint32_t h = dec_tri_hash(canon[t], dsize - 1);
    for (;;) {
      if (dup[h] == kDecNoSlot) { dup[h] = t; break; }
      if (dec_same_corners(canon[dup[h]], canon[t])) { dup[h] = std::min(dup[h], t); break; }
      h = (h + 1) & (dsize - 1);
    }
    own[t] = h;
  }
  // k_dec_count / k_dec_write: the survivors in input order; the two stable sorts; k_dec_emit
  int bits = 1;
  while (bits < 32 && ((uint32_t)(n - 1) >> bits) != 0) ++bits;
  std::vector<uint32_t> vals;
  for (int t = 0; t < n_in; ++t) if (own[t] != kDecNoSlot && dup[own[t]] == (uint32_t)t) vals.push_back((uint32_t)t);
  std::stable_sort(vals.begin(), vals.end(), [&](uint32_t x, uint32_t y) { return dec_key_ab(canon[x], bits) < dec_key_ab(canon[y], bits); });
  std::stable_sort(vals.begin(), vals.end(), [&](uint32_t x, uint32_t y) { return canon[x].p < canon[y].p; });
  for (size_t j = 0; j < vals.size(); ++j) { out[3 * j] = canon[vals[j]].p; out[3 * j + 1] = canon[vals[j]].a; out[3 * j + 2] = canon[vals[j]].b; }
  return (int)vals.size();
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("decimate_host")
    src = d / "decimate_host.cpp"
    src.write_text(HARNESS)
    lib = d / "libdecimate_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", SRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_decimate(L, pos, r2, tri, cell, reverse=0):
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3] = pos
    r = np.ascontiguousarray(r2, np.float32)
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    out, vmap, cnt = np.zeros((max(t.shape[0], 1), 3), np.uint32), np.zeros(n, np.uint32), np.zeros(5, np.uint32)
    T = L.host_decimate(n, _ptr(S), _ptr(r), _ptr(t), t.shape[0], C.c_float(cell), reverse, _ptr(out), _ptr(vmap), _ptr(cnt))
    if T < 0:
        return T, None, None
    st = dict(n_in=t.shape[0], n_not_live=int(cnt[0]), n_used_vertices=int(cnt[1]), n_cells=int(cnt[2]), n_collapsed=int(cnt[3]),
              n_duplicates=int(cnt[4]) - T, n_triangles=T)
    return out[:T].copy(), vmap, st


def _compare(L, m, tri, cell, what):
    pos, _, r2 = m
    want, wmap, wst = dr.decimate(pos, r2, tri, cell)
    for reverse in (0, 1):
        got, vmap, st = host_decimate(L, pos, r2, tri, cell, reverse)
        print("%s, cell %g, lanes %s: %s" % (what, cell, "downwards" if reverse else "upwards", st))
        assert st == wst and got.tobytes() == want.tobytes() and vmap.tobytes() == wmap.tobytes()
    return wst


def test_sphere_on_the_host(host):
    m = mr.sphere_map()
    tri = mr.triangulate(*m)[0]
    assert _compare(host, m, tri, 0.03, "sphere")["n_triangles"] == 6059
    assert _compare(host, m, tri, 0.1, "sphere")["n_triangles"] == 2112
    # a stale array: a tenth of the slots merged
    r2 = m[2].copy()
    r2[::10] = -1.0
    assert _compare(host, (m[0], m[1], r2), tri, 0.1, "sphere, stale")["n_not_live"] > 0


def test_plane_on_the_host(host):
    m = mr.plane_map()
    tri = mr.triangulate(*m)[0]
    assert _compare(host, m, tri, 2.0, "plane")["n_triangles"] == 766
    assert host_decimate(host, m[0], m[2], tri, 1e-5)[0] == -2           # the coordinate range
    bad = tri.copy()
    bad[5, 1] = m[0].shape[0]
    assert host_decimate(host, m[0], m[2], bad, 2.0)[0] == -1


def test_oracle_grown_map_on_the_host(host, orc):
    from oracle_pipeline import OraclePipeline
    from test_golden import G, run_golden_stream
    fx, fy, cx, cy = [float(v) for v in G["intr"]]
    h, w = G["depth"].shape[1:]
    po = OraclePipeline(w, h, fx, fy, cx, cy, 30000, small_pre(w))
    run_golden_stream(po)
    m = mr.map_of_rows(po.recon.surfels(), po.recon.surfels_size)
    tri = mr.triangulate(*m)[0]
    assert _compare(host, m, tri, 0.05, "grown map")["n_triangles"] == 5349
