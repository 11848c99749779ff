"""The arithmetic and the union-find of smx_components.hip without a GPU: smx_components.hpp holds the order key and its
inverse, diag2, the pass predicate, the rank record and cc_find / cc_unite as inline functions templated on how a word of
`parent` is loaded, compare-and-swapped and min'd.  This test compiles them for the host with the project's
-ffp-contract=off and walks the passes of the kernels one "lane" after the other -- forwards, backwards and in a seeded
shuffled order -- with plain words behind the three operations.  Everything has to equal the model of
tests/components_ref.py exactly, as on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
import mesh_ref as mr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

HARNESS = r'''
#define SMX_COMPONENTS_HOST_ONLY 1
#include "smx_components.hpp"
#include <algorithm>
#include <vector>
using namespace smx;

struct Words {                       // one lane at a time: the three operations on plain words
  uint32_t* parent;
  unsigned long long loads, hooks;
  uint32_t load(uint32_t i) { ++loads; return parent[i]; }
  uint32_t cas(uint32_t i, uint32_t expected, uint32_t desired) {
    const uint32_t old = parent[i];
    if (old == expected) { parent[i] = desired; ++hooks; }
    return old;
  }
  void min(uint32_t i, uint32_t v) { parent[i] = std::min(parent[i], v); }
};

struct Row { uint32_t label, n_vertices, n_triangles, kept; float lo[3], hi[3]; };
struct Acc { uint32_t n_vertices, n_triangles, nlo[3], hi[3]; };

// returns T_out, or -1 (an index out of range) / -3 (an invariant of the forest is broken).  S: [n][4] smooth x y z -,
// r2: [n]; lanes_t [n_in] and lanes_v [n]: the order in which the triangle and the slot passes walk their lanes.
// counters: not live, used, components, kept, largest, loads of parent.  table: room for n rows.
extern "C" int host_components(int n, const float* S, const float* r2, const uint32_t* tri, int n_in, uint32_t min_triangles,
                               float min_diagonal, uint32_t keep_largest, const uint32_t* lanes_t, const uint32_t* lanes_v,
                               uint32_t* out, uint32_t* label, Row* table, unsigned long long* counters) {
  for (int k = 0; k < 6; ++k) counters[k] = 0;
  auto live = [&](uint32_t i) { return cc_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], r2[i]); };
  std::vector<uint32_t> parent((size_t)n, kCcNoSlot), tcomp((size_t)n_in, kCcNoSlot);
  // k_cc_mark
  for (int l = 0; l < n_in; ++l) {
    const uint32_t t = lanes_t[l];
    const uint32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    if (i0 >= (uint32_t)n || i1 >= (uint32_t)n || i2 >= (uint32_t)n) return -1;
    if (live(i0) && live(i1) && live(i2)) { parent[i0] = i0; parent[i1] = i1; parent[i2] = i2; tcomp[t] = 0; } else ++counters[0];
  }
  // k_cc_link
  Words m{parent.data(), 0, 0};
  for (int l = 0; l < n_in; ++l) {
    const uint32_t t = lanes_t[l];
    if (tcomp[t] == kCcNoSlot) continue;
    cc_unite(m, tri[3 * t], tri[3 * t + 1]);
    cc_unite(m, tri[3 * t], tri[3 * t + 2]);
    for (int c = 0; c < 3; ++c) if (parent[tri[3 * t + c]] > tri[3 * t + c]) return -3;
  }
  // k_cc_flatten, the scan, k_cc_number
  for (int l = 0; l < n; ++l) {
    const uint32_t i = lanes_v[l];
    label[i] = m.load(i) != kCcNoSlot ? cc_find(m, i) : kCcNoSlot;
    if (label[i] != kCcNoSlot) ++counters[1];
  }
  for (int i = 0; i < n; ++i) if (parent[i] != kCcNoSlot && parent[i] > (uint32_t)i) return -3;
  counters[5] = m.loads;
  uint32_t C = 0;
  for (int i = 0; i < n; ++i) if (label[i] == (uint32_t)i) parent[i] = C++;
  counters[2] = C;
  // k_cc_measure_vertices / _triangles (accumulators start at zero; lo is kept as ~key)
  std::vector<Acc> acc(C, Acc{0, 0, {0, 0, 0}, {0, 0, 0}});
  for (int l = 0; l < n; ++l) {
    const uint32_t i = lanes_v[l];
    if (label[i] == kCcNoSlot) continue;
    const uint32_t c = parent[label[i]];
    if (label[i] == i) table[c].label = i;
    ++acc[c].n_vertices;
    for (int q = 0; q < 3; ++q) {
      const uint32_t k = cc_key(S[4 * (size_t)i + q]);
      acc[c].nlo[q] = std::max(acc[c].nlo[q], ~k);
      acc[c].hi[q] = std::max(acc[c].hi[q], k);
    }
  }
  for (int l = 0; l < n_in; ++l) {
    const uint32_t t = lanes_t[l];
    if (tcomp[t] == kCcNoSlot) continue;
    tcomp[t] = parent[label[tri[3 * t]]];
    ++acc[tcomp[t]].n_triangles;
  }
  // k_cc_pass, the sort, k_cc_rank
  std::vector<std::pair<unsigned long long, uint32_t>> rec;
  for (uint32_t d = 0; d < C; ++d) {
    Row& row = table[d];
    row.n_vertices = acc[d].n_vertices; row.n_triangles = acc[d].n_triangles;
    for (int q = 0; q < 3; ++q) { row.lo[q] = cc_unkey(~acc[d].nlo[q]); row.hi[q] = cc_unkey(acc[d].hi[q]); }
    const bool pass = cc_passes(row.n_triangles, cc_diag2(row.lo, row.hi), min_triangles, min_diagonal);
    row.kept = pass;
    counters[4] = std::max<unsigned long long>(counters[4], row.n_triangles);
    if (keep_largest > 0) rec.push_back({pass ? cc_rank_record(row.n_triangles, row.label) : kCcNoRecord, d});
    else counters[3] += pass;
  }
  if (keep_largest > 0) {
    std::stable_sort(rec.begin(), rec.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    for (uint32_t j = 0; j < C; ++j) {
      const bool kept = j < keep_largest && rec[j].first != kCcNoRecord;
      table[rec[j].second].kept = kept;
      counters[3] += kept;
    }
  }
  // k_cc_count / k_cc_write
  int T = 0;
  for (int t = 0; t < n_in; ++t)
    if (tcomp[t] != kCcNoSlot && table[tcomp[t]].kept) { for (int c = 0; c < 3; ++c) out[3 * T + c] = tri[3 * t + c]; ++T; }
  return T;
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("components_host")
    src = d / "components_host.cpp"
    src.write_text(HARNESS)
    lib = d / "libcomponents_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", SRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_components(L, pos, r2, tri, order, min_triangles=0, min_diagonal=0.0, keep_largest=0):
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3] = pos
    r = np.ascontiguousarray(r2, np.float32)
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    n_in = t.shape[0]
    if order == "forward":
        lanes_t, lanes_v = np.arange(n_in, dtype=np.uint32), np.arange(n, dtype=np.uint32)
    elif order == "reverse":
        lanes_t, lanes_v = np.arange(n_in, dtype=np.uint32)[::-1].copy(), np.arange(n, dtype=np.uint32)[::-1].copy()
    else:
        rng = np.random.default_rng(order)
        lanes_t, lanes_v = rng.permutation(n_in).astype(np.uint32), rng.permutation(n).astype(np.uint32)
    out, label = np.zeros((max(n_in, 1), 3), np.uint32), np.zeros(n, np.uint32)
    table, cnt = np.zeros(max(n, 1), cr.COMPONENT_DTYPE), np.zeros(6, np.uint64)
    T = L.host_components(n, _ptr(S), _ptr(r), _ptr(t), n_in, C.c_uint32(min_triangles), C.c_float(min_diagonal),
                          C.c_uint32(keep_largest), _ptr(lanes_t), _ptr(lanes_v), _ptr(out), _ptr(label), _ptr(table), _ptr(cnt))
    if T < 0:
        return T, None, None, None, 0
    st = dict(n_in=n_in, n_not_live=int(cnt[0]), n_used_vertices=int(cnt[1]), n_components=int(cnt[2]), n_kept_components=int(cnt[3]),
              n_largest_triangles=int(cnt[4]), n_triangles=T)
    return out[:T].copy(), label, table[:int(cnt[2])].copy(), st, int(cnt[5])


def _compare(L, pos, r2, tri, what, **p):
    want, wlabels, wtable, wst = cr.components(pos, r2, tri, **p)
    loads = []
    for order in ("forward", "reverse", 7):
        got, labels, table, st, n_loads = host_components(L, pos, r2, tri, order, **p)
        print("%s %s, lanes %s: %s, %d loads of parent" % (what, p, order, st, n_loads))
        assert st == wst and got.tobytes() == want.tobytes() and labels.tobytes() == wlabels.tobytes()
        assert table.tobytes() == wtable.tobytes()
        loads.append(n_loads)
    cr.check_properties(tri, want, wlabels, wtable, wst)
    return wst, loads


def strip(first, count, descending=True):
    """`count` triangles of a strip over the slots first .. first + count + 1, the slot indices descending along it."""
    k = np.arange(count, dtype=np.int64)
    top = first + count + 1
    v = (top - k) if descending else (first + k)
    s = -1 if descending else 1
    return np.stack([v, v + s, v + 2 * s], axis=1).astype(np.uint32)


def test_strips_give_deep_trees_and_one_component(host):
    n = 4096 + 2 + 5
    rng = np.random.default_rng(5)
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    r2 = np.ones(n, np.float32)
    tri = strip(3, 4096)
    st, loads = _compare(host, pos, r2, tri, "descending strip")
    assert st["n_components"] == 1 and st["n_used_vertices"] == 4098 and st["n_largest_triangles"] == 4096
    # path halving at work: the finds stay within a small multiple of the unions, whatever the order of the lanes
    assert max(loads) < 40 * 4096
    perm = np.arange(n)
    perm[3:3 + 4098] = 3 + rng.permutation(4098)
    st, loads = _compare(host, pos, r2, perm[tri.astype(np.int64)].astype(np.uint32), "permuted strip")
    assert st["n_components"] == 1 and st["n_used_vertices"] == 4098 and max(loads) < 40 * 4096
    # and cut in three by two dead slots
    r2[1000], r2[3000] = -1.0, -1.0
    st, _ = _compare(host, pos, r2, tri, "cut strip", min_triangles=1000, keep_largest=2)
    assert st["n_components"] == 3 and st["n_not_live"] == 6 and st["n_kept_components"] == 2


def test_hand_cases_on_the_host(host):
    pos = np.zeros((30, 3), np.float32)
    pos[:, 0] = np.arange(30)
    pos[:, 1] = np.where(np.arange(30) % 2 == 0, 0.0, -0.0)
    r2 = np.ones(30, np.float32)
    r2[12] = -1.0
    tri = np.array([[20, 21, 22], [0, 1, 2], [2, 3, 4],                    # an isolated triangle; a bowtie
                    [10, 11, 12], [8, 9, 10], [12, 13, 14],                # a bridge with a dead corner (two triangles go)
                    [15, 16, 17], [16, 17, 18], [24, 25, 26], [25, 26, 27], [26, 27, 28]], np.uint32)
    st, _ = _compare(host, pos, r2, tri, "hand cases")
    assert st["n_components"] == 5 and st["n_not_live"] == 2
    for p in (dict(min_triangles=2), dict(min_diagonal=3.0), dict(min_diagonal=float(np.nextafter(np.float32(3), np.float32(4)))),
              dict(keep_largest=1), dict(keep_largest=2), dict(min_triangles=2, keep_largest=7)):
        _compare(host, pos, r2, tri, "hand cases", **p)
    bad = tri.copy()
    bad[4, 2] = 30
    assert host_components(host, pos, r2, bad, "forward")[0] == -1
    st, _ = _compare(host, pos, r2, np.zeros((0, 3), np.uint32), "empty")
    assert st["n_components"] == 0 and st["n_triangles"] == 0


def test_sphere_and_plane_on_the_host(host):
    for name, m in (("sphere", mr.sphere_map()), ("plane", mr.plane_map())):
        tri = mr.triangulate(*m)[0]
        pos, _, r2 = m
        st, _ = _compare(host, pos, r2, tri, name)
        assert st["n_largest_triangles"] > 3000
        # a stale array: a tenth of the slots merged, which tears pieces off
        r2m = r2.copy()
        r2m[::10] = -1.0
        st, _ = _compare(host, pos, r2m, tri, name + ", stale", min_triangles=4)
        assert st["n_not_live"] > 0
        shuffled = tri[np.random.default_rng(11).permutation(tri.shape[0])]
        _compare(host, pos, r2m, shuffled, name + ", stale, shuffled", keep_largest=1)
