"""The arithmetic of smx_decimate.hip on the host, walked one "lane" after the other.  Test infrastructure shared by
tests/test_decimate_kernel_host.py and tests/test_decimate_cases.py, as tests/track_host.py is for the tracking kernels.

smx_decimate.hpp (part 1) holds the cell coordinate, key, centre, d2, value word, hashes and the canonical rotation as plain
inline functions.  The program below compiles them for the host with the project's -ffp-contract=off and walks the passes of
the kernels: the same two open-addressing tables, with a compare-and-swap and a minimum that one lane at a time makes trivial.
The lanes of every pass that meets others through a table go upwards (order 0), downwards (1) or in a shuffled order seeded
with `order` (any other value).  Beside the output the walk reports a census of what it did: per table the probe steps, the
longest chain and the wraps past the last entry, the table sizes, the `bits` of the sort key and how often an entry of the
triangle table was lowered by a later lane.

The same source is a shared library (host_library: the walk and thin exports of the header's functions, so that Python
restatements can be held to them bit for bit) and a program with its own main (host_program: one case from a file, the
output's bytes on stdout), which is what runs under the sanitizers.  Nothing loaded into Python is sanitized."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

N_COUNTERS = 5
CENSUS = ("cell_steps", "cell_longest", "cell_wraps", "tri_steps", "tri_longest", "tri_wraps", "cell_table", "tri_table", "bits",
          "lowered")

PROGRAM = r'''
#define SMX_DECIMATE_HOST_ONLY 1
#include "smx_decimate.hpp"
#include <stdio.h>
#include <algorithm>
#include <vector>
using namespace smx;

struct Cell { unsigned long long key, word; };

// The order in which the lanes of one pass arrive: upwards, downwards, or a Fisher-Yates shuffle driven by a 64-bit LCG.
static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  for (uint32_t i = 0; i < count; ++i) l[i] = order == 1 ? count - 1 - i : i;
  if (order > 1) {
    unsigned long long s = 0x9E3779B97F4A7C15ull * order + count;
    for (uint32_t i = count; i > 1; --i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(l[i - 1], l[(uint32_t)((s >> 33) % i)]);
    }
  }
  return l;
}

// returns T_out, or -1 (an index out of range) / -2 (a cell coordinate out of range); counters: not live, used, cells,
// collapsed, alive; census: see CENSUS in decimate_host.py.  S: [n][4] smooth x y z -, r2: [n].
extern "C" int host_decimate(int n, const float* S, const float* r2, const uint32_t* tri, int n_in, float cell_size, uint32_t order,
                             uint32_t* out, uint32_t* vmap, uint32_t* counters, uint32_t* census) {
  for (int k = 0; k < 5; ++k) counters[k] = 0;
  for (int k = 0; k < 10; ++k) census[k] = 0;
  const float inv = 1.0f / cell_size;
  auto live = [&](uint32_t i) { return dec_live(S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2], r2[i]); };
  for (int i = 0; i < n; ++i) vmap[i] = kDecNoSlot;
  // k_dec_mark
  for (uint32_t t : lanes((uint32_t)n_in, order)) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= (uint32_t)n || i1 >= (uint32_t)n || i2 >= (uint32_t)n) return -1;
    if (live(i0) && live(i1) && live(i2)) { vmap[i0] = 0; vmap[i1] = 0; vmap[i2] = 0; } else ++counters[0];
  }
  // k_dec_insert
  const uint32_t cells = dec_table_size((uint32_t)std::min<unsigned long long>((unsigned long long)n, 3ull * n_in));
  census[6] = cells;
  std::vector<Cell> table(cells, Cell{kDecEmpty, kDecEmpty});
  for (uint32_t i : lanes((uint32_t)n, order)) {
    if (vmap[i] == kDecNoSlot) continue;
    ++counters[1];
    const float* s = S + 4 * (size_t)i;
    int32_t cx, cy, cz;
    if (!(dec_cell_coord(s[0], inv, &cx) && dec_cell_coord(s[1], inv, &cy) && dec_cell_coord(s[2], inv, &cz))) return -2;
    const unsigned long long key = dec_cell_key(cx, cy, cz), word = dec_value_word(dec_d2(s[0], s[1], s[2], cx, cy, cz, cell_size), i);
    uint32_t h = dec_hash(key, cells - 1), chain = 0;
    for (;;) {
      if (table[h].key == kDecEmpty) { table[h].key = key; ++counters[2]; break; }
      if (table[h].key == key) break;
      if (h == cells - 1) ++census[2];
      h = (h + 1) & (cells - 1);
      ++chain;
    }
    census[0] += chain;
    census[1] = std::max(census[1], chain);
    table[h].word = std::min(table[h].word, word);
    vmap[i] = h;
  }
  // k_dec_lookup
  for (int i = 0; i < n; ++i) if (vmap[i] != kDecNoSlot) vmap[i] = dec_word_slot(table[vmap[i]].word);
  // k_dec_remap
  std::vector<DecTri> canon((size_t)n_in);
  for (int t = 0; t < n_in; ++t) {
    const uint32_t a = vmap[tri[3 * (size_t)t]], b = vmap[tri[3 * (size_t)t + 1]], c = vmap[tri[3 * (size_t)t + 2]];
    canon[t] = DecTri{kDecNoSlot, kDecNoSlot, kDecNoSlot};
    if (a == kDecNoSlot || b == kDecNoSlot || c == kDecNoSlot) continue;
    if (dec_collapsed(a, b, c)) { ++counters[3]; continue; }
    ++counters[4];
    canon[t] = dec_canonical(a, b, c);
  }
  // k_dec_dups
  const uint32_t dsize = dec_table_size((uint32_t)n_in);
  census[7] = dsize;
  std::vector<uint32_t> dup(dsize, kDecNoSlot), own((size_t)n_in, kDecNoSlot);
  for (uint32_t t : lanes((uint32_t)n_in, order)) {
    if (canon[t].p == kDecNoSlot) continue;
    uint32_t h = dec_tri_hash(canon[t], dsize - 1), chain = 0;
    for (;;) {
      if (dup[h] == kDecNoSlot) { dup[h] = t; break; }
      if (dec_same_corners(canon[dup[h]], canon[t])) { if (t < dup[h]) { dup[h] = t; ++census[9]; } break; }
      if (h == dsize - 1) ++census[5];
      h = (h + 1) & (dsize - 1);
      ++chain;
    }
    census[3] += chain;
    census[4] = std::max(census[4], chain);
    own[t] = h;
  }
  // k_dec_count / k_dec_write: the survivors in input order; the two stable sorts; k_dec_emit
  int bits = 1;
  while (bits < 32 && ((uint32_t)(n - 1) >> bits) != 0) ++bits;
  census[8] = (uint32_t)bits;
  std::vector<uint32_t> vals;
  for (int t = 0; t < n_in; ++t) if (own[t] != kDecNoSlot && dup[own[t]] == (uint32_t)t) vals.push_back((uint32_t)t);
  std::stable_sort(vals.begin(), vals.end(), [&](uint32_t x, uint32_t y) { return dec_key_ab(canon[x], bits) < dec_key_ab(canon[y], bits); });
  std::stable_sort(vals.begin(), vals.end(), [&](uint32_t x, uint32_t y) { return canon[x].p < canon[y].p; });
  for (size_t j = 0; j < vals.size(); ++j) { out[3 * j] = canon[vals[j]].p; out[3 * j + 1] = canon[vals[j]].a; out[3 * j + 2] = canon[vals[j]].b; }
  return (int)vals.size();
}

// The header's functions as they are, for the restatements in Python.
extern "C" uint32_t x_dec_hash(unsigned long long k, uint32_t mask) { return dec_hash(k, mask); }
extern "C" uint32_t x_dec_tri_hash(uint32_t p, uint32_t a, uint32_t b, uint32_t mask) { return dec_tri_hash(DecTri{p, a, b}, mask); }
extern "C" uint32_t x_dec_table_size(uint32_t entries) { return dec_table_size(entries); }
extern "C" int x_dec_cell_coord(float x, float inv, int32_t* c) { return dec_cell_coord(x, inv, c) ? 1 : 0; }
extern "C" float x_dec_cell_centre(int32_t c, float cell_size) { return dec_cell_centre(c, cell_size); }
extern "C" float x_dec_d2(float x, float y, float z, int32_t cx, int32_t cy, int32_t cz, float cell_size) {
  return dec_d2(x, y, z, cx, cy, cz, cell_size);
}

#if defined(DECIMATE_HOST_MAIN)
template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, stdout); }

// case file: u32 n, n_in, order; f32 cell; f32 S[n][4]; f32 r2[n]; u32 tri[n_in][3]
// stdout:    i32 T (or the refusal); u32 counters[5], census[10]; then, if T >= 0, u32 out[T][3], vmap[n]
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[3];
  float cell;
  if (!get(f, head, 3) || !get(f, &cell, 1)) return 2;
  std::vector<float> S(4 * (size_t)head[0]), r2(head[0]);
  std::vector<uint32_t> tri(3 * (size_t)head[1]), out(3 * (size_t)head[1] + 3), vmap((size_t)head[0] + 1);
  if (!get(f, S.data(), S.size()) || !get(f, r2.data(), r2.size()) || !get(f, tri.data(), tri.size())) return 2;
  fclose(f);
  uint32_t counters[5], census[10];
  const int32_t T = host_decimate((int)head[0], S.data(), r2.data(), tri.data(), (int)head[1], cell, head[2], out.data(), vmap.data(),
                                  counters, census);
  put(&T, 1); put(counters, 5); put(census, 10);
  if (T >= 0) { put(out.data(), 3 * (size_t)T); put(vmap.data(), head[0]); }
  return fflush(stdout) == 0 ? 0 : 2;
}
#endif
'''

UPWARDS, DOWNWARDS, SHUFFLED = 0, 1, 7       # the lane orders (SHUFFLED: the seed)
ORDERS = (UPWARDS, DOWNWARDS, SHUFFLED)
ORDER_NAMES = {UPWARDS: "upwards", DOWNWARDS: "downwards", SHUFFLED: "shuffled"}


def _build(d, flags, name):
    src = d / "decimate_host.cpp"
    src.write_text(PROGRAM)
    target = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(target)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(target)


def host_library(d):
    """The walk and the header's exports as a shared library built in directory d (a pathlib path)."""
    L = C.CDLL(_build(d, ["-shared", "-fPIC"], "libdecimate_host.so"))
    L.x_dec_hash.argtypes, L.x_dec_hash.restype = [C.c_uint64, C.c_uint32], C.c_uint32
    L.x_dec_tri_hash.argtypes, L.x_dec_tri_hash.restype = [C.c_uint32] * 4, C.c_uint32
    L.x_dec_table_size.argtypes, L.x_dec_table_size.restype = [C.c_uint32], C.c_uint32
    L.x_dec_cell_coord.argtypes, L.x_dec_cell_coord.restype = [C.c_float, C.c_float, C.POINTER(C.c_int32)], C.c_int
    L.x_dec_cell_centre.argtypes, L.x_dec_cell_centre.restype = [C.c_int32, C.c_float], C.c_float
    L.x_dec_d2.argtypes, L.x_dec_d2.restype = [C.c_float] * 3 + [C.c_int32] * 3 + [C.c_float], C.c_float
    return L


def host_program(d, sanitized=False):
    """The same source as a program of its own (path of the executable), optionally under address and undefined-behaviour
    sanitizers."""
    flags = ["-DDECIMATE_HOST_MAIN=1"]
    if sanitized:
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    return _build(d, flags, "decimate_host_san" if sanitized else "decimate_host")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _inputs(pos, r2, tri):
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3] = pos
    return S, np.ascontiguousarray(r2, np.float32), np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)


def _stats(n_in, cnt, T):
    return dict(n_in=n_in, n_not_live=int(cnt[0]), n_used_vertices=int(cnt[1]), n_cells=int(cnt[2]), n_collapsed=int(cnt[3]),
                n_duplicates=int(cnt[4]) - T, n_triangles=T)


def host_walk(L, pos, r2, tri, cell, order=UPWARDS):
    """(triangles_out, vertex_map, stats, census) of the walk in the given lane order, or (rc, None, None, None) if refused."""
    S, r, t = _inputs(pos, r2, tri)
    n = S.shape[0]
    out, vmap = np.zeros((max(t.shape[0], 1), 3), np.uint32), np.zeros(max(n, 1), np.uint32)
    cnt, cen = np.zeros(N_COUNTERS, np.uint32), np.zeros(len(CENSUS), np.uint32)
    T = L.host_decimate(n, _ptr(S), _ptr(r), _ptr(t), t.shape[0], C.c_float(cell), C.c_uint32(order), _ptr(out), _ptr(vmap), _ptr(cnt),
                        _ptr(cen))
    if T < 0:
        return T, None, None, None
    return out[:T].copy(), vmap[:n].copy(), _stats(t.shape[0], cnt, T), dict(zip(CENSUS, (int(v) for v in cen)))


def host_decimate(L, pos, r2, tri, cell, reverse=0):
    """(triangles_out, vertex_map, stats) of the walk, lanes upwards or (reverse != 0) downwards."""
    return host_walk(L, pos, r2, tri, cell, DOWNWARDS if reverse else UPWARDS)[:3]


def run_program(exe, case_path, pos, r2, tri, cell, order=UPWARDS):
    """One case through the stand-alone program: the same tuple as host_walk, read from the bytes it prints."""
    S, r, t = _inputs(pos, r2, tri)
    with open(case_path, "wb") as f:
        f.write(np.array([S.shape[0], t.shape[0], order], np.uint32).tobytes() + np.array([cell], np.float32).tobytes())
        f.write(S.tobytes() + r.tobytes() + t.tobytes())
    p = subprocess.run([exe, str(case_path)], capture_output=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:].decode(errors="replace"))
    raw = np.frombuffer(p.stdout, np.uint32)
    T = int(raw[:1].view(np.int32)[0])
    if T < 0:
        assert raw.size == 16
        return T, None, None, None
    assert raw.size == 16 + 3 * T + S.shape[0]
    out, vmap = raw[16:16 + 3 * T].reshape(-1, 3).copy(), raw[16 + 3 * T:].copy()
    return out, vmap, _stats(t.shape[0], raw[1:6], T), dict(zip(CENSUS, (int(v) for v in raw[6:16])))
