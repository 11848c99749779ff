"""smx_merge.hpp, the arithmetic the kernels of smx_recon_merge_map call, compiled for the host (-ffp-contract=off) into a stand-alone
program with its own main and walked in lane order: move, select, number, append and blend a "lane" at a time, forwards and
backwards, over every case of tests/merge_cases.py in both modes.  The program is handed the model's candidate lists (the
neighbour search has its own tests) and must equal the model (tests/merge_ref.py) byte for byte.  The same program is built
with the sanitizers and run directly.  CPU only."""
import subprocess

import numpy as np
import pytest

import merge_cases as mc
import merge_ref as mr
import ray_host

PROGRAM = r'''
#define SMX_MERGE_HOST_ONLY 1
#include "smx_merge.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
using namespace smx;

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }
static uint32_t word_of(float f) { uint32_t w; memcpy(&w, &f, 4); return w; }
static float float_of(uint32_t w) { float f; memcpy(&f, &w, 4); return f; }
static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  std::iota(l.begin(), l.end(), 0u);
  if (order == 1) std::reverse(l.begin(), l.end());
  return l;
}

struct Map {                       // rows [25][n], as the debug download gives them
  uint32_t n;
  std::vector<float> rows;
  float& f(int row, uint32_t i) { return rows[(size_t)row * n + i]; }
  uint32_t u(int row, uint32_t i) { return word_of(f(row, i)); }
  void set_u(int row, uint32_t i, uint32_t w) { f(row, i) = float_of(w); }
  MgVec vec(int row, uint32_t i) { return MgVec{f(row, i), f(row + 1, i), f(row + 2, i)}; }
  void set_vec(int row, uint32_t i, const MgVec& v) { f(row, i) = v.x; f(row + 1, i) = v.y; f(row + 2, i) = v.z; }
};
enum { N_SRC, N_LIVE, N_BAD, N_MATCHED, N_APPENDED, N_BLENDED, N_SATURATED, N_DROPPED, OLD_SIZE, NEW_SIZE, WORDS };

// Returns 0, or 1 (the over-full refusal: out = dst as it stood).
static int host_merge(Map dst, Map& src, const float* T, float factor_sq, float cos_max, float cap, int k, int mode, uint32_t frame,
                      uint32_t max_surfels, const int32_t* cnt, const uint32_t* idx, uint32_t order, Map* out, std::vector<uint32_t>* s2d,
                      uint32_t* st) {
  const uint32_t n = src.n, old_size = dst.n;
  for (int e = 0; e < WORDS; ++e) st[e] = 0;
  st[N_SRC] = n; st[OLD_SIZE] = st[NEW_SIZE] = old_size;
  // k_merge_move
  std::vector<MgMoved> mv(n);
  std::vector<uint32_t> cls(n), match(n, 0xA5A5A5A5u);
  for (uint32_t i : lanes(n, order)) {
    mv[i] = mg_move_slot(T, src.vec(0, i), src.vec(3, i), src.vec(8, i), src.f(7, i), factor_sq);
    cls[i] = mv[i].cls;
    st[N_LIVE] += cls[i] != kMergeDead; st[N_BAD] += cls[i] == kMergeBad;
  }
  // k_merge_select: N_d from dst as it stood (dst is a copy, `out` is what is written)
  for (uint32_t i : lanes(n, order)) {
    if (cls[i] != kMergeAppend) continue;
    bool saturated;
    const uint32_t m = mg_select(mv[i].N, idx + (size_t)i * k, std::min(std::max(cnt[i], 0), k), k, cos_max,
                                 [&](uint32_t d) { return dst.vec(8, d); }, &saturated);
    if (m != kMergeNone) { cls[i] = kMergeMatched; match[i] = m; }
    st[N_MATCHED] += m != kMergeNone; st[N_SATURATED] += saturated;
  }
  // k_merge_count, the scan, k_merge_map
  std::vector<unsigned long long> keys;
  std::vector<uint32_t> vals;
  uint32_t rank = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (cls[i] == kMergeAppend) match[i] = old_size + rank++;
    else if (cls[i] == kMergeMatched) { keys.push_back(match[i]); vals.push_back(i); }
    else match[i] = kMergeNone;
  }
  st[N_APPENDED] = rank;
  *out = dst;
  *s2d = match;
  if ((unsigned long long)old_size + rank > max_surfels) return 1;
  // grow the rows
  Map o;
  o.n = old_size + rank;
  o.rows.assign((size_t)25 * o.n, 0.0f);
  for (int r = 0; r < 25; ++r)
    for (uint32_t i = 0; i < old_size; ++i) o.f(r, i) = dst.f(r, i);
  // k_merge_append
  for (uint32_t i : lanes(n, order)) {
    if (cls[i] != kMergeAppend) continue;
    const uint32_t d = match[i];
    o.set_vec(0, d, mv[i].P); o.set_vec(3, d, mv[i].S); o.set_vec(8, d, mv[i].N);
    o.f(6, d) = src.f(6, i); o.f(7, d) = src.f(7, i);
    o.set_u(17, d, frame); o.set_u(18, d, frame); o.set_u(24, d, src.u(24, i));
    for (int e = 0; e < 4; ++e)
      o.set_u(19 + e, d, mg_link(src.u(19 + e, i), n, [&](uint32_t l) { return cls[l]; }, [&](uint32_t l) { return match[l]; }, &st[N_DROPPED]));
  }
  // the stable sort of the pairs, k_merge_blend: the head of a run walks it
  if (mode == 1) {
    std::vector<uint32_t> perm(keys.size());
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    const uint32_t np = (uint32_t)perm.size();
    for (uint32_t j : lanes(np, order)) {
      const unsigned long long key = keys[perm[j]];
      if (j != 0 && keys[perm[j - 1]] == key) continue;
      ++st[N_BLENDED];
      const uint32_t d = (uint32_t)key;
      MgBlend b{dst.vec(0, d), dst.vec(3, d), dst.vec(8, d), dst.f(6, d), dst.f(7, d)};
      for (uint32_t e = j; e < np && keys[perm[e]] == key; ++e) {
        const uint32_t i = vals[perm[e]];
        mg_blend_step(b, mv[i].P, mv[i].S, mv[i].N, src.f(6, i), src.f(7, i), cap);
      }
      o.set_vec(0, d, b.P); o.set_vec(3, d, b.S); o.set_vec(8, d, b.N);
      o.f(6, d) = b.c; o.f(7, d) = b.r;
      o.set_u(18, d, frame);
    }
  }
  st[NEW_SIZE] = o.n;
  *out = o;
  return 0;
}

// case file: u32 n_dst, n_src, k, mode, frame, max_surfels; f32 factor_sq, cos_max, cap, T[12]; f32 dst[25][n_dst], src[25][n_src];
//            i32 cnt[n_src]; u32 idx[n_src][k]
// result file, per order (0 forwards, 1 backwards): i32 rc; u32 stats[WORDS]; u32 n_out; f32 rows[25][n_out]; u32 s2d[n_src]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[6];
  float prm[15];
  if (!get(f, head, 6) || !get(f, prm, 15)) return 2;
  Map dst, src;
  dst.n = head[0]; src.n = head[1];
  dst.rows.resize((size_t)25 * dst.n); src.rows.resize((size_t)25 * src.n);
  std::vector<int32_t> cnt(src.n);
  std::vector<uint32_t> idx((size_t)src.n * head[2]);
  if (!get(f, dst.rows.data(), dst.rows.size()) || !get(f, src.rows.data(), src.rows.size()) || !get(f, cnt.data(), cnt.size()) ||
      !get(f, idx.data(), idx.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order = 0; order < 2; ++order) {
    Map out;
    std::vector<uint32_t> s2d;
    uint32_t st[WORDS];
    const int32_t rc = host_merge(dst, src, prm + 3, prm[0], prm[1], prm[2], (int)head[2], (int)head[3], head[4], head[5], cnt.data(), idx.data(),
                                  order, &out, &s2d, st);
    put(o, &rc, 1); put(o, st, (size_t)WORDS); put(o, &out.n, 1); put(o, out.rows.data(), out.rows.size()); put(o, s2d.data(), s2d.size());
  }
  fclose(o);
  return 0;
}
'''

STATS = ("n_src_slots", "n_src_live", "n_bad", "n_matched", "n_appended", "n_blended_dst", "n_saturated", "links_dropped", "old_size", "new_size")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("merge_host")
    return ray_host.build(d, PROGRAM, [], "merge_host"), ray_host.build(d, PROGRAM, ray_host.SANITIZE, "merge_host_san")


@pytest.fixture(scope="module")
def modelled():
    """Every (case, mode) with the model's answer, computed once."""
    out = []
    for c in mc.cases():
        for mode in (mr.KEEP_DST, mr.BLEND):
            out.append((c, mode, mr.merge_model(c.dst, c.src, c.T, c.params(mode), c.max_surfels)))
    return out


def run_host(exe, work, c, mode, lists):
    p = c.params(mode)
    k, n = int(p["k"]), c.src.shape[1]
    cnt = np.array([len(l) for l in lists], np.int32)
    idx = np.full((n, k), 0xDEADBEEF, np.uint32)
    for i, l in enumerate(lists):
        idx[i, :len(l)] = l
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([c.dst.shape[1], n, k, mode, p["frame_index"], c.max_surfels], np.uint32).tobytes())
        f.write(np.array([p["radius_factor_squared"], mr.cos_max_of(p["max_normal_angle_deg"]), p["confidence_cap"]], np.float32).tobytes())
        f.write(c.T.astype(np.float32).tobytes() + np.ascontiguousarray(c.dst, np.float32).tobytes() + np.ascontiguousarray(c.src, np.float32).tobytes())
        f.write(cnt.tobytes() + idx.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (c.name, r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint32), 0, []
    for order in range(2):
        rc = int(raw[at:at + 1].view(np.int32)[0])
        st = dict(zip(STATS, (int(v) for v in raw[at + 1:at + 11])))
        n_out = int(raw[at + 11])
        at += 12
        rows = raw[at:at + 25 * n_out].copy().view(np.float32).reshape(25, n_out)
        at += 25 * n_out
        s2d = raw[at:at + n].copy()
        at += n
        runs.append((order, rc, st, rows, s2d))
    assert at == raw.size
    return runs


def check(c, mode, model, runs):
    rows, s2d, st, ex = model
    for order, rc, hst, hrows, hs2d in runs:
        what = (c.name, mode, order)
        assert rc == (1 if ex["failed"] else 0), what
        assert hst == st, (what, hst, st)
        assert hrows.shape == rows.shape and np.array_equal(mr.comparable(hrows), mr.comparable(rows)), what
        if not ex["failed"]:
            assert np.array_equal(hs2d, s2d), what


def test_host_walk_equals_the_model(programs, modelled, tmp_path):
    for c, mode, model in modelled:
        check(c, mode, model, run_host(programs[0], tmp_path, c, mode, model[3]["lists"]))


def test_host_walk_under_the_sanitizers(programs, modelled, tmp_path):
    for c, mode, model in modelled:
        check(c, mode, model, run_host(programs[1], tmp_path, c, mode, model[3]["lists"]))


def test_header_compiles_alone_for_the_host(tmp_path):
    ray_host.build(tmp_path, '#define SMX_MERGE_HOST_ONLY 1\n#include "smx_merge.hpp"\n'
                   'int main() { return smx::mg_live(-1.0f) ? 1 : 0; }\n', ["-Werror"], "merge_alone")
