"""The arithmetic of smx_sample.hip without a GPU: part 1 of smx_sample.hpp holds the weight of a triangle, the saturating sum, the
random words, the stratum, the search in the two-level prefix, the point, the normal and the fixed-point words of the comparison
as inline functions.  This test compiles them for the host with the project's -ffp-contract=off into a stand-alone program (its
own main: it reads a case file and writes a result file) and walks weights, scan, draw and sums one "lane" after the other --
forwards, backwards and in a seeded shuffled order; the scan of the blocks as a left fold and as a tree, which have to agree.
Every output byte and every statistic has to equal the brute-force model of tests/sample_ref.py, as on the device.  The same
program is also built with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import numpy as np
import pytest

import decimate_ref as dec
import distance_ref as dr
import sample_ref as sr
from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

PROGRAM = r'''
#define SMX_SAMPLE_HOST_ONLY 1
#include "smx_sample.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
using namespace smx;
typedef unsigned long long u64;

static std::vector<uint32_t> lanes(uint32_t count, uint32_t order) {
  std::vector<uint32_t> l(count);
  std::iota(l.begin(), l.end(), 0u);
  if (order == 1) std::reverse(l.begin(), l.end());
  if (order > 1) { std::mt19937 g(order); std::shuffle(l.begin(), l.end(), g); }
  return l;
}
// the saturated sum of v[lo, hi) as a balanced tree
static u64 tree(const std::vector<u64>& v, size_t lo, size_t hi) {
  if (hi <= lo) return 0;
  if (hi - lo == 1) return smp_sat_add(0, v[lo]);
  const size_t mid = lo + (hi - lo) / 2;
  return smp_sat_add(tree(v, lo, mid), tree(v, mid, hi));
}
struct Words { const u64* p; u64 operator()(uint32_t i) const { return p[i]; } };

enum { N_IN = 0, N_NOT_LIVE, N_REPEATED, N_RANGE, N_ZERO, N_SAMPLES, N_NONE, N_HIT, TOTAL, STRIDE, WORDS };

// Returns 0, -1 (an index out of range), -2 (W == 2^62) or -3 (the fold and the tree disagree).
static int host_sample(uint32_t n, const float* S4, const uint32_t* tri, uint32_t n_in, uint32_t n_samples, uint32_t seed, uint32_t order,
                       float* points, uint32_t* out_tri, float* bary, float* normals, u64* stats) {
  for (int k = 0; k < WORDS; ++k) stats[k] = 0;
  stats[N_IN] = n_in; stats[N_SAMPLES] = n_samples;
  auto pos = [&](uint32_t i) { return TgVec{S4[4 * (size_t)i], S4[4 * (size_t)i + 1], S4[4 * (size_t)i + 2]}; };
  auto live = [&](uint32_t i) { return dec_live(S4[4 * (size_t)i], S4[4 * (size_t)i + 1], S4[4 * (size_t)i + 2], S4[4 * (size_t)i + 3]); };
  // k_smp_weights: q per lane in any order, then the sums inside each block and the blocks' weights
  std::vector<u64> q(n_in, 0);
  for (uint32_t t : lanes(n_in, order)) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= n || i1 >= n || i2 >= n) return -1;
    const TgVec a = pos(i0), b = pos(i1), c = pos(i2);
    const uint32_t cls = tg_classify(i0, i1, i2, live(i0), live(i1), live(i2), a, b, c);
    if (cls == kTgDropNotLive) ++stats[N_NOT_LIVE];
    if (cls == kTgDropRepeated) ++stats[N_REPEATED];
    if (cls == kTgDropRange) ++stats[N_RANGE];
    if (cls == kTgInR) { q[t] = smp_weight(smp_face(a, b, c).a); if (q[t] == 0) ++stats[N_ZERO]; }
  }
  const uint32_t nb = (n_in + kSmpBlock - 1) / kSmpBlock;
  std::vector<u64> incl(n_in, 0), sums(nb, 0), off(nb, 0);
  for (uint32_t t = 0; t < n_in; ++t) {
    incl[t] = (t % kSmpBlock ? incl[t - 1] : 0) + q[t];
    sums[t / kSmpBlock] = incl[t];
  }
  // k_smp_scan: as a left fold and as a tree
  u64 W = 0;
  for (uint32_t b = 0; b < nb; ++b) { off[b] = W; W = smp_sat_add(W, sums[b]); }
  if (W != tree(sums, 0, nb)) return -3;
  for (uint32_t b = 0; b < nb; ++b) if (off[b] != tree(sums, 0, b)) return -3;
  if (W >= kSmpSat) return -2;
  stats[TOTAL] = W;
  const u64 S = n_samples ? W / n_samples : 0;
  stats[STRIDE] = S;
  // k_smp_draw
  const bool none = W < n_samples;
  stats[N_NONE] = none ? n_samples : 0;
  const Words o{off.data()}, in{incl.data()};
  for (uint32_t k : lanes(n_samples, order)) {
    if (none) {
      out_tri[k] = kSmpNone;
      for (int c = 0; c < 3; ++c) points[3 * (size_t)k + c] = normals[3 * (size_t)k + c] = NAN;
      bary[2 * (size_t)k] = bary[2 * (size_t)k + 1] = NAN;
      continue;
    }
    const uint32_t t = smp_find(o, nb, in, n_in, smp_stratum(k, S, smp_rand(k, 0, seed)));
    const uint32_t before = k == 0 ? kSmpNone : smp_find(o, nb, in, n_in, smp_stratum(k - 1, S, smp_rand(k - 1, 0, seed)));
    if (before != t) ++stats[N_HIT];
    const TgVec A = pos(tri[3 * (size_t)t]), B = pos(tri[3 * (size_t)t + 1]), C = pos(tri[3 * (size_t)t + 2]);
    const SmpFace f = smp_face(A, B, C);
    float v, w;
    smp_bary(smp_rand(k, 1, seed), smp_rand(k, 2, seed), &v, &w);
    const TgVec P = smp_point(A, f, v, w), N = smp_normal(f);
    out_tri[k] = t;
    points[3 * (size_t)k] = P.x; points[3 * (size_t)k + 1] = P.y; points[3 * (size_t)k + 2] = P.z;
    normals[3 * (size_t)k] = N.x; normals[3 * (size_t)k + 1] = N.y; normals[3 * (size_t)k + 2] = N.z;
    bary[2 * (size_t)k] = v; bary[2 * (size_t)k + 1] = w;
  }
  return 0;
}

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

// case file: u32 n, n_in, n_samples, seed, n_orders; u32 orders[]; f32 S[n][4]; u32 tri[n_in][3]; u32 nearest[n_samples];
//            f32 distance[n_samples]  (the answers of a distance call for the samples, for the three sums)
// result file, per order: i32 rc; u32 pad; u64 stats[WORDS]; u64 sums[3]; f32 points[n_samples][3]; u32 tri[n_samples];
//            f32 bary[n_samples][2]; f32 normals[n_samples][3]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[5];
  if (!get(f, head, 5)) return 2;
  const uint32_t ns = head[2];
  std::vector<uint32_t> orders(head[4]), tri(3 * (size_t)head[1]), nearest(ns);
  std::vector<float> S(4 * (size_t)head[0]), distance(ns);
  if (!get(f, orders.data(), orders.size()) || !get(f, S.data(), S.size()) || !get(f, tri.data(), tri.size()) ||
      !get(f, nearest.data(), nearest.size()) || !get(f, distance.data(), distance.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order : orders) {
    std::vector<float> points(3 * (size_t)ns, 0.0f), bary(2 * (size_t)ns, 0.0f), normals(3 * (size_t)ns, 0.0f);
    std::vector<uint32_t> out_tri(ns, 0xA5A5A5A5u);
    u64 stats[WORDS], sums[3] = {0, 0, 0};
    const int32_t rc[2] = {host_sample(head[0], S.data(), tri.data(), head[1], ns, head[3], order, points.data(), out_tri.data(), bary.data(),
                                       normals.data(), stats), 0};
    for (uint32_t k : lanes(ns, order)) {                    // k_cmp_sums
      if (nearest[k] == 0xFFFFFFFFu) continue;
      const uint32_t dq = cmp_dq(distance[k]);
      u64 lo, hi;
      cmp_square(dq, &lo, &hi);
      sums[0] += dq; sums[1] += lo; sums[2] += hi;
    }
    put(o, rc, 2); put(o, stats, (size_t)WORDS); put(o, sums, 3);
    put(o, points.data(), points.size()); put(o, out_tri.data(), out_tri.size()); put(o, bary.data(), bary.size());
    put(o, normals.data(), normals.size());
  }
  fclose(o);
  return 0;
}
'''

ORDERS = (0, 1, 7)      # forwards, backwards, shuffled with seed 7
WORDS = 10


def _build(d, flags, name):
    src = d / "sample_host.cpp"
    src.write_text(PROGRAM)
    exe = d / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-I", SRC, "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("sample_host")


@pytest.fixture(scope="module")
def program(work):
    return _build(work, [], "sample_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return _build(work, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "sample_host_san")


def host_sample(exe, work, pos, r2, tri, n_samples, seed, nearest=None, distance=None):
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3], S[:, 3] = pos, r2
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    nearest = np.full(n_samples, sr.NONE, np.uint32) if nearest is None else np.ascontiguousarray(nearest, np.uint32)
    distance = np.full(n_samples, np.inf, np.float32) if distance is None else np.ascontiguousarray(distance, np.float32)
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, t.shape[0], n_samples, seed, len(ORDERS)], np.uint32).tobytes())
        f.write(np.array(ORDERS, np.uint32).tobytes() + S.tobytes() + t.tobytes() + nearest.tobytes() + distance.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, runs, P = np.fromfile(res, np.uint32), 0, [], n_samples
    for _ in ORDERS:
        rc = int(raw[at:at + 1].view(np.int32)[0])
        words = raw[at + 2:at + 2 + 2 * (WORDS + 3)].copy().view(np.uint64)
        st = dict(zip(sr.SAMPLE_STAT_NAMES, (int(v) for v in words[:WORDS])))
        at += 2 + 2 * (WORDS + 3)
        out = dict(rc=rc, stats=st, sums=tuple(int(v) for v in words[WORDS:]),
                   points=raw[at:at + 3 * P].copy().view(np.float32).reshape(-1, 3), tri=raw[at + 3 * P:at + 4 * P].copy(),
                   bary=raw[at + 4 * P:at + 6 * P].copy().view(np.float32).reshape(-1, 2),
                   normals=raw[at + 6 * P:at + 9 * P].copy().view(np.float32).reshape(-1, 3))
        at += 9 * P
        runs.append(out)
    assert at == raw.size
    return runs


def _compare(exe, work, pos, r2, tri, n_samples, seed, what, nearest=None, distance=None, sums=None):
    want = sr.sample(pos, r2, tri, n_samples, seed)
    for order, got in zip(ORDERS, host_sample(exe, work, pos, r2, tri, n_samples, seed, nearest, distance)):
        assert got["rc"] == 0 and got["stats"] == want["stats"], (what, order, got["stats"], want["stats"])
        for name in ("points", "tri", "bary", "normals"):
            assert got[name].tobytes() == want[name].tobytes(), (what, order, name)
        if sums is not None:
            assert got["sums"] == sums, (what, order)
    return want


big_map = sr.big_map


def test_the_world_on_the_host(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097):
        for seed in (0, 0xFFFFFFFF):
            want = _compare(program, work, pos, r2, tri, n, seed, "world %d %d" % (n, seed))
            assert want["stats"]["n_none"] == 0


def test_block_edges_and_64_bit_weights_on_the_host(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    for n_in in (0, 1, 255, 256, 257, 513):
        _compare(program, work, pos, r2, tri[:n_in], 300, 3, "n_in %d" % n_in)
    bp, br, bt = big_map()
    for n in (1, 7, 4096):
        want = _compare(program, work, bp, br, bt, n, 5, "big %d" % n)
        assert want["stats"]["stride"] >> 32 != 0 and want["stats"]["n_none"] == 0
    # W < n_samples: every sample is "none"; W == 0 with collinear triangles only
    want = _compare(program, work, bp, br, bt[[0, 2]], 1000000, 0, "tiny")
    assert want["stats"]["n_none"] == 1000000 and 0 < want["stats"]["total_weight"] < 1000000
    line = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [3.0, 3.0, 0.0]])
    want = _compare(program, work, line, np.full(4, 0.01), np.array([[0, 1, 2], [1, 2, 3]], np.uint32), 10, 0, "collinear")
    assert want["stats"]["total_weight"] == 0 and want["stats"]["n_zero_weight"] == 2 and want["stats"]["n_none"] == 10


def test_saturation_and_an_index_out_of_range_on_the_host(program, work):
    bp, br, bt = big_map()
    # the largest triangle the range allows has q = 2^44.79: 262 144 of them sum to 2^62.79 (refused), 131 072 to 2^61.79
    many = np.tile(bt[1:2], (262144, 1))
    assert [r["rc"] for r in host_sample(program, work, bp, br, many, 10, 0)] == [-2, -2, -2]
    with pytest.raises(ValueError):
        sr.sample(bp, br, many, 10, 0)
    for count in (131072, 32768):
        want = _compare(program, work, bp, br, many[:count], 1000, 9, "%d large triangles" % count)
        assert want["stats"]["total_weight"] > 1 << 59
    bad = bt.copy()
    bad[2, 1] = 9
    assert [r["rc"] for r in host_sample(program, work, bp, br, bad, 10, 0)] == [-1, -1, -1]


def test_the_three_sums_on_the_host(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    coarse = dec.decimate(pos, r2, tri, 0.1)[0]
    side = sr.compare_side(pos, r2, coarse, tri, 0.02, 1500, 4)
    assert 0 < side["distance"]["n_matched"] < 1500          # (some samples have no match: they add nothing)
    _compare(program, work, pos, r2, coarse, 1500, 4, "sums", side["_"]["nearest"], side["_"]["distance"],
             (side["sum_d"], side["sum_sq_lo"], side["sum_sq_hi"]))
    # the largest words: every distance 16 m
    full = np.full(1500, 16.0, np.float32)
    got = host_sample(program, work, pos, r2, coarse, 1500, 4, np.zeros(1500, np.uint32), full)[0]
    assert got["sums"] == (1500 << 24, 0, 1500 << 16)


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    pos, nrm, r2, tri, _ = dr.world()
    for n, seed in ((257, 0), (4097, 0xFFFFFFFF)):
        _compare(sanitized, work, pos, r2, tri, n, seed, "world, sanitized")
    _compare(sanitized, work, pos, r2, tri[:513], 300, 3, "513, sanitized")
    bp, br, bt = big_map()
    _compare(sanitized, work, bp, br, bt, 4096, 5, "big, sanitized")
    _compare(sanitized, work, bp, br, bt[[0, 2]], 1000, 0, "tiny, sanitized")
    assert [r["rc"] for r in host_sample(sanitized, work, bp, br, np.tile(bt[1:2], (262144, 1)), 10, 0)] == [-2, -2, -2]
