"""The lattice, a sample's share of a pose's score and the choice of the starts without a GPU: smx_global.hpp holds them as plain
inline functions, which the kernels and the glue of smx_global.hip call.  This test compiles the header for the host with the
project's -ffp-contract=off into a stand-alone program (its own main: it reads a case file and writes a result file) and holds
it to the model of tests/global_ref.py: the lattice byte for byte for k = 1 .. 3 with two anchors; every word of every pose's
score where the program is handed the query's answers (the model's brute-force association) and walks a pose's samples the way a
workgroup does, forwards and backwards; the order of the starts with and without ties.  The same program is also built with
-fsanitize=address,undefined and run directly."""
import subprocess

import numpy as np
import pytest

import global_ref as gr
import ray_host
import register_ref as rr

PROGRAM = r'''
#define SMX_GLOBAL_HOST_ONLY 1
#include <math.h>
#include <string.h>
#include "smx_global.hpp"
#include <cstdio>
#include <vector>
using namespace smx;

template <class T> static bool get(FILE* f, T* p, size_t count) { return count == 0 || fread(p, sizeof(T), count, f) == count; }
template <class T> static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

struct Score { unsigned long long cost; uint32_t n_ok, n_matched, n_rim, reserved; };

// case file: u32 n_lattices; per lattice u32 k, A; f64 centre[3], anchors[A][3]
//            u32 n_scores; per score u32 P, m, q_word, reject_rim, backwards; f32 moved[P m][3]; u32 t[P m]; f32 distance[P m];
//                          u32 byte[P m]; f32 A[P m][3], B[P m][3], C[P m][3]
//            u32 n_selects; per select u32 P, n_starts; u64 cost[P]
// result file: per lattice u32 count; f32 poses[count][12].  per score Score[P].  per select u32 M; u32 order[M]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  uint32_t n = 0;
  if (!get(f, &n, 1)) return 2;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t head[2];
    double centre[3];
    if (!get(f, head, 2) || !get(f, centre, 3)) return 2;
    std::vector<double> anchors(3 * (size_t)head[1]);
    if (!get(f, anchors.data(), anchors.size())) return 2;
    const uint32_t count = glob_lattice_rotations((int)head[0]) * head[1];
    std::vector<float> poses(12 * (size_t)count);
    glob_lattice((int)head[0], centre, anchors.data(), head[1], poses.data());
    put(o, &count, 1); put(o, poses.data(), poses.size());
  }
  if (!get(f, &n, 1)) return 2;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t head[5];
    if (!get(f, head, 5)) return 2;
    const uint32_t P = head[0], m = head[1], q_word = head[2];
    const bool rim = head[3] != 0, backwards = head[4] != 0;
    const size_t S = (size_t)P * m;
    std::vector<float> moved(3 * S), distance(S), A(3 * S), B(3 * S), C(3 * S);
    std::vector<uint32_t> t(S), byte(S);
    if (!get(f, moved.data(), 3 * S) || !get(f, t.data(), S) || !get(f, distance.data(), S) || !get(f, byte.data(), S) || !get(f, A.data(), 3 * S) ||
        !get(f, B.data(), 3 * S) || !get(f, C.data(), 3 * S)) return 2;
    std::vector<Score> out(P);
    for (uint32_t pose = 0; pose < P; ++pose) {
      // k_glob_score: 256 lanes, lane l visits the samples l, l + 256, ...; the lanes' words are added as integers
      unsigned long long cost = 0;
      uint32_t n_ok = 0, n_matched = 0, n_rim = 0;
      for (uint32_t l = 0; l < (uint32_t)kGlobBlock; ++l) {
        const uint32_t lane = backwards ? kGlobBlock - 1 - l : l;
        for (uint32_t j = lane; j < m; j += kGlobBlock) {
          const size_t s = (size_t)pose * m + j;
          const TgVec Pm{moved.at(3 * s), moved.at(3 * s + 1), moved.at(3 * s + 2)};
          const bool on_rim = rim && t.at(s) != 0xFFFFFFFFu &&
                              glob_on_rim(byte.at(s), Pm, TgVec{A[3 * s], A[3 * s + 1], A[3 * s + 2]}, TgVec{B[3 * s], B[3 * s + 1], B[3 * s + 2]},
                                          TgVec{C[3 * s], C[3 * s + 1], C[3 * s + 2]});
          glob_sample(Pm, t.at(s), distance.at(s), q_word, on_rim, cost, n_ok, n_matched, n_rim);
        }
      }
      out[pose] = Score{cost, n_ok, n_matched, n_rim, 0u};
    }
    put(o, out.data(), out.size());
  }
  if (!get(f, &n, 1)) return 2;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t head[2];
    if (!get(f, head, 2)) return 2;
    std::vector<unsigned long long> cost(head[0]);
    if (!get(f, cost.data(), cost.size())) return 2;
    uint32_t order[kGlobMaxStarts];
    const uint32_t M = glob_select([&](uint32_t j) { return cost.at(j); }, head[0], head[1], order);
    put(o, &M, 1); put(o, order, M);
  }
  fclose(f);
  fclose(o);
  return 0;
}
'''

LATTICES = [(k, np.array([0.3, -0.2, 0.7]), np.array([[1.0, 2.0, 3.0], [-0.5, 0.25, 0.125]])) for k in (1, 2, 3)]
LATTICES.append((2, np.array([1e-3, 17.25, -63.0]), np.array([[0.1, 0.2, 0.3]])))
SCORES = [("base set, k = 1 about its pose, stride 3", 0.02), ("base set, k = 1 about its pose, stride 3", 0.5), ("bracket, k = 2, stride 4", gr.BRACKET_BOUND),
          ("bracket, k = 2, stride 4, rim rejected", gr.BRACKET_BOUND), ("bracket, one pose", gr.BRACKET_BOUND)]


def _selects():
    rng = np.random.default_rng(3)
    ties = rng.integers(0, 5, 300).astype(np.uint64)                  # many equal costs: the index decides
    spread = rng.integers(0, 1 << 40, 1000).astype(np.uint64)
    return [(ties, 8), (ties, 64), (spread, 8), (spread[:5], 8), (spread[:1], 1), (np.sort(spread)[::-1].copy(), 64), (np.zeros(100, np.uint64), 64)]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("global_host")


def _run(exe, work):
    """The program on every lattice, score case (forwards and backwards) and selection: (lattices, scores, orders)."""
    case, res = work / "case.bin", work / "result.bin"
    score_inputs = []
    with open(case, "wb") as f:
        f.write(np.uint32(len(LATTICES)).tobytes())
        for k, c, a in LATTICES:
            f.write(np.array([k, a.shape[0]], np.uint32).tobytes() + c.astype(np.float64).tobytes() + a.astype(np.float64).tobytes())
        f.write(np.uint32(2 * len(SCORES)).tobytes())
        for name, q in SCORES:
            c = gr.cases()[name]
            pts = np.ascontiguousarray(c["points"], np.float32)
            S = pts[::c["stride"]]
            moved = np.concatenate([rr.move(T, S) for T in c["poses"]])
            a = gr.association(gr.mesh_of(c), moved, q, True)
            for backwards in (0, 1):
                f.write(np.array([c["poses"].shape[0], S.shape[0], gr.q_word(q), int(c["rim"]), backwards], np.uint32).tobytes())
                f.write(moved.tobytes() + a["t"].tobytes() + a["distance"].tobytes() + a["byte"].tobytes() + a["A"].tobytes() + a["B"].tobytes() + a["C"].tobytes())
                score_inputs.append((name, q, c["poses"].shape[0]))
        sel = _selects()
        f.write(np.uint32(len(sel)).tobytes())
        for cost, n_starts in sel:
            f.write(np.array([cost.size, n_starts], np.uint32).tobytes() + cost.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at = np.fromfile(res, np.uint8), 0
    lattices, scores, orders = [], [], []
    for _ in LATTICES:
        count = int(raw[at:at + 4].view(np.uint32)[0])
        lattices.append(raw[at + 4:at + 4 + 48 * count].view(np.float32).reshape(-1, 3, 4).copy())
        at += 4 + 48 * count
    for name, q, P in score_inputs:
        scores.append((name, q, raw[at:at + 24 * P].view(gr.SCORE_DTYPE).copy()))
        at += 24 * P
    for _ in sel:
        M = int(raw[at:at + 4].view(np.uint32)[0])
        orders.append(raw[at + 4:at + 4 + 4 * M].view(np.uint32).copy())
        at += 4 + 4 * M
    assert at == raw.size
    return lattices, scores, orders


def _check(exe, work):
    lattices, scores, orders = _run(exe, work)
    for (k, c, a), got in zip(LATTICES, lattices):
        want = gr.lattice(k, c, a)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (k, a.shape)
    for name, q, got in scores:
        want = gr.golden_case(name, q)
        for word in ("cost", "n_ok", "n_matched", "n_rim", "reserved"):
            assert np.array_equal(got[word], want[word]), (name, q, word, np.flatnonzero(got[word] != want[word])[:5])
    for (cost, n_starts), got in zip(_selects(), orders):
        assert np.array_equal(got.astype(np.int64), gr.select(cost, n_starts)), (cost.size, n_starts)
    return scores


def test_the_lattice_the_scores_and_the_choice_on_the_host(work):
    scores = _check(ray_host.build(work, PROGRAM, [], "global_host"), work)
    rim = [s for name, _, s in scores if "rim" in name]
    assert rim and all(int(s["n_rim"].sum()) > 0 for s in rim), "the rim case rejects matches"
    world = [s for name, _, s in scores if name.startswith("base set")]
    assert all(np.all(s["n_ok"] < 86) and np.any(s["n_matched"] < s["n_ok"]) for s in world), "BAD and unmatched samples are met"


def test_the_program_under_the_sanitizers(work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    _check(ray_host.build(work, PROGRAM, ray_host.SANITIZE, "global_host_san"), work)
