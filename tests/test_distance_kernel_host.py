"""The arithmetic, the cell functions and the table operations of smx_distance.hip without a GPU: smx_distance.hpp holds step 1's
classes, the closest point of step 3, the key, the sign, the cell of a coordinate, a triangle's box and entry count, insert and
look-up in the open-addressing cell table (templated on how an entry is read, claimed and bumped) and the query of one point as
inline functions.  This test compiles them for the host with the project's -ffp-contract=off into a stand-alone program (its
own main: it reads a case file and writes a result file) and walks mark, index, query and stats one "lane" after the other --
forwards, backwards and in a seeded shuffled order -- with plain words behind the table operations.  Every output byte and
every statistic has to equal the brute-force model of tests/distance_ref.py, as on the device.  The same program is also
built with -fsanitize=address,undefined and run directly."""
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import ray_host

PROGRAM = r'''
#define SMX_DISTANCE_HOST_ONLY 1
#include "smx_distance.hpp"
''' + ray_host.GRID_BUILD + r'''
enum { N_IN = 0, N_NOT_LIVE, N_REPEATED, N_RANGE, N_POINTS, N_BAD, N_MATCHED, MAX_BITS, HIST, N_WIDE = HIST + 32, N_ENTRIES, N_CELLS, CELL, WORDS };

// Returns 0, or -1 (an index out of range).
static int host_distance(uint32_t n, const float* S, const uint32_t* tri, uint32_t n_in, const float* pts, uint32_t n_points, float max_distance,
                         float cell_size, int is_signed, uint32_t order, uint32_t* nearest, float* distance, float* closest, uint32_t* stats) {
  for (int k = 0; k < WORDS; ++k) stats[k] = 0;
  stats[N_IN] = n_in; stats[N_POINTS] = n_points;
  auto pos = [&](uint32_t i) { return TgVec{S[4 * (size_t)i], S[4 * (size_t)i + 1], S[4 * (size_t)i + 2]}; };
  auto point = [&](uint32_t p) { return TgVec{pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2]}; };
  // mark and index: the exact boxes, c >= 1.125 max_distance
  HostGrid g;
  if (host_tg_build(n, S, tri, n_in, cell_size, order, [&](float given) { return dist_cell_size(given, max_distance); }, tg_box, &g) != 0) return -1;
  const float cell = g.cell;
  const uint32_t mask = g.mask;
  const Tab tab = g.tab();
  const std::vector<uint32_t>& wide_t = g.wide_t;
  stats[N_NOT_LIVE] = g.n_not_live; stats[N_REPEATED] = g.n_repeated; stats[N_RANGE] = g.n_range;
  stats[N_WIDE] = (uint32_t)wide_t.size(); stats[N_ENTRIES] = g.E; stats[N_CELLS] = g.n_cells;
  __builtin_memcpy(&stats[CELL], &cell, 4);
  // k_dist_query, k_dist_stats
  const float max2 = max_distance * max_distance;
  const Recs cell_recs{g.recs.data()}, wrecs{g.wide_recs.data()};
  for (uint32_t p : lanes(n_points, order)) {
    const TgVec P = point(p);
    unsigned long long key = kTgNone;
    if (tg_point_ok(P)) key = dist_query(tab, mask, cell_recs, wrecs, (uint32_t)wide_t.size(), P, cell, max2);
    else ++stats[N_BAD];
    uint32_t t = 0xFFFFFFFFu;
    float d = INFINITY;
    TgVec Q{NAN, NAN, NAN};
    if (key != kTgNone) {
      t = (uint32_t)key;
      const TgVec A = pos(tri[3 * (size_t)t]), B = pos(tri[3 * (size_t)t + 1]), C = pos(tri[3 * (size_t)t + 2]);
      uint32_t region;
      Q = dist_closest(P, A, B, C, &region);
      d = sqrtf(tg_key_float(key));
      ++stats[N_MATCHED];
      ++stats[HIST + dist_bin(d, max_distance)];
      stats[MAX_BITS] = std::max(stats[MAX_BITS], (uint32_t)(key >> 32));
      if (is_signed && dist_negative(P, Q, A, B, C)) d = -d;
    }
    nearest[p] = t; distance[p] = d;
    closest[3 * (size_t)p] = Q.x; closest[3 * (size_t)p + 1] = Q.y; closest[3 * (size_t)p + 2] = Q.z;
  }
  return 0;
}

// case file: u32 n, n_in, n_points, signed, n_orders; f32 max_distance, cell_size; u32 orders[]; f32 S[n][4]; u32 tri[n_in][3];
//            f32 points[n_points][3]
// result file, per order: i32 rc; u32 stats[WORDS]; u32 nearest[n_points]; f32 distance[n_points]; f32 closest[n_points][3]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[5];
  float prm[2];
  if (!get(f, head, 5) || !get(f, prm, 2)) return 2;
  std::vector<uint32_t> orders(head[4]), tri(3 * (size_t)head[1]);
  std::vector<float> S(4 * (size_t)head[0]), pts(3 * (size_t)head[2]);
  if (!get(f, orders.data(), orders.size()) || !get(f, S.data(), S.size()) || !get(f, tri.data(), tri.size()) || !get(f, pts.data(), pts.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order : orders) {
    std::vector<uint32_t> nearest(head[2], 0xA5A5A5A5u);
    std::vector<float> distance(head[2], 0.0f), closest(3 * (size_t)head[2], 0.0f);
    uint32_t stats[WORDS];
    const int32_t rc = host_distance(head[0], S.data(), tri.data(), head[1], pts.data(), head[2], prm[0], prm[1], (int)head[3], order,
                                     nearest.data(), distance.data(), closest.data(), stats);
    put(o, &rc, 1); put(o, stats, (size_t)WORDS);
    put(o, nearest.data(), nearest.size()); put(o, distance.data(), distance.size()); put(o, closest.data(), closest.size());
  }
  fclose(o);
  return 0;
}
'''

ORDERS = (0, 1, 7)      # forwards, backwards, shuffled with seed 7
WORDS = 8 + 32 + 4


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("distance_host")


@pytest.fixture(scope="module")
def program(work):
    return ray_host.build(work, PROGRAM, [], "distance_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return ray_host.build(work, PROGRAM, ray_host.SANITIZE, "distance_host_san")


def host_distance(exe, work, pos, r2, tri, points, max_distance, cell_size=0.0, signed=False):
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3], S[:, 3] = pos, r2
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    P = pts.shape[0]
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, t.shape[0], P, int(signed), len(ORDERS)], np.uint32).tobytes())
        f.write(np.array([max_distance, cell_size], np.float32).tobytes())
        f.write(np.array(ORDERS, np.uint32).tobytes() + S.tobytes() + t.tobytes() + pts.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint32), 0, []
    for _ in ORDERS:
        rc = int(raw[at:at + 1].view(np.int32)[0])
        w = raw[at + 1:at + 1 + WORDS]
        st = dict(zip(dr.STAT_NAMES, (int(v) for v in w[:8])))
        st["histogram"] = [int(v) for v in w[8:40]]
        st.update(n_wide=int(w[40]), n_entries=int(w[41]), n_cells=int(w[42]), cell_size_used=float(w[43:44].view(np.float32)[0]))
        at += 1 + WORDS
        nearest, distance = raw[at:at + P].copy(), raw[at + P:at + 2 * P].copy().view(np.float32)
        closest = raw[at + 2 * P:at + 5 * P].copy().view(np.float32).reshape(-1, 3)
        at += 5 * P
        runs.append((rc, nearest, distance, closest, st))
    assert at == raw.size
    return runs


def _compare(exe, work, world, model, points, what, max_distance, cell_size, signed):
    pos, nrm, r2, tri, _ = world
    wn, wd, wc, wst = dr.answer(model, max_distance, signed)
    wst.pop("max_distance")
    if cell_size > 0:
        wst.update(dr.structure(pos, r2, tri, cell_size, max_distance))
    differing = 0
    for order, (rc, nearest, distance, closest, st) in zip(ORDERS, host_distance(exe, work, pos, r2, tri, points, max_distance, cell_size, signed)):
        assert rc == 0
        used = st.pop("cell_size_used")
        if cell_size > 0:
            assert used == float(dr.cell_used(cell_size, max_distance))
        else:
            assert used >= float(dr.cell_used(0.0, max_distance))
            for k in ("n_wide", "n_entries", "n_cells"):
                st.pop(k)
        assert st == wst, (what, order, st, wst)
        differing += sum(int(a.tobytes() != b.tobytes()) for a, b in ((nearest, wn), (distance, wd), (closest, wc)))
    print("%s max %.3f cell %g signed %d: %d matched, %d differing arrays" % (what, max_distance, cell_size, signed, wst["n_matched"], differing))
    assert differing == 0, what


CELLS = lambda m: (0.0, float(dr.MARGIN * dr.F(m)), 1e-3, 100.0)      # noqa: E731


def test_every_point_set_on_the_host(program, work):
    world = dr.world()
    for k, (name, pts) in enumerate(dr.point_sets().items()):
        m = dr.model_of(name)
        for j, md in enumerate(dr.MAX_DISTANCES):
            # every cell size for two of the sets, one in rotation for the others (1e-3 at 0.002 puts nearly all of R on the wide list)
            cells = CELLS(md) if name in ("vertices 0 / 1 / 5 mm", "around the hand-made triangles") else (CELLS(md)[(k + j) % 4],)
            for cs in cells:
                _compare(program, work, world, m, pts, name, md, cs, bool((k + j) & 1))


def test_an_index_out_of_range_and_empty_inputs_on_the_host(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    pts = dr.point_sets()["NaN, inf and 65 m"]
    bad = tri.copy()
    bad[77, 2] = pos.shape[0]
    assert [r[0] for r in host_distance(program, work, pos, r2, bad, pts, 0.02)] == [-1, -1, -1]
    none = np.zeros((0, 3), np.uint32)
    for rc, nearest, distance, closest, st in host_distance(program, work, pos, r2, none, pts, 0.02):
        assert rc == 0 and np.all(nearest == dr.INVALID) and np.all(np.isinf(distance)) and np.all(np.isnan(closest))
        assert st["n_matched"] == 0 and st["n_bad_points"] == 7 and st["n_entries"] == 0
    for rc, nearest, distance, closest, st in host_distance(program, work, pos, r2, tri, np.zeros((0, 3), np.float32), 0.02, 0.05):
        assert rc == 0 and nearest.size == 0 and st["n_points"] == 0 and st["n_entries"] == dr.structure(pos, r2, tri, 0.05, 0.02)["n_entries"]


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    world = dr.world()
    for name, md, cs in (("around the hand-made triangles", 0.5, 0.0), ("around the hand-made triangles", 0.02, 1e-3),
                         ("NaN, inf and 65 m", 0.002, 0.05), ("multiples of c", 0.02, float(dr.MARGIN * dr.F(0.02)))):
        _compare(sanitized, work, world, dr.model_of(name), dr.point_sets()[name], name + ", sanitized", md, cs, True)
