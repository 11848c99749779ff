"""The first-record rule and the winner-from-record read of smx_distscene without a GPU: smx_distscene.hpp holds them as plain
inline functions beside the distance arithmetic of smx_distance.hpp.  This test compiles them for the host with the project's
-ffp-contract=off into a stand-alone program (its own main: it reads a case file and writes a result file).  The program
walks the build (mark, index), then the first phase one record after the other, OVERWRITES the map array with NaN and the
triangle array with 0xFFFFFFFF, and only then queries: at every max_distance the scene's bound allows, every pass forwards,
backwards and in a seeded shuffled order.  Every output byte and every statistic has to equal the brute-force model of
tests/distance_ref.py, and first_rec the rule of tests/distscene_ref.py.  The same program is also built with
-fsanitize=address,undefined and run directly."""
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import distscene_ref as sr
import ray_host

PROGRAM = r'''
#define SMX_DISTSCENE_HOST_ONLY 1
#include "smx_distscene.hpp"
''' + ray_host.GRID_BUILD + r'''
enum { N_IN = 0, N_NOT_LIVE, N_REPEATED, N_RANGE, N_POINTS, N_BAD, N_MATCHED, MAX_BITS, HIST, N_WIDE = HIST + 32, N_ENTRIES, N_CELLS, CELL, WORDS };

// What a scene keeps: the grid, first_rec, the bound.  Nothing of the map, nothing of the triangle array.
struct HostScene {
  HostGrid g;
  std::vector<uint32_t> first_rec;
  uint32_t n_in = 0;
  float max_distance = 0.0f;
};

// smx_recon_build_distscene a lane at a time.  Returns 0, or -1 (an index out of range).
static int host_build(uint32_t n, const float* S, const uint32_t* tri, uint32_t n_in, float max_distance, float cell_size, uint32_t order,
                      HostScene* sc) {
  if (host_tg_build(n, S, tri, n_in, cell_size, order, [&](float given) { return dist_cell_size(given, max_distance); }, tg_box, &sc->g) != 0) return -1;
  sc->n_in = n_in; sc->max_distance = max_distance;
  // k_dscene_first: a lane per record, the cell records first, then the wide list
  const uint32_t E = sc->g.E, Wd = (uint32_t)sc->g.wide_t.size();
  sc->first_rec.assign(n_in, kDsceneNoRec);
  for (uint32_t j : lanes(E + Wd, order)) {
    const bool wide = j >= E;
    const uint32_t position = wide ? j - E : j;
    const uint32_t t = wide ? sc->g.wide_recs[position].t : sc->g.recs[position].t;
    sc->first_rec.at(t) = dscene_first_min(sc->first_rec.at(t), dscene_first_word(position, wide));
  }
  return 0;
}

// smx_distscene_query a lane at a time: reads the scene and the points, nothing else.
static void host_query(HostScene& sc, const float* pts, uint32_t n_points, float q, int is_signed, uint32_t order, uint32_t* nearest,
                       float* distance, float* closest, uint32_t* stats) {
  for (int k = 0; k < WORDS; ++k) stats[k] = 0;
  const HostGrid& g = sc.g;
  stats[N_IN] = sc.n_in; stats[N_POINTS] = n_points;
  stats[N_NOT_LIVE] = g.n_not_live; stats[N_REPEATED] = g.n_repeated; stats[N_RANGE] = g.n_range;
  stats[N_WIDE] = (uint32_t)g.wide_t.size(); stats[N_ENTRIES] = g.E; stats[N_CELLS] = g.n_cells;
  __builtin_memcpy(&stats[CELL], &g.cell, 4);
  const Tab tab = sc.g.tab();
  const Recs cell_recs{g.recs.data()}, wrecs{g.wide_recs.data()};
  const float max2 = q * q;
  for (uint32_t p : lanes(n_points, order)) {
    const TgVec P{pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2]};
    unsigned long long key = kTgNone;
    if (tg_point_ok(P)) key = dist_query(tab, g.mask, cell_recs, wrecs, (uint32_t)g.wide_t.size(), P, g.cell, max2);
    else ++stats[N_BAD];
    uint32_t t = 0xFFFFFFFFu;
    float d = INFINITY;
    TgVec Q{NAN, NAN, NAN};
    if (key != kTgNone) {
      t = (uint32_t)key;
      TgVec A, B, C;
      uint32_t held = 0xFFFFFFFFu;
      dscene_winner(sc.first_rec.at(t), cell_recs, wrecs, &A, &B, &C, &held);
      if (held != t) { fprintf(stderr, "first_rec[%u] names a record of triangle %u\n", t, held); exit(3); }
      uint32_t region;
      Q = dist_closest(P, A, B, C, &region);
      d = sqrtf(tg_key_float(key));
      ++stats[N_MATCHED];
      ++stats[HIST + dist_bin(d, q)];
      stats[MAX_BITS] = std::max(stats[MAX_BITS], (uint32_t)(key >> 32));
      if (is_signed && dist_negative(P, Q, A, B, C)) d = -d;
    }
    nearest[p] = t; distance[p] = d;
    closest[3 * (size_t)p] = Q.x; closest[3 * (size_t)p + 1] = Q.y; closest[3 * (size_t)p + 2] = Q.z;
  }
}

// case file: u32 n, n_in, n_points, signed, n_orders, n_queries; f32 max_distance, cell_size; f32 q[n_queries]; u32 orders[];
//            f32 S[n][4]; u32 tri[n_in][3]; f32 points[n_points][3]
// result file, per order: i32 rc; u32 n_wide; u32 first_rec[n_in]; u32 wide_t[n_wide];
//            per query: u32 stats[WORDS]; u32 nearest[n_points]; f32 distance[n_points]; f32 closest[n_points][3]
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[6];
  float prm[2];
  if (!get(f, head, 6) || !get(f, prm, 2)) return 2;
  std::vector<float> qs(head[5]);
  std::vector<uint32_t> orders(head[4]), tri(3 * (size_t)head[1]);
  std::vector<float> S(4 * (size_t)head[0]), pts(3 * (size_t)head[2]);
  if (!get(f, qs.data(), qs.size()) || !get(f, orders.data(), orders.size()) || !get(f, S.data(), S.size()) || !get(f, tri.data(), tri.size()) ||
      !get(f, pts.data(), pts.size())) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t order : orders) {
    HostScene sc;
    std::vector<float> map = S;
    std::vector<uint32_t> array = tri;
    const int32_t rc = host_build(head[0], map.data(), array.data(), head[1], prm[0], prm[1], order, &sc);
    // a snapshot: what the build read is gone before the first query
    std::fill(map.begin(), map.end(), NAN);
    std::fill(array.begin(), array.end(), 0xFFFFFFFFu);
    const uint32_t n_wide = rc == 0 ? (uint32_t)sc.g.wide_t.size() : 0u;
    put(o, &rc, 1); put(o, &n_wide, 1);
    if (rc != 0) continue;
    put(o, sc.first_rec.data(), sc.first_rec.size()); put(o, sc.g.wide_t.data(), sc.g.wide_t.size());
    for (float q : qs) {
      std::vector<uint32_t> nearest(head[2], 0xA5A5A5A5u);
      std::vector<float> distance(head[2], 0.0f), closest(3 * (size_t)head[2], 0.0f);
      uint32_t stats[WORDS];
      host_query(sc, pts.data(), head[2], q, (int)head[3], order, nearest.data(), distance.data(), closest.data(), stats);
      put(o, stats, (size_t)WORDS);
      put(o, nearest.data(), nearest.size()); put(o, distance.data(), distance.size()); put(o, closest.data(), closest.size());
    }
  }
  fclose(o);
  return 0;
}
'''

ORDERS = (0, 1, 7)      # forwards, backwards, shuffled with seed 7
WORDS = 8 + 32 + 4


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("distscene_host")


@pytest.fixture(scope="module")
def program(work):
    return ray_host.build(work, PROGRAM, [], "distscene_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return ray_host.build(work, PROGRAM, ray_host.SANITIZE, "distscene_host_san")


def host_scene(exe, work, pos, r2, tri, points, max_distance, cell_size, qs, signed=False):
    """[(rc, first_rec, wide_t, {q: (nearest, distance, closest, stats)})] per order of ORDERS."""
    n = pos.shape[0]
    S = np.zeros((n, 4), np.float32)
    S[:, :3], S[:, 3] = pos, r2
    t = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    P, n_in = pts.shape[0], t.shape[0]
    case, res = work / "case.bin", work / "result.bin"
    with open(case, "wb") as f:
        f.write(np.array([n, n_in, P, int(signed), len(ORDERS), len(qs)], np.uint32).tobytes())
        f.write(np.array([max_distance, cell_size], np.float32).tobytes() + np.array(qs, np.float32).tobytes())
        f.write(np.array(ORDERS, np.uint32).tobytes() + S.tobytes() + t.tobytes() + pts.tobytes())
    r = subprocess.run([exe, str(case), str(res)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, runs = np.fromfile(res, np.uint32), 0, []
    for _ in ORDERS:
        rc, n_wide = int(raw[at:at + 1].view(np.int32)[0]), int(raw[at + 1])
        at += 2
        if rc != 0:
            runs.append((rc, None, None, {}))
            continue
        first, wide_t = raw[at:at + n_in].copy(), raw[at + n_in:at + n_in + n_wide].copy()
        at += n_in + n_wide
        answers = {}
        for q in qs:
            w = raw[at:at + WORDS]
            st = dict(zip(dr.STAT_NAMES, (int(v) for v in w[:8])))
            st["histogram"] = [int(v) for v in w[8:40]]
            st.update(n_wide=int(w[40]), n_entries=int(w[41]), n_cells=int(w[42]), cell_size_used=float(w[43:44].view(np.float32)[0]))
            at += WORDS
            nearest, distance = raw[at:at + P].copy(), raw[at + P:at + 2 * P].copy().view(np.float32)
            closest = raw[at + 2 * P:at + 5 * P].copy().view(np.float32).reshape(-1, 3)
            at += 5 * P
            answers[q] = (nearest, distance, closest, st)
        runs.append((rc, first, wide_t, answers))
    assert at == raw.size
    return runs


def _check_first(first, wide_t, pos, r2, tri, cell_used, what):
    """first_rec against the rule: the model's smallest position for every triangle with cell records, the top bit and the
    triangle's own place in the wide list for the others, NO_REC outside R."""
    want, is_wide = sr.first_records(pos, r2, tri, cell_used)
    assert first[~is_wide].tobytes() == want[~is_wide].tobytes(), what
    assert np.all(first[is_wide] & sr.WIDE_BIT) and np.all(first[is_wide] != sr.NO_REC), what
    assert np.array_equal(wide_t[(first[is_wide] & ~np.uint32(sr.WIDE_BIT)).astype(np.int64)], np.flatnonzero(is_wide).astype(np.uint32)), what
    assert int(np.sum(is_wide)) == wide_t.size and np.unique(wide_t).size == wide_t.size, what


def _compare(exe, work, name, bound, cell_size, signed):
    pos, nrm, r2, tri, _ = dr.world()
    pts, model = dr.point_sets()[name], dr.model_of(name)
    qs = sr.queries(bound)
    matched = differing = 0
    for order, (rc, first, wide_t, answers) in zip(ORDERS, host_scene(exe, work, pos, r2, tri, pts, bound, cell_size, qs, signed)):
        assert rc == 0
        used = next(iter(answers.values()))[3]["cell_size_used"]
        if cell_size > 0:
            assert used == float(dr.cell_used(cell_size, bound))
        else:
            assert used >= float(dr.cell_used(0.0, bound))
        _check_first(first, wide_t, pos, r2, tri, used, (name, bound, cell_size, order))
        for q in qs:
            nearest, distance, closest, st = answers[q]
            wn, wd, wc, wst = dr.answer(model, q, signed)
            wst.pop("max_distance")
            st = dict(st)
            assert st.pop("cell_size_used") == used
            if cell_size > 0:
                wst.update(dr.structure(pos, r2, tri, cell_size, bound))          # (the structure is the build's, whatever q is)
            else:
                for k in ("n_wide", "n_entries", "n_cells"):
                    st.pop(k)
            assert st == wst, (name, bound, cell_size, q, order, st, wst)
            differing += sum(int(a.tobytes() != b.tobytes()) for a, b in ((nearest, wn), (distance, wd), (closest, wc)))
            matched += wst["n_matched"]
    print("%s bound %.3f cell %g signed %d: queries %s, %d matched in all, %d differing arrays" % (name, bound, cell_size, signed, qs, matched, differing))
    assert differing == 0, name
    return matched


def test_every_point_set_at_every_build_and_query_on_the_host(program, work):
    for j, (bound, cell) in enumerate(sr.BUILDS):
        matched = 0
        for k, name in enumerate(dr.point_sets()):
            # the explicit cell of the build for every set; the library's choice and everything in 8 cells in rotation
            cells = (cell, sr.OTHER_CELLS[(k + j) % 2]) if name in (sr.TILE_SET, "around the hand-made triangles") else (cell,)
            for cs in cells:
                matched += _compare(program, work, name, bound, cs, bool((k + j) & 1))
        assert matched > 0, bound


def test_an_index_out_of_range_and_empty_inputs_on_the_host(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    pts = dr.point_sets()["NaN, inf and 65 m"]
    bad = tri.copy()
    bad[77, 2] = pos.shape[0]
    assert [r[0] for r in host_scene(program, work, pos, r2, bad, pts, 0.02, 0.0, (0.02,))] == [-1, -1, -1]
    none = np.zeros((0, 3), np.uint32)
    for rc, first, wide_t, answers in host_scene(program, work, pos, r2, none, pts, 0.02, 0.0, (0.002, 0.02)):
        assert rc == 0 and first.size == 0 and wide_t.size == 0
        for nearest, distance, closest, st in answers.values():
            assert np.all(nearest == dr.INVALID) and np.all(np.isinf(distance)) and np.all(np.isnan(closest))
            assert st["n_matched"] == 0 and st["n_bad_points"] == 7 and st["n_entries"] == 0
    for rc, first, wide_t, answers in host_scene(program, work, pos, r2, tri, np.zeros((0, 3), np.float32), 0.02, 0.05, (0.02,)):
        assert rc == 0 and answers[0.02][0].size == 0 and answers[0.02][3]["n_entries"] == dr.structure(pos, r2, tri, 0.05, 0.02)["n_entries"]
        _check_first(first, wide_t, pos, r2, tri, 0.05, "no points")


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the headers' host code."""
    for name, bound, cs in (("around the hand-made triangles", 0.5, 0.5625), ("around the hand-made triangles", 0.02, 0.0),
                            ("NaN, inf and 65 m", 0.002, 0.00225), ("multiples of c", 0.02, 0.0225)):
        _compare(sanitized, work, name, bound, cs, True)
