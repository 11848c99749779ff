"""The clouds of tests/nn_cases.py without a GPU: every case keeps the margin rule of tests/nn_model.py, takes the routes
it claims through the model of the dispatch of smx_nn.hip, has the match counts it was designed to have (by brute force,
oracle.nn_bruteforce), and the union of the cases reaches every cell of the coverage table below.
tests/test_gpu_nn_cases.py runs the same cases on the device."""
import os
import re

import numpy as np
import pytest

import nn_cases as nc
import nn_model as nm

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "surfelmeshing_amd", "csrc", "smx_nn.hip")
CASES = nc.cases()
TILES_REGIMES = ("staged", "streamed", "one_round", "several_rounds", "everything")
ATTRIBUTES = ("K%4==0", "K%4!=0", "truncated", "not truncated", "filter", "no filter", "batch", "self")

# Cells of the table that cannot occur, each with its reason.
IMPOSSIBLE = {
    ("no_ball", "truncated"): "a query without a ball has no match, and K >= 1",
}
# `everything` x staged may look impossible and is not: the `everything` regime hands
# lane 0 all n_valid records as one range, and that range is staged when n_valid <= kStage.  bricks_corners_k64 reaches it.


@pytest.fixture(scope="module")
def models():
    return {c.name: nm.CaseModel(c.points, c.cell, c.queries, c.r2, c.state, c.skip_mask) for c in CASES}


def test_the_models_constants_are_the_kernels():
    src = open(SRC).read()
    for pat, val in ((r"constexpr int kTile = (\d+)", nm.K_TILE), (r"constexpr int kLaneCap = (\d+)", nm.LANE_CAP),
                     (r"constexpr int kStageL = (\d+)", nm.STAGE_L), (r"constexpr int kStage = (\d+)", nm.STAGE),
                     (r"kManyBricks = 1ull << (\d+)", 15), (r"constexpr int kBlock = (\d+)", nm.CHUNK)):
        assert int(re.search(pat, src).group(1)) == val, pat
    assert nm.MANY_BRICKS == 1 << 15
    for text in ("if (n_max <= 16u)", "if (n_max <= 8u)", "if (nbricks > 64ull)", "if (kept > (uint32_t)kStageL)",
                 "if (cnt > (uint32_t)kLaneCap) redo = true;", "nbricks > kManyBricks", "total <= (uint32_t)kStage",
                 "sqrtf(r2) * 1.0001f + 1e-6f + fabsf(q) * 2.4e-7f", "if (!(d <= 2097152.0))", "3 * axis_bits > 56"):
        assert text in src, text


def test_cases_are_small_float32_and_named_once():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.points.dtype == np.float32 and c.points.shape[1] == 3 and len(c.points) <= 16385
        assert len(c.points) <= 4096 or c.name.startswith("build_n")
        assert c.queries is None or (c.queries.dtype == np.float32 and len(c.queries) <= 4096)
        assert 1 <= c.K <= 64


def test_margin_rule(models):
    for c in CASES:
        m = models[c.name]
        print("%-24s range edge %.3g, cell coordinate %.3g, box face %.3g cell; records on a face %d" % (
            c.name, m.range_margin, m.coord_margin, m.box_margin(), sum(k.near_in for k in m.chunks)))
        nm.assert_margins(m, c.name)


def test_every_case_takes_the_routes_it_names(models):
    for c in CASES:
        m = models[c.name]
        got = m.routes() | m.tiles_regimes(2)
        assert c.expect <= got, (c.name, sorted(c.expect - got))


def test_brute_force_counts_are_the_designed_ones(models):
    for c in CASES:
        m = models[c.name]
        cnt = nc.reference(c)[0]
        assert np.array_equal(np.minimum(m.counts, c.K), cnt), c.name           # the model's numpy brute force = the oracle's
        d = c.designed
        if isinstance(d, np.ndarray):
            assert np.array_equal(m.counts, d), (c.name, m.counts, d)
        elif isinstance(d, dict) and "tiles" in d:
            assert list(np.diff(m.tile_starts)) == d["tiles"], (c.name, list(np.diff(m.tile_starts)), d["tiles"])
        elif isinstance(d, dict) and "nbricks" in d:
            for ch in m.chunks:
                assert len(ch.qid) == 1
                want = d["nbricks"][int(ch.qid[0])]
                assert want is None or ch.nbricks == want, (c.name, ch.qid, ch.nbricks, want)
        elif isinstance(d, dict) and "stats" in d:
            g, s = m.index.grid, d["stats"]
            assert g.passes == s["passes"] and float(g.cell) == s["cell"] and g.doublings == s.get("doublings", 0), c.name
            assert "dim" not in s or [int(v) for v in g.dim] == s["dim"], c.name
            assert "n" not in s or m.index.n_indexed == s["n"]
        elif isinstance(d, dict):
            for q, want in d.items():
                assert m.counts[q] == want, (c.name, q, m.counts[q], want)
            assert len(d) >= 200


def test_the_oracle_takes_the_degenerate_radii(models):
    c = nc.by_name()["degenerate"]
    cnt, d2, idx = nc.reference(c)
    assert np.array_equal(cnt, np.minimum(c.designed, c.K))
    r2 = np.asarray(c.r2)
    assert r2[0] == 0 and cnt[0] == 1 and d2[0, 0] == 0                           # r^2 = 0 at a point: the point itself
    assert r2[1] < 0 and np.isnan(r2[2]) and cnt[1] == 0 and cnt[2] == 0
    assert np.isinf(r2[3]) and r2[4] == np.float32(1e30) and cnt[3] == 64 and cnt[4] == 64
    assert np.isnan(c.queries[16, 0]) and np.isnan(c.queries[17, 2]) and cnt[16] == 0 and cnt[17] == 0
    routes = models[c.name].route
    assert [routes[i] for i in (1, 2, 11, 12, 13, 16, 17)] == ["no_ball"] * 7
    assert routes[3] == routes[4] == "redo_stage" and routes[0] == "net8"


def _direct_morton(bx, by, bz):
    v = 0
    for k in range(21):
        v |= ((bx >> k) & 1) << (3 * k) | ((by >> k) & 1) << (3 * k + 1) | ((bz >> k) & 1) << (3 * k + 2)
    return v


def test_point_keys_equal_a_direct_morton_computation(models):
    for c in CASES:
        ix = models[c.name].index
        g = ix.grid
        cells = np.floor((c.points.astype(np.float64) - g.min.astype(np.float64)) / float(g.cell)).astype(np.int64)
        cells = np.minimum(np.maximum(cells, 0), g.dim - 1)
        step = max(1, len(cells) // 600)                                         # (every point of the small clouds, 600 of the large)
        for i in range(0, len(cells), step):
            x, y, z = (int(v) for v in cells[i])
            want = (_direct_morton(x >> 2, y >> 2, z >> 2) << 6) | ((z & 3) << 4) | ((y & 3) << 2) | (x & 3)
            assert int(ix.keys[i]) == want, (c.name, i)
        assert int(ix.keys.max()) < int(ix.sentinel) and int(ix.sentinel).bit_length() == g.key_bits


def test_every_threshold_has_a_case_on_each_side(models):
    n_max, kept, totals, nbricks, passes, doublings, tile_len, self_tile_len, counts = (set() for _ in range(9))
    n_points = set()
    for c in CASES:
        m = models[c.name]
        passes.add(m.index.grid.passes)
        doublings.add(m.index.grid.doublings)
        n_points.add(len(c.points))
        (self_tile_len if m.self_query else tile_len).update(int(v) for v in np.diff(m.tile_starts))
        for ch in m.chunks:
            n_max.add(ch.n_max)
            kept.add(ch.kept)
            nbricks.add(ch.nbricks)
            counts.update(int(v) for v in ch.counts)
            if ch.tiles:
                totals.update(ch.tiles["round_totals"])
                nbricks.add(ch.tiles["nbricks"])
    assert {8, 9, 16, 17, 32} <= n_max and {32, 33} <= counts
    assert {256, 257} <= kept and {1536, 1537} <= totals
    assert {64, 80, 1 << 15} <= nbricks and any(v > 1 << 15 for v in nbricks)
    assert passes == {2, 3, 4, 5, 6, 7, 8} and doublings == {0, 1, 2}
    assert {2047, 2048, 2049, 16384, 16385} <= n_points
    assert {1, 63, 64} <= tile_len and {1, 64} <= self_tile_len
    # runs that straddle a 256-thread chunk are cut there: a run of 300 behind 200 gives 56, 64 x 3, 52
    assert list(np.diff(models["qtiles_n300_p200"].tile_starts)) == [64, 64, 64, 8, 56, 64, 64, 64, 52]
    assert list(np.diff(models["stiles_n257_p255"].tile_starts)) == [64, 64, 64, 63, 1, 64, 64, 64, 64]


def _coverage(models):
    """{(row, attribute): first case that reaches it}, rows = lanes routes and tiles regimes, query mode 2."""
    seen = {}
    for c in CASES:
        m = models[c.name]
        fixed = ["K%4==0" if c.K % 4 == 0 else "K%4!=0", "filter" if c.state is not None else "no filter",
                 "self" if m.self_query else "batch"]
        for ch in m.chunks:
            trunc = ch.counts > c.K
            for k, route in enumerate(ch.routes):
                for a in fixed + ["truncated" if trunc[k] else "not truncated"]:
                    seen.setdefault((route, a), c.name)
            if ch.tiles:
                redone = np.array([r.startswith("redo") for r in ch.routes])
                t = ch.tiles
                rows = [k for k in ("staged", "streamed", "everything") if t[k]] + ["several_rounds" if t["rounds"] > 1 else "one_round"]
                for row in rows:
                    for a in fixed + (["truncated"] if trunc[redone].any() else []) + (["not truncated"] if (~trunc[redone]).any() else []):
                        seen.setdefault((row, a), c.name)
    return seen


def test_coverage_table(models):
    seen = _coverage(models)
    holes = []
    for row in nm.LANE_ROUTES + TILES_REGIMES:
        print("%-15s" % row + "".join(" | %s: %s" % (a, seen.get((row, a), "IMPOSSIBLE" if (row, a) in IMPOSSIBLE else "-")) for a in ATTRIBUTES))
        for a in ATTRIBUTES:
            if (row, a) in IMPOSSIBLE:
                assert (row, a) not in seen, "%s x %s is listed as impossible (%s) and %s reaches it" % (row, a, IMPOSSIBLE[(row, a)], seen[(row, a)])
            elif (row, a) not in seen:
                holes.append((row, a))
    assert not holes, holes
    # and the wavefront-per-query kernel alone (query mode 0) meets the same regimes over whole tiles
    mode0 = set()
    for c in CASES:
        mode0 |= models[c.name].tiles_regimes(0)
    assert set(TILES_REGIMES) <= mode0


def test_removing_a_case_leaves_a_hole(models):
    """The table is not met by accident: without the cases built for a cell, the cell is empty."""
    def without(groups):
        keep = {c.name: models[c.name] for c in CASES if c.group not in groups}
        saved = list(CASES)
        try:
            CASES[:] = [c for c in saved if c.name in keep]
            return _coverage(keep)
        finally:
            CASES[:] = saved
    assert ("everything", "batch") not in without({"bricks"})
    assert ("redo_bricks", "self") not in without({"bricks"})
    assert ("no_ball", "batch") not in without({"degenerate", "stage"})
    assert ("streamed", "K%4!=0") not in without({"stage", "bricks", "lattice"})
