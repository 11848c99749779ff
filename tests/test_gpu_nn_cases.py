"""The neighbour search on the clouds of tests/nn_cases.py: constructed cases that sit on both sides of every threshold of
the dispatch of smx_nn.hip (tests/nn_model.py says which route each takes, tests/test_nn_cases.py asserts it on the CPU).
Every query of every case, under the three query modes, through the batch entry point and -- for the self-query cases --
through smx_nn_query_self: counts, indices and dist^2 bits equal oracle.nn_bruteforce, no tolerance; the modes equal one
another; with statistics on, results == counts.sum(); for the build cases stats() is the model's grid."""
import numpy as np
import pytest

import nn_cases as nc
import nn_model as nm

pytestmark = pytest.mark.gpu

CASES = nc.cases()
GROUPS = list(dict.fromkeys(c.group for c in CASES))


def _equal(case, got, want, what):
    """Counts, and the first `count` entries of every row (rows beyond the count are not compared)."""
    cnt, d2, idx = got
    wcnt, wd2, widx = want
    bad = np.flatnonzero(cnt != wcnt)
    assert bad.size == 0, "%s %s: counts differ at queries %s: %s, want %s" % (case.name, what, bad[:8], cnt[bad[:8]], wcnt[bad[:8]])
    m = np.arange(case.K)[None, :] < wcnt[:, None]
    rows = np.flatnonzero(np.any((idx != widx) & m, axis=1))
    assert rows.size == 0, "%s %s: indices differ at queries %s: %s, want %s" % (case.name, what, rows[:4], idx[rows[0]][m[rows[0]]], widx[rows[0]][m[rows[0]]])
    rows = np.flatnonzero(np.any((d2.view(np.uint32) != wd2.view(np.uint32)) & m, axis=1))
    assert rows.size == 0, "%s %s: dist^2 bits differ at queries %s" % (case.name, what, rows[:4])


def _run_case(nn, case, check_stats=False):
    pts = case.points
    want = nc.reference(case)
    nn.Build(pts[:, 0], pts[:, 1], pts[:, 2], case.cell)
    if check_stats:
        st, model = nn.stats(), nm.Index(pts, case.cell).stats()
        got = {k: st[k] for k in model}
        print("%s: stats %s, model %s" % (case.name, got, model))
        assert got == model and st["n_points"] == len(pts)
    q = pts if case.queries is None else case.queries
    first = None
    far = np.tile(np.nanmax(pts, axis=0) + np.float32(1.0), (len(q), 1)).astype(np.float32)
    for mode in (2, 0, 1):
        # The host rows are copied from staging rows the handle keeps from call to call: a kernel that leaves an entry
        # unwritten would hand back the previous call's.  So every mode starts from rows that belong to another query:
        # the K nearest of a place outside the cloud, by the kernel that shares nothing with the default path.
        nn.set_query_mode(1)
        nn.FindNearestSurfelsWithinRadius(far, np.float32(np.inf), case.K)
        nn.set_query_mode(mode)
        nn.set_stats_enabled(True)
        got = nn.FindNearestSurfelsWithinRadius(q, case.r2, case.K, state=case.state, skip_mask=case.skip_mask)
        results = nn.stats()["results"]
        nn.set_stats_enabled(False)
        _equal(case, got, want, "batch, mode %d" % mode)
        assert results == int(got[0].sum()), (case.name, mode, results, int(got[0].sum()))
        if first is None:
            first = got
        else:                                                                         # the modes equal one another
            _equal(case, got, first, "mode %d against mode 2" % mode)
    if case.queries is None:
        for mode in (2, 0):
            nn.set_query_mode(mode)
            nn.set_stats_enabled(True)
            got = nn.FindNearestOfIndexedPoints(len(pts), case.K, radius_squared=case.r2, factor=1.0, state=case.state,
                                                skip_mask=case.skip_mask)
            results = nn.stats()["results"]
            nn.set_stats_enabled(False)
            _equal(case, got, want, "self, mode %d" % mode)
            assert results == int(got[0].sum()), (case.name, mode, results, int(got[0].sum()))
    nn.set_query_mode(2)


@pytest.mark.parametrize("group", GROUPS)
def test_every_query_equals_brute_force_in_every_mode(smx, group):
    """One handle per group, rebuilt for every cloud of the group (the workspace is reused from case to case)."""
    nn = smx.SurfelNeighborIndex()
    for case in CASES:
        if case.group == group:
            _run_case(nn, case, check_stats=(group == "build"))
    nn.close()


def test_one_handle_rebuilt_large_small_large(smx):
    """The brick table of the large build is kept for the small one and is simply sparser there; the self tiles are cut anew."""
    cases = nc.by_name()
    nn = smx.SurfelNeighborIndex()
    for name in nc.REBUILD_SEQUENCE:
        _run_case(nn, cases[name], check_stats=True)
    nn.close()


def test_the_tile_kernels_regimes_show_in_its_statistics(smx):
    """Query mode 0, one query per call: the tile kernel tests the records of the region's bricks (`distance_tests`) and
    stages the rounds that fit (`staged_candidates`).  2^15 bricks are still walked brick by brick, one more is `everything`
    (every indexed point); 1536 records are staged, 1537 streamed.  The rows themselves cannot tell these apart."""
    cases = nc.by_name()
    nn = smx.SurfelNeighborIndex()
    nn.set_query_mode(0)
    for name in ("bricks_k64", "bricks_corners_k64", "tiles_total_1536_k64", "tiles_total_1537_k64", "stage_kept_257"):
        case = cases[name]
        pts = case.points
        nn.Build(pts[:, 0], pts[:, 1], pts[:, 2], case.cell)
        ix = nm.Index(pts, case.cell)
        r2 = np.broadcast_to(case.r2, (len(case.queries),))
        seen = set()
        for j in range(len(case.queries)):
            t = nm.CaseModel(pts, case.cell, case.queries[j:j + 1], r2[j:j + 1], index=ix).chunks[0].tiles0
            nn.set_stats_enabled(True)
            nn.FindNearestSurfelsWithinRadius(case.queries[j:j + 1], r2[j:j + 1], case.K)
            st = nn.stats()
            nn.set_stats_enabled(False)
            print("%s query %d: %s, tests %d, staged %d" % (name, j, t, st["distance_tests"], st["staged_candidates"]))
            assert st["distance_tests"] == sum(t["round_totals"]), (name, j)
            assert st["staged_candidates"] == sum(v for v in t["round_totals"] if v <= nm.STAGE), (name, j)
            assert t["everything"] == (t["round_totals"] == [ix.n_indexed] and t["nbricks"] > nm.MANY_BRICKS)
            seen |= {k for k in ("staged", "streamed", "everything") if t[k]} | {t["nbricks"]}
        if name == "bricks_k64":
            assert {"staged", "streamed", "everything", 64, 80, 1 << 15} <= seen
    nn.close()
