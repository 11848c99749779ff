"""The model of smx_recon_mesh_distance (tests/distance_ref.py) against itself and against the definition, without a GPU:
the fixtures reach every region and many ties, the float32 statement of the contract's step 3 stays within a measured bound of
the float64 definition, the answer does not depend on the order of the triangle array, and the grid's counts reproduce."""
import numpy as np

import distance_ref as dr

# Measured on these fixtures before any kernel existed: over all point sets and the three max_distance values
# the largest |distance32 - distance64| over the matched points is 2.233e-7 m (a point 0.4 m from the sphere), and 10 points
# change between matched and none, each with its float64 distance within that of max_distance.  The gate is 4 x the maximum;
# it is 0.045 % of the smallest max_distance (0.25 % would put step 3's statement at fault).
OBSERVED_MAX_ERROR = 2.233e-7
GATE = 4.0 * OBSERVED_MAX_ERROR


def test_the_models_constants_are_the_librarys():
    from surfelmeshing_amd import _lib
    assert (dr.BINS, dr.WIDE_CELLS, float(dr.MAX_COORD)) == (_lib.DIST_BINS, _lib.DIST_WIDE_CELLS, _lib.DIST_MAX_COORD)
    assert float(dr.MARGIN) == _lib.DIST_MARGIN and dr.INVALID == 0xFFFFFFFF
    assert tuple(n for n, _ in _lib.DistanceStats._fields_[:len(dr.STAT_NAMES)]) == tuple(dr.STAT_NAMES)


def _regular_world():
    """The world without its two degenerate hand-made triangles (one position twice, three collinear slots): for those the
    contract's NaN rule decides, not the geometry, so the definition is not asked about them."""
    pos, nrm, r2, tri, info = dr.world()
    keep = np.ones(tri.shape[0], bool)
    keep[[info["hand_tri"] + 2, info["hand_tri"] + 3]] = False
    return pos, r2, np.ascontiguousarray(tri[keep])


def test_the_fixtures_reach_every_region_and_many_ties():
    regions, ties = np.zeros(7, np.int64), 0
    for name in dr.point_sets():
        m = dr.model_of(name)
        cand = dr.answer(m, 0.5)[0] != dr.INVALID
        regions += np.bincount(m["region"][cand], minlength=7)[:7]
        ties += int(np.sum(m["ties"][cand] > 1))
    print("winners by region %s: %s; points whose winner is decided by t: %d" % (dr.REGIONS, regions.tolist(), ties))
    assert np.all(regions >= 20) and ties >= 100


def test_step_1_and_step_2_on_the_hand_made_triangles():
    pos, nrm, r2, tri, info = dr.world()
    R, t_of, counts = dr.classify(pos, r2, tri)
    plane_dead = dr.classify(pos, r2, tri[:info["hand_tri"]])[2]["n_not_live"]
    assert counts == dict(n_in=tri.shape[0], n_not_live=plane_dead + 1, n_repeated=1, n_out_of_range=1) and plane_dead > 0
    assert R.shape[0] == tri.shape[0] - plane_dead - 3 and np.all(np.diff(t_of.astype(np.int64)) > 0)
    m = dr.model_of("NaN, inf and 65 m")
    assert int(np.sum(m["bad"])) == 7 and np.all(m["t"][m["bad"]] == dr.INVALID)      # (64 m itself is a good point)
    n, d, c, st = dr.answer(m, 0.02, True)
    assert st["n_bad_points"] == 7 and np.all(np.isinf(d[m["bad"]])) and np.all(np.isnan(c[m["bad"]]))
    # the NaN rule: a point beside the doubled corner gets no number from that triangle, but still an answer
    hm = dr.model_of("around the hand-made triangles")
    assert np.all(np.isfinite(hm["d2"][~hm["bad"]]))


def test_the_model_against_the_float64_definition():
    pos, r2, tri = _regular_world()
    worst, flips, late = 0.0, 0, 0
    for name, pts in dr.point_sets().items():
        m = dr.brute(pos, r2, tri, pts) if name == "around the hand-made triangles" else dr.model_of(name)
        d64 = dr.definition64(pos, r2, tri, pts)
        for md in dr.MAX_DISTANCES:
            nearest, d32, _, _ = dr.answer(m, md)
            cand, cand64 = nearest != dr.INVALID, d64 <= md
            err = np.abs(d32[cand].astype(np.float64) - d64[cand])
            differ = cand != cand64
            worst = max(worst, float(err.max()) if err.size else 0.0)
            flips += int(np.sum(differ))
            late += int(np.sum(np.abs(d64[differ] - md) > GATE))
            print("%-34s max_distance %.3f: %4d matched, max |d32 - d64| %.3e m, %d decisions differ" % (
                name, md, int(np.sum(cand)), float(err.max()) if err.size else 0.0, int(np.sum(differ))))
    print("over all: max |d32 - d64| %.4e m (gate %.4e), %d decisions differ, %d of them beyond the gate" % (worst, GATE, flips, late))
    assert worst <= GATE and GATE <= 0.0025 * min(dr.MAX_DISTANCES)
    assert late == 0


def test_the_answer_does_not_depend_on_the_order_of_the_array():
    pos, nrm, r2, tri, _ = dr.world()
    rev = np.ascontiguousarray(tri[::-1])
    T = tri.shape[0]
    for name in ("vertices 0 / 1 / 5 mm", "around the hand-made triangles"):
        pts = dr.point_sets()[name]
        a, b = dr.model_of(name), dr.brute(pos, r2, rev, pts)
        for md in (0.002, 0.5):
            na, da, ca, sa = dr.answer(a, md, True)
            nb, db, cb, sb = dr.answer(b, md, True)
            matched = na != dr.INVALID
            assert np.array_equal(matched, nb != dr.INVALID)
            # ties go to the other triangle: the magnitudes agree bit for bit, and each nearest is a triangle of the tie
            assert np.abs(da).tobytes() == np.abs(db).tobytes() and sa["histogram"] == sb["histogram"]
            back = (T - 1 - nb[matched].astype(np.int64))
            same = back == na[matched]
            assert np.all(a["ties"][matched][~same] > 1) and np.all(back[~same] > na[matched][~same])
            assert int(np.sum(~same)) > 0 and ca[matched][same].tobytes() == cb[matched][same].tobytes()


def test_the_grid_counts_reproduce():
    pos, nrm, r2, tri, _ = dr.world()
    want = {0.00225: dict(n_wide=9553, n_entries=534, n_cells=534), 0.05: dict(n_wide=9, n_entries=60087, n_cells=12567),
            100.0: dict(n_wide=0, n_entries=10190, n_cells=8)}
    for cs, w in want.items():
        got = dr.structure(pos, r2, tri, cs, 0.002)
        print(cs, got)
        assert got == w
        assert dr.structure(pos, r2, np.ascontiguousarray(tri[::-1]), cs, 0.002) == got
    # below 1.125 x max_distance the cell is that
    assert dr.structure(pos, r2, tri, 1e-3, 0.002) == dr.structure(pos, r2, tri, float(dr.MARGIN * dr.F(0.002)), 0.002)
    R = dr.classify(pos, r2, tri)[0]
    assert want[100.0]["n_entries"] >= R.shape[0]
