"""The model of smx_recon_raycast_mesh (tests/raycast_ref.py) against a float64 statement of the definition, and its own
properties: on every ray set but the one aimed exactly at vertices and edges float32 and float64 agree on hit / no hit for every
ray; where both hit, t agrees within a bound; an accepted hit lies outside its triangle's box by far less than SLACK; removing a
triangle that wins nowhere changes nothing; `cull` 1 and 2 partition the candidates of `cull` 0."""
import numpy as np

import distance_ref as dr
import raycast_ref as rr

AIMED = "aimed at vertices and edges"
# |t32 - t64| where both hit, over all sets (on the aimed set: where both hit the same triangle): the observed maximum is 3.591e-3
# in units of |D|, on a ray of "BAD and limits" with |D_k| = 2^-10 that crosses 20 m (2.2e-5 m along the ray); the largest of
# the other sets is 2.1e-6 ("pinhole", 2.2e-6 m).  The bound is 4 x the observed maximum.
T_OBSERVED = 3.591e-3
T_BOUND = 4 * T_OBSERVED


def test_the_model_against_the_float64_definition():
    pos, nrm, r2, tri, _ = dr.world()
    worst, worst_exc = 0.0, -np.inf
    for name, (rays, t0, t1) in rr.ray_sets().items():
        m = rr.model_of(name)
        hit, t, uv, st = rr.answer(m, 0)
        t64, i64 = rr.definition64(pos, r2, tri, rays, t0, t1)
        h32, h64 = hit != rr.INVALID, i64 != rr.INVALID
        both = h32 & h64
        if name == AIMED:                   # (a ray that slips through a crack hits the far side: only the same triangle compares)
            both = both & (hit == i64)
        dt = float(np.abs(t[both].astype(np.float64) - t64[both]).max()) if np.any(both) else 0.0
        same = int(np.sum(hit[both] == i64[both]))
        dm = float((np.abs(t[both].astype(np.float64) - t64[both]) * np.linalg.norm(rays[both, 3:].astype(np.float64), axis=1)).max()) if np.any(both) else 0.0
        print("%s: %d of %d hit in float32, %d in float64, %d on the same triangle; max |t32 - t64| %.4g (%.3g m along the ray); largest excursion %.3g m"
              % (name, int(h32.sum()), rays.shape[0], int(h64.sum()), same, dt, dm, m["max_excursion"]))
        if name == AIMED:
            print("%s: %d cracks (float64 hits, float32 does not), %d the other way" % (name, int(np.sum(h64 & ~h32)), int(np.sum(h32 & ~h64))))
        elif name != "t_min = t_max":       # (a range of one float: which side of it t falls on is rounding, in either format)
            assert np.array_equal(h32, h64), (name, np.flatnonzero(h32 != h64)[:10])
        worst, worst_exc = max(worst, dt), max(worst_exc, m["max_excursion"])
    print("max |t32 - t64| over all sets: %.3g (bound %.3g); largest excursion %.3g m (bound %.3g)" % (worst, T_BOUND, worst_exc, float(rr.SLACK) / 64))
    assert worst <= T_BOUND
    assert worst_exc < float(rr.SLACK) / 64


def test_removing_a_triangle_that_wins_nowhere_changes_nothing():
    pos, nrm, r2, tri, _ = dr.world()
    name = "around the hand-made triangles"
    rays, t0, t1 = rr.ray_sets()[name]
    hit, t, uv, st = rr.answer(rr.model_of(name), 0)
    losers = np.setdiff1d(np.unique(rr.model_of(name)["pairs"][:, 1]), hit[hit != rr.INVALID])
    assert losers.size > 0
    others = np.setdiff1d(np.random.default_rng(3).permutation(tri.shape[0])[:500], hit)      # and 500 more that win nowhere
    keep = np.ones(tri.shape[0], bool)
    keep[losers] = False
    keep[others] = False
    new_pos = np.cumsum(keep) - 1
    h2, t2, uv2, st2 = rr.answer(rr.brute(pos, r2, tri[keep], rays, t0, t1), 0)
    want = np.where(hit != rr.INVALID, new_pos[np.minimum(hit, tri.shape[0] - 1)], rr.INVALID).astype(np.uint32)
    assert h2.tobytes() == want.tobytes() and t2.tobytes() == t.tobytes() and uv2.tobytes() == uv.tobytes()


def test_cull_1_and_2_partition_the_candidates_of_cull_0():
    for name in ("around the hand-made triangles", "inside-out", "pinhole"):
        m = rr.model_of(name)
        a0, a1, a2 = (rr.answer(m, c) for c in (0, 1, 2))
        k = lambda a: (a[1].view(np.uint32).astype(np.uint64) << np.uint64(32)) | a[0].astype(np.uint64)      # noqa: E731
        assert np.array_equal(k(a0), np.minimum(k(a1), k(a2)))
        both = (a1[0] != rr.INVALID) & (a2[0] != rr.INVALID)
        assert not np.any(a1[0][both] == a2[0][both])                    # no triangle is a candidate on both sides
        assert a0[3]["n_hit"] == int(np.sum((a1[0] != rr.INVALID) | (a2[0] != rr.INVALID)))
        assert a0[3]["n_front_hits"] <= a1[3]["n_hit"] and a1[3]["n_front_hits"] == a1[3]["n_hit"] and a2[3]["n_front_hits"] == 0
    m = rr.model_of("around the hand-made triangles")
    assert rr.answer(m, 1)[3]["n_hit"] > 0 and rr.answer(m, 2)[3]["n_hit"] > 0
