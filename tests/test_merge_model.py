"""Properties of the model of smx_recon_merge_map (tests/merge_ref.py) and of the hand-built cases (tests/merge_cases.py): CPU
only.  What the device is then held to, byte for byte, is this model (tests/test_gpu_merge.py), so the model itself is checked
against what a merge must mean, and the cases against mutants of the definition: each mutant has to fail a named case."""
import numpy as np
import pytest

import merge_cases as mc
import merge_ref as mr

F = np.float32


@pytest.fixture(scope="module")
def case_list():
    return mc.cases()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(mr.comparable(a), mr.comparable(b))


def test_census_reaches_every_decision(case_list):
    table = mc.census(case_list)
    wanted = ["dst size 1023", "dst size 1024", "dst size 1025", "append crosses the 1024-slot edge", "empty src", "empty dst",
              "src merged slots interleaved", "NaN radius is live", "BAD position", "BAD smooth position", "BAD normal",
              "equal d2: lower index wins", "d2 == r2 matches", "d2 one ulp outside: appended", "dot == cos_max matches",
              "dot one ulp below: appended", "first k incompatible, compatible behind: unmatched, n_saturated", "k = 1", "k = 64",
              "3 sources onto one dst slot, order matters", "7 sources onto one dst slot, order matters", "W == 0", "W < 0",
              "len2 == 0: N stays", "confidence cap reached", "link to appended", "link to matched", "link to merged", "link to BAD",
              "link invalid", "capacity exactly full", "capacity one short: refused", "pose with rotation and translation", "identity pose"]
    assert not [d for d in wanted if d not in table]
    assert len({c.name for c in case_list}) == len(case_list)


def test_cases_decide_what_they_claim(case_list):
    by = {c.name: c for c in case_list}

    def run(name, mode=mr.KEEP_DST):
        c = by[name]
        return c, mr.merge_model(c.dst, c.src, c.T, c.params(mode), c.max_surfels)

    c, (rows, s2d, st, ex) = run("on_the_ball_and_one_ulp_outside")
    assert list(s2d) == [0, 1] and (st["n_matched"], st["n_appended"]) == (1, 1)
    c, (rows, s2d, st, ex) = run("normal_at_cos_max_and_one_ulp_below")
    assert list(s2d) == [0, 2]
    c, (rows, s2d, st, ex) = run("equal_d2_lower_index_wins")
    assert list(s2d) == [3]
    c, (rows, s2d, st, ex) = run("saturated_k3")
    assert (st["n_saturated"], st["n_appended"]) == (1, 1)
    c, (rows, s2d, st, ex) = run("not_saturated_k4")
    assert list(s2d) == [3] and st["n_saturated"] == 0
    c, (rows, s2d, st, ex) = run("nan_radius_and_bad_slots")
    assert st["n_bad"] == 3 and st["n_src_live"] == 8 and list(s2d[2:5]) == [mr.INVALID] * 3 and s2d[1] == 21 and s2d[5] == 22
    c, (rows, s2d, st, ex) = run("links_of_each_kind")
    assert list(s2d) == [4, 0, mr.INVALID, mr.INVALID, 5, 6]
    u = mr.u32(rows)
    assert list(u[19:23, 5]) == [4, mr.INVALID, mr.INVALID, mr.INVALID] and list(u[19:23, 6]) == [mr.INVALID, 5, mr.INVALID, 4]
    assert st["links_dropped"] == 4
    c, (rows, s2d, st, ex) = run("capacity_exactly_full")
    assert not ex["failed"] and rows.shape[1] == 42
    c, (rows, s2d, st, ex) = run("capacity_one_short")
    assert ex["failed"] and _same(rows, c.dst) and st["n_appended"] == 12 and st["new_size"] == 30
    # blend decisions
    c, (rows, s2d, st, ex) = run("blend_W_not_positive", mr.BLEND)
    assert np.array_equal(mr.u32(rows)[0:11, 0:2], mr.u32(c.dst)[0:11, 0:2]) and list(mr.u32(rows)[18]) == [5, 5, 5]
    assert rows[6, 2] == F(2.0)
    c, (rows, s2d, st, ex) = run("blend_opposed_normals_len2_zero", mr.BLEND)
    assert np.array_equal(rows[8:11], c.dst[8:11]) and list(rows[6]) == [2.0, 2.0]
    c, (rows, s2d, st, ex) = run("blend_confidence_cap", mr.BLEND)
    assert list(rows[6]) == [2.5, 2.5]
    for name in ("blend_3_onto_one", "blend_7_onto_one"):
        c, (rows, s2d, st, ex) = run(name, mr.BLEND)
        assert st["n_blended_dst"] == 1 and set(s2d) == {1}
        assert np.isfinite(rows[0:11, 1]).all()
        n = rows[8:11, 1].astype(np.float64)
        assert abs(np.dot(n, n) - 1.0) < 1e-6


def test_self_merge_at_identity_changes_nothing(case_list):
    """A copy of a map into itself at the identity under KEEP_DST: every live slot matches, nothing is appended, every byte stays."""
    m = mc.chain_links(mc.plane(700))
    m[7, 5::11] = F(-1.0)
    rows, s2d, st, ex = mr.merge_model(m, m.copy(), mc.IDENTITY, mr.params())
    live = ~(m[7] < 0)
    assert st["n_matched"] == int(live.sum()) == st["n_src_live"] and st["n_appended"] == 0 and st["n_bad"] == 0
    assert np.array_equal(s2d[live], np.nonzero(live)[0]) and (s2d[~live] == mr.INVALID).all()
    assert _same(rows, m)


def test_far_away_merge_is_the_concatenation(case_list):
    """A map moved 10 m away appends every live slot: the result is the concatenation, with links shifted."""
    a = mc.chain_links(mc.plane(300))
    b = mc.chain_links(mc.plane(200, conf=2.0, color0=0x00334455))
    T = mc.IDENTITY.copy()
    T[11] = F(10.0)
    p = mr.params(frame_index=6)
    rows, s2d, st, ex = mr.merge_model(a, b, T, p)
    assert st["n_appended"] == 200 and st["n_matched"] == 0 and st["links_dropped"] == 0 and rows.shape[1] == 500
    assert np.array_equal(s2d, 300 + np.arange(200, dtype=np.uint32))
    assert _same(rows[:, :300], a)
    want = b.copy()
    want[2] = want[5] = F(10.0)
    uw = mr.u32(want)
    uw[17] = uw[18] = 6
    for r in range(19, 23):
        uw[r] = np.where(uw[r] == mr.INVALID, mr.INVALID, uw[r] + np.uint32(300))
    assert _same(rows[:, 300:], want)


def test_split_sphere_comes_back_whole():
    """A noise-free sphere split into x < 0.2 and x > -0.2, the second half stored in its own frame: under the true pose
    n_matched is the overlap's count and the live count is the whole sphere's."""
    n = 1500
    i = np.arange(n) + 0.5
    phi, theta = np.arccos(1 - 2 * i / n), np.pi * (1 + 5 ** 0.5) * i
    pts = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)]).astype(F)
    rows = mr.blank_rows(n)
    rows[0:3] = rows[3:6] = rows[8:11] = pts
    rows[6], rows[7] = F(1.0), F(0.02 * 0.02)      # (the points are 0.09 apart)
    first, second = rows[:, pts[0] < 0.2], rows[:, pts[0] > -0.2]
    overlap = int(((pts[0] < 0.2) & (pts[0] > -0.2)).sum())
    T = mc.rot_pose((0.3, -1.0, 0.5), 71.0, (1.5, 0.25, -3.0))
    for mode in (mr.KEEP_DST, mr.BLEND):
        out, s2d, st, ex = mr.merge_model(first, mc.in_own_frame(second, T), T, mr.params(mode=mode))
        assert st["n_matched"] == overlap and st["n_bad"] == 0 and st["n_saturated"] == 0
        assert out.shape[1] == n and int((~(out[7] < 0)).sum()) == n
        # every point of the sphere is there, to the rounding of the stored frame
        d = np.abs(np.sort(out[3:6].astype(np.float64), axis=1) - np.sort(pts.astype(np.float64), axis=1)).max()
        assert d < 1e-5, d


MUTANT_FAILS = {"tie_high_index": "equal_d2_lower_index_wins", "blend_reversed": "blend_7_onto_one", "normal_gt": "normal_at_cos_max_and_one_ulp_below",
                "ball_lt": "on_the_ball_and_one_ulp_outside"}


@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_every_mutant_fails_its_case(case_list, mutant):
    """A wrong tie rule, a reversed blend order, > for >= (and < for <= on the ball): each gives other bytes on a named case."""
    assert set(MUTANT_FAILS) == set(mr.MUTANTS)
    failing = []
    for c in case_list:
        for mode in (mr.KEEP_DST, mr.BLEND):
            good = mr.merge_model(c.dst, c.src, c.T, c.params(mode), c.max_surfels)
            bad = mr.merge_model(c.dst, c.src, c.T, c.params(mode), c.max_surfels, mutant=mutant)
            if not _same(good[0], bad[0]) or good[2] != bad[2]:
                failing.append(c.name)
    print("%s -> %s" % (mutant, sorted(set(failing))))
    assert MUTANT_FAILS[mutant] in failing


def test_reversed_blend_order_gives_other_bits(case_list):
    """The two order cases decide: walking their sources downwards gives other bits (so the order is observable)."""
    for name in ("blend_3_onto_one", "blend_7_onto_one"):
        c = next(c for c in case_list if c.name == name)
        good = mr.merge_model(c.dst, c.src, c.T, c.params(mr.BLEND))[0]
        bad = mr.merge_model(c.dst, c.src, c.T, c.params(mr.BLEND), mutant="blend_reversed")[0]
        assert not _same(good, bad), name


def test_remap_triangles_drops_triangles_that_lose_a_corner():
    s2d = np.array([5, mr.INVALID, 7, 0, 9], np.uint32)
    tri = np.array([[0, 2, 3], [0, 1, 2], [4, 3, 2]], np.uint32)
    assert mr.remap_triangles(tri, s2d).tolist() == [[5, 7, 0], [9, 0, 7]]
    from surfelmeshing_amd import meshing
    assert meshing.remap_triangles(tri, s2d).tolist() == [[5, 7, 0], [9, 0, 7]]
