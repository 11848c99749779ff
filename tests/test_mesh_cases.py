"""The maps of tests/mesh_cases.py without a GPU: every case keeps the margin rule, reaches the decisions it claims (read
off the float64 / Qhull model's own lists, stars and filter verdicts, and off the ring rows of the host build), has the
stars the definition gives, and comes out of the host build of smx_mesh.hpp exactly as out of the model: the same array,
the same star set, the same statistics, no cap.  One-token mutants of a copy of smx_mesh.hpp show which case catches what.
tests/test_gpu_mesh_cases.py makes the same comparison on the device."""
import math
import re

import numpy as np
import pytest

import mesh_cases as mc
import mesh_ref as mr
import mesh_update_ref as mu
from mesh_host import SRC, build_host, host, host_triangulate  # noqa: F401

DECISIONS = ["D%d" % k for k in range(1, 13)]


class Ref:
    """The model's view of a map: lists, stars, overflowed slots, uncapped degrees, triangles, statistics."""

    def __init__(self, pos, nrm, r2, prm):
        self.lists, self.live, self.truncated = mr.candidate_lists(pos, nrm, r2, prm)
        self.stars, _, _, self.n_overflow = mr.stars(pos, nrm, r2, prm)
        self.tri, self.stats, self.all_star = mr.triangulate(pos, nrm, r2, prm)
        self.degree, self.pairs, self.overflowed = {}, {}, set()
        cap = mr.MAX_STAR_DEGREE
        try:
            mr.MAX_STAR_DEGREE = 1 << 30
            for p in self.stars:
                s = mr.star_of(*self.lists[p])
                self.degree[p], self.pairs[p] = len(set(v for e in s for v in e)), len(s)
                if self.degree[p] > cap:
                    self.overflowed.add(p)
        finally:
            mr.MAX_STAR_DEGREE = cap
        assert len(self.overflowed) == self.n_overflow
        self.owned = {p: int(np.sum(self.tri[:, 0] == p)) for p in self.stars}

    def members(self, p):
        return set(v for e in self.stars[p] for v in e)


@pytest.fixture(scope="module")
def all_cases():
    return mc.cases()


@pytest.fixture(scope="module")
def swept(all_cases):
    return {c.name: (mc.sweep(c.pos, c.nrm, c.r2, c.prm, c.exempt), Ref(c.pos, c.nrm, c.r2, c.prm)) for c in all_cases}


def _assert_margins(name, sw):
    for kind, (ratio, where, _) in sorted(sw.margins.items()):
        print("  %-12s %-22s least margin %.3g at %s" % (name, kind, ratio, where))
        assert ratio >= mc.Case.margin_of(kind), "%s breaks the margin rule: %s is %.3g of its terms at %s" % (name, kind, ratio, where)


def _assert_host_equals_model(L, m, prm, what):
    got, got_stars, st = host_triangulate(L, *m, prm)
    want, wst, want_stars = mr.triangulate(*m, prm)
    assert got.tobytes() == want.tobytes(), "%s: the arrays differ\n%s\n%s" % (what, got, want)
    assert got_stars == want_stars, "%s: star triangles differ: %s" % (what, sorted(sorted(t) for t in got_stars ^ want_stars)[:20])
    assert st == {k: wst[k] for k in st}, "%s: host %s, model %s" % (what, st, wst)
    return wst


def test_cases_are_small_float32_valued_and_named_once(all_cases):
    assert len(set(c.name for c in all_cases)) == len(all_cases)
    for c in all_cases:
        assert c.pos.shape[0] <= 2000 and c.claims <= set(DECISIONS)
        for a in c.map:
            assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64), equal_nan=True)


def test_margin_rule_and_the_star_by_definition(all_cases, swept):
    for c in all_cases:
        sw, ref = swept[c.name]
        _assert_margins(c.name, sw)
        assert set(sw.stars) == set(ref.stars)
        for p in ref.stars:
            assert sw.stars[p] == ref.stars[p], "%s slot %d: by definition %s, model %s" % (c.name, p, sw.stars[p], ref.stars[p])
        assert sw.overflow == ref.overflowed and sw.star_triangles == ref.all_star
        assert len(sw.full) == ref.stats["truncated_lists"] and sum(sw.owned.values()) == ref.stats["n_triangles"]
        # (the owner hands mesh_triangle_filter its pair counter-clockwise about its own normal: never an accepted 2)
        assert 2 not in sw.verdict.values()


def test_host_build_equals_the_model_exactly(all_cases, host):
    for c in all_cases:
        st = _assert_host_equals_model(host, c.map, c.prm, c.name)
        print("  %-12s %4d slots: %s" % (c.name, c.pos.shape[0], st))


def _angles(P):
    out = []
    for k in range(3):
        e, f = P[(k + 1) % 3] - P[k], P[(k + 2) % 3] - P[k]
        out.append(math.degrees(math.acos((e @ f) / math.sqrt((e @ e) * (f @ f)))))
    return out


def _agreed(ref, t):
    p, a, b = t
    return (frozenset((a, b)) in ref.stars[p] and frozenset((p, b)) in ref.stars[a] and frozenset((p, a)) in ref.stars[b])


def _in_output(ref, t):
    return frozenset(t) in mr.as_set(ref.tri)


def reached(c, sw, ref, rings, meta):
    """The decision ids the case reaches, each by its own check; a check that does not apply to the case's map is skipped
    through its role names."""
    out, roles, n = set(), c.roles, c.pos.shape[0]
    deg = lambda p: int(meta[p] & 0xFF)
    mask = lambda p: (int(meta[p]) >> 8) & 0xFFFF
    if "rings" in roles or "owners" in roles:
        d16 = [p for p in ref.stars if ref.degree[p] == 16 and ref.pairs[p] == 16]
        for p in d16:      # a full row, the pair from entry 15 to entry 0, meta bit 23
            assert deg(p) == 16 and mask(p) == 0xFFFF and (int(meta[p]) >> 23) & 1 and np.all(rings[p] < n)
        if any(p < min(ref.members(p)) for p in d16) and any(p > max(ref.members(p)) for p in d16):
            out.add("D1")
        over = [p for p in ref.overflowed]
        for p in over:
            assert int(meta[p]) == 0x80000000 and np.all(rings[p] == 0xFFFFFFFF) and not ref.stars[p]
        if any(ref.degree[p] == 17 for p in over):
            out.add("D2")
        if (any(ref.degree[p] == 40 for p in over) and any(ref.degree[p] == 63 and p in sw.full for p in over)
                and c.prm.max_neighbors == 64 and ref.stats["truncated_lists"] >= 1):
            out.add("D3")
        # D4: the ring members' star triangles with an overflowed hub as a corner: in the star set once each, never output
        sides = set()
        for h in over:
            if ref.degree[h] != 17:
                continue
            with_h = [t for t in ref.all_star if h in t]
            others = set(v for t in with_h for v in t) - {h}
            assert len(with_h) == 17 and not any(_in_output(ref, t) for t in with_h) and h not in ref.tri
            sides.add("below" if h < min(others) else "above" if h > max(others) else "between")
        if {"below", "above"} <= sides:
            out.add("D4")
    if "trip" in roles:
        a, b, m_, l_ = roles["trip"]
        assert a % 4 == 0 and [b, m_, l_] == [a + 1, a + 2, a + 3]
        if (a in ref.overflowed and ref.degree[b] == 16 and c.r2[m_] < 0 and ref.live[l_] and ref.lists[l_][0].size == 0
                and sw.candidates[l_] == 0 and n % 4 != 0):
            out.add("D5")
    if "owners" in roles:
        ok = roles["owners"][:2] == [255, 256]
        last = roles["owners"][2]
        ok &= int(ref.tri[-1, 0]) == last and np.all(ref.tri[-16:, 0] == last) and last == n - 17
        for p in roles["owners"]:
            ok &= ref.owned[p] == 16 and deg(p) == 16
            ring_order = [(int(rings[p][i]), int(rings[p][(i + 1) % 16])) for i in range(16)]
            ok &= ring_order != sorted(ring_order)                     # the insertion loop of the write pass shifts entries
        ok &= bool(np.any(ref.tri[:, 1] > ref.tri[:, 2]))              # filter_and_orient swapped the index order somewhere
        if ok:
            out.add("D6")
    if "d12_hub" in roles:
        h, gone = roles["d12_hub"], {roles["d12_merged"], roles["d12_nan"]}
        in_ball = np.sum((c.pos[roles["d12_merged"]] - c.pos[h]) ** 2) < c.r2[h]
        used = set(int(v) for v in ref.tri.ravel()) | set(v for t in ref.all_star for v in t) | set(int(v) for v in rings[rings < n])
        if ref.pairs[h] == ref.degree[h] == 8 and in_ball and not (gone & used) and np.isnan(c.pos[roles["d12_nan"], 0]) and ref.owned[h] == 8:
            out.add("D12")
    if "boundary_hub" in roles and c.prm.max_angle_between_normals_deg == 90.0:
        h, lone = roles["boundary_hub"], roles["lonely"]
        one_cand = [p for p in ref.stars if sw.candidates[p] == 1]
        two = [p for p in ref.stars if ref.degree[p] == 2 and ref.pairs[p] == 1]
        ok = ref.degree[lone] == 0 and deg(lone) == 0 and bool(one_cand) and all(deg(p) == 0 for p in one_cand)
        ok &= bool(two) and all(deg(p) == 2 and bin(mask(p)).count("1") == 1 for p in two)
        ok &= ref.degree[h] == 5 and ref.pairs[h] == 4 and deg(h) == 5 and mask(h) == 0b01111     # the closing pair bit is clear
        if ok:
            out.add("D7")
        # D8 a: a list that holds only p; c: a slot along p's normal is in the ball, passes the normal test, is dropped
        hub, above = roles["d8c_hub"], roles["d8c_above"]
        d2 = np.sum((c.pos[above] - c.pos[hub]) ** 2)
        if (sw.candidates[lone] == 0 and d2 <= c.r2[hub] and c.nrm[above] @ c.nrm[hub] > 0 and above not in ref.lists[hub][0]
                and ref.degree[hub] == 6 and ref.owned[hub] == 6 and not any(above in t for t in ref.all_star)):
            out.add("D8")
        p, a, b = roles["d9_radii"]
        t = frozenset((p, a, b))
        radii = (t in ref.all_star and not _in_output(ref, t) and frozenset((a, b)) in ref.stars[p]
                 and np.sum((c.pos[a] - c.pos[b]) ** 2) > c.r2[a] and b not in ref.lists[a][0])
        p, a, b, d = roles["d9_planes"]
        t = frozenset((p, a, b))
        planes = (t in ref.all_star and not _in_output(ref, t) and frozenset((a, b)) in ref.stars[p] and frozenset((p, a)) in ref.stars[b]
                  and frozenset((p, b)) not in ref.stars[a] and {p, b, d} <= set(int(v) for v in ref.lists[a][0]))
        if radii and planes and ref.stats["n_star_triangles"] == len(ref.all_star) > ref.stats["n_triangles"]:
            out.add("D9")
    if "d10_thin" in roles:
        lo, hi = c.prm.min_triangle_angle_deg, c.prm.max_triangle_angle_deg
        why = set()
        for role in ("d10_thin", "d10_flat", "d10_normal"):
            t = tuple(roles[role])
            if not _agreed(ref, t) or mr.filter_and_orient(t, c.pos, c.nrm, c.prm) is not None:
                continue
            ang = _angles(c.pos[list(t)])
            tn = np.cross(c.pos[t[1]] - c.pos[t[0]], c.pos[t[2]] - c.pos[t[0]])
            tn = tn * np.sign(tn @ (c.nrm[t[0]] + c.nrm[t[1]] + c.nrm[t[2]]))
            if min(ang) < lo and max(ang) <= hi:
                why.add("min")
            elif max(ang) > hi and min(ang) >= lo:
                why.add("max")
            elif min(tn @ c.nrm[k] for k in t) < 0:
                why.add("normal")
        out |= set("D10:" + w for w in why)
    if "up" in roles:
        sheet = lambda p: p % 2
        own_only = all(sheet(v) == sheet(p) for p in ref.stars for e in ref.stars[p] for v in e)
        both = set(sheet(int(t[0])) for t in ref.tri) == {0, 1}
        if c.prm.max_angle_between_normals_deg == 90.0 and own_only and both:
            out.add("D8:apart")
        if c.prm.max_angle_between_normals_deg > 90.0 and not own_only:
            out.add("D8:mixed")
    if "f1" in roles:
        f = c.prm.search_radius_factor
        r = roles["f1" if f == 1.0 else "f2"]
        p = r["p"]
        rr = np.float32(f) * np.float32(f) * np.float32(c.r2[p])
        d2 = lambda j: np.float32(np.sum((c.pos[j] - c.pos[p]) ** 2))       # (exact in float64, and representable)
        if (d2(r["on"]) == rr and d2(r["off"]) == np.nextafter(rr, np.float32(np.inf)) and float(d2(r["off"])) == np.sum((c.pos[r["off"]] - c.pos[p]) ** 2)
                and r["on"] in ref.lists[p][0] and r["off"] not in ref.lists[p][0]
                and frozenset((p, r["on"], r["inside"])) in ref.all_star and not any(r["off"] in t for t in ref.all_star if p in t)):
            out.add("D11:%g" % f)
    return out


def test_every_decision_is_reached(all_cases, swept, host):
    table = {}
    for c in all_cases:
        sw, ref = swept[c.name]
        _, _, _, rings, meta = host_triangulate(host, *c.map, c.prm, with_rings=True)
        got = reached(c, sw, ref, rings, meta)
        for d in got:
            table.setdefault(d, []).append(c.name)
        assert c.claims <= set(d.split(":")[0] for d in got), "%s claims %s, reaches %s" % (c.name, sorted(c.claims), sorted(got))
    print("\ndecision -> cases")
    for d in sorted(table, key=lambda s: (int(re.sub(r"\D", "", s.split(":")[0])), s)):
        print("  %-14s %s" % (d, ", ".join(table[d])))
    print("not constructible:")
    for k, v in mc.NOT_CONSTRUCTIBLE.items():
        print("  %s: %s" % (k, v))
    assert set(d.split(":")[0] for d in table) == set(DECISIONS)
    # the parts of a decision that need different parameters are reached by different cases
    assert {"D8", "D8:apart", "D8:mixed", "D10:min", "D10:max", "D10:normal", "D11:1", "D11:2"} <= set(table), sorted(table)


def test_update_steps_keep_the_margin_rule_and_do_what_they_say(host):
    steps, roles = mc.update_steps()
    assert [s[0] for s in steps] == ["U0", "U1", "U2", "U3", "U4", "U5"]
    seen = {}
    for name, m, touched in steps:
        if name in ("U2", "U5"):       # (the map of the step before U1, and U4's, again)
            prev = steps[0][1] if name == "U2" else steps[4][1]
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(m, prev))
            seen[name] = seen["U0" if name == "U2" else "U4"]
            continue
        sw = mc.sweep(*m, mr.Params())
        _assert_margins(name, sw)
        ref = Ref(*m, mr.Params())
        assert all(sw.stars[p] == ref.stars[p] for p in ref.stars)
        _assert_host_equals_model(host, m, mr.Params(), name)
        seen[name] = ref
    n = [s[1][0].shape[0] for s in steps]
    for k in range(1, 6):      # rows touched since the step before, and the work list: below the default full_above_fraction
        assert int(mu.changed_mask(steps[k - 1][1], steps[k][1]).sum()) == steps[k][2], steps[k][0]
        dirty = int(mu.dirty_mask(steps[k - 1][1], steps[k][1], mr.Params()).sum())
        print("  %s: %d rows touched, a work list of %d of %d slots" % (steps[k][0], steps[k][2], dirty, n[k]))
        assert dirty <= 0.2 * n[k] and (dirty > 0) == (steps[k][2] > 0)
    h1, h3, h4 = roles["u1_hub"], roles["u3_hub"], roles["u4_hub"]
    u0, u1, u3, u4 = seen["U0"], seen["U1"], seen["U3"], seen["U4"]
    assert u0.degree[h1] == 17 and h1 in u0.overflowed and u0.owned[h1] == 0
    assert u1.degree[h1] == 16 and u1.owned[h1] == 16 and u1.stats["star_overflow"] == u0.stats["star_overflow"] - 1
    assert u0.degree[h3] == 16 and u0.owned[h3] == 16 and u3.degree[h3] == 15 and u3.owned[h3] == 15 and u3.stats["n_live"] == n[0] - 1
    assert u3.degree[h4] == 16 and u3.owned[h4] == 16 and n[4] == n[3] + 1 and (n[4] - 1) in u4.lists[h4][0]
    assert u4.degree[h4] == 17 and h4 in u4.overflowed and u4.owned[h4] == 0
    print("\nstep -> map: U1-U5 are steps of the composite map (%d slots, %d after U4)" % (n[0], n[4]))


MUTANTS = [
    ("degree mask 0xF", "return meta & 0xFFu;", "return meta & 0xFu;"),
    ("ring lookup stops at entry 14", "for (int t = 0; t < kMeshMaxStarDegree; ++t) {", "for (int t = 0; t < kMeshMaxStarDegree - 1; ++t) {"),
    ("pair mask shifted by 9", "((meta >> (8 + t)) & 1u)", "((meta >> (9 + t)) & 1u)"),
    ("wrap reads ring[(t + 1) % 16]", ": ring[0];", ": ring[(t + 1) % kMeshMaxStarDegree];"),
    ("third corner's normal unchecked", " && mesh_dot(n, nb) > 0.0f", ""),
    ("largest angle at p unchecked", "c0 <= cos_min_angle && c0 >= cos_max_angle", "c0 <= cos_min_angle"),
]
_caught = {}


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_a_mutant_of_the_header_is_caught(mutant, all_cases, tmp_path):
    what, old, new = mutant
    text = open(SRC + "/smx_mesh.hpp").read()
    assert text.count(old) == 1, "%s: %d matches" % (what, text.count(old))
    (tmp_path / "smx_mesh.hpp").write_text(text.replace(old, new))
    L = build_host(tmp_path, header_dir=tmp_path)      # (the library stays on disk while loaded: a reused inode would alias it)
    caught = []
    for c in all_cases:
        got, got_stars, st = host_triangulate(L, *c.map, c.prm)
        want, wst, want_stars = mr.triangulate(*c.map, c.prm)
        if got.tobytes() != want.tobytes() or got_stars != want_stars or st != {k: wst[k] for k in st}:
            caught.append(c.name)
    _caught[what] = caught
    print("\nmutant -> cases")
    for k, v in _caught.items():
        print("  %-34s %s" % (k, ", ".join(v) or "-"))
    assert caught, "no case notices: " + what
