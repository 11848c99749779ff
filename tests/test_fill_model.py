"""The model of smx_recon_fill_holes (tests/fill_ref.py) against a brute-force version written here: dictionaries of
half-edges instead of sorted keys, loops by a depth-first walk over the gaps with three colours instead of a walk from every
unvisited vertex, the geometry on float32 arrays instead of scalars.  Random soups, the hand cases of tests/fill_cases.py and
the noisy sphere; the consequences of the contract's item 6 are asserted on every output."""
import collections

import numpy as np
import pytest

import fill_cases as fc
import fill_ref as fr
import mesh_ref as mr

F = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cos_at(at, b, c):
    e, f = b - at, c - at
    with np.errstate(invalid="ignore", divide="ignore"):
        return _dot(e, f) / np.sqrt(_dot(e, e) * _dot(f, f))


def brute_filter(P, N, cmin, cmax):
    """P, N: float32 [3, 3] corner positions and normals of (p, a, b).  The value of the library's triangle filter."""
    c = [_cos_at(P[k], P[(k + 1) % 3], P[(k + 2) % 3]) for k in range(3)]
    if not all(x <= cmin and x >= cmax for x in c):
        return 0
    a, b = P[1] - P[0], P[2] - P[0]
    n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
    s = _dot(n, (N[0] + N[1]) + N[2])
    if not (s > 0) and not (s < 0):
        return 0
    if s < 0:
        n = -n
    if not all(_dot(n, N[k]) > 0 for k in range(3)):
        return 0
    return 2 if s < 0 else 1


def brute(pos, nrm, r2, tri, max_hole_edges=8, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0):
    pos32, nrm32 = np.asarray(pos, F), np.asarray(nrm, F)
    live = [not (r2[i] < 0) and bool(np.all(np.isfinite(pos32[i]))) for i in range(pos32.shape[0])]
    R = [tuple(int(v) for v in t) for t in np.asarray(tri).reshape(-1, 3) if all(live[int(v)] for v in t)]
    half = collections.Counter()
    for p, a, b in R:
        for u, v in ((p, a), (a, b), (b, p)):
            half[(u, v)] += 1
    pairs = {}
    for (u, v), c in half.items():
        fg = pairs.setdefault((min(u, v), max(u, v)), [0, 0])
        fg[0 if u <= v else 1] += c
    st = dict.fromkeys(fr.STAT_NAMES, 0)
    st["n_in"], st["n_not_live"], st["n_edges"] = len(np.asarray(tri).reshape(-1, 3)), len(np.asarray(tri).reshape(-1, 3)) - len(R), len(pairs)
    outs, ins = collections.defaultdict(list), collections.defaultdict(list)
    for (lo, hi), (f, g) in pairs.items():
        if f + g == 1:
            st["n_boundary_edges"] += 1
            u, v = (lo, hi) if f == 1 else (hi, lo)       # the triangle's half-edge u -> v; the gap is v -> u
            outs[v].append(u)
            ins[u].append(v)
        elif not (f == 1 and g == 1):
            st["n_nonmanifold_edges"] += 1
    touched = set(outs) | set(ins)
    simple = {w for w in touched if len(outs[w]) == 1 and len(ins[w]) == 1}
    st["n_pinched_vertices"] = len(touched - simple)
    colour, loops = {}, []
    for start in sorted(simple, reverse=True):             # (any order: a cycle is found from whichever vertex is met first)
        path, w = [], start
        while w in simple and w not in colour:
            colour[w] = 1
            path.append(w)
            w = outs[w][0]
        if colour.get(w) == 1 and w in path:
            cyc = path[path.index(w):]
            k = cyc.index(min(cyc))
            loops.append(cyc[k:] + cyc[:k])
        for v in path:
            colour[v] = 2
    listed = sorted((c for c in loops if 3 <= len(c) <= max_hole_edges), key=lambda c: c[0])
    cmin, cmax = fr.cos_limit(min_triangle_angle_deg), fr.cos_limit(max_triangle_angle_deg)
    holes, new = np.zeros(len(listed), fr.HOLE_DTYPE), []
    for row, w in zip(holes, listed):
        L = len(w)
        words = []
        for i in range(L):
            c = F(0)
            for k in range(2, L - 1):
                d = pos32[w[(i + k) % L]] - pos32[w[i]]
                c = F(c + F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
            words.append((int(np.array([c], F).view(np.uint32)[0]), w[i], i))
        i = min(words)[2]
        status = fr.FILLED
        if any((min(w[i], w[(i + k) % L]), max(w[i], w[(i + k) % L])) in pairs for k in range(2, L - 1)):
            status = fr.DIAGONAL
        elif any(brute_filter(pos32[[w[i], w[(i + k) % L], w[(i + k + 1) % L]]], nrm32[[w[i], w[(i + k) % L], w[(i + k + 1) % L]]], cmin, cmax) != 1
                 for k in range(1, L - 1)):
            status = fr.FILTER
        row["label"], row["n_edges"], row["status"] = w[0], L, status
        if status == fr.FILLED:
            for k in range(1, L - 1):
                t = [w[i], w[(i + k) % L], w[(i + k + 1) % L]]
                m = t.index(min(t))
                new.append(tuple(t[m:] + t[:m]))
    st["n_listed_loops"] = len(listed)
    st["n_filled_loops"], st["n_rejected_diagonal"], st["n_rejected_filter"] = (int(np.sum(holes["status"] == s)) for s in (1, 2, 3))
    st["n_new_triangles"], st["n_triangles"] = len(new), len(R) + len(new)
    return np.array(R + sorted(new), np.uint32).reshape(-1, 3), len(R), holes, st


def both(pos, nrm, r2, tri, what, **p):
    out, kept, holes, st = fr.fill(pos, nrm, r2, tri, **p)
    bout, bkept, bholes, bst = brute(pos, nrm, r2, tri, **p)
    print("%s %s: %s; listed loop lengths %s" % (what, p, st, np.bincount(holes["n_edges"], minlength=4)[3:].tolist()))
    assert st == bst and kept == bkept and out.tobytes() == bout.tobytes() and holes.tobytes() == bholes.tobytes(), what
    fr.check_properties(pos, nrm, r2, tri, out, kept, holes, st, **p)
    return out, kept, holes, st


def soup(seed, n=200, T=300):
    """Random triples (some with a repeated corner, some twice), open tetrahedra with outward normals, dead slots."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1, 1, (n, 3)).astype(F).astype(np.float64)
    nrm = rng.standard_normal((n, 3))
    first = 140                                            # slots 140 .. 199: fifteen tetrahedra with one face missing
    tets = []
    for k in range(15):
        q = rng.permutation(4) + first + 4 * k
        c = pos[q].mean(axis=0)
        nrm[q] = pos[q] - c
        faces = [[q[0], q[1], q[2]], [q[0], q[3], q[1]], [q[0], q[2], q[3]], [q[1], q[3], q[2]]]
        P = pos[q]
        if np.dot(np.cross(P[1] - P[0], P[2] - P[0]), P[0] - c) < 0:
            faces = [[f[0], f[2], f[1]] for f in faces]
        tets += faces[:3]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(F).astype(np.float64)
    tri = rng.integers(0, first, (T - len(tets), 3))
    tri[::17, 1] = tri[::17, 0]                            # a repeated corner
    tri[5::40] = tri[4::40][:tri[5::40].shape[0]]          # the same triangle twice
    tri = np.concatenate([tri, np.array(tets)]).astype(np.uint32)
    tri = tri[rng.permutation(tri.shape[0])]
    r2 = np.ones(n)
    r2[rng.choice(n, 12, replace=False)] = -1.0
    pos[rng.choice(n, 3, replace=False), 1] = np.nan
    return pos, nrm, r2, tri


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_soups(seed):
    pos, nrm, r2, tri = soup(seed)
    _, _, holes, st = both(pos, nrm, r2, tri, "soup %d" % seed)
    assert st["n_not_live"] > 0 and st["n_nonmanifold_edges"] > 0 and st["n_pinched_vertices"] > 0
    assert st["n_listed_loops"] >= 5 and st["n_filled_loops"] >= 1
    both(pos, nrm, r2, tri, "soup %d" % seed, max_hole_edges=3, min_triangle_angle_deg=0.0, max_triangle_angle_deg=180.0)


@pytest.mark.parametrize("case", fc.cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, pos, nrm, r2, tri, expect = case
    out, kept, holes, st = both(pos, nrm, r2, tri, name)
    for k, v in expect.items():
        assert st[k] == v, (name, k, st[k], v)


def test_deleted_triangle_comes_back_and_a_fan_leaves_its_vertex_unused():
    pos, nrm, r2, tri = fc.plane()
    one = int(fc.triangles_at(tri, fc.slot(20, 20))[0])
    out, kept, holes, st = both(pos, nrm, r2, np.delete(tri, one, axis=0), "one triangle deleted")
    assert kept == tri.shape[0] - 1 and out[kept:].tolist() == [tri[one].tolist()]     # (the sheet's triangles start at their smallest index)
    assert mr.as_set(out) == mr.as_set(tri) and holes["n_edges"].tolist() == [3]
    for d, xy in {4: (11, 8), 8: (9, 8)}.items():
        v = fc.slot(*xy)
        assert fc.triangles_at(tri, v).size == d
        out, kept, holes, st = both(pos, nrm, r2, fc.without_vertices(tri, [v]), "fan of degree %d" % d)
        assert holes["n_edges"].tolist() == [d] and st["n_new_triangles"] == d - 2 and not np.any(out == v)


def test_the_cap_on_the_loop_length():
    pos, nrm, r2, tri = fc.plane()
    by_name = {c[0]: c for c in fc.cases()}
    for L, cap, listed in ((8, 8, 1), (9, 8, 0), (9, 9, 1), (32, 32, 1), (33, 32, 0), (32, 31, 0)):
        _, _, _, _, t, _ = by_name["hole of %d edges" % L]
        _, _, holes, st = both(pos, nrm, r2, t, "hole of %d edges" % L, max_hole_edges=cap, min_triangle_angle_deg=1.0, max_triangle_angle_deg=179.0)
        assert st["n_listed_loops"] == listed and holes["n_edges"].tolist() == [L] * listed
    for bad in (dict(max_hole_edges=2), dict(max_hole_edges=33), dict(min_triangle_angle_deg=-1.0), dict(max_triangle_angle_deg=181.0),
                dict(min_triangle_angle_deg=20.0, max_triangle_angle_deg=20.0), dict(min_triangle_angle_deg=float("nan"))):
        with pytest.raises(ValueError):
            fr.fill(pos, nrm, r2, tri, **bad)
    with pytest.raises(ValueError):
        fr.fill(pos, nrm, r2, np.array([[0, 1, pos.shape[0]]], np.uint32))


def test_a_tie_goes_to_the_lower_slot():
    pos, nrm, r2, tri = fc.hexagon_map()
    out, kept, holes, st = both(pos, nrm, r2, tri, "hexagon")
    assert holes["label"].tolist() == [0, 1] and holes["status"].tolist() == [fr.FILTER, fr.FILLED]
    # cost 42 at slots 7 (2, 0) and 1 (-2, 0), 49 at the other four: the fan starts at slot 1
    assert np.all(out[kept:, 0] == 1) and out[kept:].shape[0] == 4


def test_the_holed_plane_reaches_every_status():
    pos, nrm, r2, tri = fc.holed_plane()
    for p in (dict(), dict(max_hole_edges=32), dict(min_triangle_angle_deg=1.0, max_triangle_angle_deg=179.0), dict(max_hole_edges=4)):
        _, _, holes, st = both(pos, nrm, r2, tri, "holed plane", **p)
        assert st["n_not_live"] > 0 and st["n_nonmanifold_edges"] == 1 and st["n_pinched_vertices"] >= 3
        assert st["n_filled_loops"] >= 1 and st["n_rejected_diagonal"] == 1 and st["n_rejected_filter"] >= 2


def test_sphere_with_the_defaults():
    pos, nrm, r2 = mr.sphere_map()
    tri = mr.triangulate(pos, nrm, r2)[0]
    _, _, holes, st = both(pos, nrm, r2, tri, "sphere")
    assert st["n_in"] == 6739 and st["n_boundary_edges"] == 2129
    assert st["n_listed_loops"] >= 100 and st["n_filled_loops"] >= 30
    shuffled = tri[np.random.default_rng(2).permutation(tri.shape[0])][::-1]
    out2, kept2, holes2, st2 = both(pos, nrm, r2, shuffled, "sphere, shuffled and reversed")
    out, kept, _, _ = fr.fill(pos, nrm, r2, tri)
    assert holes2.tobytes() == holes.tobytes() and out2[kept2:].tobytes() == out[kept:].tobytes() and np.array_equal(out2[:kept2], shuffled)
