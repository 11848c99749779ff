"""Hand cases for smx_recon_fill_holes, shared by the model, host and GPU tests: the 40 x 40 plane of mesh_ref.plane_map()
with holes punched into it, plus a few spare slots beside it for the triangles that belong to no sheet.

Every case is (name, pos, nrm, r2, triangles, expect) with expect a dict of statistics the case is built to give (checked
by the model test against the model AND the brute-force version, so a case cannot silently stop reaching its branch)."""
import functools

import numpy as np

import mesh_ref as mr

SIDE = 40
SPARE = 24            # slots 1600 .. 1623: off the sheet, used by islands, tetrahedra and the third triangle of an edge


@functools.lru_cache(maxsize=None)
def _plane():
    pos, nrm, r2 = mr.plane_map(SIDE)
    tri = mr.triangulate(pos, nrm, r2)[0]
    k = np.arange(SPARE, dtype=np.float64)
    spare = np.stack([60.0 + 3.0 * (k % 6), 3.0 * (k // 6) + 0.25 * (k % 2), np.zeros(SPARE)], axis=1)
    pos = np.concatenate([pos, spare])
    nrm = np.concatenate([nrm, np.tile(np.array([0.0, 0.0, 1.0]), (SPARE, 1))])
    r2 = np.concatenate([r2, np.full(SPARE, r2[0])])
    for a in (pos, nrm, r2, tri):
        a.setflags(write=False)
    return pos, nrm, r2, tri


def plane():
    """(pos, nrm, r2, triangles) -- read-only; the triangles are those of the sheet alone (3 060, 138 boundary edges)."""
    return _plane()


def slot(x, y):
    return y * SIDE + x


def without_vertices(tri, slots):
    """The array without every triangle that has a corner in `slots`: the fans of those vertices deleted."""
    return tri[~np.isin(tri, np.asarray(list(slots))).any(axis=1)]


def block(x0, y0, a, b):
    return [slot(x0 + i, y0 + j) for i in range(a) for j in range(b)]


def triangles_at(tri, v):
    return np.flatnonzero((tri == v).any(axis=1))


def tetrahedron(a, b, x, y):
    """A closed surface through the edge {a, b}: every pair interior, so a and b gain no gap."""
    return np.array([[a, b, x], [a, y, b], [a, x, y], [b, y, x]], np.uint32)


def hexagon_map():
    """A planar ring of 12 triangles around a hexagonal hole with small-integer coordinates: the costs of opposite apexes are
    equal exactly.  Inner slots 7, 3, 9, 1, 5, 11 counter-clockwise, outer slots the even ones and 13."""
    inner = np.array([[2, 0], [1, 2], [-1, 2], [-2, 0], [-1, -2], [1, -2]], np.float64)
    pos = np.zeros((14, 3))
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (14, 1))
    islots, oslots = [7, 3, 9, 1, 5, 11], [0, 2, 4, 6, 8, 13]
    pos[islots, :2] = inner
    pos[oslots, :2] = 3.0 * inner
    pos[[10, 12], :2] = [[40, 40], [41, 40]]          # unused slots
    tri = []
    for k in range(6):
        i0, i1, o0, o1 = islots[k], islots[(k + 1) % 6], oslots[k], oslots[(k + 1) % 6]
        tri += [[i0, o0, o1], [i0, o1, i1]]           # counter-clockwise seen from +z
    return pos, nrm, np.ones(14), np.array(tri, np.uint32)


def cases():
    pos, nrm, r2, tri = plane()
    S = SIDE * SIDE
    out = []

    def add(name, t, expect, r2_=None):
        out.append((name, pos, nrm, r2 if r2_ is None else r2_, np.ascontiguousarray(t, np.uint32), expect))

    add("untouched plane", tri, dict(n_boundary_edges=138, n_listed_loops=0, n_new_triangles=0, n_pinched_vertices=0))
    # one interior triangle deleted
    one = int(triangles_at(tri, slot(20, 20))[0])
    add("one triangle deleted", np.delete(tri, one, axis=0), dict(n_listed_loops=1, n_filled_loops=1, n_new_triangles=1, n_boundary_edges=141))
    # whole fans of interior vertices of degree 4 .. 8
    for d, (x, y) in {4: (11, 8), 5: (5, 15), 6: (5, 8), 7: (6, 15), 8: (9, 8)}.items():
        add("fan of degree %d deleted" % d, without_vertices(tri, [slot(x, y)]),
            dict(n_listed_loops=1, n_filled_loops=1, n_new_triangles=d - 2, n_boundary_edges=138 + d))
    # holes of exactly max_hole_edges and one more (the test runs them with max_hole_edges 8 and 32)
    add("hole of 8 edges", without_vertices(tri, block(5, 8, 1, 2)), dict(n_boundary_edges=138 + 8, n_pinched_vertices=0))
    add("hole of 9 edges", without_vertices(tri, block(8, 15, 1, 2)), dict(n_boundary_edges=138 + 9, n_pinched_vertices=0))
    add("hole of 32 edges", without_vertices(tri, block(17, 8, 3, 11)), dict(n_boundary_edges=138 + 32, n_pinched_vertices=0))
    add("hole of 33 edges", without_vertices(tri, block(7, 8, 4, 11)), dict(n_boundary_edges=138 + 33, n_pinched_vertices=0))
    # two 3-holes that share one vertex
    v = slot(11, 8)                                   # degree 4: its first and third triangle around share v only
    fan = triangles_at(tri, v)
    pair = next((int(a), int(b)) for a in fan for b in fan if a < b and np.intersect1d(tri[a], tri[b]).size == 1)
    add("two holes that touch", np.delete(tri, pair, axis=0), dict(n_pinched_vertices=1, n_listed_loops=0, n_new_triangles=0, n_boundary_edges=144))
    # islands: a triangle and a strip of two on spare slots, far from the sheet
    isl = np.array([[S, S + 1, S + 6], [S + 3, S + 4, S + 9], [S + 4, S + 10, S + 9]], np.uint32)
    add("islands", np.concatenate([tri, isl]), dict(n_listed_loops=2, n_rejected_filter=2, n_new_triangles=0, n_boundary_edges=138 + 7))
    # a 4-hole whose two diagonals both exist elsewhere: tetrahedra over spare slots
    four = without_vertices(tri, [slot(11, 8)])
    ring = np.setdiff1d(np.unique(tri[triangles_at(tri, slot(11, 8))]), [slot(11, 8)])
    centre = pos[slot(11, 8)]
    ang = np.arctan2(pos[ring, 1] - centre[1], pos[ring, 0] - centre[0])
    w = ring[np.argsort(ang)]
    tets = np.concatenate([tetrahedron(w[0], w[2], S + 12, S + 13), tetrahedron(w[1], w[3], S + 14, S + 15)])
    add("diagonal taken", np.concatenate([four, tets]), dict(n_listed_loops=1, n_rejected_diagonal=1, n_new_triangles=0, n_pinched_vertices=0))
    # an interior edge with a third triangle
    e = tri[int(triangles_at(tri, slot(30, 30))[0])]
    add("edge with three triangles", np.concatenate([tri, np.array([[e[0], e[1], S + 20]], np.uint32)]),
        dict(n_nonmanifold_edges=1, n_boundary_edges=140, n_pinched_vertices=2, n_listed_loops=0))
    # the same triangle twice: three pairs with two half-edges in one direction
    add("a triangle twice", np.concatenate([tri, tri[one:one + 1]]), dict(n_nonmanifold_edges=3, n_boundary_edges=138, n_listed_loops=0))
    # a dead corner on the rim of a hole: its fan goes as well
    rim = int(np.setdiff1d(np.unique(tri[triangles_at(tri, slot(5, 15))]), [slot(5, 15)])[0])
    dead = r2.copy()
    dead[rim] = -1.0
    add("dead corner on a rim", without_vertices(tri, [slot(5, 15)]), dict(n_not_live=int(triangles_at(without_vertices(tri, [slot(5, 15)]), rim).size)), dead)
    # several holes at once, shuffled
    many = without_vertices(tri, [slot(x, y) for x in range(4, 36, 4) for y in range(4, 36, 4)])
    add("a hole at every fourth vertex, shuffled", many[np.random.default_rng(3).permutation(many.shape[0])], dict(n_listed_loops=64, n_pinched_vertices=0))
    hp, hn, hr, ht = hexagon_map()
    out.append(("hexagon with tied costs", hp, hn, hr, ht, dict(n_listed_loops=2, n_filled_loops=1, n_rejected_filter=1, n_new_triangles=4)))
    return out


def holed_plane():
    """The sheet with every hole of the hand cases that fits beside the others, and the off-sheet triangles: one array that
    reaches every branch (used where one call has to cover them all)."""
    pos, nrm, r2, tri = plane()
    S = SIDE * SIDE
    gone = [slot(11, 8), slot(5, 15), slot(9, 15), slot(25, 30), slot(30, 5)] + block(17, 12, 3, 11) + block(30, 20, 4, 11) + block(5, 25, 1, 2)
    t = without_vertices(tri, gone)
    t = np.delete(t, int(triangles_at(t, slot(36, 36))[0]), axis=0)
    v = slot(3, 3)
    fan = triangles_at(t, v)
    pair = next((int(a), int(b)) for a in fan for b in fan if a < b and np.intersect1d(t[a], t[b]).size == 1)
    t = np.delete(t, pair, axis=0)
    ring = np.setdiff1d(np.unique(tri[triangles_at(tri, slot(11, 8))]), [slot(11, 8)])
    centre = pos[slot(11, 8)]
    w = ring[np.argsort(np.arctan2(pos[ring, 1] - centre[1], pos[ring, 0] - centre[0]))]
    e = tri[int(triangles_at(tri, slot(36, 10))[0])]
    extra = np.concatenate([np.array([[S, S + 1, S + 6], [S + 3, S + 4, S + 9], [S + 4, S + 10, S + 9], [e[0], e[1], S + 20]], np.uint32),
                            tetrahedron(w[0], w[2], S + 12, S + 13), tetrahedron(w[1], w[3], S + 14, S + 15)])
    dead = r2.copy()
    dead[slot(20, 35)] = -1.0
    return pos, nrm, dead, np.ascontiguousarray(np.concatenate([t, extra]), np.uint32)
