"""The model of smx_recon_mesh_rim (include/smx.h), shared by the model, host, API and GPU tests.

The definition is made of integers: R is distance_ref.classify's, c(u, v) comes from np.unique over the sorted index pairs of
R, an edge is a rim edge iff c == 1, a slot a rim vertex iff it ends one, and the byte of a triangle has bit k set for region k
of smx_recon_mesh_distance (A, B, AB, C, AC, BC).  rim() says that with array operations; rim_slow() says it again with a
dictionary and loops, so that the two cannot share a mistake.  cases() holds the hand-made arrays."""
import functools

import numpy as np

import decimate_cases as dc
import distance_ref as dr
import fill_cases as fc
import register_ref as rr

STAT_NAMES = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_edges", "n_rim_edges", "n_nonmanifold_edges", "n_rim_vertices",
              "n_rim_triangles")
BIT_A, BIT_B, BIT_AB, BIT_C, BIT_AC, BIT_BC = (1 << k for k in range(6))
# (first corner, second corner, bit) of the three edges; the corners' bits by column of the triangle
EDGES = ((0, 1, BIT_AB), (0, 2, BIT_AC), (1, 2, BIT_BC))
CORNER_BITS = (BIT_A, BIT_B, BIT_C)


def rim(pos, r2, tri):
    """(bytes [n_in] uint8, dict of smx_rim_stats).  ValueError on an index >= n."""
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    R, t, counts = dr.classify(pos, r2, tri)
    out = np.zeros(tri.shape[0], np.uint8)
    st = dict(counts, n_edges=0, n_rim_edges=0, n_nonmanifold_edges=0, n_rim_vertices=0, n_rim_triangles=0)
    if R.shape[0] == 0:
        return out, st
    idx = R.astype(np.uint64)
    keys = np.stack([(np.minimum(idx[:, a], idx[:, b]) << np.uint64(32)) | np.maximum(idx[:, a], idx[:, b]) for a, b, _ in EDGES], axis=1)
    uniq, inverse, c = np.unique(keys.reshape(-1), return_inverse=True, return_counts=True)
    on_rim = (c[inverse] == 1).reshape(-1, 3)
    rim_keys = uniq[c == 1]
    is_vertex = np.zeros(np.asarray(pos).shape[0], bool)
    is_vertex[(rim_keys >> np.uint64(32)).astype(np.int64)] = True
    is_vertex[(rim_keys & np.uint64(0xFFFFFFFF)).astype(np.int64)] = True
    byte = np.zeros(R.shape[0], np.uint8)
    for k, (_, _, bit) in enumerate(EDGES):
        byte |= np.where(on_rim[:, k], bit, 0).astype(np.uint8)
    for k, bit in enumerate(CORNER_BITS):
        byte |= np.where(is_vertex[R[:, k].astype(np.int64)], bit, 0).astype(np.uint8)
    out[t] = byte
    st.update(n_edges=int(uniq.size), n_rim_edges=int(np.sum(c == 1)), n_nonmanifold_edges=int(np.sum(c >= 3)),
              n_rim_vertices=int(np.sum(is_vertex)), n_rim_triangles=int(np.sum(out != 0)))
    return out, st


def rim_slow(pos, r2, tri):
    """The same answer from a dictionary of pairs, one triangle at a time."""
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    R, t, counts = dr.classify(pos, r2, tri)
    c = {}
    for row in R.tolist():
        for a, b, _ in EDGES:
            e = frozenset((row[a], row[b]))
            c[e] = c.get(e, 0) + 1
    vertices = set()
    for e, k in c.items():
        if k == 1:
            vertices |= e
    out = np.zeros(tri.shape[0], np.uint8)
    for row, at in zip(R.tolist(), t.tolist()):
        byte = 0
        for a, b, bit in EDGES:
            if c[frozenset((row[a], row[b]))] == 1:
                byte |= bit
        for k, bit in enumerate(CORNER_BITS):
            if row[k] in vertices:
                byte |= bit
        out[at] = byte
    st = dict(counts, n_edges=len(c), n_rim_edges=sum(1 for k in c.values() if k == 1), n_nonmanifold_edges=sum(1 for k in c.values() if k >= 3),
              n_rim_vertices=len(vertices), n_rim_triangles=int(np.sum(out != 0)))
    return out, st


def hit(byte, region):
    """"The closest point lies on the rim": region as distance_ref.REGIONS numbers it."""
    return bool((int(byte) >> int(region)) & 1)


# ---- cases --------------------------------------------------------------------------------------------------------------------
SIDE = 20
DEAD, FAR, NAN = SIDE * SIDE, SIDE * SIDE + 1, SIDE * SIDE + 2           # slots beside the grid
N_SLOTS = SIDE * SIDE + 3


def slot(x, y):
    return y * SIDE + x


@functools.lru_cache(maxsize=None)
def grid_map():
    """(pos, r2): a 20 x 20 grid of live slots at unit spacing, then a dead slot, a slot at 65 m and a slot at NaN.  Read-only."""
    gx, gy = np.meshgrid(np.arange(SIDE, dtype=np.float64), np.arange(SIDE, dtype=np.float64))
    pos = np.stack([gx.ravel(), gy.ravel(), np.zeros(SIDE * SIDE)], axis=1)
    pos = np.concatenate([pos, np.array([[3.0, -2.0, 0.0], [65.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])])
    r2 = np.ones(N_SLOTS)
    r2[DEAD] = -1.0
    pos.setflags(write=False)
    r2.setflags(write=False)
    return pos, r2


@functools.lru_cache(maxsize=None)
def grid_triangles():
    """Two triangles per square of the grid, row by row: 722, wound counter-clockwise.  Read-only."""
    out = []
    for y in range(SIDE - 1):
        for x in range(SIDE - 1):
            a, b, c, d = slot(x, y), slot(x + 1, y), slot(x + 1, y + 1), slot(x, y + 1)
            out += [[a, b, c], [a, c, d]]
    t = np.array(out, np.uint32)
    t.setflags(write=False)
    return t


def _wrap_array(n_in_total):
    """Triangles over the grid's slots of which two pairs hash to the LAST entry of the table an array of n_in_total triangles
    gets: the second one's probe chain wraps to entry 0.  Returns None if the grid holds no two such pairs."""
    mask = dc.dec_table_size(3 * n_in_total) - 1
    last = [(u, v) for u in range(SIDE * SIDE) for v in range(u + 1, SIDE * SIDE) if dc.dec_hash((u << 32) | v, mask) == mask]
    if len(last) < 2:
        return None, mask
    tris, used = [], set()
    for u, v in last[:3]:
        w = next(k for k in range(SIDE * SIDE) if k not in (u, v) and k not in used)
        used.add(w)
        tris.append([u, v, w])
    return np.array(tris, np.uint32), mask


def cases():
    """[(name, pos, r2, triangles, expect)]: expect = the bytes (a list, or None) and statistics the case is built to give."""
    pos, r2 = grid_map()
    g = grid_triangles()
    out = []

    def add(name, t, bytes_=None, **expect):
        out.append((name, pos, r2, np.ascontiguousarray(np.asarray(t, np.uint32).reshape(-1, 3)), bytes_, expect))

    add("one triangle", [[0, 1, 20]], [0x3F], n_edges=3, n_rim_edges=3, n_rim_vertices=3, n_rim_triangles=1)
    add("two triangles sharing an edge", [[0, 1, 20], [1, 21, 20]], [0x1F, 0x2F], n_edges=5, n_rim_edges=4, n_rim_vertices=4)
    add("a closed tetrahedron", fc.tetrahedron(0, 1, 20, 21), [0, 0, 0, 0], n_edges=6, n_rim_edges=0, n_rim_vertices=0, n_rim_triangles=0)
    add("a triangle given twice", [[0, 1, 20], [0, 1, 20]], [0, 0], n_edges=3, n_rim_edges=0, n_nonmanifold_edges=0)
    add("a triangle and its mirror image", [[0, 1, 20], [1, 0, 20]], [0, 0], n_edges=3, n_rim_edges=0)
    # {0, 1} has three triangles: not a rim edge, but 0 and 1 end the rim edges towards 20, 40 and 60
    add("three triangles on one edge", [[0, 1, 20], [1, 0, 40], [0, 1, 60]], [0x3B, 0x3B, 0x3B], n_edges=7, n_rim_edges=6, n_nonmanifold_edges=1,
        n_rim_vertices=5)
    add("a bow-tie", [[0, 1, 20], [1, 2, 22]], [0x3F, 0x3F], n_edges=6, n_rim_edges=6, n_rim_vertices=5)
    # a fan closed around slot 21: its centre is no rim vertex, the spokes are interior, the outer edges are rim
    ring = [0, 1, 2, 22, 42, 41, 40, 20]
    fan = [[21, ring[k], ring[(k + 1) % 8]] for k in range(8)]
    add("a closed fan", fan, [0x2A] * 8, n_edges=16, n_rim_edges=8, n_rim_vertices=8)
    # an open fan: the centre ends the two open spokes
    add("an open fan", fan[:5], [0x2F] + [0x2B] * 3 + [0x3B], n_rim_edges=7, n_rim_vertices=7)
    # a corner bit without an edge bit of its own: the middle one of four triangles has three interior edges, and every corner
    # of it ends a rim edge of a neighbour
    add("a triangle inside three others", [[1, 21, 20], [0, 1, 20], [1, 2, 21], [20, 21, 40]], [0x0B, 0x1F, 0x2F, 0x3B], n_edges=9, n_rim_edges=6,
        n_rim_vertices=6, n_rim_triangles=4)
    drops = np.array([[0, 1, DEAD], [0, 0, 1], [1, 20, 1], [20, 20, 20], [0, 1, FAR], [0, 1, NAN], [DEAD, DEAD, 1], [FAR, FAR, 1], [0, 1, 20],
                      [1, 21, 20]], np.uint32)
    add("dead, repeated and far corners", drops, [0] * 8 + [0x1F, 0x2F], n_not_live=3, n_repeated=4, n_out_of_range=1, n_edges=5, n_rim_edges=4)
    for m in (255, 256, 257):
        add("the first %d triangles of the grid" % m, g[:m])
    add("the grid", g, n_edges=3 * 19 * 19 + 2 * 19, n_rim_edges=4 * 19, n_nonmanifold_edges=0, n_rim_vertices=4 * 19)
    hole = fc_without(g, [slot(5, 5), slot(6, 5), slot(12, 9)])
    add("the grid with two holes", hole, n_rim_edges=4 * 19 + 8 + 6, n_rim_vertices=4 * 19 + 8 + 6)
    add("the grid shuffled, with the drops", np.concatenate([hole, drops])[np.random.default_rng(4).permutation(hole.shape[0] + drops.shape[0])],
        n_not_live=3, n_repeated=4, n_out_of_range=1)
    wrap, _ = _wrap_array(3)
    assert wrap is not None and wrap.shape[0] == 3
    add("pairs that hash to the table's last entry", wrap)
    cp, _, cr2, ct = rr.corner()
    out.append(("corner()", cp, cr2, ct, None, dict(n_rim_edges=3 * 4 * 23, n_rim_vertices=3 * 4 * 23, n_nonmanifold_edges=0)))
    return out


def fc_without(tri, slots):
    return np.ascontiguousarray(fc.without_vertices(tri, slots), np.uint32)


def refused():
    """Arrays with an index >= n, at the start, in the middle and at the end."""
    pos, r2 = grid_map()
    g = grid_triangles()
    out = []
    for where in (0, 3 * 300 + 1, 3 * g.shape[0] - 1):
        bad = g.copy()
        bad.reshape(-1)[where] = N_SLOTS
        out.append((pos, r2, bad))
    out.append((pos, r2, np.array([[0, 1, 0xFFFFFFFF]], np.uint32)))
    return out
