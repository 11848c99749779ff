"""Hand-built maps and triangle arrays that put smx_recon_decimate_mesh where its cell arithmetic, its tie,
its key fields, its range rule, its two open-addressing tables and its sort widths decide.  Shared by
tests/test_decimate_cases.py (model = brute force = host walk, census, mutants) and tests/test_gpu_decimate_cases.py (the
device against the same model).  No case calls the triangulation: the arrays are written here.

A case is a map (pos float32 [n, 3], normal, r2) with a cell size, one or more triangle arrays that the call accepts
(`arrays`), arrays it has to refuse (`refused`) and what can be said about the result by hand (`expect`: per array, entries
of the statistics, of the vertex map, or the whole output).  Cell sizes are powers of two wherever a position has to sit
exactly on a face or exactly mirrored about a centre: inv and the centres are exact then.

The module also restates dec_hash, dec_tri_hash, dec_table_size, the cell key and the `bits` rule of smx_decimate.hpp in
Python integers; the searches below use the restatements, and tests/test_decimate_cases.py holds them to the header."""
import functools
import itertools

import numpy as np

import decimate_ref as dr

F = np.float32
INV = 0xFFFFFFFF
M64 = (1 << 64) - 1
LIMIT = 1 << 20


# ---- the header's integer functions, restated ---------------------------------------------------------------------------------
def dec_hash(k, mask):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return (k & 0xFFFFFFFF) & mask


def dec_cell_key(cx, cy, cz):
    return ((cx + LIMIT) << 42) | ((cy + LIMIT) << 21) | (cz + LIMIT)


def dec_tri_hash(p, a, b, mask):
    lo, hi = min(a, b), max(a, b)
    return dec_hash(((p << 42) ^ (lo << 21) ^ hi ^ (hi << 50)) & M64, mask)


def dec_table_size(entries):
    s = 64
    while s < 0x80000000 and s < 2 * entries:
        s <<= 1
    return s


def sort_bits(n):
    """Bit length of the largest slot index n - 1 (32-bit arithmetic), at least 1."""
    bits = 1
    while bits < 32 and (((n - 1) & 0xFFFFFFFF) >> bits) != 0:
        bits += 1
    return bits


def sort_passes(n):
    """8-bit passes of the two radix sorts: by (a, b) on 2 bits, then by p on bits."""
    bits = sort_bits(n)
    return (2 * bits + 7) // 8, (bits + 7) // 8


def table_sizes(n, n_in):
    """(entries of the cell table, entries of the triangle table) of a call."""
    return dec_table_size(min(n, 3 * n_in)), dec_table_size(n_in)


# ---- cases --------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, pos, r2, cell, arrays, refused=(), expect=None, notes=None):
        self.name, self.group = name, name.split("/")[0]
        self.pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
        n = self.pos.shape[0]
        self.r2 = np.ones(n, F) if r2 is None else np.ascontiguousarray(r2, F)
        self.nrm = np.tile(np.array([0, 0, 1], F), (n, 1))
        self.cell = float(cell)
        self.arrays = [(label, np.ascontiguousarray(t, np.uint32).reshape(-1, 3)) for label, t in arrays]
        self.refused = [(label, np.ascontiguousarray(t, np.uint32).reshape(-1, 3)) for label, t in refused]
        self.expect = expect or {}
        self.notes = notes or {}

    @property
    def n(self):
        return self.pos.shape[0]

    def map(self):
        return self.pos, self.nrm, self.r2

    def __repr__(self):
        return "Case(%s)" % self.name


class _Builder:
    """Vertices and triangles by hand.  far(): a vertex in a cell of its own that nothing else comes near;
    lonely(v): a triangle of v with two fresh far corners, so that it goes only if the rule under test says so."""

    def __init__(self, cell, far_at=1000):
        self.cell, self.pos, self.r2, self.tri, self._far = F(cell), [], [], [], far_at

    def add(self, x, y, z, r2=1.0):
        self.pos.append((x, y, z))
        self.r2.append(r2)
        return len(self.pos) - 1

    def far(self):
        self._far += 2
        return self.add((F(self._far) + F(0.5)) * self.cell, F(7.5) * self.cell, F(7.5) * self.cell)

    def lonely(self, v):
        self.tri.append((v, self.far(), self.far()))

    def case(self, name, arrays=None, **kw):
        return Case(name, np.array(self.pos, F), np.array(self.r2, F), self.cell, arrays or [("all", self.tri)], **kw)


def _below(v):
    return np.nextafter(F(v), F(-np.inf))


def _faces():
    b = _Builder(0.25)
    vmap, cells = {}, 0
    for axis in range(3):
        on, below = {}, {}
        for k in (-2, -1, 0, 1):
            for v, into in ((F(k) * F(0.25), on), (_below(F(k) * F(0.25)), below)):
                p = [(F(10 * (axis + 1)) + F(0.4)) * F(0.25)] * 3        # (the other two axes: a cell that only this axis uses)
                p[axis] = v
                into[k] = b.add(*p)
                b.lonely(into[k])
        # By hand: the vertex on face k is in cell k, the one below it in cell k - 1, which it shares with the vertex on face
        # k - 1.  That one is 0.125 from the centre on the axis, the one below face k an ulp less: it wins.  Except below face
        # 0: its coordinate, the smallest negative float, leaves the distance at 0.125 after rounding: a tie, the lower slot.
        for k in (-2, -1, 0, 1):
            vmap[below[k]] = below[k]
        vmap[on[1]] = on[1]
        vmap[on[-2]], vmap[on[-1]], vmap[on[0]] = below[-1], on[-1], below[1]
        vmap[below[0]] = on[-1]
        cells += 5                                                       # -3 .. 1
    return b.case("faces", expect={"all": dict(vmap=vmap, n_collapsed=0, n_duplicates=0, n_cells=cells + 2 * 24)})


def _mul_not_div():
    cell = F(0.3)
    inv = F(1.0) / cell
    half = F(0.5) * cell                                  # the centre of cell 0 in both forms: (0 + 0.5) * cell
    # a coordinate that x * inv and x / cell put into different cells
    found = None
    for k in range(1, 4000):
        for step in range(-2, 3):
            x = F(k) * cell
            for _ in range(abs(step)):
                x = np.nextafter(x, F(np.inf) if step > 0 else F(-np.inf))
            if np.floor(x * inv) != np.floor(x / cell):
                found = x
                break
        if found is not None:
            break
    assert found is not None
    c_mul, c_div = int(np.floor(found * inv)), int(np.floor(found / cell))
    assert c_mul != c_div
    # a cell whose centre differs between ((c + 0.5) * cell) and (c * cell + 0.5 * cell), and two points about it that each
    # form gives to the other
    rng = np.random.default_rng(11)
    pair = None
    for c in range(1, 4000):
        ca, cb = (F(c) + F(0.5)) * cell, F(c) * cell + F(0.5) * cell
        if ca == cb or c in (c_mul, c_div):
            continue
        for _ in range(200):
            t = F(rng.uniform(0.05, 0.4)) * cell
            p1, p2 = ca - t, ca + t
            a1, a2, b1, b2 = (p1 - ca) * (p1 - ca), (p2 - ca) * (p2 - ca), (p1 - cb) * (p1 - cb), (p2 - cb) * (p2 - cb)
            if a1 <= a2 and b2 < b1:                       # as written the lower slot p1 wins (nearer, or a tie); distributed, p2
                pair = (c, p1, p2)
                break
        if pair:
            break
    assert pair is not None
    b = _Builder(cell)
    x_edge = b.add(found, half, half)                      # in cell c_mul, on its face
    y_mid = b.add((F(c_mul) + F(0.5)) * cell, half, half)  # the centre of c_mul: wins it
    z_mid = b.add((F(c_div) + F(0.5)) * cell, half, half)  # the centre of c_div: would win x_edge under the division
    p1 = b.add(pair[1], half, half)
    p2 = b.add(pair[2], half, half)
    for v in (x_edge, y_mid, z_mid, p1, p2):
        b.lonely(v)
    return b.case("mul_not_div", expect={"all": dict(vmap={x_edge: y_mid, y_mid: y_mid, z_mid: z_mid, p1: p1, p2: p1})},
                  notes=dict(x=float(found), c_mul=c_mul, c_div=c_div, centre_cell=pair[0], x_edge=x_edge))


D2_FORMS = ("d2_fma_z", "d2_fma_y", "d2_fma_both", "d2_assoc")


def _rounding_decides():
    cell = F(1.0)
    cells = [(0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 0, 0), (-1, -1, 0), (0, 1, 0), (1, 1, -1)]
    b = _Builder(cell)
    vmap, pairs = {}, []
    for k, (form, c) in enumerate(zip(D2_FORMS + D2_FORMS, cells)):
        rng = np.random.default_rng(100 + k)
        c = np.array(c, F)
        x = (c + rng.uniform(0.02, 0.98, (1 << 18, 3)).astype(F)).astype(F)
        assert np.all(np.floor(x) == c)
        d = x - (c + F(0.5)) * cell
        plain, other = dr.d2_of(d[:, 0], d[:, 1], d[:, 2]), dr.d2_of(d[:, 0], d[:, 1], d[:, 2], form)
        order = np.argsort(plain.view(np.uint32), kind="stable")
        w, l = order[:-1], order[1:]
        hit = np.flatnonzero((plain[w] < plain[l]) & (other[w] >= other[l]))
        assert hit.size > 0, form
        w, l = w[hit[0]], l[hit[0]]
        lo = b.add(*x[l])                                  # the farther one as written gets the lower slot, which a tie favours
        hi = b.add(*x[w])
        b.lonely(lo)
        b.lonely(hi)
        vmap[lo], vmap[hi] = hi, hi
        pairs.append((form, lo, hi))
    return b.case("rounding_decides", expect={"all": dict(vmap=vmap)}, notes=dict(pairs=pairs))


TIES_BIG = 4096


def _ties():
    b = _Builder(1.0)
    for _ in range(TIES_BIG):
        b.add(5.25, 0.75, 0.5)                             # slots 0 .. 4095: one position in cell (5, 0, 0)
    m = [b.add(0.75, 0.75, 0.5), b.add(0.25, 0.75, 0.5), b.add(0.25, 0.25, 0.5), b.add(0.75, 0.25, 0.5)]   # mirrored about (0.5, 0.5, 0.5)
    s = [b.add(2.3, 0.6, 0.5), b.add(2.3, 0.6, 0.5)]       # two slots at one position
    g, h = b.add(8.5, 0.5, 0.5), b.add(10.5, 0.5, 0.5)
    last = b.add(5.5, 0.5, 0.5)                            # the centre of the big cell, in the LAST slot
    tri = [(v, g, h) for v in reversed(m)]                 # the lower slot later in the array
    tri += [(s[1], h, g), (s[0], g, h)]
    tri += [(int(i), g, h) for i in np.random.default_rng(5).permutation(TIES_BIG)]
    assert tri[6][0] != 0
    vm = {v: m[0] for v in m}
    vm.update({s[0]: s[0], s[1]: s[0], g: g, h: h})
    vm0, vm1 = dict(vm), dict(vm)
    vm0.update({0: 0, 1: 0, TIES_BIG - 1: 0, last: INV})
    vm1.update({0: last, TIES_BIG - 1: last, last: last})
    out0 = sorted([(0, g, h), (m[0], g, h), (s[0], h, g)])
    out1 = sorted([(m[0], g, h), (s[0], h, g), (g, h, last)])
    return b.case("ties", arrays=[("slot0", tri), ("last", [(last, g, h)] + tri)],
                  expect={"slot0": dict(vmap=vm0, out=out0, n_cells=5), "last": dict(vmap=vm1, out=out1, n_cells=5)},
                  notes=dict(mirrored=m))


def _key_field_cells():
    ext = (-LIMIT, LIMIT - 1)
    cells = []
    for corner in itertools.product(ext, repeat=3):
        cells.append(corner)
        for axis in range(3):
            inward, partner = list(corner), list(corner)
            inward[axis] += 1 if corner[axis] < 0 else -1                 # bit 0 of the field
            partner[axis] = 0 if corner[axis] < 0 else -1                 # bit 20 of the field
            cells += [tuple(inward), tuple(partner)]
    assert len(set(cells)) == len(cells) == 56
    return cells


def _key_fields():
    b = _Builder(1.0)
    cells = _key_field_cells()
    for c in cells:
        b.lonely(b.add(*(F(v) + F(0.5) for v in c)))
    n = len(b.pos)
    return b.case("key_fields", expect={"all": dict(vmap={i: i for i in range(n)}, n_cells=n, n_triangles=len(cells))}, notes=dict(cells=cells))


def _range_edges():
    b = _Builder(1.0)
    hi, lo = np.nextafter(F(LIMIT), F(0)), F(-LIMIT)       # c = 2^20 - 1 and c = -2^20
    over, under = F(LIMIT), _below(F(-LIMIT))              # c = 2^20 and c = -2^20 - 1
    g, h = b.far(), b.far()

    def on_axes(v):
        out = []
        for axis in range(3):
            p = [F(0.5)] * 3
            p[axis] = v
            out.append(b.add(*p))
        return out
    his, los = on_axes(hi), on_axes(lo)
    p = [F(0.5)] * 3
    p[1] = over
    v_over = b.add(*p)
    p = [F(0.5)] * 3
    p[2] = under
    v_under = b.add(*p)
    t_hi = [(v, g, h) for v in his] + [tuple(his)]
    t_lo = [(v, h, g) for v in los] + [tuple(los)]
    return b.case("range_edges", arrays=[("accept_hi", t_hi), ("accept_lo", t_lo)],
                  refused=[("refuse_hi", t_hi + [(v_over, g, h)]), ("refuse_lo", [(v_under, g, h)] + t_lo)],
                  expect={"accept_hi": dict(n_triangles=4, n_cells=5), "accept_lo": dict(n_triangles=4, n_cells=5)},
                  notes=dict(hi=float(hi), lo=float(lo), over=float(over), under=float(under)))


def _huge_cell():
    cell = F(1e38)
    mags = (F(1.0), F(0.5), F(3e5))
    pos = []
    for j in range(3):
        for s in range(8):                                  # slot = 8 j + s: the lowest slot of sign cell s is s
            pos.append([(-1 if (s >> a) & 1 else 1) * mags[(j + a) % 3] for a in range(3)])
    pos += [[F(0.0), F(1.0), F(1.0)], [F(-0.0), F(1.0), F(1.0)]]        # slots 24, 25: +0 and -0 both floor to cell 0
    v = lambda s, j: 8 * (j % 3) + (s % 8)
    tri = [(v(s, j), v(s + 1, j + 1), v(s + 3, j + 2)) for j in range(3) for s in range(8)]
    tri += [(24, v(1, 0), v(3, 1)), (v(3, 2), 25, v(1, 1))]
    vmap = {8 * j + s: s for j in range(3) for s in range(8)}
    vmap.update({24: 0, 25: 0})
    return Case("huge_cell", np.array(pos, F), None, cell, [("all", tri)],
                expect={"all": dict(vmap=vmap, n_cells=8, n_used_vertices=26, n_triangles=8, n_collapsed=0)})


def _cell_table_wrap():
    cell = F(0.25)
    starts = []
    for cx, cy in itertools.product(range(64), range(8)):
        if dec_hash(dec_cell_key(cx, cy, 0), 63) >= 62:
            starts.append((cx, cy, 0))
        if len(starts) == 10:
            break
    assert len(starts) == 10
    rng = np.random.default_rng(21)
    pos = []
    for j in range(3):
        for c in starts:                                    # slot = 10 j + cell: neighbouring lanes carry different keys
            pos.append((np.array(c, F) + rng.uniform(0.1, 0.9, 3).astype(F)) * cell)
    pos = np.array(pos, F)
    assert np.all(np.floor(pos * F(4.0)) == np.array(starts * 3, F))
    tri = [(10 * j + c, 10 * ((j + 1) % 3) + (c + 1) % 10, 10 * ((j + 2) % 3) + (c + 2) % 10) for j in range(3) for c in range(10)]
    assert table_sizes(30, len(tri)) == (64, 64)
    return Case("cell_table_wrap", pos, None, cell, [("all", tri)], expect={"all": dict(n_cells=10, n_used_vertices=30)}, notes=dict(cells=starts))


def _tri_table_wrap():
    cell = F(0.25)
    pool = 24
    pos = np.array([((F(3 * i) + F(0.5)) * cell, F(0.5) * cell, F(0.5) * cell) for i in range(pool)], F)     # every slot its own cell
    sets = [t for t in itertools.combinations(range(pool), 3) if dec_tri_hash(t[0], t[1], t[2], 63) >= 62][:10]
    assert len(sets) == 10
    tri = [(p, a, b) if k % 2 == 0 else (p, b, a) for k, (p, a, b) in enumerate(sets)]
    out = sorted(tri)
    # the last four sets again, in the other winding and rotated: upwards, each one's chain passes the entries of the sets
    # before it; downwards, these come first and are lowered later
    for k in (9, 8, 7, 6):
        p, a, b = tri[k]
        tri.append((a, p, b))
    tri += [(0, 1, 2), (3, 5, 4)]
    out = sorted(out + [(0, 1, 2), (3, 5, 4)])
    assert len(set(tuple(sorted(t)) for t in tri)) == 12 and table_sizes(pool, len(tri))[1] == 64
    return Case("tri_table_wrap", pos, None, cell, [("all", tri)], expect={"all": dict(out=out, n_duplicates=4, n_collapsed=0)}, notes=dict(sets=sets))


ONE_SET_TRIANGLES = 4096


def _one_corner_set():
    rng = np.random.default_rng(31)
    centres = {"A": (0.5, 0.5, 0.5), "B": (2.5, 0.5, 0.5), "C": (0.5, 2.5, 0.5)}
    pos, where = np.zeros((18, 3), F), {}
    reps = {"A": 5, "B": 9, "C": 13}                      # the slots at the centres: not the lowest of their cells
    members = {"A": [0, 3, 5, 6, 14, 17], "B": [1, 4, 7, 9, 12, 15], "C": [2, 8, 10, 11, 13, 16]}
    for name, slots in members.items():
        for s in slots:
            off = np.zeros(3) if s == reps[name] else rng.uniform(0.05, 0.45, 3) * rng.choice([-1, 1], 3)
            pos[s] = np.array(centres[name]) + off
            where[s] = name
    tri = []
    for _ in range(ONE_SET_TRIANGLES):
        t = [int(rng.choice(members[k])) for k in "ABC"]
        if rng.integers(2):
            t = [t[0], t[2], t[1]]
        r = int(rng.integers(3))
        tri.append(tuple(t[r:] + t[:r]))
    tri[0] = (1, 0, 2)                                      # -> (9, 5, 13) = (5, 13, 9): a rotation of the back-facing winding
    tri[-1] = (17, 15, 16)                                  # -> (5, 9, 13): front-facing, the earliest of the reversed array
    kinds = set()
    for t in tri:
        k = [where[v] for v in t]
        kinds.add((k.index("A"), k[(k.index("A") + 1) % 3]))
    assert len(kinds) == 6                                  # all three rotations in both windings
    vmap = {s: reps[where[s]] for s in range(18)}
    return Case("one_corner_set", pos, None, 1.0, [("forwards", tri), ("reversed", tri[::-1])],
                expect={"forwards": dict(out=[(5, 13, 9)], vmap=vmap, n_duplicates=ONE_SET_TRIANGLES - 1),
                        "reversed": dict(out=[(5, 9, 13)], vmap=vmap, n_duplicates=ONE_SET_TRIANGLES - 1)})


def _line(n):
    """Slot i in a unit cell of its own: (i mod 256, i div 256, 0) + 0.5."""
    i = np.arange(n)
    return np.stack([(i & 255) + 0.5, (i >> 8) + 0.5, np.full(n, 0.5)], axis=1).astype(F)


def _table_sizes():
    out = []
    for n in (32, 33):
        tri = [(i, i + 1, i + 2) for i in range(n - 2)]
        assert table_sizes(n, len(tri))[0] == (64 if n == 32 else 128)
        out.append(Case("table_sizes/used%d" % n, _line(n), None, 1.0, [("all", tri)],
                        expect={"all": dict(out=tri, n_cells=n, n_used_vertices=n)}))
    assert 3 * 1 < 1000 and table_sizes(1000, 1) == (64, 64)
    out.append(Case("table_sizes/one_in_1000", _line(1000), None, 1.0, [("all", [(500, 999, 0)])],
                    expect={"all": dict(out=[(0, 500, 999)], n_cells=3, n_used_vertices=3)}))
    rng = np.random.default_rng(41)
    perms = list(itertools.permutations(range(3)))
    tri = [(2, 1, 0)] + [perms[int(k)] for k in rng.integers(6, size=299)]
    assert 3 < 3 * len(tri) and table_sizes(3, 300) == (64, 1024)
    out.append(Case("table_sizes/300_on_3", _line(3), None, 1.0, [("all", tri)],
                    expect={"all": dict(out=[(0, 2, 1)], n_duplicates=299, n_cells=3)}))
    return out


SORT_WIDTHS = {3: 0, 16: 6, 17: 6, 256: 60, 257: 60, 4096: 300, 4097: 300, 65536: 300, 65537: 3000}    # n: random triangles


def _sort_widths():
    out = []
    for n, extra in SORT_WIDTHS.items():
        bits = sort_bits(n)
        top = 1 << (bits - 1)
        if n == 3:
            tri = [(1, 0, 2)]
        else:
            # (0, 1, top) against (0, 1, 2): with (a << (bits - 1)) | b the top bit of b runs into a = 1, which holds it already,
            # and the key of the first becomes that of (0, 1, 0).  Slot n - 1 as a and as b; the largest p there is, n - 3.
            tri = [(0, 1, top), (0, 1, 2), (0, n - 1, 3), (1, 4, n - 1), (n - 3, n - 1, n - 2)]
            rng = np.random.default_rng(n)
            while len(tri) < 5 + extra:
                t = tuple(int(v) for v in rng.choice(n, 3, replace=False))
                tri.append(t)
            tri = [tri[k] for k in np.random.default_rng(n + 1).permutation(len(tri))]
        out.append(Case("sort_widths/%d" % n, _line(n), None, 1.0, [("all", tri)], expect={"all": dict(n_collapsed=0, n_not_live=0)},
                        notes=dict(bits=bits, passes=sort_passes(n))))
    return out


def _corners():
    b = _Builder(1.0)
    a1, a2 = b.add(0.3, 0.5, 0.5), b.add(0.6, 0.5, 0.5)    # 0, 1: one cell, 1 is nearer to its centre
    bb, cc = b.add(2.5, 0.5, 0.5), b.add(4.5, 0.5, 0.5)    # 2, 3
    m = b.add(6.5, 0.5, 0.5, r2=-1.0)                      # 4: merged
    x = b.add(8.5, 0.5, 0.5)                               # 5: live, only in a dropped triangle: stays out of U
    y = b.add(10.5, 0.5, 0.5)                              # 6: live, in a dropped triangle and in a kept one
    nan = b.add(np.nan, 0.5, 0.5)                          # 7
    inf = b.add(12.5, np.inf, 0.5)                         # 8
    d, e = b.add(14.5, 0.5, 0.5), b.add(16.5, 0.5, 0.5)    # 9, 10
    z = b.add(8.4, 0.5, 0.5)                               # 11: in x's cell, farther from the centre: x would win it if x were in U
    b.add(20.5, 0.5, 0.5)                                  # 12: in no triangle
    tri = [(x, m, y),                                       # not live
           (y, d, e),
           (a1, a2, bb),                                    # r0 == r1 only
           (bb, a1, a2),                                    # r1 == r2 only
           (a1, bb, a2),                                    # r0 == r2 only
           (nan, bb, cc), (bb, inf, cc),                    # not live
           (bb, bb, cc),                                    # a corner repeated: r0 == r1
           (cc, d, cc),                                     # a corner repeated: r0 == r2 only
           (z, bb, cc),
           (a1, bb, cc),                                    # -> (1, 2, 3)
           (a2, cc, bb)]                                    # -> (1, 3, 2): the same corners, later: dropped
    return b.case("corners", arrays=[("all", tri)], expect={"all": dict(
        out=[(1, 2, 3), (2, 3, 11), (6, 9, 10)], vmap=dict(zip(range(13), [1, 1, 2, 3, INV, INV, 6, INV, INV, 9, 10, 11, INV])),
        n_in=12, n_not_live=3, n_used_vertices=8, n_cells=7, n_collapsed=5, n_duplicates=1, n_triangles=3)})


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in the order of the table in DESIGN.md 5g."""
    return tuple([_faces(), _mul_not_div(), _rounding_decides(), _ties(), _key_fields(), _range_edges(), _huge_cell(),
                  _cell_table_wrap(), _tri_table_wrap(), _one_corner_set()] + _table_sizes() + _sort_widths() + [_corners()])


def case(name):
    return {c.name: c for c in cases()}[name]


GROUPS = ("faces", "mul_not_div", "rounding_decides", "ties", "key_fields", "range_edges", "huge_cell", "cell_table_wrap",
          "tri_table_wrap", "one_corner_set", "table_sizes", "sort_widths", "corners")
