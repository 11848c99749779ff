"""The cases of tests/decimate_cases.py without a GPU.  For every case the model (decimate_ref.decimate) has to equal a brute
force written here -- dictionaries of cells, Python loops, one scalar np.float32 expression per operation -- and the host
walk of the kernels' passes (tests/decimate_host.py) in three lane orders: triangle array, vertex map and every statistic,
for equality; what a case says by hand about its result has to hold.  The Python restatements of the hashes, the table size
and the `bits` rule are held to the header's own functions.  The census proves from the model's and the walk's own numbers
that each case still reaches the decision it was built for, and every one-decision mutant of the model has to change the
output of the case named for it (KILLED_AT), or be listed with the reason why no case can (UNNOTICEABLE).  The same source
as the walk also runs once as a program of its own under the address and undefined-behaviour sanitizers.
tests/test_gpu_decimate_cases.py runs the same cases on the device against the same model."""
import ctypes as C

import numpy as np
import pytest

import decimate_cases as dc
import decimate_host as dh
import decimate_ref as dr

F = np.float32
NAMES = [c.name for c in dc.cases()]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("decimate_cases")


@pytest.fixture(scope="module")
def host(work):
    return dh.host_library(work)


_MODEL = {}


def model(c, label):
    """(out, vmap, stats) of the model for an accepted array of a case, computed once."""
    if (c.name, label) not in _MODEL:
        _MODEL[(c.name, label)] = dr.decimate(c.pos, c.r2, dict(c.arrays)[label], c.cell)
    return _MODEL[(c.name, label)]


# ---- the brute force ----------------------------------------------------------------------------------------------------------
def brute(pos, r2, tri, cell):
    cell = F(cell)
    inv = F(1.0) / cell
    n = pos.shape[0]
    live = [not (r2[i] < 0) and bool(np.all(np.isfinite(pos[i]))) for i in range(n)]
    kept, st = [], dict(n_in=len(tri), n_not_live=0, n_used_vertices=0, n_cells=0, n_collapsed=0, n_duplicates=0, n_triangles=0)
    for t in tri:
        t = [int(v) for v in t]
        if live[t[0]] and live[t[1]] and live[t[2]]:
            kept.append(t)
        else:
            st["n_not_live"] += 1
    used = sorted({v for t in kept for v in t})
    st["n_used_vertices"] = len(used)
    cells, cell_of = {}, {}
    with np.errstate(over="ignore", under="ignore"):
        for i in used:
            x, c = [F(v) for v in pos[i]], []
            for a in range(3):
                f = np.floor(x[a] * inv)
                if not (f >= F(-1048576.0) and f < F(1048576.0)):
                    raise dr.CellRangeError("slot %d" % i)
                c.append(int(f))
            dx, dy, dz = (x[a] - (F(c[a]) + F(0.5)) * cell for a in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            word = (int(F(d2).view(np.uint32)), i)
            cell_of[i] = tuple(c)
            if tuple(c) not in cells or word < cells[tuple(c)]:
                cells[tuple(c)] = word
    st["n_cells"] = len(cells)
    vmap = np.full(n, 0xFFFFFFFF, np.uint32)
    for i in used:
        vmap[i] = cells[cell_of[i]][1]
    first = {}
    for t in kept:
        r = [int(vmap[v]) for v in t]
        if r[0] == r[1] or r[1] == r[2] or r[0] == r[2]:
            st["n_collapsed"] += 1
            continue
        k = r.index(min(r))
        if frozenset(r) in first:
            st["n_duplicates"] += 1
        else:
            first[frozenset(r)] = (r[k], r[(k + 1) % 3], r[(k + 2) % 3])
    out = np.array(sorted(first.values()), np.uint32).reshape(-1, 3)
    st["n_triangles"] = out.shape[0]
    return out, vmap, st


def _same(got, want, what):
    assert got[2] == want[2], (what, got[2], want[2])
    assert got[0].dtype == np.uint32 and got[0].tobytes() == want[0].tobytes(), what
    assert got[1].dtype == np.uint32 and got[1].tobytes() == want[1].tobytes(), what


@pytest.mark.parametrize("name", NAMES)
def test_model_brute_force_and_host_walk_agree(host, name):
    c = dc.case(name)
    assert c.pos.dtype == F and c.arrays
    for label, tri in c.arrays:
        want = model(c, label)
        dr.check_properties(*want)
        _same(brute(c.pos, c.r2, tri, c.cell), want, (name, label, "brute force"))
        for order in dh.ORDERS:
            got = dh.host_walk(host, c.pos, c.r2, tri, c.cell, order)
            _same(got[:3], want, (name, label, dh.ORDER_NAMES[order]))
        # what the case says by hand
        out, vmap, st = want
        for k, v in c.expect.get(label, {}).items():
            if k == "vmap":
                assert {i: int(vmap[i]) for i in v} == v, (name, label)
            elif k == "out":
                assert out.tolist() == [list(t) for t in v], (name, label)
            else:
                assert st[k] == v, (name, label, k)
        print("%s/%s: %s" % (name, label, st))
    for label, tri in c.refused:
        with pytest.raises(dr.CellRangeError):
            dr.decimate(c.pos, c.r2, tri, c.cell)
        with pytest.raises(dr.CellRangeError):
            brute(c.pos, c.r2, tri, c.cell)
        for order in dh.ORDERS:
            assert dh.host_walk(host, c.pos, c.r2, tri, c.cell, order)[0] == -2, (name, label)


def test_every_required_case_is_there():
    assert {c.group for c in dc.cases()} == set(dc.GROUPS)
    assert max(c.n for c in dc.cases()) == 65537
    assert max(t.shape[0] for c in dc.cases() for _, t in c.arrays + c.refused) < 5000


# ---- the restatements against the header ----------------------------------------------------------------------------------------
def test_restatements_equal_the_header(host):
    rng = np.random.default_rng(2024)
    keys = [int(k) for k in rng.integers(0, 1 << 63, 10000, dtype=np.uint64)]
    keys += [0, 1, (1 << 63) - 1, (1 << 63), (1 << 64) - 1, 1 << 21, 1 << 42, 1 << 20, 1 << 41, 1 << 62,
             dc.dec_cell_key(-dc.LIMIT, -dc.LIMIT, -dc.LIMIT), dc.dec_cell_key(dc.LIMIT - 1, dc.LIMIT - 1, dc.LIMIT - 1)]
    masks = [63, 127, 1023, 8191, (1 << 31) - 1, 0xFFFFFFFF]
    for i, k in enumerate(keys):
        m = masks[i % len(masks)]
        assert dc.dec_hash(k, m) == host.x_dec_hash(k, m), hex(k)
    tris = rng.integers(0, 1 << 32, (10000, 3), dtype=np.uint64).tolist()
    tris += [[0, 1, 2], [0, 2, 1], [0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFE], [0, 0xFFFFFFFF, 1], [65534, 65536, 65535], [0, (1 << 21) - 1, 1 << 21],
             [(1 << 22) - 1, 1 << 22, (1 << 22) + 1]]
    for i, (p, a, b) in enumerate(tris):
        m = masks[i % len(masks)]
        assert dc.dec_tri_hash(p, a, b, m) == host.x_dec_tri_hash(p, a, b, m), (p, a, b)
        assert dc.dec_tri_hash(p, a, b, m) == dc.dec_tri_hash(p, b, a, m)
    sizes = [int(v) for v in rng.integers(0, 1 << 32, 10000, dtype=np.uint64)]
    sizes += [0, 1, 31, 32, 33, 63, 64, 65, 4096, 4097, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    for e in sizes:
        assert dc.dec_table_size(e) == host.x_dec_table_size(e), e
    assert dc.dec_table_size(32) == 64 and dc.dec_table_size(33) == 128
    # `bits`: the walk reports the value it used; a call with one triangle on a map of n slots
    for n in (3, 4, 5, 16, 17, 255, 256, 257, 4096, 4097, 65536, 65537):
        pos = np.zeros((n, 3), F)
        pos[:3] = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]]
        cen = dh.host_walk(host, pos, np.ones(n, F), np.array([[0, 1, 2]], np.uint32), 1.0)[3]
        assert cen["bits"] == dc.sort_bits(n) == dr.sort_bits(n) == (n - 1).bit_length(), n
    assert [dc.sort_passes(n) for n in (3, 16, 17, 256, 257, 4096, 4097, 65536, 65537)] == \
        [(1, 1), (1, 1), (2, 1), (2, 1), (3, 2), (3, 2), (4, 2), (4, 2), (5, 3)]


# ---- the header's float functions, for the census -----------------------------------------------------------------------------
def _coord(host, x, cell):
    c = C.c_int32(0)
    ok = host.x_dec_cell_coord(C.c_float(x), C.c_float(F(1.0) / F(cell)), C.byref(c))
    return c.value if ok else None


def _cell(host, p, cell):
    return tuple(_coord(host, v, cell) for v in p)


def _d2(host, p, cell):
    c = _cell(host, p, cell)
    return F(host.x_dec_d2(C.c_float(p[0]), C.c_float(p[1]), C.c_float(p[2]), c[0], c[1], c[2], C.c_float(cell)))


def _used(c, label):
    return np.flatnonzero(model(c, label)[1] != dr.INVALID)


def _walks(host, c, label):
    return {o: dh.host_walk(host, c.pos, c.r2, dict(c.arrays)[label], c.cell, o)[3] for o in dh.ORDERS}


def test_float_expressions_equal_the_header(host):
    """dec_cell_coord, dec_cell_centre and dec_d2 against one scalar np.float32 operation each, on the cases' own vertices
    (up to 300 of each case) and, for the coordinate, on both sides of the range."""
    with np.errstate(over="ignore", under="ignore"):
        for c in dc.cases():
            cell = F(c.cell)
            inv = F(1.0) / cell
            for i in _used(c, c.arrays[0][0])[:300]:
                p = c.pos[i]
                k = [int(np.floor(F(x) * inv)) for x in p]
                assert list(_cell(host, p, cell)) == k, (c.name, i)
                centre = [(F(v) + F(0.5)) * cell for v in k]
                assert [F(host.x_dec_cell_centre(v, C.c_float(cell))).view(np.uint32) for v in k] == [v.view(np.uint32) for v in centre]
                dx, dy, dz = (F(x) - m for x, m in zip(p, centre))
                assert _d2(host, p, cell).view(np.uint32) == F((dx * dx + dy * dy) + dz * dz).view(np.uint32), (c.name, i)
    for x, want in ((1048575.9375, 1048575), (1048576.0, None), (-1048576.0, -1048576), (-1048576.125, None), (np.nan, None),
                    (np.inf, None), (-0.0, 0), (-1e-45, -1)):
        assert _coord(host, F(x), 1.0) == want, x


# ---- the census: each case reaches what it was built for --------------------------------------------------------------------------
def test_census_faces(host):
    c = dc.case("faces")
    seen = set()
    for i in _used(c, "all"):
        for a in range(3):
            x = c.pos[i, a]
            for k in (-2, -1, 0, 1):
                if x == F(k) * F(0.25):
                    assert _coord(host, x, 0.25) == k               # on the face: the cell above
                    seen.add((a, k, "on"))
                if x == np.nextafter(F(k) * F(0.25), F(-np.inf)):
                    assert _coord(host, x, 0.25) == k - 1           # one float below it: the cell below
                    seen.add((a, k, "below"))
    assert len(seen) == 24
    assert np.any((c.pos < 0) & (c.pos > -1e-40))                   # the face at zero is approached through a subnormal


def test_census_mul_not_div(host):
    c = dc.case("mul_not_div")
    cell = F(c.cell)
    assert np.log2(float(cell)) % 1 != 0
    used = _used(c, "all")
    differ = [i for i in used if any(_coord(host, x, cell) != int(np.floor(F(x) / cell)) for x in c.pos[i])]
    assert c.notes["x_edge"] in differ
    centres = [k for i in used for k in _cell(host, c.pos[i], cell)
               if F(host.x_dec_cell_centre(k, C.c_float(cell))) != F(k) * cell + F(0.5) * cell]
    assert c.notes["centre_cell"] in centres
    assert F(host.x_dec_cell_centre(c.notes["centre_cell"], C.c_float(cell))) == (F(c.notes["centre_cell"]) + F(0.5)) * cell


def test_census_rounding_decides(host):
    c = dc.case("rounding_decides")
    vmap = model(c, "all")[1]
    forms = set()
    for form, lo, hi in c.notes["pairs"]:
        assert lo < hi and _cell(host, c.pos[lo], 1.0) == _cell(host, c.pos[hi], 1.0)
        assert _d2(host, c.pos[hi], 1.0) < _d2(host, c.pos[lo], 1.0)              # the header, as written: the higher slot is nearer
        k = F(np.array(_cell(host, c.pos[lo], 1.0), F) + F(0.5))
        other = [dr.d2_of(*(F(v) for v in c.pos[i] - k), form) for i in (lo, hi)]
        assert other[1] >= other[0]                                               # the other form: farther, or a tie that the lower slot wins
        assert int(vmap[lo]) == hi
        forms.add(form)
    assert forms == set(dc.D2_FORMS)
    st = model(c, "all")[2]
    assert st["n_used_vertices"] - st["n_cells"] == len(c.notes["pairs"]) >= 2 * len(dc.D2_FORMS)


def test_census_ties(host):
    c = dc.case("ties")
    tri = dict(c.arrays)["slot0"]
    at = {int(v): k for k, v in reversed(list(enumerate(tri[:, 0])))}              # where a slot first occurs in the array
    m = c.notes["mirrored"]
    assert len({int(_d2(host, c.pos[i], 1.0).view(np.uint32)) for i in m}) == 1 and len({tuple(c.pos[i]) for i in m}) == 4
    assert all(at[m[0]] > at[i] for i in m[1:]) and m[0] == min(m)               # equal d2 bits, the lower slot later in the input
    big = np.arange(dc.TIES_BIG)
    assert np.all(c.pos[big] == c.pos[0]) and at[0] > min(at[int(i)] for i in big[1:])
    assert np.all(model(c, "slot0")[1][big] == 0)
    last = c.n - 1
    assert np.all(model(c, "last")[1][big] == last) and _cell(host, c.pos[last], 1.0) == _cell(host, c.pos[0], 1.0)
    assert _d2(host, c.pos[last], 1.0) < _d2(host, c.pos[0], 1.0)


def test_census_key_fields_and_range_edges(host):
    c = dc.case("key_fields")
    cells = [_cell(host, c.pos[i], 1.0) for i in _used(c, "all")]
    assert len(set(cells)) == len(cells)
    ext = (-dc.LIMIT, dc.LIMIT - 1)
    assert all((x, y, z) in cells for x in ext for y in ext for z in ext)
    keys = {dc.dec_cell_key(*k) for k in cells}
    for bit in (0, 20, 21, 41, 42, 62):                                            # bit 0 and bit 20 of each field
        assert sum(1 for k in keys if k ^ (1 << bit) in keys) >= 8, bit
    c = dc.case("range_edges")
    for label, extreme in (("accept_hi", dc.LIMIT - 1), ("accept_lo", -dc.LIMIT)):
        used = _used(c, label)
        for a in range(3):
            assert extreme in [_coord(host, c.pos[i, a], 1.0) for i in used], (label, a)
    for (label, tri), f in zip(c.refused, (1048576.0, -1048577.0)):
        fl = np.floor(c.pos[np.unique(tri)])
        assert np.sum(fl == f) == 1 and np.all((fl == f) | ((fl >= -dc.LIMIT) & (fl < dc.LIMIT))), label   # one coordinate, one cell too far


def test_census_huge_cell(host):
    c = dc.case("huge_cell")
    inv = F(1.0) / F(c.cell)
    tiny = np.finfo(F).tiny
    prod = c.pos * inv
    assert 0 < inv < tiny                                                         # inv itself is subnormal
    assert np.any((prod < 0) & (prod > -tiny)) and np.any((prod > 0) & (prod < tiny))
    assert {_cell(host, p, c.cell) for p in c.pos} == {(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)}
    assert all(np.isposinf(_d2(host, p, c.cell)) for p in c.pos)                 # every slot of a cell ties
    assert model(c, "all")[2]["n_cells"] == 8


def test_census_tables(host):
    c = dc.case("cell_table_wrap")
    st = model(c, "all")[2]
    assert c.n <= 32 and st["n_used_vertices"] >= 3 * st["n_cells"] and st["n_cells"] >= 10
    for order, cen in _walks(host, c, "all").items():
        assert cen["cell_table"] == 64 and cen["cell_wraps"] >= 1 and cen["cell_longest"] >= 8, (order, cen)
    assert all(dc.dec_hash(dc.dec_cell_key(*k), 63) >= 62 for k in c.notes["cells"])
    c = dc.case("tri_table_wrap")
    out, _, st = model(c, "all")
    assert st["n_in"] <= 32 and sum(1 for p, a, b in out.tolist() if dc.dec_tri_hash(p, a, b, 63) >= 62) >= 8
    walks = _walks(host, c, "all")
    for order, cen in walks.items():
        assert cen["tri_table"] == 64 and cen["tri_wraps"] >= 1 and cen["tri_longest"] >= 8, (order, cen)
    assert walks[dh.UPWARDS]["lowered"] == 0 and walks[dh.DOWNWARDS]["lowered"] == st["n_duplicates"] == 4
    c = dc.case("one_corner_set")
    for label in ("forwards", "reversed"):
        walks = _walks(host, c, label)
        assert model(c, label)[2]["n_in"] == 16 * 256                             # 16 workgroups
        assert walks[dh.UPWARDS]["lowered"] == 0 and walks[dh.DOWNWARDS]["lowered"] >= 4095 and walks[dh.SHUFFLED]["lowered"] >= 3
    # the table sizes on either side of their switches
    seen = {}
    for name in ("used32", "used33", "one_in_1000", "300_on_3"):
        c = dc.case("table_sizes/" + name)
        cen = _walks(host, c, "all")[dh.UPWARDS]
        seen[name] = (cen["cell_table"], cen["tri_table"])
        assert seen[name] == dc.table_sizes(c.n, model(c, "all")[2]["n_in"])
    assert seen["used32"][0] == 64 and model(dc.case("table_sizes/used32"), "all")[2]["n_cells"] * 2 == 64      # exactly half full
    assert seen["used33"][0] == 128
    assert seen["one_in_1000"] == (64, 64) and seen["300_on_3"] == (64, 1024)
    assert 3 * 1 < dc.case("table_sizes/one_in_1000").n and dc.case("table_sizes/300_on_3").n < 3 * 300


def test_census_sort_widths(host):
    pairs, most = set(), 0
    for n in dc.SORT_WIDTHS:
        c = dc.case("sort_widths/%d" % n)
        out, _, st = model(c, "all")
        cen = _walks(host, c, "all")[dh.UPWARDS]
        assert c.n == n and cen["bits"] == c.notes["bits"] == dc.sort_bits(n)
        pairs.add(dc.sort_passes(n))
        most = max(most, st["n_triangles"])
        assert st["n_used_vertices"] == st["n_cells"] and (n < 256 or st["n_used_vertices"] <= n // 2)     # nothing collapses; mostly unused
        if n > 3:
            top = 1 << (cen["bits"] - 1)
            # slot n - 1 as a and as b; p is the smallest of three, so n - 3 is the largest there is (it has the top bit of
            # `bits` where n is a power of two; at 2^k + 1 only slot n - 1 has it)
            assert n - 1 in out[:, 1] and n - 1 in out[:, 2] and out[:, 0].max() == n - 3 and np.any(out[:, 2] == top)
            assert (n - 3 >= top) == (n & (n - 1) == 0) and n - 1 >= top
            tri = dict(c.arrays)["all"]
            assert not np.array_equal(out, tri)                                                  # the input is not in order already
    assert pairs == {(1, 1), (2, 1), (3, 2), (4, 2), (5, 3)}
    assert most > 2048                                                                           # more than one sort tile


# ---- mutants ------------------------------------------------------------------------------------------------------------------
# mutant -> the (case, array) whose result has to differ from the model's under it
KILLED_AT = {
    "trunc": ("faces", "all"), "div": ("mul_not_div", "all"), "centre_distributed": ("mul_not_div", "all"),
    "d2_fma_z": ("rounding_decides", "all"), "d2_fma_y": ("rounding_decides", "all"), "d2_fma_both": ("rounding_decides", "all"),
    "d2_assoc": ("rounding_decides", "all"), "ftz": ("huge_cell", "all"), "tie_high": ("ties", "slot0"),
    "key_shift20": ("key_fields", "all"), "range_hi_far": ("range_edges", "refuse_hi"), "range_hi_early": ("range_edges", "accept_hi"),
    "range_lo_far": ("range_edges", "refuse_lo"), "range_lo_early": ("range_edges", "accept_lo"),
    "same_winding_only": ("one_corner_set", "forwards"), "latest_duplicate": ("one_corner_set", "forwards"),
    "sorted_triple": ("one_corner_set", "forwards"), "no_r0r2": ("corners", "all"), "u_all_live": ("corners", "all"),
    "bits_minus_1": ("sort_widths/17", "all"),
}
# mutant -> why no case can notice it (none: every decision of the list is visible in the call's results)
UNNOTICEABLE = {}


def _result(c, label, mutant=None):
    tri = dict(c.arrays + c.refused)[label]
    try:
        out, vmap, st = dr.decimate(c.pos, c.r2, tri, c.cell, mutant=mutant)
    except dr.CellRangeError:
        return "refused"
    return out.tobytes(), vmap.tobytes(), tuple(sorted(st.items()))


def test_mutant_list_is_the_models():
    assert set(KILLED_AT) | set(UNNOTICEABLE) == set(dr.MUTANTS) and not set(KILLED_AT) & set(UNNOTICEABLE)


@pytest.mark.parametrize("mut", sorted(KILLED_AT))
def test_a_mutant_of_the_model_is_noticed_at_its_case(mut):
    name, label = KILLED_AT[mut]
    c = dc.case(name)
    want, got = _result(c, label), _result(c, label, mut)
    where = [k for k, (w, g) in enumerate(zip(want, got)) if w != g] if "refused" not in (want, got) else ["refused"]
    print("\n%-20s (%s)\n    noticed at %s/%s in %s" % (mut, dr.MUTANTS[mut], name, label, where))
    assert want != got


def test_mutants_where_they_are_meant_to_bite():
    # each contracted or re-associated d2 gives exactly its own pairs to the lower slot
    c = dc.case("rounding_decides")
    for form in dc.D2_FORMS:
        vmap = dr.decimate(c.pos, c.r2, dict(c.arrays)["all"], c.cell, mutant=form)[1]
        assert all(int(vmap[lo]) == lo and int(vmap[hi]) == lo for f, lo, hi in c.notes["pairs"] if f == form), form
    # bits - 1: every width with more than one triangle notices
    for n in dc.SORT_WIDTHS:
        c = dc.case("sort_widths/%d" % n)
        assert (_result(c, "all") != _result(c, "all", "bits_minus_1")) == (n > 3), n
    # the triangle-table case and the reversed array notice the duplicate rules as well; a strict winner is no tie to move
    assert _result(dc.case("tri_table_wrap"), "all") != _result(dc.case("tri_table_wrap"), "all", "same_winding_only")
    c = dc.case("ties")
    assert np.all(dr.decimate(c.pos, c.r2, dict(c.arrays)["last"], c.cell, mutant="tie_high")[1][:dc.TIES_BIG] == c.n - 1)
    assert _result(dc.case("one_corner_set"), "reversed") != _result(dc.case("one_corner_set"), "reversed", "latest_duplicate")
    # x / cell moves the vertex on the face; the distributed centre moves the pair about the centre
    c = dc.case("mul_not_div")
    e = c.notes["x_edge"]
    assert int(dr.decimate(c.pos, c.r2, dict(c.arrays)["all"], c.cell, mutant="div")[1][e]) != int(model(c, "all")[1][e])


def test_an_unnoticeable_mutant_is_noticed_nowhere_and_says_why():
    """Not a pass for the cases: the list is what they cannot show, with the reason.  (If a case does notice one, the entry
    belongs in KILLED_AT.)  The list is empty today."""
    for mut, why in UNNOTICEABLE.items():
        assert why
        for c in dc.cases():
            for label, _ in c.arrays + c.refused:
                assert _result(c, label) == _result(c, label, mut), (mut, c.name, label)


# ---- the walk as a program of its own, under the sanitizers ---------------------------------------------------------------------
def test_the_program_under_the_sanitizers(work):
    """Run directly, once: address and undefined-behaviour sanitizers on the header's host code and on the walk."""
    exe = dh.host_program(work, sanitized=True)
    picks = [("cell_table_wrap", "all", dh.SHUFFLED), ("tri_table_wrap", "all", dh.DOWNWARDS), ("ties", "last", dh.SHUFFLED),
             ("huge_cell", "all", dh.UPWARDS), ("key_fields", "all", dh.DOWNWARDS), ("corners", "all", dh.SHUFFLED),
             ("one_corner_set", "forwards", dh.DOWNWARDS), ("sort_widths/65537", "all", dh.SHUFFLED), ("table_sizes/300_on_3", "all", dh.UPWARDS)]
    for name, label, order in picks:
        c = dc.case(name)
        got = dh.run_program(exe, work / "case.bin", c.pos, c.r2, dict(c.arrays)[label], c.cell, order)
        _same(got[:3], model(c, label), (name, label, "sanitized"))
    c = dc.case("range_edges")
    for label, tri in c.refused:
        assert dh.run_program(exe, work / "case.bin", c.pos, c.r2, tri, c.cell)[0] == -2
