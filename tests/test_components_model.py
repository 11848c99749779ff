"""The model of smx_recon_mesh_components (tests/components_ref.py) against an independent breadth-first search written here,
on random triangle soups, and on hand cases whose answers are known: a bowtie, a bridge with a dead corner, the boundary of
each threshold, the keep_largest tie, and the box of -0.0 / +0.0."""
from collections import deque

import numpy as np
import pytest

import components_ref as cr

INVALID = 0xFFFFFFFF


def _bfs(pos, r2, tri, min_triangles, min_diagonal, keep_largest):
    """Python sets and a queue; the box by a comparison that knows -0 < +0; the float32 arithmetic as written in smx.h."""
    n = pos.shape[0]
    pos = pos.astype(np.float32)
    live = [not (r2[i] < 0) and all(np.isfinite(pos[i])) for i in range(n)]
    rem = [k for k, t in enumerate(tri) if all(live[int(v)] for v in t)]
    adj = {}
    for k in rem:
        p, a, b = (int(v) for v in tri[k])
        for u, v in ((p, a), (a, b), (b, p)):
            adj.setdefault(u, set()).add(v)
            adj.setdefault(v, set()).add(u)
    labels = np.full(n, INVALID, np.uint32)
    comps = []
    for s in sorted(adj):
        if labels[s] != INVALID:
            continue
        labels[s] = s
        members, queue = [s], deque([s])
        while queue:
            u = queue.popleft()
            for v in adj[u]:
                if labels[v] == INVALID:
                    labels[v] = s
                    members.append(v)
                    queue.append(v)
        comps.append((s, members))

    def below(x, y):                   # the total order of k(f): by value, -0 below +0
        return x < y or (x == y and np.signbit(x) and not np.signbit(y))
    rows = []
    for s, members in comps:
        lo, hi = pos[members[0]].copy(), pos[members[0]].copy()
        for v in members[1:]:
            for k in range(3):
                if below(pos[v][k], lo[k]):
                    lo[k] = pos[v][k]
                if below(hi[k], pos[v][k]):
                    hi[k] = pos[v][k]
        nt = sum(1 for k in rem if labels[int(tri[k][0])] == s)
        d = hi - lo
        d2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        md = np.float32(min_diagonal)
        rows.append(dict(label=s, n_vertices=len(members), n_triangles=nt, lo=lo, hi=hi,
                         passes=nt >= min_triangles and d2 >= np.float32(md * md)))
    passing = sorted((r for r in rows if r["passes"]), key=lambda r: (-r["n_triangles"], r["label"]))
    kept = {r["label"] for r in (passing[:keep_largest] if keep_largest > 0 else passing)}
    out = [tri[k] for k in rem if int(labels[int(tri[k][0])]) in kept]
    return np.array(out, np.uint32).reshape(-1, 3), labels, rows, kept, len(tri) - len(rem)


def _same(pos, r2, tri, **p):
    out, labels, table, st = cr.components(pos, r2, tri, **p)
    bout, blabels, rows, kept, not_live = _bfs(pos, r2, tri, p.get("min_triangles", 0), p.get("min_diagonal", 0.0), p.get("keep_largest", 0))
    assert out.tobytes() == bout.tobytes() and labels.tobytes() == blabels.tobytes()
    assert [int(v) for v in table["label"]] == [r["label"] for r in rows]
    assert [int(v) for v in table["n_vertices"]] == [r["n_vertices"] for r in rows]
    assert [int(v) for v in table["n_triangles"]] == [r["n_triangles"] for r in rows]
    assert [int(v) for v in table["kept"]] == [int(r["label"] in kept) for r in rows]
    if rows:
        assert table["lo"].tobytes() == np.array([r["lo"] for r in rows], np.float32).tobytes()
        assert table["hi"].tobytes() == np.array([r["hi"] for r in rows], np.float32).tobytes()
    assert st == dict(n_in=len(tri), n_not_live=not_live, n_used_vertices=int(np.sum(labels != INVALID)), n_components=len(rows),
                      n_kept_components=len(kept), n_largest_triangles=max([r["n_triangles"] for r in rows] or [0]),
                      n_triangles=out.shape[0])
    cr.check_properties(tri, out, labels, table, st)
    return out, labels, table, st


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_soups_against_breadth_first_search(seed):
    rng = np.random.default_rng(seed)
    n = 200
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    r2 = np.full(n, 0.01, np.float32)
    r2[rng.permutation(n)[:15]] = -1.0                      # some dead slots
    pos[rng.permutation(n)[:3], 1] = np.nan
    # 300 local triangles (three different slots within six of an anchor), so that the soup falls into pieces of many sizes
    anchors = rng.choice(n - 6, 45, replace=False)
    rows = []
    while len(rows) < 300:
        t = anchors[rng.integers(0, 45)] + rng.choice(6, 3, replace=False)
        rows.append(t)
    tri = np.array(rows, np.uint32)
    _, _, table, st = _same(pos, r2, tri)
    assert st["n_components"] > 3 and st["n_not_live"] > 0
    _same(pos, r2, tri, min_triangles=3)
    _same(pos, r2, tri, min_diagonal=0.8)
    _same(pos, r2, tri, min_triangles=2, min_diagonal=0.5, keep_largest=2)
    _same(pos, r2, tri[rng.permutation(tri.shape[0])], keep_largest=1)


def _flat(n):
    pos = np.zeros((n, 3), np.float32)
    pos[:, 0] = np.arange(n)
    return pos, np.ones(n, np.float32)


def test_a_bowtie_is_one_component():
    pos, r2 = _flat(5)
    tri = np.array([[0, 1, 2], [2, 3, 4]], np.uint32)       # two triangles that touch in slot 2 only
    out, labels, table, st = _same(pos, r2, tri)
    assert st["n_components"] == 1 and list(labels) == [0] * 5 and out.tobytes() == tri.tobytes()
    assert int(table["n_vertices"][0]) == 5 and int(table["n_triangles"][0]) == 2


def test_a_bridge_with_a_dead_corner_gives_two_components():
    pos, r2 = _flat(7)
    r2[3] = -1.0
    tri = np.array([[4, 5, 6], [2, 3, 4], [0, 1, 2]], np.uint32)     # the middle one would join the other two
    out, labels, table, st = _same(pos, r2, tri)
    assert st["n_components"] == 2 and st["n_not_live"] == 1
    assert list(labels) == [0, 0, 0, INVALID, 4, 4, 4] and list(table["label"]) == [0, 4]
    assert out.tobytes() == tri[[0, 2]].tobytes()


def test_the_boundary_of_each_threshold():
    # components of 1, 2 and 3 triangles
    pos, r2 = _flat(12)
    tri = np.array([[0, 1, 2], [3, 4, 5], [4, 5, 6], [7, 8, 9], [8, 9, 10], [9, 10, 11]], np.uint32)
    _, _, table, _ = _same(pos, r2, tri, min_triangles=2)
    assert list(table["n_triangles"]) == [1, 2, 3] and list(table["kept"]) == [0, 1, 1]      # a count equal to the threshold keeps
    _, _, table, _ = _same(pos, r2, tri, min_triangles=3)
    assert list(table["kept"]) == [0, 0, 1]
    # a box of 3 x 4 x 0: diagonal exactly 5
    pos = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32)
    r2, tri = np.ones(3, np.float32), np.array([[0, 1, 2]], np.uint32)
    out, _, table, _ = _same(pos, r2, tri, min_diagonal=5.0)
    assert out.shape[0] == 1 and list(table["hi"][0]) == [3, 4, 0]
    out, _, table, _ = _same(pos, r2, tri, min_diagonal=float(np.nextafter(np.float32(5), np.float32(6))))
    assert out.shape[0] == 0 and int(table["kept"][0]) == 0


def test_keep_largest_ties_and_more_than_pass():
    pos, r2 = _flat(14)
    tri = np.array([[11, 12, 13], [0, 1, 2], [1, 2, 3], [4, 5, 6], [5, 6, 7], [8, 9, 10]], np.uint32)   # sizes 2 (label 0), 2 (4), 1 (8), 1 (11)
    out, _, table, st = _same(pos, r2, tri, keep_largest=1)
    assert list(table["kept"]) == [1, 0, 0, 0] and out.tobytes() == tri[1:3].tobytes()       # the tie goes to the lower label
    out, _, table, _ = _same(pos, r2, tri, keep_largest=3)
    assert list(table["kept"]) == [1, 1, 1, 0] and out.tobytes() == tri[1:].tobytes()
    out, _, table, st = _same(pos, r2, tri, keep_largest=9)                                  # more than there are
    assert st["n_kept_components"] == 4 and out.tobytes() == tri.tobytes()
    out, _, table, st = _same(pos, r2, tri, min_triangles=2, keep_largest=3)                 # more than pass
    assert list(table["kept"]) == [1, 1, 0, 0] and st["n_largest_triangles"] == 2


def test_the_box_orders_minus_zero_below_plus_zero():
    pos = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0], [1.0, 0.0, 1.0]], np.float32)
    _, _, table, _ = _same(pos, np.ones(3, np.float32), np.array([[0, 1, 2]], np.uint32))
    lo, hi = table["lo"][0], table["hi"][0]
    assert np.signbit(lo[0]) and np.signbit(lo[1]) and not np.signbit(hi[1]) and hi[0] == 1.0
    assert lo.tobytes() == np.array([-0.0, -0.0, 1.0], np.float32).tobytes()
    assert hi.tobytes() == np.array([1.0, 0.0, 1.0], np.float32).tobytes()
    # the key is a bijection that orders as the floats do
    f = np.array([-np.inf, -1.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = cr.order_key(f)
    assert np.all(np.diff(k.astype(np.int64)) > 0) and cr.order_unkey(k).tobytes() == f.tobytes()


def test_the_model_refuses_what_the_library_refuses():
    pos, r2 = _flat(3)
    with pytest.raises(ValueError):
        cr.components(pos, r2, np.array([[0, 1, 3]], np.uint32))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cr.components(pos, r2, np.array([[0, 1, 2]], np.uint32), min_diagonal=bad)
    out, labels, table, st = cr.components(pos, r2, np.zeros((0, 3), np.uint32))
    assert out.shape == (0, 3) and np.all(labels == INVALID) and table.shape == (0,) and st["n_components"] == 0
