"""The model of smx_recon_fill_holes (include/smx.h): the edge report of a triangle array and its small holes closed by fans,
in numpy.

Every quantity of the contract is an integer or a float32 expression written out below operation by operation (numpy rounds
each float32 operation once and never contracts a * b + c; its float32 division and square root are correctly rounded), so
results are compared with the library's for equality.  Deliberately another route than the kernels': the half-edge counts
come from sorted keys (np.unique) where smx_fill.hip fills a hash table with atomics, and the loops are found by following
next in Python from every unvisited vertex where the kernel lets every slot walk a bounded number of steps."""
import math

import numpy as np

MAX_HOLE_EDGES = 32
FILLED, DIAGONAL, FILTER = 1, 2, 3
HOLE_DTYPE = np.dtype([("label", "<u4"), ("n_edges", "<u4"), ("status", "<u4")])
STAT_NAMES = ("n_in", "n_not_live", "n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_pinched_vertices", "n_listed_loops",
              "n_filled_loops", "n_rejected_diagonal", "n_rejected_filter", "n_new_triangles", "n_triangles")
F = np.float32


def live_mask(pos32, r2):
    return ~(np.asarray(r2) < 0) & np.all(np.isfinite(pos32), axis=1)


def check_params(max_hole_edges, min_triangle_angle_deg, max_triangle_angle_deg):
    lo, hi = F(min_triangle_angle_deg), F(max_triangle_angle_deg)
    if not (int(max_hole_edges) == max_hole_edges and 3 <= max_hole_edges <= MAX_HOLE_EDGES):
        raise ValueError("max_hole_edges must be 3 .. %d" % MAX_HOLE_EDGES)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo < hi <= 180):
        raise ValueError("the angles must be finite with 0 <= min < max <= 180")


def cos_limit(deg):
    """(float)cos((double)deg * pi / 180) with deg a float32."""
    return F(math.cos(float(F(deg)) * (3.14159265358979323846 / 180.0)))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _angle_cos(at, b, c):
    e, f = _sub(b, at), _sub(c, at)
    with np.errstate(invalid="ignore", divide="ignore"):
        return _dot(e, f) / np.sqrt(_dot(e, e) * _dot(f, f))


def triangle_filter(P, A, B, nP, nA, nB, cos_min, cos_max):
    """mesh_triangle_filter of smx_mesh.hpp on float32 scalars (tuples of three): 0 rejected, 1 (P, A, B) counter-clockwise
    seen from the side the oriented normal points to, 2 the other winding."""
    c0, c1, c2 = _angle_cos(P, A, B), _angle_cos(A, B, P), _angle_cos(B, P, A)
    if not (c0 <= cos_min and c0 >= cos_max and c1 <= cos_min and c1 >= cos_max and c2 <= cos_min and c2 >= cos_max):
        return 0
    a, b = _sub(A, P), _sub(B, P)
    n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    total = tuple((nP[k] + nA[k]) + nB[k] for k in range(3))
    s = _dot(n, total)
    if not (s > 0) and not (s < 0):
        return 0
    flip = s < 0
    if flip:
        n = (-n[0], -n[1], -n[2])
    if not (_dot(n, nP) > 0 and _dot(n, nA) > 0 and _dot(n, nB) > 0):
        return 0
    return 2 if flip else 1


def _vec(a, i):
    return (a[i, 0], a[i, 1], a[i, 2])       # numpy float32 scalars


def d2(pos32, at, other):
    d = _sub(_vec(pos32, other), _vec(pos32, at))
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def canonical(t):
    p, a, b = t
    if p < a and p < b:
        return (p, a, b)
    if a < b:
        return (a, b, p)
    return (b, p, a)


def edge_report(n, t):
    """t [T, 3] int64, the triangles of R.  Returns (pair keys ascending (lo << 32 | hi, uint64), f, g, out, in, next)."""
    u = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    v = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    key = (lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64)
    up = u <= v
    keys, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    f = np.bincount(inv[up], minlength=keys.size).astype(np.int64)
    g = np.bincount(inv[~up], minlength=keys.size).astype(np.int64)
    klo, khi = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    bu, bd = (f == 1) & (g == 0), (f == 0) & (g == 1)       # the triangle's half-edge is lo -> hi / hi -> lo
    src = np.concatenate([khi[bu], klo[bd]])                 # the gaps run the other way
    dst = np.concatenate([klo[bu], khi[bd]])
    out, inn = np.bincount(src, minlength=n), np.bincount(dst, minlength=n)
    nxt = np.full(n, -1, np.int64)
    nxt[src] = dst                                           # (read only where out == 1)
    return keys, f, g, out, inn, nxt


def find_loops(out, inn, nxt):
    """Every cycle of simple vertices, as a list of slots starting at its smallest."""
    simple = (out == 1) & (inn == 1)
    seen = np.zeros(out.size, bool)
    loops = []
    for w in np.flatnonzero(simple):
        if seen[w]:
            continue
        chain, cur = [int(w)], int(nxt[w])
        seen[w] = True
        while cur != w and simple[cur] and not seen[cur]:
            chain.append(cur)
            seen[cur] = True
            cur = int(nxt[cur])
        if cur == w:
            k = chain.index(min(chain))
            loops.append(chain[k:] + chain[:k])
    loops.sort(key=lambda c: c[0])
    return loops, simple


def fill(pos, nrm, r2, triangles, max_hole_edges=8, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0):
    """pos [n, 3] smooth positions, nrm [n, 3] normals, r2 [n] RadiusSquared, triangles [T, 3] slot indices in any order.
    Returns (triangles_out [T_out, 3] uint32, n_kept, holes [n_listed] HOLE_DTYPE, stats dict)."""
    check_params(max_hole_edges, min_triangle_angle_deg, max_triangle_angle_deg)
    pos32 = np.ascontiguousarray(np.asarray(pos), dtype=np.float32)
    nrm32 = np.ascontiguousarray(np.asarray(nrm), dtype=np.float32)
    n = pos32.shape[0]
    tri = np.asarray(triangles, dtype=np.uint32).reshape(-1, 3)
    if tri.size and int(tri.max()) >= n:
        raise ValueError("an index is >= the slot count")
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["n_in"] = tri.shape[0]
    live = live_mask(pos32, r2)
    t_all = tri.astype(np.int64)
    remaining = np.all(live[t_all], axis=1) if t_all.size else np.zeros(0, bool)
    stats["n_not_live"] = int(t_all.shape[0] - remaining.sum())
    kept = tri[remaining]
    keys, f, g, out, inn, nxt = edge_report(n, t_all[remaining])
    stats["n_edges"] = int(keys.size)
    stats["n_boundary_edges"] = int(np.sum(f + g == 1))
    stats["n_nonmanifold_edges"] = int(np.sum(~((f + g == 1) | ((f == 1) & (g == 1)))))
    loops, simple = find_loops(out, inn, nxt)
    stats["n_pinched_vertices"] = int(np.sum((out + inn > 0) & ~simple))
    listed = [c for c in loops if 3 <= len(c) <= max_hole_edges]
    stats["n_listed_loops"] = len(listed)
    holes = np.zeros(len(listed), HOLE_DTYPE)
    pairs = set(keys.tolist())
    cmin, cmax = cos_limit(min_triangle_angle_deg), cos_limit(max_triangle_angle_deg)
    new = []
    for row, w in zip(holes, listed):
        L = len(w)
        best = None
        for i in range(L):
            c = F(0.0)
            for k in range(2, L - 1):
                c = c + d2(pos32, w[i], w[(i + k) % L])
            assert c.dtype == np.float32
            word = (int(np.asarray(c, np.float32).view(np.uint32)) << 32) | w[i]
            if best is None or word < best[0]:
                best = (word, i)
        i = best[1]
        status = FILLED
        if any(((min(w[i], w[(i + k) % L]) << 32) | max(w[i], w[(i + k) % L])) in pairs for k in range(2, L - 1)):
            status = DIAGONAL
        else:
            for k in range(1, L - 1):
                a, b = w[(i + k) % L], w[(i + k + 1) % L]
                if triangle_filter(_vec(pos32, w[i]), _vec(pos32, a), _vec(pos32, b), _vec(nrm32, w[i]), _vec(nrm32, a), _vec(nrm32, b),
                                   cmin, cmax) != 1:
                    status = FILTER
                    break
        row["label"], row["n_edges"], row["status"] = w[0], L, status
        if status == FILLED:
            new += [canonical((w[i], w[(i + k) % L], w[(i + k + 1) % L])) for k in range(1, L - 1)]
    new.sort()
    stats["n_filled_loops"] = int(np.sum(holes["status"] == FILLED))
    stats["n_rejected_diagonal"] = int(np.sum(holes["status"] == DIAGONAL))
    stats["n_rejected_filter"] = int(np.sum(holes["status"] == FILTER))
    stats["n_new_triangles"] = len(new)
    res = np.concatenate([kept, np.array(new, np.uint32).reshape(-1, 3)])
    stats["n_triangles"] = int(res.shape[0])
    return res, int(kept.shape[0]), holes, stats


def check_properties(pos, nrm, r2, tri_in, out, n_kept, holes, stats, **params):
    """The consequences of contract item 6, on any output."""
    tri_in = np.asarray(tri_in, np.uint32).reshape(-1, 3)
    out = np.asarray(out, np.uint32).reshape(-1, 3)
    n = np.asarray(pos).shape[0]
    pos32 = np.asarray(pos, np.float32)
    live = live_mask(pos32, r2)
    keep = np.all(live[tri_in.astype(np.int64)], axis=1) if tri_in.size else np.zeros(0, bool)
    assert n_kept == int(keep.sum()) and np.array_equal(out[:n_kept], tri_in[keep]), "R is not kept in input order"
    assert stats["n_triangles"] == out.shape[0] == n_kept + stats["n_new_triangles"]
    new = out[n_kept:].astype(np.int64)
    if new.shape[0]:
        assert np.all(new[:, 0] < new[:, 1]) and np.all(new[:, 0] < new[:, 2]), "a new triangle does not start at its smallest index"
        rows = [tuple(r) for r in new.tolist()]
        assert rows == sorted(rows) and len(set(rows)) == len(rows), "the new run is not strictly ascending"
    assert np.all(np.diff(holes["label"].astype(np.int64)) > 0), "the holes table is not ascending by label"
    filled = holes[holes["status"] == FILLED]
    assert stats["n_listed_loops"] == holes.shape[0] and stats["n_filled_loops"] == filled.shape[0]
    assert stats["n_filled_loops"] + stats["n_rejected_diagonal"] + stats["n_rejected_filter"] == stats["n_listed_loops"]
    assert int(np.sum(filled["n_edges"].astype(np.int64) - 2)) == stats["n_new_triangles"]
    # the edges before and after
    _, f0, g0, out0, in0, nxt0 = edge_report(n, tri_in[keep].astype(np.int64))
    _, f1, g1, _, _, _ = edge_report(n, out.astype(np.int64))
    ok0, ok1 = (f0 + g0 == 1) | ((f0 == 1) & (g0 == 1)), (f1 + g1 == 1) | ((f1 == 1) & (g1 == 1))
    if np.all(ok0):
        assert np.all(ok1), "a manifold input has become non-manifold"
    assert int(np.sum(f1 + g1 == 1)) == stats["n_boundary_edges"] - int(np.sum(filled["n_edges"])), "boundary edges are not down by L per loop"
    # the loops are vertex-disjoint cycles of simple vertices that start at their smallest slot
    seen = set()
    for row in holes:
        w, cyc = int(row["label"]), []
        for _ in range(int(row["n_edges"])):
            assert out0[w] == 1 and in0[w] == 1 and w not in seen
            seen.add(w)
            cyc.append(w)
            w = int(nxt0[w])
        assert w == int(row["label"]) == min(cyc)
    # a second call fills nothing and returns its input
    again, kept2, holes2, st2 = fill(pos, nrm, r2, out, **params)
    assert st2["n_new_triangles"] == 0 and kept2 == out.shape[0] and again.tobytes() == out.tobytes(), "a second call is not an identity"
    assert np.array_equal(holes2, holes[holes["status"] != FILLED])
