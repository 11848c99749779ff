"""The model of smx_recon_triangulate (include/smx.h): numpy + scipy in float64, with Qhull doing the geometry.

Deliberately another implementation than the kernels': every slot's star comes from scipy.spatial.Delaunay of its
projected candidates (the simplices incident to the origin), where smx_mesh.hpp wraps the star with an in-circle
tournament.  Candidates come from a cKDTree ball query truncated to the K nearest by (d^2, index)."""
import math

import numpy as np
from scipy.spatial import Delaunay, QhullError, cKDTree

MAX_STAR_DEGREE = 16


class Params:
    def __init__(self, max_angle_between_normals_deg=90.0, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0,
                 search_radius_factor=1.0, max_neighbors=64):
        self.max_angle_between_normals_deg = max_angle_between_normals_deg
        self.min_triangle_angle_deg = min_triangle_angle_deg
        self.max_triangle_angle_deg = max_triangle_angle_deg
        self.search_radius_factor = search_radius_factor
        self.max_neighbors = max_neighbors


def map_of_rows(rows, n=None):
    """(smooth positions [n,3], normals [n,3], RadiusSquared [n]) of surfel rows [25, >= n], as float64."""
    n = rows.shape[1] if n is None else n
    r = np.asarray(rows)[:, :n].astype(np.float64)
    return r[3:6].T.copy(), r[8:11].T.copy(), r[7].copy()


def live_mask(pos, r2):
    return ~(r2 < 0) & np.all(np.isfinite(pos), axis=1)


def basis(n):
    """Any orthonormal basis (u, v) with (u, v, n) right-handed."""
    n = n / np.linalg.norm(n)
    e = np.zeros(3)
    e[np.argmin(np.abs(n))] = 1.0
    u = np.cross(n, e)
    u /= np.linalg.norm(u)
    return u, np.cross(n, u)


def candidate_lists(pos, nrm, r2, prm):
    """Per slot: the candidate indices (after all three drops) and their projections; plus the truncated-list count."""
    n = pos.shape[0]
    live = live_mask(pos, r2)
    ids = np.nonzero(live)[0]
    out = [None] * n
    truncated = 0
    if ids.size == 0:
        return out, live, truncated
    tree = cKDTree(pos[ids])
    cosn = math.cos(math.radians(prm.max_angle_between_normals_deg))
    f2 = float(np.float32(prm.search_radius_factor) * np.float32(prm.search_radius_factor))
    for p in ids:
        rr = f2 * r2[p]
        near = ids[np.asarray(tree.query_ball_point(pos[p], math.sqrt(rr) * (1 + 1e-9) + 1e-300), dtype=np.int64)]
        d2 = np.sum((pos[near] - pos[p]) ** 2, axis=1)
        keep = d2 <= rr
        near, d2 = near[keep], d2[keep]
        order = np.lexsort((near, d2))[:prm.max_neighbors]
        if order.size == prm.max_neighbors:
            truncated += 1
        near = near[order]
        near = near[near != p]
        near = near[nrm[near] @ nrm[p] > cosn]
        u, v = basis(nrm[p])
        d = pos[near] - pos[p]
        xy = np.stack([d @ u, d @ v], axis=1) if near.size else np.zeros((0, 2))
        ok = np.sum(xy * xy, axis=1) > 1e-12 * r2[p]
        out[p] = (near[ok], xy[ok])
    return out, live, truncated


def star_of(cand, xy):
    """The star of the origin: a set of frozenset({a, b}) of slot indices, or None if the ring is too long."""
    if cand.size < 2:
        return set()
    pts = np.vstack([np.zeros((1, 2)), xy])
    try:
        tri = Delaunay(pts).simplices
    except QhullError:
        return set()
    star = set()
    for s in tri[np.any(tri == 0, axis=1)]:
        a, b = [int(cand[k - 1]) for k in s if k != 0]
        star.add(frozenset((a, b)))
    nbrs = set()
    for e in star:
        nbrs |= e
    return None if len(nbrs) > MAX_STAR_DEGREE else star


def stars(pos, nrm, r2, prm):
    lists, live, truncated = candidate_lists(pos, nrm, r2, prm)
    out, overflow = {}, 0
    for p in np.nonzero(live)[0]:
        s = star_of(*lists[p])
        if s is None:
            overflow += 1
            s = set()
        out[int(p)] = s
    return out, live, truncated, overflow


def _angles_ok(P, prm):
    lo, hi = math.radians(prm.min_triangle_angle_deg), math.radians(prm.max_triangle_angle_deg)
    for k in range(3):
        e, f = P[(k + 1) % 3] - P[k], P[(k + 2) % 3] - P[k]
        den = math.sqrt((e @ e) * (f @ f))
        if not den > 0:
            return False
        a = math.acos(max(-1.0, min(1.0, (e @ f) / den)))
        if not lo <= a <= hi:
            return False
    return True


def filter_and_orient(t, pos, nrm, prm):
    """None, or the triangle (p, a, b): p smallest, counter-clockwise seen from the oriented normal's side."""
    p, a, b = sorted(t)
    P = pos[[p, a, b]]
    if not _angles_ok(P, prm):
        return None
    tn = np.cross(P[1] - P[0], P[2] - P[0])
    s = tn @ (nrm[p] + nrm[a] + nrm[b])
    if s == 0:
        return None
    if s < 0:
        tn, a, b = -tn, b, a
    if not (tn @ nrm[p] > 0 and tn @ nrm[a] > 0 and tn @ nrm[b] > 0):
        return None
    return (p, a, b)


def triangulate(pos, nrm, r2, prm=None):
    """Returns (triangles [T,3] uint32 in the contract's order, stats dict, star triangle set)."""
    prm = prm or Params()
    st, live, truncated, overflow = stars(pos, nrm, r2, prm)
    all_star = set()
    for p, s in st.items():
        for e in s:
            all_star.add(frozenset((p,) + tuple(e)))
    out = []
    for t in all_star:
        p, a, b = tuple(t)
        if (frozenset((a, b)) in st[p] and frozenset((p, b)) in st.get(a, ()) and frozenset((p, a)) in st.get(b, ())):
            o = filter_and_orient(t, pos, nrm, prm)
            if o is not None:
                out.append(o)
    out.sort()
    tri = np.array(out, np.uint32).reshape(-1, 3)
    stats = {"n_live": int(live.sum()), "n_star_triangles": len(all_star), "n_triangles": tri.shape[0],
             "star_overflow": overflow, "truncated_lists": truncated}
    return tri, stats, all_star


def filter_mask(tri, pos, nrm, prm):
    """filter_and_orient's verdict for many triangles at once (True = kept)."""
    tri = np.asarray(tri).reshape(-1, 3).astype(np.int64)
    P = pos[tri]
    lo, hi = math.radians(prm.min_triangle_angle_deg), math.radians(prm.max_triangle_angle_deg)
    ok = np.ones(tri.shape[0], bool)
    for k in range(3):
        e, f = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
        den = np.sqrt(np.sum(e * e, axis=1) * np.sum(f * f, axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            a = np.arccos(np.clip(np.sum(e * f, axis=1) / den, -1.0, 1.0))
        ok &= (den > 0) & (a >= lo) & (a <= hi)
    tn = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    s = np.sum(tn * (nrm[tri[:, 0]] + nrm[tri[:, 1]] + nrm[tri[:, 2]]), axis=1)
    tn = tn * np.sign(s)[:, None]
    ok &= s != 0
    for k in range(3):
        ok &= np.sum(tn * nrm[tri[:, k]], axis=1) > 0
    return ok


def _keys(tri):
    """One sortable record per triangle, corners in ascending order."""
    t = np.sort(np.asarray(tri).reshape(-1, 3).astype(np.uint32), axis=1)
    return np.ascontiguousarray(t).view([("a", "u4"), ("b", "u4"), ("c", "u4")]).reshape(-1)


def as_set(tri):
    return set(frozenset(int(v) for v in t) for t in np.asarray(tri).reshape(-1, 3))


def assert_sets_close(got, want, what=""):
    """The comparison rule for sets: a symmetric difference of at most ceil(0.001 T_model) triangles (float32 against
    float64 signs on near-cocircular quadruples); the differing triangles are printed."""
    g, w = np.unique(_keys(got)), np.unique(_keys(want))
    only_g, only_w = np.setdiff1d(g, w), np.setdiff1d(w, g)
    diff = only_g.size + only_w.size
    cap = math.ceil(0.001 * w.size)
    print("%s: %d differing triangles of %d (cap %d)" % (what, diff, w.size, cap))
    if diff:
        print("  only in the result: %s\n  only in the reference: %s" % (only_g[:20].tolist(), only_w[:20].tolist()))
    assert diff <= cap, "%s: %d differing triangles, cap %d (reference %d, got %d)" % (what, diff, cap, w.size, g.size)
    return diff


def check_properties(tri, pos, nrm, r2, prm=None):
    """The properties that follow from the definition, on a full output (no exclusions)."""
    prm = prm or Params()
    tri = np.asarray(tri).reshape(-1, 3).astype(np.int64)
    n = pos.shape[0]
    if tri.shape[0] == 0:
        return
    live = live_mask(pos, r2)
    assert tri.min() >= 0 and tri.max() < n and np.all(live[tri]), "an index is not live"
    assert np.all(tri[:, 0] < tri[:, 1]) and np.all(tri[:, 0] < tri[:, 2]), "p is not the smallest index"
    assert np.all(tri[:, 1] != tri[:, 2])
    a, b = tri[:-1], tri[1:]
    ordered = (a[:, 0] < b[:, 0]) | ((a[:, 0] == b[:, 0]) & ((a[:, 1] < b[:, 1]) | ((a[:, 1] == b[:, 1]) & (a[:, 2] < b[:, 2]))))
    assert np.all(ordered), "not in (strictly) lexicographic order"
    assert np.unique(_keys(tri)).size == tri.shape[0], "a triangle appears twice"
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [0, 2]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert counts.max() <= 2, "an edge is in %d triangles" % counts.max()
    # (the inequality as smx_nn decides it: float32 differences, squares and left-to-right sum, float32 factor^2 r^2)
    f2 = np.float32(prm.search_radius_factor) * np.float32(prm.search_radius_factor)
    d = pos[edges[:, 0]].astype(np.float32) - pos[edges[:, 1]].astype(np.float32)
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    bound = f2 * np.minimum(r2[edges[:, 0]], r2[edges[:, 1]]).astype(np.float32)
    assert d2.dtype == np.float32 and bound.dtype == np.float32
    assert np.all(d2 <= bound), "an edge is longer than the smaller ball"
    P = pos[tri]
    lo, hi = math.radians(prm.min_triangle_angle_deg), math.radians(prm.max_triangle_angle_deg)
    for k in range(3):
        e, f = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
        c = np.sum(e * f, axis=1) / np.sqrt(np.sum(e * e, axis=1) * np.sum(f * f, axis=1))
        a = np.arccos(np.clip(c, -1, 1))
        # (the kernel compares float32 cosines: a few units of 2^-24 in the cosine are, at the limits' default 10 / 170
        # degrees, 4 * 6e-8 / sin(10 deg) = 1.4e-6 rad in the angle; 1e-5 covers that and nothing a filter would miss)
        assert np.all(a >= lo - 1e-5) and np.all(a <= hi + 1e-5), "an interior angle is outside the limits"
    tn = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    for k in range(3):
        assert np.all(np.sum(tn * nrm[tri[:, k]], axis=1) > 0), "winding against a corner's normal"


# ---- fixtures of the issue ----
def plane_map(side=40, jitter=0.3, r=2.1, seed=0):
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-jitter, jitter, (side * side, 2))
    pos = np.concatenate([xy, np.zeros((xy.shape[0], 1))], axis=1).astype(np.float32).astype(np.float64)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (pos.shape[0], 1))
    r2 = np.full(pos.shape[0], np.float64(np.float32(r * r)))
    return pos, nrm, r2


NO_ANGLE_LIMITS = dict(min_triangle_angle_deg=0.0, max_triangle_angle_deg=180.0)


def global_delaunay_short(pos, r2, nrm=None, prm=None):
    """Triangles of the global 2-D Delaunay triangulation of a planar map whose edges all have d^2 <= r^2; with nrm and
    prm, of those the ones that pass the definition's triangle filters (slivers along the hull do not, at 10 degrees)."""
    tri = Delaunay(pos[:, :2]).simplices
    keep = np.ones(tri.shape[0], bool)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        keep &= np.sum((pos[tri[:, a]] - pos[tri[:, b]]) ** 2, axis=1) <= np.minimum(r2[tri[:, a]], r2[tri[:, b]])
    tri = tri[keep]
    if prm is not None:
        tri = tri[filter_mask(tri, pos, nrm, prm)]
    return tri


def sphere_map(n=4000, normal_noise=0.05, radial_noise=0.003, seed=1):
    """Random points on the unit sphere; radii 2.2 x spacing x U(0.9, 1.2) with spacing = sqrt(4 pi / n)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = d * (1.0 + radial_noise * rng.standard_normal((n, 1)))
    nrm = d + normal_noise * rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    spacing = math.sqrt(4 * math.pi / n)
    r = 2.2 * spacing * rng.uniform(0.9, 1.2, n)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(pos), f32(nrm), f32(r * r)


def rows_of_map(pos, nrm, r2):
    """Surfel rows [25, n] (float32) holding a map: raw = smooth position, confidence 1, no links."""
    n = pos.shape[0]
    rows = np.zeros((25, n), np.float32)
    rows[0:3] = pos.T
    rows[3:6] = pos.T
    rows[6] = 1.0
    rows[7] = r2
    rows[8:11] = nrm.T
    rows[19:23] = np.full((4, n), 0xFFFFFFFF, np.uint32).view(np.float32)
    return rows
