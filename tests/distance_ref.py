"""The model of smx_recon_mesh_distance (include/smx.h), shared by the model, host, API and GPU tests.

The model is BRUTE FORCE: every point against every triangle of R in numpy float32, each operation of the contract's step 3
written out as one numpy operation (one rounding each, no contraction), chunked over the points.  It knows no grid, so it
cannot share a mistake of the search structure.  Because the key of step 4 orders by dist2 first, the smallest key over the
candidates is the smallest key over all of R if that one is a candidate and "none" otherwise; the model therefore keeps one
winner per (triangle array, point set) and applies max_distance afterwards (answer()).

It also holds a float64 statement of the DEFINITION (definition64: the distance to the plane where the projection falls inside
the triangle, else the smallest of the distances to the three segments -- not Ericson's branches), the grid's counts for an
explicit cell_size (structure()), and the case builders (world(), point_sets())."""
import functools

import numpy as np

import fill_cases as fc
import mesh_ref as mr

INVALID = 0xFFFFFFFF
MAX_COORD = np.float32(64.0)
WIDE_CELLS = 64
BINS = 32
MARGIN = np.float32(1.125)
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "inside")
STAT_NAMES = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_points", "n_bad_points", "n_matched", "max_dist2_bits")
MAX_PAIRS = 30_000_000
F = np.float32


def live_mask(pos32, r2):
    return ~(np.asarray(r2) < 0) & np.all(np.isfinite(pos32), axis=1)


def classify(pos, r2, tri):
    """Step 1: (R's rows of tri, their input positions t, dict of the three drop counts).  ValueError on an index >= n."""
    pos32 = np.asarray(pos).astype(F)
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    if tri.size and int(tri.max()) >= pos32.shape[0]:
        raise ValueError("index out of range")
    idx = tri.astype(np.int64)
    live = np.all(live_mask(pos32, r2)[idx], axis=1) if tri.size else np.zeros(0, bool)
    repeated = live & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2]))
    rest = live & ~repeated
    with np.errstate(invalid="ignore"):
        far = rest & np.any(np.abs(pos32[idx]) > MAX_COORD, axis=(1, 2)) if tri.size else rest
    keep = rest & ~far
    counts = dict(n_in=int(tri.shape[0]), n_not_live=int(np.sum(~live)), n_repeated=int(np.sum(repeated)), n_out_of_range=int(np.sum(far)))
    return tri[keep], np.flatnonzero(keep).astype(np.uint32), counts


def bad_points(points):
    p = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return ~np.all(np.isfinite(p), axis=1) | np.any(np.abs(p) > MAX_COORD, axis=1)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _closest(P, A, B, C):
    """Step 3 on broadcastable tuples of three float32 arrays: (Q as a tuple, region).  Every branch is evaluated for every
    pair and the first matching one selected; float32 throughout."""
    sub = lambda u, v: (u[0] - v[0], u[1] - v[1], u[2] - v[2])                      # noqa: E731
    add = lambda u, v: (u[0] + v[0], u[1] + v[1], u[2] + v[2])                      # noqa: E731
    mul = lambda s, u: (s * u[0], s * u[1], s * u[2])                               # noqa: E731
    with np.errstate(all="ignore"):
        ab, ac, ap = sub(B, A), sub(C, A), sub(P, A)
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        in_a = (d1 <= 0) & (d2 <= 0)
        bp = sub(P, B)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        in_b = (d3 >= 0) & (d4 <= d3)
        vc = d1 * d4 - d3 * d2
        in_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        q_ab = add(A, mul(d1 / (d1 - d3), ab))
        cp = sub(P, C)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        in_c = (d6 >= 0) & (d5 <= d6)
        vb = d5 * d2 - d1 * d6
        in_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        q_ac = add(A, mul(d2 / (d2 - d6), ac))
        va = d3 * d6 - d5 * d4
        in_bc = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
        q_bc = add(B, mul((d4 - d3) / ((d4 - d3) + (d5 - d6)), sub(C, B)))
        s = (va + vb) + vc
        v, w = vb / s, vc / s
        v = np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)        # held to the triangle; a NaN stays one
        lim = F(1) - v
        w = np.where(w < 0, F(0), np.where(w > lim, lim, w)).astype(F)
        q_in = add(add(A, mul(v, ab)), mul(w, ac))
    conds = [in_a, in_b, in_ab, in_c, in_ac, in_bc]
    shape = np.broadcast(in_a, in_b).shape
    region = np.select(conds, list(range(6)), 6).astype(np.uint8)
    full = lambda x: np.broadcast_to(x, shape)                                      # noqa: E731
    Q = tuple(np.select(conds, [full(A[k]), full(B[k]), q_ab[k], full(C[k]), q_ac[k], q_bc[k]], q_in[k]).astype(F) for k in range(3))
    return Q, region


def _dist2(P, Q):
    with np.errstate(all="ignore"):
        e = (P[0] - Q[0], P[1] - Q[1], P[2] - Q[2])
        return _dot(e, e)


def brute(pos, r2, tri, points, chunk_pairs=1 << 20):
    """The winner of every point over ALL of R, whatever max_distance: dict of d2 (float32, +inf where no triangle gives a
    number or the point is BAD), t, Q [P,3], negative (the sign test of step 4), region, ties (triangles of R with the winner's
    dist2).  At most MAX_PAIRS point-triangle pairs."""
    pos32 = np.asarray(pos).astype(F)
    R, t_of, counts = classify(pos, r2, tri)
    pts = np.ascontiguousarray(points, F).reshape(-1, 3)
    n_p, n_r = pts.shape[0], R.shape[0]
    assert n_p * max(n_r, 1) <= MAX_PAIRS, "%d x %d pairs" % (n_p, n_r)
    bad = bad_points(pts)
    out = dict(d2=np.full(n_p, np.inf, F), t=np.full(n_p, INVALID, np.uint32), Q=np.full((n_p, 3), np.nan, F),
               negative=np.zeros(n_p, bool), region=np.full(n_p, 255, np.uint8), ties=np.zeros(n_p, np.int64), bad=bad, counts=counts)
    if n_r == 0 or n_p == 0:
        return out
    corners = [tuple(pos32[R[:, c].astype(np.int64), k][None, :] for k in range(3)) for c in range(3)]
    step = max(1, chunk_pairs // n_r)
    for lo in range(0, n_p, step):
        sl = slice(lo, min(n_p, lo + step))
        P = tuple(pts[sl, k][:, None] for k in range(3))
        Q, region = _closest(P, *corners)
        d2 = _dist2(P, Q)
        with np.errstate(invalid="ignore"):
            key = np.where(d2 >= 0, (d2.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | t_of[None, :].astype(np.uint64),
                           np.uint64(0xFFFFFFFFFFFFFFFF))
        win = np.argmin(key, axis=1)
        rows = np.arange(win.size)
        wd2 = d2[rows, win]
        ok = ~np.isnan(wd2) & ~bad[sl]
        out["d2"][sl] = np.where(ok, wd2, np.inf)
        out["t"][sl] = np.where(ok, t_of[win], INVALID)
        for k in range(3):
            out["Q"][sl, k] = np.where(ok, Q[k][rows, win], np.nan)
        out["region"][sl] = np.where(ok, region[rows, win], 255)
        out["ties"][sl] = np.where(ok, np.sum(d2 == wd2[:, None], axis=1), 0)
        # the sign of the winner: dot(e, cross(ab, ac)) < 0
        A, B, C = (tuple(c[k][0, win] for k in range(3)) for c in corners)
        Pw, Qw = tuple(pts[sl, k] for k in range(3)), tuple(Q[k][rows, win] for k in range(3))
        with np.errstate(all="ignore"):
            e = tuple(Pw[k] - Qw[k] for k in range(3))
            ab, ac = tuple(B[k] - A[k] for k in range(3)), tuple(C[k] - A[k] for k in range(3))
            cr = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
            out["negative"][sl] = ok & (_dot(e, cr) < 0)
    return out


def answer(model, max_distance, signed=False):
    """Steps 4 and 5 for one max_distance on a brute() result: (nearest, distance, closest, stats)."""
    m = F(max_distance)
    cand = model["d2"] <= m * m
    nearest = np.where(cand, model["t"], INVALID).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.where(cand, model["d2"], F(0))).astype(F)
    mag = d.copy()
    if signed:
        d = np.where(model["negative"], -d, d).astype(F)
    distance = np.where(cand, d, F(np.inf)).astype(F)
    closest = np.where(cand[:, None], model["Q"], F(np.nan)).astype(F)
    stats = dict(model["counts"])
    stats.update(n_points=int(cand.size), n_bad_points=int(np.sum(model["bad"])), n_matched=int(np.sum(cand)),
                 max_dist2_bits=int(model["d2"][cand].view(np.uint32).max()) if np.any(cand) else 0)
    bins = np.minimum(BINS - 1, ((mag[cand] * F(32.0)) / m).astype(np.uint32))
    stats["histogram"] = np.bincount(bins, minlength=BINS).astype(np.int64).tolist()
    stats["max_distance"] = float(m)
    return nearest, distance, closest, stats


def cell_used(cell_size, max_distance):
    return max(F(cell_size), MARGIN * F(max_distance))


def structure(pos, r2, tri, cell_size, max_distance):
    """n_wide, n_entries, n_cells of the grid for an explicit cell_size > 0."""
    pos32 = np.asarray(pos).astype(F)
    R, _, _ = classify(pos, r2, tri)
    c = cell_used(cell_size, max_distance)
    p = pos32[R.astype(np.int64)]                                 # [r, 3 corners, 3 axes]
    lo = np.floor(p.min(axis=1) / c).astype(np.int64)
    hi = np.floor(p.max(axis=1) / c).astype(np.int64)
    dims = hi - lo + 1
    cells = dims[:, 0] * dims[:, 1] * dims[:, 2]
    wide = cells > WIDE_CELLS
    keys = []
    for j in range(WIDE_CELLS):
        m = ~wide & (cells > j)
        if not np.any(m):
            break
        nx, ny = dims[m, 0], dims[m, 1]
        cx, cy, cz = lo[m, 0] + j % nx, lo[m, 1] + (j // nx) % ny, lo[m, 2] + j // (nx * ny)
        keys.append(((cx + (1 << 20)) << 42) | ((cy + (1 << 20)) << 21) | (cz + (1 << 20)))
    n_cells = int(np.unique(np.concatenate(keys)).size) if keys else 0
    return dict(n_wide=int(np.sum(wide)), n_entries=int(np.sum(cells[~wide])), n_cells=n_cells)


def definition64(pos, r2, tri, points, chunk_pairs=1 << 20):
    """The definition in float64 on the float32 inputs: per point the smallest distance to a triangle of R (+inf without R).
    Inside the triangle's prism the distance to its plane, otherwise the smallest distance to its three segments."""
    pos64 = np.asarray(pos).astype(F).astype(np.float64)
    R, _, _ = classify(pos, r2, tri)
    pts = np.ascontiguousarray(points, F).reshape(-1, 3).astype(np.float64)
    out = np.full(pts.shape[0], np.inf)
    if R.shape[0] == 0:
        return out
    A, B, C = (pos64[R[:, k].astype(np.int64)][None, :, :] for k in range(3))
    n = np.cross(B - A, C - A)
    nn = np.sum(n * n, axis=2)

    def segment(P, U, V):
        d = V - U
        dd = np.sum(d * d, axis=2)
        with np.errstate(all="ignore"):
            s = np.clip(np.where(dd > 0, np.sum((P - U) * d, axis=2) / dd, 0.0), 0.0, 1.0)
        q = U + s[..., None] * d
        return np.sqrt(np.sum((P - q) ** 2, axis=2))
    step = max(1, chunk_pairs // R.shape[0])
    for lo in range(0, pts.shape[0], step):
        P = pts[lo:lo + step][:, None, :]
        best = np.minimum(np.minimum(segment(P, A, B), segment(P, B, C)), segment(P, C, A))
        with np.errstate(all="ignore"):
            inside = (nn > 0)
            for U, V in ((A, B), (B, C), (C, A)):
                inside = inside & (np.sum(np.cross(V - U, P - U) * n, axis=2) >= 0)
            plane = np.abs(np.sum((P - A) * n, axis=2)) / np.sqrt(nn)
        best = np.where(inside, np.minimum(best, plane), best)
        out[lo:lo + step] = best.min(axis=1)
    out[bad_points(points)] = np.inf
    return out


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
HAND_AT = np.array([-3.0, 0.0, 0.0])
MAX_DISTANCES = (0.002, 0.02, 0.5)


def _f32(a):
    return np.asarray(a).astype(F).astype(np.float64)


@functools.lru_cache(maxsize=None)
def world():
    """(pos, nrm, r2, triangles, info): the noisy sphere triangulated by mesh_ref (slots 0 .. 3999), the holed plane of
    fill_cases scaled to the sphere's spacing at x = 3, and twelve hand-made triangles at x = -3: a dead slot, a repeated
    index, two slots at one position, three collinear slots, one long triangle for the wide list, one corner at 65 m, the same
    triangle twice and once more with the other winding, and four ordinary ones.  Read-only."""
    sp, sn, sr = mr.sphere_map()
    stri = mr.triangulate(sp, sn, sr)[0]
    pp, pn, pr, ptri = fc.holed_plane()
    hand = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0],          # 0 1 2: an ordinary triangle (and its copies)
                     [0.3, 0.0, 0.0], [0.3, 0.0, 0.0], [0.3, 0.1, 0.0],          # 3 4: one position
                     [0.5, 0.0, 0.0], [0.55, 0.05, 0.0], [0.6, 0.1, 0.0],        # 6 7 8: collinear
                     [0.0, 0.5, 0.0], [1.0, 0.5, 0.02], [0.0, 0.6, 0.3],         # 9 10 11: long (the wide list)
                     [68.0, 0.0, 0.0],                                           # 12: at 65 m once HAND_AT is added
                     [0.0, -0.3, 0.0],                                           # 13: dead
                     [0.0, 0.0, 0.2], [0.1, 0.0, 0.2], [0.0, 0.1, 0.25], [0.1, 0.1, 0.2]]) + HAND_AT     # 14 .. 17
    n0 = sp.shape[0] + pp.shape[0]
    h = lambda *k: [n0 + v for v in k]                                              # noqa: E731
    htri = np.array([h(13, 0, 1), h(0, 0, 1), h(3, 4, 5), h(6, 7, 8), h(9, 10, 11), h(12, 0, 2), h(0, 1, 2), h(0, 1, 2), h(0, 2, 1),
                     h(14, 15, 16), h(15, 17, 16), h(1, 2, 5)], np.uint32)
    pos = np.concatenate([sp, _f32(pp * 0.05 + np.array([3.0, 0.0, 0.0])), _f32(hand)])
    nrm = np.concatenate([sn, pn, np.tile(np.array([0.0, 0.0, 1.0]), (hand.shape[0], 1))])
    hr = np.full(hand.shape[0], 0.01)
    hr[13] = -1.0
    r2 = np.concatenate([sr, _f32(np.where(pr < 0, -1.0, pr * 0.0025)), _f32(hr)])
    tri = np.ascontiguousarray(np.concatenate([stri, ptri + np.uint32(sp.shape[0]), htri]), np.uint32)
    info = dict(n_sphere=sp.shape[0], n_sphere_tri=stri.shape[0], n_plane_tri=ptri.shape[0], hand_first=n0, hand_tri=tri.shape[0] - 12)
    for a in (pos, nrm, r2, tri):
        a.setflags(write=False)
    return pos, nrm, r2, tri, info


@functools.lru_cache(maxsize=None)
def point_sets():
    """name -> [m, 3] float32 (read-only), m <= 4096 and m x triangles <= MAX_PAIRS."""
    pos, nrm, r2, tri, info = world()
    rng = np.random.default_rng(11)
    ns, nt = info["n_sphere"], info["n_sphere_tri"]
    sp = pos[:ns]
    out_dir = sp / np.linalg.norm(sp, axis=1, keepdims=True)
    used = np.unique(tri[:nt])
    pick = used[rng.permutation(used.size)[:300]].astype(np.int64)
    sets = {}
    sets["vertices 0 / 1 / 5 mm"] = np.concatenate([sp[pick] + k * out_dir[pick] for k in (0.0, 0.001, 0.005)])
    T = tri[rng.permutation(nt)[:700]].astype(np.int64)
    mid = 0.5 * (pos[T[:, 0]] + pos[T[:, 1]])
    sets["edge midpoints moved outward"] = mid + 0.002 * mid / np.linalg.norm(mid, axis=1, keepdims=True)
    T = tri[rng.permutation(nt)[:350]].astype(np.int64)
    cen = (pos[T[:, 0]] + pos[T[:, 1]] + pos[T[:, 2]]) / 3.0
    fn = np.cross(pos[T[:, 1]] - pos[T[:, 0]], pos[T[:, 2]] - pos[T[:, 0]])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    sets["centroids moved both ways"] = np.concatenate([cen + 0.003 * fn, cen - 0.003 * fn])
    few = pick[:80]
    sets["shell at max_distance"] = np.concatenate([sp[few] + (m * f) * out_dir[few] for m in MAX_DISTANCES for f in (0.999, 1.0, 1.001)])
    grid = []
    for m in MAX_DISTANCES:
        c = MARGIN * F(m)
        grid.append((np.rint(sp[pick[:230]].astype(F) / c) * c).astype(F))
    sets["multiples of c"] = np.concatenate(grid)
    box = rng.uniform(-1.3, 1.3, (500, 3))
    near_plane = np.array([3.0, 0.0, 0.0]) + rng.uniform(-0.2, 2.2, (200, 3)) * np.array([1.0, 1.0, 0.02])
    sets["random in the box"] = np.concatenate([box, near_plane])
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [65.0, 0, 0], [0, -64.5, 0], [0, 0, 1e30], [np.nan] * 3, [64.0, 64.0, -64.0]])
    good = sp[pick[:24]] + 0.001
    sets["NaN, inf and 65 m"] = np.concatenate([bad[:4], good[:12], bad[4:], good[12:]])
    hp = pos[info["hand_first"]:]
    hand = [hp + d for d in ([0, 0, 0], [0, 0, 0.001], [0, 0, -0.004], [0.003, 0.002, 0.0], [-0.01, -0.01, 0.01])]
    along = HAND_AT + np.stack([np.linspace(-0.05, 1.05, 60), np.full(60, 0.52), np.linspace(0.0, 0.05, 60)], axis=1)
    inside = HAND_AT + np.stack([rng.uniform(0, 0.1, 100), rng.uniform(0, 0.1, 100), rng.uniform(-0.01, 0.26, 100)], axis=1)
    sets["around the hand-made triangles"] = np.concatenate(hand + [along, inside])
    done = {}
    for k, v in sets.items():
        a = np.ascontiguousarray(v, F)
        assert a.shape[0] <= 4096 and a.shape[0] * tri.shape[0] <= MAX_PAIRS, k
        a.setflags(write=False)
        done[k] = a
    return done


_MODELS = {}


def model_of(name):
    """brute() of the world against one point set, computed once per process and left unchanged."""
    if name not in _MODELS:
        pos, nrm, r2, tri, _ = world()
        m = brute(pos, r2, tri, point_sets()[name])
        for v in m.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _MODELS[name] = m
    return _MODELS[name]
