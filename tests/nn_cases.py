"""Constructed clouds and query sets that put the neighbour search (surfelmeshing_amd/csrc/smx_nn.hip) on both sides of
every threshold of its dispatch (test infrastructure, no GPU needed).  tests/nn_model.py says which route a case takes;
tests/test_nn_cases.py asserts, without a GPU, that the cases reach what they claim and keep the margin rule;
tests/test_gpu_nn_cases.py compares every row with brute force on the device.

All coordinates are dyadic fractions of a power-of-two cell, so cell coordinates are exact in float32, and query points
sit away from cell faces.  Every cloud but the build clouds starts with an anchor point at the origin and has no negative
coordinate: the grid's min is (0, 0, 0) whatever else the cloud holds, and "cell 2.5" below means 2.5 cells from it.

A case is a Case tuple; `queries is None` means the self-query (every indexed point asks with r2[i]).  `expect` names the
lanes routes / tiles regimes the case exists to reach, `designed` the match counts it was built to have (None where the
count is not the point of the case; a dict {query: count} where only some are designed)."""
from collections import OrderedDict, namedtuple

import numpy as np

F = np.float32

Case = namedtuple("Case", "name points cell queries r2 K state skip_mask expect designed group")

CLUSTER_SIZES = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100)
SWEEP_K = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
LATTICE_M = OrderedDict([(0, 1), (1, 7), (2, 19), (3, 27), (4, 33), (5, 57), (6, 81), (8, 93), (9, 123)])   # r^2 / h^2 -> interior count
TILE_N = (63, 64, 65, 128, 129, 255, 256, 257, 300)
TILE_P = (0, 200, 255)
SELF_TILE_N = (64, 65, 129, 257)


def _f(a):
    return np.ascontiguousarray(a, F)


# ---- exact-count clusters ------------------------------------------------------------------------------------------------
def _cluster_offsets(c, rng):
    """c offsets in units of cell / 64, each component within +-12: the centre when c is odd, mirror pairs about the centre
    (equal dist^2 from it), and for c >= 4 a quarter exact duplicates of other members (ties resolved by index)."""
    dup = c // 4
    rest, seen = [], set()
    if (c - dup) % 2:
        rest.append((0, 0, 0))
    while len(rest) < c - dup:
        o = tuple(int(v) for v in rng.integers(-12, 13, 3))
        if o == (0, 0, 0) or o in seen:
            continue
        seen |= {o, tuple(-v for v in o)}
        rest += [o, tuple(-v for v in o)]
    rest = rest[:c - dup]
    out = rest + [rest[i % len(rest)] for i in range(dup)]
    return np.array(out, np.int64)[rng.permutation(c)]


def cluster_cloud(sizes, cell, seed):
    """Anchor + one cluster per size: centres at cells 8.5 + 16 k (four bricks apart), members within 0.19 cell of the centre
    in every axis (diameter 0.65 cell).  Returns points, centres [len(sizes), 3], member index lists."""
    rng = np.random.default_rng(seed)
    pts, centres, members = [np.zeros((1, 3))], [], []
    n = 1
    for i, c in enumerate(sizes):
        ctr = (np.array([i % 4, (i // 4) % 4, i // 16], np.float64) * 16 + 8.5) * cell
        pts.append(ctr + _cluster_offsets(c, rng) * (cell / 64.0))
        centres.append(ctr)
        members.append(np.arange(n, n + c))
        n += c
    return _f(np.concatenate(pts)), _f(np.array(centres)), members


R_BATCH, R_SELF = 0.45, 0.75        # cells: a centre sees its cluster, a member sees its cluster


def _cluster_cases():
    cell = 0.25
    pts, ctr, mem = cluster_cloud(CLUSTER_SIZES, cell, 1)
    exp = {"net8", "net16", "rank", "redo_count", "staged", "one_round"}
    yield Case("clusters_batch", pts, cell, ctr, _f((R_BATCH * cell) ** 2), 64, None, 0, exp, np.array(CLUSTER_SIZES), "clusters")
    own = np.ones(len(pts), np.int64)
    for m in mem:
        own[m] = len(m)
    yield Case("clusters_self", pts, cell, None, np.full(len(pts), (R_SELF * cell) ** 2, F), 64, None, 0, exp, own, "clusters")
    yield Case("clusters_self_k6", pts, cell, None, np.full(len(pts), (R_SELF * cell) ** 2, F), 6, None, 0, exp, own, "clusters")


def _sweep_cases():
    cell = 0.25
    sizes = sorted({c for k in SWEEP_K for c in (k - 1, k, k + 1) if c >= 1})
    pts, ctr, _ = cluster_cloud(sizes, cell, 2)
    for k in SWEEP_K:
        sel = [sizes.index(c) for c in (k - 1, k, k + 1) if c >= 1]
        yield Case("ksweep_K%d" % k, pts, cell, ctr[sel], _f((R_BATCH * cell) ** 2), k, None, 0, set(),
                   np.array([sizes[i] for i in sel]), "ksweep")


# ---- the state filter: geometric count on one side of 8 / 16 / 32, filtered count on the other ------------------------------
FILTER_PAIRS = ((12, 8), (9, 8), (20, 16), (17, 16), (40, 32), (33, 32), (36, 17), (64, 9), (100, 33), (8, 8), (5, 0))


def _filter_cases():
    cell = 0.25
    pts, ctr, mem = cluster_cloud([g for g, _ in FILTER_PAIRS], cell, 3)
    rng = np.random.default_rng(33)
    state = (rng.integers(0, 2, len(pts)) * 1 + rng.integers(0, 2, len(pts)) * 4).astype(np.uint8)    # bits the mask ignores
    own = np.ones(len(pts), np.int64)
    for m, (g, f) in zip(mem, FILTER_PAIRS):
        state[rng.permutation(m)[:g - f]] |= 2
        own[m] = f
    exp = {"net8", "net16", "rank", "redo_count"}
    yield Case("filter_batch", pts, cell, ctr, _f((R_BATCH * cell) ** 2), 64, state, 2, exp, np.array([f for _, f in FILTER_PAIRS]), "filter")
    yield Case("filter_self_k7", pts, cell, None, np.full(len(pts), (R_SELF * cell) ** 2, F), 7, state, 2, exp, own, "filter")


# ---- mixed chunks: 64 queries of one brick, one long list among short ones ----------------------------------------------------
def _mixed_cases():
    cell, d = 0.5, 0.5 / 128
    c = np.array([2.5, 2.5, 2.5]) * cell
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64)
    pts = _f(np.concatenate([np.zeros((1, 3)), [c + axes[i % 6] * (i + 1) * d for i in range(40)]]))   # point i + 1 at distance (i + 1) d
    lanes = np.arange(64)

    def case(name, counts, k, exp):
        r2 = _f(((np.asarray(counts) + 0.5) * d) ** 2)
        return Case(name, pts, cell, _f(np.tile(c, (64, 1))), r2, k, None, 0, exp, np.asarray(counts), "mixed")
    yield case("mixed_8", 1 + lanes % 8, 64, {"net8"})
    a = 1 + lanes % 8
    a[37] = 9
    yield case("mixed_9", a, 10, {"net16"})
    yield case("mixed_16", 1 + lanes % 16, 64, {"net16"})
    a = 1 + lanes % 16
    a[5] = 17
    yield case("mixed_17", a, 12, {"rank"})
    yield case("mixed_32", 1 + lanes % 32, 64, {"rank"})
    a = 1 + lanes % 32
    a[11] = 33
    yield case("mixed_33", a, 64, {"rank", "redo_count"})
    a = 1 + lanes % 32
    a[[0, 13, 63]] = (33, 36, 40)
    yield case("mixed_33s", a, 33, {"rank", "redo_count"})
    a = 1 + lanes % 8
    a[20] = 34
    yield case("mixed_8_and_34", a, 5, {"net8", "redo_count"})     # the long list leaves: the short ones take the 8-input network


# ---- lattice: d^2 == r^2 wholesale, shells of ties, matches one radius away across cell and brick faces ----------------------
def _lattice_cases():
    h = 2.0 ** -6
    cell = 4 * h
    off = 14.5                      # lattice point j lies at cell (j + 14.5) / 4: an eighth of a cell off the faces, j = 2 opens brick 1
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    pts = _f(np.concatenate([np.zeros((1, 3)), (g + off) * h]))
    interior = np.all((g >= 3) & (g <= 8), axis=1)
    for m, cnt in LATTICE_M.items():
        des = {int(i): cnt for i in np.flatnonzero(interior)}
        yield Case("lattice_m%d" % m, pts, cell, pts[1:], _f(m * h * h), 64, None, 0, set(), des, "lattice")
    des = {int(i) + 1: 27 for i in np.flatnonzero(interior)}
    yield Case("lattice_self_m3_k10", pts, cell, None, np.full(len(pts), 3 * h * h, F), 10, None, 0, set(), des, "lattice")


# ---- stage capacity -------------------------------------------------------------------------------------------------------
def _stage_cases():
    cell = 0.5
    # two queries in opposite corners of brick (1, 1, 1) with small balls: their box spans the brick and keeps the lattice in it
    lat = np.stack(np.meshgrid(4.3125 + 0.375 * np.arange(8), 4.3125 + 0.375 * np.arange(8), 4.3125 + 0.8125 * np.arange(4),
                               indexing="ij"), -1).reshape(-1, 3)
    q = _f(np.array([[4.25, 4.25, 4.25], [7.75, 7.75, 7.75]]) * cell)
    r2 = _f((0.2 * cell) ** 2)
    far = [[8.5, 8.5, 8.5]]                                          # (in the next brick: the grid reaches past the second query)
    p256 = _f(np.concatenate([np.zeros((1, 3)), lat, far]) * cell)
    # (the 257th: in the brick's last cell, so the last record of the region in key order, and a match of the second query)
    p257 = _f(np.concatenate([np.zeros((1, 3)), lat, far, [[7.6875, 7.6875, 7.6875]]]) * cell)
    yield Case("stage_kept_256", p256, cell, q, r2, 8, None, 0, {"net8"}, np.array([1, 0]), "stage")
    yield Case("stage_kept_257", p257, cell, q, r2, 8, None, 0, {"redo_stage", "staged"}, np.array([1, 1]), "stage")
    # one brick of 1536 / 1537 records, a ball inside it with more than 32 matches: staged / streamed in k_query_tiles
    lat = np.stack(np.meshgrid(4.125 + 0.25 * np.arange(16), 4.125 + 0.25 * np.arange(16), 4.125 + 0.75 * np.arange(6),
                               indexing="ij"), -1).reshape(-1, 3)
    q = _f(np.array([[6.0, 6.0, 6.0], [5.0, 5.0, 5.0]]) * cell)
    r2 = _f(np.array([1.2 * cell, 0.3 * cell]) ** 2)
    p1536 = _f(np.concatenate([np.zeros((1, 3)), lat]) * cell)
    p1537 = _f(np.concatenate([np.zeros((1, 3)), lat, [[7.9375, 7.9375, 7.9375]]]) * cell)
    for k in (64, 7):
        yield Case("tiles_total_1536_k%d" % k, p1536, cell, q, r2, k, None, 0, {"redo_stage", "staged"}, None, "stage")
        yield Case("tiles_total_1537_k%d" % k, p1537, cell, q, r2, k, None, 0, {"redo_stage", "streamed"}, None, "stage")


# ---- brick regions --------------------------------------------------------------------------------------------------------
def brick_cloud():
    """140 cells (35 bricks) per axis, sparse: five points at each of the eight corners, 2000 points at random cell centres,
    and six points five cells from each of the two small-region queries."""
    cell = 0.25
    rng = np.random.default_rng(4)
    corner = np.array([[x, y, z] for x in (0.0, 139.5) for y in (0.0, 139.5) for z in (0.0, 139.5)])
    inward = np.where(corner == 0, 1.0, -1.0)
    pts = [corner] + [corner + inward * o for o in (0.0625, 0.125, 0.1875, 0.25)]
    pts.append(rng.integers(1, 139, (2000, 3)) + 0.5)
    for c in ((60.5, 60.5, 60.5), (54.125, 60.5, 60.5)):
        pts += [np.array(c) + s * 5.0 * np.eye(3)[a][None] for a in range(3) for s in (-1, 1)]
    pts.append(np.array([[47.9375, 60.5, 60.5]]))                   # in the fifth brick of the 5 x 4 x 4 region
    pts.append(np.array([p for p, _, _ in BRICK_QUERIES]))          # a point at every query: the self-query case asks from there
    pts = np.concatenate(pts)
    order = np.r_[0, 1 + rng.permutation(len(pts) - 1)]             # (the origin corner first: the anchor)
    return _f(pts[order] * cell), cell


BRICK_QUERIES = (   # position (cells), radius (cells), bricks of the region
    ((60.5, 60.5, 60.5), 6.2, 4 * 4 * 4),
    ((54.125, 60.5, 60.5), 6.25, 5 * 4 * 4),
    ((68.5, 68.5, 68.5), 61.75, 32 ** 3),
    ((70.125, 68.5, 66.5), 63.25, 33 * 32 * 33),
    ((66.5, 66.5, 66.5), 65.75, 34 ** 3),
    ((100.5, 100.5, 100.5), 1.25, None),
)


def _brick_cases():
    pts, cell = brick_cloud()
    qc = np.array([p for p, _, _ in BRICK_QUERIES])
    q = _f(qc * cell)
    r2 = _f((np.array([r for _, r, _ in BRICK_QUERIES]) * cell) ** 2)
    exp = {"redo_bricks", "staged", "streamed", "one_round", "several_rounds", "everything", "row_continued"}
    des = {"nbricks": [b for _, _, b in BRICK_QUERIES]}
    for k in (1, 64):
        yield Case("bricks_k%d" % k, pts, cell, q, r2, k, None, 0, exp, des, "bricks")
    # the same regions from inside the cloud: self-queries, most points with a small ball, the points at the query places with
    # the balls above, a state filter on
    n = len(pts)
    r2s = np.full(n, (1.28125 * cell) ** 2, F)
    for i in range(len(BRICK_QUERIES)):
        hit = np.flatnonzero(np.all(pts == q[i], axis=1))
        r2s[hit] = r2[i]
    state = np.random.default_rng(44).integers(0, 4, n).astype(np.uint8)
    yield Case("bricks_self_filter_k5", pts, cell, None, r2s, 5, state, 1, exp - {"row_continued"}, None, "bricks")
    # the widest regions over the 40 corner points alone: `everything` with a total that fits the stage, lists that fit K
    corners = np.concatenate([np.zeros((1, 3), F), pts[np.any((pts > 0) & (pts < 1.0 * cell) | (pts > 138.5 * cell), axis=1) &
                                                       np.all((pts < 1.0 * cell) | (pts > 138.5 * cell), axis=1)]])
    yield Case("bricks_corners_k64", corners, cell, q[2:5], r2[2:5], 64, None, 0, {"redo_bricks", "everything", "staged", "several_rounds"},
               None, "bricks")


# ---- degenerate balls -------------------------------------------------------------------------------------------------------
def _degenerate_cases():
    cell = 0.5
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3) + 0.5
    pts = _f(np.concatenate([np.zeros((1, 3)), g]) * cell)             # anchor = the min corner; (7.5, 7.5, 7.5) = the max corner
    nan, inf = float("nan"), float("inf")
    ball, out = (1.3 * cell) ** 2, (0.6 * cell) ** 2
    rows = [  # position (cells), r^2, count
        ((1.5, 1.5, 1.5), 0.0, 1), ((1.5, 2.5, 1.5), -1.0, 0), ((2.5, 1.5, 1.5), nan, 0),
        ((5.5, 5.5, 5.5), inf, 513), ((1.5, 5.5, 5.5), 1e30, 513),
        # outside past each face, the ball reaching the first layer of points
        ((-0.7, 3.5, 3.5), ball, 1), ((8.7, 3.5, 3.5), ball, 1), ((3.5, -0.7, 3.5), ball, 1),
        ((3.5, 8.7, 3.5), ball, 1), ((3.5, 3.5, -0.7), ball, 1), ((3.5, 3.5, 8.7), ball, 1),
        # the ball stays outside
        ((-3.0, 3.5, 3.5), ball, 0), ((11.0, 3.5, 3.5), ball, 0), ((3.5, 3.5, 11.0), ball, 0),
        # the grid's min and max corners
        ((0.0, 0.0, 0.0), out, 1), ((7.5, 7.5, 7.5), out, 1),
        ((nan, 3.5, 3.5), ball, 0), ((3.5, 3.5, nan), inf, 0),
    ]
    q = _f(np.array([p for p, _, _ in rows]) * cell)
    r2 = _f([r for _, r, _ in rows])
    yield Case("degenerate", pts, cell, q, r2, 64, None, 0, {"no_ball", "redo_stage", "net8"}, np.array([c for _, _, c in rows]), "degenerate")
    # the same from inside: self-queries with a state filter, every 37th point without a ball (r^2 < 0 or NaN), three with r^2 = inf
    n = len(pts)
    r2s = np.full(n, out, F)
    r2s[5::37] = -1.0
    r2s[11::37] = nan
    r2s[[100, 300, 500]] = inf
    state = (np.random.default_rng(8).integers(0, 4, n)).astype(np.uint8)
    live = int(np.sum((state & 1) == 0))
    des = np.where((state & 1) == 0, 1, 0)
    des[5::37] = des[11::37] = 0
    des[[100, 300, 500]] = live
    yield Case("degenerate_self_filter_k3", pts, cell, None, r2s, 3, state, 1, {"no_ball", "redo_stage", "net8"}, des, "degenerate")


# ---- query tiles ------------------------------------------------------------------------------------------------------------
def designed_tiles(runs):
    """Tile lengths for sorted runs of equal brick (lengths): cut at every multiple of 256 and every 64 after a cut."""
    out, pos = [], 0
    for length in runs:
        end = pos + length
        while pos < end:
            nxt = min(end, pos + 64, (pos // 256 + 1) * 256)
            out.append(nxt - pos)
            pos = nxt
    return out


def _tile_cases():
    cell = 0.5
    g = np.stack(np.meshgrid(np.arange(8), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3) + 0.5
    pts = _f(np.concatenate([np.zeros((1, 3)), g]) * cell)              # bricks (0, 0, 0) and (1, 0, 0): Morton 0 and 1
    sub = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3) * 0.5 + 0.25   # 512 places in a brick

    def places(n, brick_x, rng):
        return (sub[rng.permutation(512)[:n]] + [4.0 * brick_x, 0, 0]) * cell
    for n in TILE_N:
        for p in TILE_P:
            rng = np.random.default_rng(1000 * n + p)
            q = np.concatenate([places(p, 0, rng), places(n, 1, rng)])
            q = q[rng.permutation(len(q))]                              # (the sort brings the bricks together)
            r2 = _f((np.where(rng.integers(0, 3, len(q)) == 0, 1.2, 0.6) * cell) ** 2)
            yield Case("qtiles_n%d_p%d" % (n, p), pts, cell, _f(q), r2, 9, None, 0, set(),
                       {"tiles": designed_tiles([p, n] if p else [n])}, "qtiles")
    for n in SELF_TILE_N:
        for p in TILE_P:
            rng = np.random.default_rng(2000 * n + p)
            cloud = np.concatenate([np.zeros((1, 3)), places(p - 1, 0, rng) if p else np.zeros((0, 3)), places(n, 1, rng)])
            cloud[1:] = cloud[1 + rng.permutation(len(cloud) - 1)]
            runs = [p, n] if p else [1, n]                               # (the anchor is a point of brick 0)
            yield Case("stiles_n%d_p%d" % (n, p), _f(cloud), cell, None, np.full(len(cloud), (0.3 * cell) ** 2, F), 4, None, 0, set(),
                       {"tiles": designed_tiles(runs)}, "stiles")


# ---- build ------------------------------------------------------------------------------------------------------------------
PASSES_AXIS_BITS = OrderedDict([(2, 1), (3, 4), (4, 6), (5, 9), (6, 12), (7, 14), (8, 17)])    # radix passes -> bits per axis of the brick number


def scatter_cloud(extent_cells, cell, n, seed, clump=40):
    """Anchor at the origin, a point at (extent + 0.5) cells in every axis, a clump beside each, n points at random cell centres."""
    rng = np.random.default_rng(seed)
    top = extent_cells + 0.5
    pts = [np.zeros((1, 3)), np.full((1, 3), top), rng.integers(0, 4, (clump, 3)) + 0.5, top - rng.integers(1, 5, (clump, 3)),
           rng.integers(0, extent_cells, (n, 3)) + 0.5]
    pts = np.concatenate(pts)
    pts[2:] = pts[2 + rng.permutation(len(pts) - 2)]
    return _f(pts * cell)


def _build_cases():
    cell = 2.0 ** -10
    for passes, ab in PASSES_AXIS_BITS.items():
        pts = scatter_cloud(2 ** (ab + 1), cell, 1500, 50 + passes)
        sel = np.random.default_rng(passes).permutation(len(pts))[:300]
        stats = {"passes": passes, "dim": [2 ** (ab + 1) + 1] * 3, "cell": cell}
        yield Case("build_passes_%d" % passes, pts, cell, pts[sel], _f((1.1 * cell) ** 2), 16, None, 0, set(), {"stats": stats}, "build")
    rng = np.random.default_rng(60)
    one = _f(np.concatenate([np.zeros((1, 3)), rng.integers(0, 32, (49, 3)) / 64.0]) * cell)
    yield Case("build_single_cell", one, cell, None, np.full(50, (0.25 * cell) ** 2, F), 64, None, 0, set(),
               {"stats": {"passes": 2, "dim": [1, 1, 1], "cell": cell}}, "build")
    for times, extent in ((1, 384.0), (2, 768.0)):
        c0 = 2.0 ** -12
        cf = c0 * 2 ** times
        pts = scatter_cloud(int(extent / cf), cf, 600, 70 + times)
        sel = np.random.default_rng(times).permutation(len(pts))[:200]
        stats = {"passes": 8, "dim": [786433] * 3, "cell": cf, "doublings": times}
        yield Case("build_cell_doubled_%dx" % times, pts, c0, pts[sel], _f((1.1 * cf) ** 2), 16, None, 0, set(), {"stats": stats}, "build")
    for n in (2047, 2048, 2049, 16384, 16385):
        rng = np.random.default_rng(n)
        pts = _f(np.concatenate([np.zeros((1, 3)), rng.integers(0, 64, (n - 1, 3)) + 0.5]) * cell)
        stats = {"passes": 3, "cell": cell, "n": n}
        if n < 4096:
            yield Case("build_n%d" % n, pts, cell, None, np.full(n, (1.1 * cell) ** 2, F), 8, None, 0, set(), {"stats": stats}, "build")
        else:
            sel = rng.permutation(n)[:600]
            yield Case("build_n%d" % n, pts, cell, pts[sel], _f((1.1 * cell) ** 2), 8, None, 0, set(), {"stats": stats}, "build")


REBUILD_SEQUENCE = ("build_n16385", "build_single_cell", "build_n16385")      # one handle: large, small, large (the table is reused sparser)

_CACHE = []


def cases():
    """All cases, in order, built once (the arrays are shared: do not write to them)."""
    if not _CACHE:
        for gen in (_cluster_cases, _sweep_cases, _filter_cases, _mixed_cases, _lattice_cases, _stage_cases, _brick_cases,
                    _degenerate_cases, _tile_cases, _build_cases):
            _CACHE.extend(gen())
        for c in _CACHE:
            for a in (c.points, c.queries, c.r2, c.state):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return list(_CACHE)


def by_name():
    return OrderedDict((c.name, c) for c in cases())


_REF = {}


def reference(case):
    """oracle.nn_bruteforce of every query of a case: (counts [nq], dist2 [nq, K], indices [nq, K]), computed once."""
    if case.name not in _REF:
        import oracle as orc
        orc.build()
        p = case.points
        q = p if case.queries is None else case.queries
        r2 = np.broadcast_to(np.asarray(case.r2, F), (len(q),))
        cnt, d2, idx = np.zeros(len(q), np.int32), np.zeros((len(q), case.K), F), np.zeros((len(q), case.K), np.uint32)
        x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
        for j in range(len(q)):
            cnt[j], d2[j], idx[j] = orc.nn_bruteforce(x, y, z, q[j], float(r2[j]), case.K, state=case.state, skip_mask=case.skip_mask)
        _REF[case.name] = (cnt, d2, idx)
    return _REF[case.name]
