"""A numpy restatement of the DISPATCH of surfelmeshing_amd/csrc/smx_nn.hip (test infrastructure, no GPU needed): which
grid smx_nn_build lays out, which key a point and a query get, where k_tile_flags cuts the tiles, and which route every
query of a tile takes through k_query_lanes and k_query_tiles.  It does not restate the answer: that stays
oracle.nn_bruteforce.  Everything the kernels compute in float32 is computed in float32 here, in the same order of
operations (the build has -ffp-contract=off).

The margin rule.  A route means something only if rounding cannot flip it: the device's sqrtf and its division need not
agree with numpy's in the last bit.  So every float decision is reported with its distance from the threshold, in cells,
and assert_margins fails when
  * a range edge ((q -+ rad - min) / cell) lies within MARGIN = 1e-3 cell of a cell boundary that decides something (the
    lower edge is clamped to cell 0 below the grid and the upper edge to the last cell above it: no decision there);
  * a point's or a query's own cell coordinate is not computed exactly and lies within MARGIN of a boundary;
  * a record lies within MARGIN cell of a face of the tile's float box, with ONE class left in: a record INSIDE the box
    by at least SLACK_SHARE of what cover_radius adds whatever the radius (1e-6 + 2.4e-7 |q|, several rounding errors of
    q -+ rad).  That is where a match at exactly one radius from the tile's outermost query lies -- the face is
    rad = 1.0001 r + 1e-6 + ... from the query and the match r -- so a lattice query, or a query with r^2 = 0 at a point,
    cannot be farther from the face than 1e-4 r + 1e-6; that such a record is kept is what those cases test, through the
    answer.  The rounding of q -+ rad is at most an ulp of |q| + rad (1.2e-7 of it) and a last-bit difference in sqrtf moves
    rad by 6e-8 r, against a slack of 1e-4 r + 1e-6 + 2.4e-7 |q|: `kept` counts such records as kept; `near_in` says how many.
Counts (matches against 8 / 16 / 32, kept against 256, region totals against 1536, bricks against 64 and 2^15) are
integers once the float decisions are safe; the model reports them so that the cases can be read against the thresholds."""
import numpy as np

F = np.float32
K_TILE = 64                  # kTile
CHUNK = 256                  # threads of a k_tile_flags workgroup
LANE_CAP = 32                # kLaneCap
STAGE_L = 256                # kStageL
STAGE = 1536                 # kStage
MANY_BRICKS = 1 << 15        # kManyBricks
MARGIN = 1e-3                # cells
SLACK_SHARE = 0.5

LANE_ROUTES = ("net8", "net16", "rank", "redo_count", "redo_bricks", "redo_stage", "no_ball")


def bit_length(v):
    return int(v).bit_length()


def spread3(v):
    """Bit k of the 21-bit v -> bit 3 k (numpy uint64 arrays; the masks of smx_nn.hip)."""
    v = np.asarray(v, np.uint64) & np.uint64(0x1FFFFF)
    for s, m in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                 (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(s))) & np.uint64(m)
    return v


def brick_index(b):
    """Morton number of brick coordinates b [n, 3]."""
    b = np.asarray(b, np.int64)
    return spread3(b[:, 0]) | (spread3(b[:, 1]) << np.uint64(1)) | (spread3(b[:, 2]) << np.uint64(2))


def indexable(p):
    with np.errstate(invalid="ignore"):
        return np.all(np.abs(p) <= F(3.0e38), axis=1)


class Grid:
    pass


def grid_of(points, cell):
    """The Grid of smx_nn_build over the indexable points, or None when there is none."""
    p = np.asarray(points, F).reshape(-1, 3)
    ok = indexable(p)
    if not ok.any():
        return None
    g = Grid()
    g.min, mx = p[ok].min(0), p[ok].max(0)
    g.n_indexed = int(ok.sum())
    cell, g.doublings = F(cell), 0
    while True:
        d = np.floor((mx.astype(np.float64) - g.min.astype(np.float64)) / np.float64(cell)) + 1.0
        fits = bool(np.all(d <= 2097152.0))
        if fits:
            g.dim = np.maximum(d.astype(np.int64), 1)
            g.bdim = (g.dim + 3) >> 2
            g.axis_bits = max(1, max(bit_length(b - 1) for b in g.bdim))
            if 3 * g.axis_bits <= 56:
                break
        cell = F(cell * F(2.0))
        g.doublings += 1
    g.cell = cell
    g.brick_bits = 3 * g.axis_bits
    g.key_bits = g.brick_bits + 6 + 1          # bit_length of the sentinel (1 << brick_bits) << 6
    g.passes = (g.key_bits + 7) // 8
    g.query_passes = (g.brick_bits + 7) // 8
    return g


def cell_value(g, p):
    """(p - min) / cell as the kernels compute it (float32)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(p, F) - g.min) / g.cell


def cell_coord(g, p):
    with np.errstate(invalid="ignore"):
        v = np.floor(cell_value(g, p))
        c = np.where(np.isnan(v), F(0), np.clip(v, F(0), (g.dim - 1).astype(F)))
    return c.astype(np.int64)


def coord_margin(g, p):
    """Distance of a cell coordinate from the nearest boundary, in cells; inf where float32 computed it exactly."""
    p = np.asarray(p, F)
    v = cell_value(g, p).astype(np.float64)
    exact = (p.astype(np.float64) - g.min.astype(np.float64)) / np.float64(g.cell)
    with np.errstate(invalid="ignore"):
        m = np.abs(v - np.rint(v))
        m = np.where((v == exact) | ~np.isfinite(v) | (v < -MARGIN) | (v > g.dim + MARGIN), np.inf, m)
    return m


def point_keys(g, points):
    """(key [n] uint64, sentinel) of k_point_keys."""
    p = np.asarray(points, F).reshape(-1, 3)
    c = cell_coord(g, p)
    local = ((c[:, 2] & 3) << 4) | ((c[:, 1] & 3) << 2) | (c[:, 0] & 3)
    key = (brick_index(c >> 2) << np.uint64(6)) | local.astype(np.uint64)
    sentinel = np.uint64(1 << (g.brick_bits + 6))
    return np.where(indexable(p), key, sentinel), sentinel


def query_keys(g, q):
    return brick_index(cell_coord(g, np.asarray(q, F).reshape(-1, 3)) >> 2)


def tile_cut(brick_keys):
    """k_tile_flags + k_tile_starts over sorted brick keys: start positions of the tiles, then n.  A tile starts where the
    brick changes, at every 256-thread chunk start, and every 64 positions after either."""
    n = len(brick_keys)
    starts, last = [], 0
    for j in range(n):
        t = j % CHUNK
        if t == 0 or brick_keys[j - 1] != brick_keys[j]:
            last = t
        if (t - last) % K_TILE == 0:
            starts.append(j)
    return starts + [n]


class Index:
    """Sorted records and the brick table of a build."""

    def __init__(self, points, cell):
        self.points = np.asarray(points, F).reshape(-1, 3)
        self.grid = g = grid_of(self.points, cell)
        self.n = len(self.points)
        if g is None:
            self.n_indexed = self.n_bricks = 0
            return
        self.keys, self.sentinel = point_keys(g, self.points)
        self.order = np.argsort(self.keys, kind="stable")
        self.n_indexed = g.n_indexed
        self.order = self.order[:self.n_indexed]
        self.sorted_keys = self.keys[self.order]
        bk = self.sorted_keys >> np.uint64(6)
        cut = np.flatnonzero(np.r_[True, bk[1:] != bk[:-1]])
        self.table = {int(bk[s]): (int(s), int(e)) for s, e in zip(cut, np.r_[cut[1:], len(bk)])}
        self.n_bricks = len(self.table)
        self.self_tiles = tile_cut(bk)
        self.sorted_pos = self.points[self.order]

    def stats(self):
        g = self.grid
        return {"cell_size": float(g.cell), "dim": [int(v) for v in g.dim], "n_indexed": self.n_indexed,
                "n_bricks": self.n_bricks, "key_bits": g.key_bits}

    def region_records(self, kb, bn, first=0, count=None):
        """(total, sorted-record positions) of bricks [first, first + count) of the region, x fastest."""
        nb = int(bn[0]) * int(bn[1]) * int(bn[2])
        last = nb if count is None else min(nb, first + count)
        b = np.arange(first, last, dtype=np.int64)
        xyz = np.stack([kb[0] + b % bn[0], kb[1] + (b // bn[0]) % bn[1], kb[2] + b // (bn[0] * bn[1])], 1)
        rec = []
        for m in brick_index(xyz):
            se = self.table.get(int(m))
            if se:
                rec.append(np.arange(se[0], se[1]))
        rec = np.concatenate(rec) if rec else np.zeros(0, np.int64)
        return len(rec), rec


def cover_radius(r2, q):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(np.asarray(r2, F)) * F(1.0001) + F(1e-6) + np.abs(np.asarray(q, F)) * F(2.4e-7)


def ranges(g, q, r2):
    """Per query: ball [nq], lo / hi [nq, 3] cells, float box edges [nq, 3] each, and the margin of the range edges."""
    q, r2 = np.asarray(q, F).reshape(-1, 3), np.asarray(r2, F).reshape(-1)
    dim = g.dim.astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        want = r2 >= 0
        rad = cover_radius(r2[:, None], q)
        blo, bhi = q - rad, q + rad
        vlo, vhi = (blo - g.min) / g.cell, (bhi - g.min) / g.cell
        flo, fhi = np.floor(vlo), np.floor(vhi)
        lo = np.where(flo >= 0, np.where(flo < dim, flo, dim), F(0))
        hi = np.where(fhi >= 0, np.where(fhi < dim, fhi, dim - 1), F(-1))
        ball = want & np.all(lo <= hi, axis=1)
        # lower edge: boundaries 1 .. dim decide; upper edge: boundaries 0 .. dim - 1
        a, b = vlo.astype(np.float64), vhi.astype(np.float64)
        dd = g.dim.astype(np.float64)
        mlo = np.where(a < 1, 1 - a, np.where(a > dd, a - dd, np.abs(a - np.rint(a))))
        mhi = np.where(b < 0, -b, np.where(b > dd - 1, b - (dd - 1), np.abs(b - np.rint(b))))
        m = np.minimum(np.where(np.isnan(mlo), np.inf, mlo), np.where(np.isnan(mhi), np.inf, mhi))
        m = np.where(want[:, None], m, np.inf)
    return ball, lo.astype(np.int64), hi.astype(np.int64), blo, bhi, m.min(1)


def brute_counts(points, q, r2, state=None, skip_mask=0):
    """Matches per query, float32, the kernels' order of operations (also oracle.nn_bruteforce's: the CPU test compares)."""
    p = np.asarray(points, F).reshape(-1, 3)
    q, r2 = np.asarray(q, F).reshape(-1, 3), np.asarray(r2, F).reshape(-1)
    live = np.ones(len(p), bool) if state is None else (np.asarray(state, np.uint8) & np.uint8(skip_mask)) == 0
    out = np.zeros(len(q), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(q), 256):
            d = p[None, :, :] - q[s:s + 256, None, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            out[s:s + 256] = ((d2 <= r2[s:s + 256, None]) & live[None, :]).sum(1)
    return out


class Chunk:
    """One tile of <= 64 queries as k_query_lanes sees it, and what k_query_tiles does with it."""


def _tiles_regime(ix, lo, hi, lanes):
    """k_query_tiles over the ball lanes `lanes` (positions into lo / hi): region, rounds, staged / streamed."""
    t = {"lanes": len(lanes)}
    if not len(lanes):
        return None
    rlo, rhi = lo[lanes].min(0), hi[lanes].max(0)
    kb = rlo >> 2
    bn = (rhi >> 2) - kb + 1
    nb = int(bn[0]) * int(bn[1]) * int(bn[2])
    t["nbricks"], t["everything"] = nb, nb > MANY_BRICKS
    if t["everything"]:
        totals = [ix.n_indexed]
    else:
        totals = [ix.region_records(kb, bn, b0, 64)[0] for b0 in range(0, nb, 64)]
    t["rounds"] = len(totals)
    t["round_totals"] = totals
    t["rounds_with_records"] = sum(1 for v in totals if v)
    t["staged"] = any(0 < v <= STAGE for v in totals)
    t["streamed"] = any(v > STAGE for v in totals)
    return t


def chunk_model(ix, qid, qpos, ball, lo, hi, blo, bhi, counts):
    g = ix.grid
    c = Chunk()
    c.qid, c.counts = np.asarray(qid), np.asarray(counts)
    n = len(qid)
    c.routes = ["no_ball"] * n
    c.nbricks = c.total = c.kept = c.near_in = c.near_out = 0
    c.box_margin = np.inf
    c.n_max = 0
    lanes = np.flatnonzero(ball)
    c.tiles0 = _tiles_regime(ix, lo, hi, lanes)        # query mode 0: the tile kernel answers every lane of the tile
    c.tiles = None                                      # query mode 2: the tile kernel answers the marked lanes
    if not len(lanes):
        return c
    rlo, rhi = lo[lanes].min(0), hi[lanes].max(0)
    kb = rlo >> 2
    bn = (rhi >> 2) - kb + 1
    c.nbricks = int(bn[0]) * int(bn[1]) * int(bn[2])
    redo = np.zeros(n, bool)
    if c.nbricks > 64:
        redo[lanes] = True
        for k in lanes:
            c.routes[k] = "redo_bricks"
    else:
        c.total, rec = ix.region_records(kb, bn)
        flo, fhi = blo[lanes].min(0), bhi[lanes].max(0)
        p = ix.sorted_pos[rec].astype(np.float64)
        inside_by = np.minimum(p - flo.astype(np.float64), fhi.astype(np.float64) - p).min(1) if len(rec) else np.zeros(0)
        with np.errstate(invalid="ignore"):
            pf = ix.sorted_pos[rec]
            inside = np.all((pf >= flo) & (pf <= fhi), axis=1) if len(rec) else np.zeros(0, bool)
        assert np.array_equal(inside, inside_by >= 0)
        c.kept = int(inside.sum())
        tol = MARGIN * float(g.cell)
        slack = SLACK_SHARE * (1e-6 + 2.4e-7 * np.abs(p).max(1)) if len(rec) else np.zeros(0)
        near = np.abs(inside_by) < tol
        on_shell = near & inside & (inside_by >= slack)            # the class the margin rule leaves in
        c.near_in, c.near_out = int((near & inside).sum()), int((near & ~inside).sum())
        bad = near & ~on_shell
        c.box_margin = float(np.abs(inside_by[bad]).min() / float(g.cell)) if bad.any() else np.inf
        if c.kept > STAGE_L:
            redo[lanes] = True
            for k in lanes:
                c.routes[k] = "redo_stage"
        else:
            for k in lanes:
                if c.counts[k] > LANE_CAP:
                    redo[k] = True
                    c.routes[k] = "redo_count"
    nn = np.where(redo | ~ball, 0, c.counts)
    c.n_max = int(nn.max()) if n else 0
    sort_route = "net8" if c.n_max <= 8 else "net16" if c.n_max <= 16 else "rank"
    c.sort_route = sort_route
    for k in lanes:
        if not redo[k]:
            c.routes[k] = sort_route
    c.tiles = _tiles_regime(ix, lo, hi, np.flatnonzero(redo))
    return c


class CaseModel:
    """The dispatch of one (points, cell, queries, r2, state, skip_mask): batch when queries is given, self otherwise."""

    def __init__(self, points, cell, queries, r2, state=None, skip_mask=0, counts=None, index=None):
        self.index = ix = index if index is not None else Index(points, cell)
        self.chunks, self.self_query = [], queries is None
        self.range_margin = self.coord_margin = np.inf
        g = ix.grid
        if g is None:
            return
        pts = ix.points
        if self.self_query:
            qid_sorted = ix.order
            q = pts
            starts = ix.self_tiles
            r2 = np.broadcast_to(np.asarray(r2, F), (ix.n,))
        else:
            q = np.asarray(queries, F).reshape(-1, 3)
            r2 = np.broadcast_to(np.asarray(r2, F), (len(q),))
            qk = query_keys(g, q)
            qid_sorted = np.argsort(qk, kind="stable")
            starts = tile_cut(qk[qid_sorted])
            with np.errstate(invalid="ignore"):
                fin = np.all(np.isfinite(q), axis=1)
            self.coord_margin = float(coord_margin(g, q[fin]).min()) if fin.any() else np.inf
        self.coord_margin = min(self.coord_margin, float(coord_margin(g, pts[indexable(pts)]).min()))
        self.tile_starts = starts
        self.counts = brute_counts(pts, q, r2, state, skip_mask) if counts is None else np.asarray(counts)
        ball, lo, hi, blo, bhi, m = ranges(g, q, r2)
        self.ball = ball
        self.range_margin = float(m[qid_sorted].min()) if len(qid_sorted) else np.inf
        for s, e in zip(starts[:-1], starts[1:]):
            ids = qid_sorted[s:e]
            self.chunks.append(chunk_model(ix, ids, q[ids], ball[ids], lo[ids], hi[ids], blo[ids], bhi[ids], self.counts[ids]))
        self.route = {}
        for c in self.chunks:
            for k, i in enumerate(c.qid):
                self.route[int(i)] = c.routes[k]

    def routes(self):
        return set(self.route.values())

    def tiles_regimes(self, mode=2):
        """Names of the k_query_tiles regimes reached: staged, streamed, one_round, several_rounds, everything."""
        out = set()
        for c in self.chunks:
            t = c.tiles if mode == 2 else c.tiles0
            if not t:
                continue
            out |= {k for k in ("staged", "streamed", "everything") if t[k]}
            out.add("several_rounds" if t["rounds"] > 1 else "one_round")
            if t["rounds_with_records"] > 1:
                out.add("row_continued")
        return out

    def box_margin(self):
        return min([c.box_margin for c in self.chunks] + [np.inf])


def assert_margins(model, name=""):
    assert model.range_margin >= MARGIN, "%s: a range edge lies %.3g cell from a cell boundary" % (name, model.range_margin)
    assert model.coord_margin >= MARGIN, "%s: a cell coordinate lies %.3g cell from a boundary" % (name, model.coord_margin)
    assert model.box_margin() >= MARGIN, "%s: a record lies %.3g cell from a face of its tile's box" % (name, model.box_margin())
