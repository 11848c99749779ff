"""The model of smx_recon_triangulate_update's rule (include/smx.h), on top of tests/mesh_ref.py: which slots changed, the
set D of slots whose star is recomputed, the set A of slots whose owned triangles and star-triangle count are recomputed,
and the patch of an old result on A.  A map is the triple (pos [n,3], nrm [n,3], r2 [n]) of mesh_ref, float64 arrays that
hold float32 values."""
import numpy as np

import mesh_ref as mr


def words(m):
    """The seven words of every slot as uint32 [n,7]: smooth x, y, z; RadiusSquared; normal x, y, z."""
    pos, nrm, r2 = m
    w = np.concatenate([pos, r2[:, None], nrm], axis=1).astype(np.float32)
    return np.ascontiguousarray(w).view(np.uint32)


def changed_mask(old, new, mut=()):
    """changed(i): i >= n_prev, or any of the seven words differs bitwise (NaN equals itself, -0 differs from +0).
    mut: one-decision mutants of the predicate (MUTANTS below), for the tests that show which case notices which."""
    n_prev, n = old[0].shape[0], new[0].shape[0]
    assert n >= n_prev
    wo, wn = words(old), words(new)[:n_prev]
    differs = wo != wn
    if "ignore_radius" in mut:
        differs[:, 3] = False
    if "ignore_normal" in mut:
        differs[:, 4:7] = False
    if "zero_equal" in mut:
        differs &= ((wo | wn) & np.uint32(0x7FFFFFFF)) != 0
    if "nan_equal" in mut:
        differs &= ~np.isnan(wn.view(np.float32))
    out = np.ones(n, bool)
    out[:n_prev] = np.any(differs, axis=1)
    return out


def _within(q_pos32, q_bound32, pts32, strict=False):
    """For every q: is some point within its ball, decided as smx_nn decides it (float32 differences, squares, a left-to-
    right sum, against the float32 product)?"""
    hit = np.zeros(q_pos32.shape[0], bool)
    if pts32.shape[0] == 0:
        return hit
    for lo in range(0, q_pos32.shape[0], 512):
        d = q_pos32[lo:lo + 512, None, :] - pts32[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        b = q_bound32[lo:lo + 512, None]
        hit[lo:lo + 512] = np.any(d2 < b if strict else d2 <= b, axis=1)
    return hit


def dirty_mask(old, new, prm, changed=None, mut=()):
    """D: every changed slot, and every unchanged live slot with a changed slot's current position (if that slot is live
    now) or snapshot position (if it was live then) within f2 r2_q."""
    changed = changed_mask(old, new) if changed is None else changed
    n_prev = old[0].shape[0]
    pos, _, r2 = new
    live_now = mr.live_mask(pos, r2)
    live_then = mr.live_mask(old[0], old[2])
    pts = [pos[changed & live_now] if "no_current" not in mut else pos[:0],
           old[0][changed[:n_prev] & live_then] if "no_ghosts" not in mut else pos[:0]]
    pts32 = np.concatenate(pts).astype(np.float32)
    f2 = np.float32(prm.search_radius_factor) * np.float32(prm.search_radius_factor)
    q = np.nonzero(~changed & live_now)[0]
    with np.errstate(invalid="ignore"):
        hit = _within(pos[q].astype(np.float32), f2 * r2[q].astype(np.float32), pts32, strict="lt_ball" in mut)
    out = changed.copy()
    out[q[hit]] = True
    return out


def ring_members(star):
    out = set()
    for e in star:
        out |= e
    return out


def reagree_mask(dirty, old_stars, new_stars, n, mut=()):
    """A: D and every member of the old and of the new ring of every slot in D (stars as mesh_ref.stars gives them)."""
    out = dirty.copy()
    for p in np.nonzero(dirty)[0]:
        old_ring = ring_members(old_stars.get(int(p), ())) if "no_old_rings" not in mut else set()
        new_ring = ring_members(new_stars.get(int(p), ())) if "no_new_rings" not in mut else set()
        for m in old_ring | new_ring:
            if m < n:
                out[m] = True
    return out


def agree(stars, m, prm, owners=None):
    """mesh_ref.triangulate's agreement and filters over given stars.  Returns (the triangles whose smallest corner is in
    `owners` (all if None), in the contract's order, and per slot the distinct star triangles counted at it: a star
    triangle is counted at the smallest of the corners whose star holds it)."""
    pos, nrm, _ = m
    all_star = set()
    for p, s in stars.items():
        for e in s:
            all_star.add(frozenset((p,) + tuple(e)))
    out, counted = [], {}
    for t in all_star:
        c = sorted(t)
        holds = [x for x in c if frozenset(y for y in c if y != x) in stars.get(x, ())]
        counted[holds[0]] = counted.get(holds[0], 0) + 1
        if len(holds) == 3 and (owners is None or owners[c[0]]):
            o = mr.filter_and_orient(t, pos, nrm, prm)
            if o is not None:
                out.append(o)
    out.sort()
    return np.array(out, np.uint32).reshape(-1, 3), counted


def patch(old_tri, old_stars, new_stars, dirty, reagree, new, prm):
    """The update as the rule describes it: stars of D from the new map, the others kept; triangles owned by A recomputed,
    the others copied from the old result."""
    stars = {p: (new_stars[p] if dirty[p] else old_stars.get(p, set())) for p in new_stars}   # (live now; if not in D, live before)
    fresh, _ = agree(stars, new, prm, owners=reagree)
    kept = old_tri[~reagree[old_tri[:, 0].astype(np.int64)]]
    both = np.concatenate([kept.reshape(-1, 3), fresh.reshape(-1, 3)])
    order = np.lexsort((both[:, 2], both[:, 1], both[:, 0]))
    return both[order].astype(np.uint32), kept.shape[0]


def perturb(m, among, rng, n_move=30, n_merge=10, n_radius=5, n_normal=5, n_append=20):
    """The issue's perturbation, confined to the slots `among`: moves n_move slots within their tangent plane by 0.3 of
    their radius, marks n_merge merged, scales n_radius radii by 1.3, tilts n_normal normals, and appends n_append slots
    next to slots of `among`.  Returns (the new map, the indices of the perturbed old slots)."""
    pos, nrm, r2 = (a.copy() for a in m)
    n = pos.shape[0]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    pick = rng.choice(np.asarray(among), n_move + n_merge + n_radius + n_normal, replace=False)
    mv, mg, rd, nm = np.split(pick, np.cumsum([n_move, n_merge, n_radius]))

    def tangent(idx):
        t = rng.standard_normal((idx.size, 3))
        t -= np.sum(t * nrm[idx], axis=1, keepdims=True) * nrm[idx]
        return t / np.linalg.norm(t, axis=1, keepdims=True)
    pos[mv] = f32(pos[mv] + 0.3 * np.sqrt(r2[mv])[:, None] * tangent(mv))
    r2[mg] = -1.0
    r2[rd] = f32(1.3 * r2[rd])
    tilted = nrm[nm] + 0.2 * rng.standard_normal((nm.size, 3))
    nrm[nm] = f32(tilted / np.linalg.norm(tilted, axis=1, keepdims=True))
    src = rng.choice(np.asarray(among), n_append, replace=False)
    new_pos = f32(m[0][src] + 0.4 * np.sqrt(m[2][src])[:, None] * tangent(src))
    out = (np.concatenate([pos, new_pos]), np.concatenate([nrm, m[1][src]]), np.concatenate([r2, m[2][src]]))
    assert np.all(changed_mask(m, out)[pick]) and out[0].shape[0] == n + n_append
    return out, pick


# ---- the coarse filter in front of the reverse test, the path choice, and one whole call ----
# One-decision mutants of this model: name -> what the mutant does.  A test names the step of tests/mesh_update_cases.py
# at which each changes n_changed, n_dirty, the mode or the patched bytes.
MUTANTS = {
    "no_ghosts": "snapshot positions of changed slots are not tested against the balls",
    "no_current": "current positions of changed slots are not tested against the balls",
    "no_old_rings": "the members of the old ring of a slot of D are not put into A",
    "no_new_rings": "the members of the new ring of a slot of D are not put into A",
    "lt_ball": "d2 < f2 r2 instead of <= in the ball test",
    "ignore_radius": "changed() does not compare the RadiusSquared word",
    "ignore_normal": "changed() does not compare the normal words",
    "zero_equal": "changed() takes -0 for +0",
    "nan_equal": "changed() takes a NaN now for equal to anything",
    "face7": "the filter probes the slot's cell and its 6 face neighbours",
    "cells19": "the filter probes 19 cells (no corners)",
    "trunc": "the filter's cell index truncates towards zero instead of floorf",
    "no_mark_ghosts": "ghosts do not set their cell's bit",
    "no_radius": "the filter is applied whatever the radius of the ball",
    "radius_without_f2": "the filter's radius condition compares r2, not f2 r2, with h^2 / 4",
    "ge_path": "the full path is chosen at n_dirty >= fraction n",
}
NEAR_BITS_LOG2 = 27
CELL_LIMIT = np.float32(1048576.0)


def coarse_cell(x, y, z, inv_h, trunc=False):
    """mesh_coarse_cell of smx_mesh.hpp on arrays: (ok [m] bool, cells [m,3] int32; rows where ok is False hold 0).  The
    product is float32 and the comparison is written so that a NaN fails it."""
    c = np.stack([np.asarray(v, np.float32) * np.float32(inv_h) for v in (x, y, z)], axis=-1)
    assert c.dtype == np.float32
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(c) < CELL_LIMIT, axis=-1)
    safe = np.where(ok[..., None], c, np.float32(0.0))
    cells = (np.trunc(safe) if trunc else np.floor(safe)).astype(np.int32)
    return ok, cells


def coarse_bit(ix, iy, iz):
    """mesh_coarse_bit of smx_mesh.hpp on arrays of int32: the bit's number in the table, uint32 arithmetic throughout."""
    with np.errstate(over="ignore"):
        u = [np.asarray(v).astype(np.int32).astype(np.uint32) for v in (ix, iy, iz)]
        h = u[0] * np.uint32(73856093) ^ u[1] * np.uint32(19349663) ^ u[2] * np.uint32(83492791)
        h = h ^ (h >> np.uint32(15))
        h = h * np.uint32(0x2C1B3C6D)
        h = h ^ (h >> np.uint32(12))
    return h & np.uint32((1 << NEAR_BITS_LOG2) - 1)


OFFSETS27 = np.array([(c % 3 - 1, (c // 3) % 3 - 1, c // 9 - 1) for c in range(27)], np.int32)


class Filter:
    """What the coarse filter does on one call: .no_filter (a changed point or ghost had no cell: nobody is filtered),
    .subject (unchanged slots that are probed), .by_radius (unchanged live slots let through because f2 r2 > h^2 / 4),
    .by_cell (unchanged slots with a radius small enough whose own coordinates have no cell), .out (the slots left out
    of the reverse test), .mark_cells ([k,3] cells of the marks), .mark_of (cell tuple -> count)."""


def coarse_filter(old, new, prm, cell, changed=None, mut=()):
    changed = changed_mask(old, new) if changed is None else changed
    n_prev, n = old[0].shape[0], new[0].shape[0]
    pos, _, r2 = new
    live_now, live_then = mr.live_mask(pos, r2), mr.live_mask(old[0], old[2])
    h = np.float32(cell)
    inv_h = np.float32(1.0) / h
    max_r2 = np.float32(0.25) * h * h
    f2 = np.float32(prm.search_radius_factor) * np.float32(prm.search_radius_factor)
    trunc = "trunc" in mut
    marks = [pos[changed & live_now]]
    if "no_mark_ghosts" not in mut:
        marks.append(old[0][changed[:n_prev] & live_then])
    marks = np.concatenate(marks).astype(np.float32)
    ok, mcells = coarse_cell(marks[:, 0], marks[:, 1], marks[:, 2], inv_h, trunc)
    f = Filter()
    f.no_filter = bool(np.any(~ok))
    f.mark_cells = mcells[ok]
    table = set(int(b) for b in coarse_bit(f.mark_cells[:, 0], f.mark_cells[:, 1], f.mark_cells[:, 2]))
    unchanged = ~changed
    # (reverse_r2 is RadiusSquared where the slot is unchanged and live and 0 elsewhere; the rows of merged slots are NaN)
    rr = np.where(unchanged & live_now, r2, 0.0).astype(np.float32)
    with np.errstate(invalid="ignore"):
        small = f2 * rr <= max_r2
        if "radius_without_f2" in mut:
            small = rr <= max_r2
    if "no_radius" in mut:
        small = np.ones(n, bool)
    p32 = np.where((r2 < 0)[:, None], np.nan, pos).astype(np.float32)
    has_cell, cells = coarse_cell(p32[:, 0], p32[:, 1], p32[:, 2], inv_h, trunc)
    f.by_radius = unchanged & live_now & ~small
    f.by_cell = unchanged & live_now & small & ~has_cell
    f.subject = unchanged & small & has_cell & (not f.no_filter)
    f.out = np.zeros(n, bool)
    f.via = {}
    offsets = OFFSETS27
    if "face7" in mut:
        offsets = offsets[np.abs(offsets).sum(axis=1) <= 1]
    if "cells19" in mut:
        offsets = offsets[np.abs(offsets).sum(axis=1) <= 2]
    for i in np.nonzero(f.subject)[0]:
        nb = cells[i][None, :] + offsets
        bits = coarse_bit(nb[:, 0], nb[:, 1], nb[:, 2])
        hit = [k for k, b in enumerate(bits) if int(b) in table]
        f.out[i] = not hit
        f.via[int(i)] = [tuple(int(v) for v in offsets[k]) for k in hit]
    return f


def filtered_out(old, new, prm, cell, mut=()):
    """The unchanged slots k_mesh_reverse_rows leaves out of the reverse test (a bool mask over the new map's slots)."""
    return coarse_filter(old, new, prm, cell, mut=mut).out


def chooses_full(n_dirty, fraction, n, mut=()):
    """The path choice of mesh_triangulate_update: doubles of the slot counts and of the float32 fraction, strictly above."""
    lhs, rhs = float(n_dirty), float(np.float32(fraction)) * float(n)
    return lhs >= rhs if "ge_path" in mut else lhs > rhs


DEFAULT_FRACTION = 0.2


class Truth:
    """mesh_ref's view of one map: .map, .prm, .stars (mesh_ref.stars), .tri and .stats (mesh_ref.triangulate)."""

    def __init__(self, m, prm):
        self.map, self.prm = m, prm
        found = mr.stars(*m, prm)
        self.stars = found[0]
        stars_fn = mr.stars
        mr.stars = lambda *a, **k: found       # (triangulate's own call of stars on the same arguments: not computed twice)
        try:
            self.tri, self.stats, _ = mr.triangulate(*m, prm)
        finally:
            mr.stars = stars_fn
        self.n = m[0].shape[0]


def same_params(a, b):
    keys = ("max_angle_between_normals_deg", "min_triangle_angle_deg", "max_triangle_angle_deg", "search_radius_factor", "max_neighbors")
    return all(getattr(a, k) == getattr(b, k) for k in keys)


class Call:
    """What one smx_recon_triangulate_update call reports and returns, by the model: .mode, .n_changed, .n_ghosts,
    .n_dirty, .n_reagreed, .n_kept_triangles, .tri; on the incremental path also the masks .changed, .dirty, .reagree
    and .filter (a Filter; None when no reverse test runs)."""

    def stats(self):
        return dict(mode=self.mode, n_changed=self.n_changed, n_dirty=self.n_dirty, n_reagreed=self.n_reagreed,
                    n_kept_triangles=self.n_kept_triangles)


def model_call(prev, cur, cell, fraction=None, mut=()):
    """The call on the map of `cur` (a Truth) with the kept state of `prev` (a Truth, or None: no state).  With a mutant
    the stars outside the mutant's D and the triangles outside its A are the previous call's, as on the device."""
    fraction = DEFAULT_FRACTION if fraction is None or fraction < 0 else fraction
    c = Call()
    n = cur.n
    c.mode = 1 if prev is None else 2 if not same_params(prev.prm, cur.prm) else 3 if n < prev.n else 0
    c.filter = None
    if c.mode != 0:
        c.n_changed = c.n_dirty = c.n_reagreed = n
        c.n_ghosts, c.n_kept_triangles, c.tri = 0, 0, cur.tri
        return c
    old, new, prm = prev.map, cur.map, cur.prm
    c.changed = changed_mask(old, new, mut)
    c.n_changed = int(c.changed.sum())
    c.n_ghosts = int((c.changed[:prev.n] & mr.live_mask(old[0], old[2])).sum())
    if c.n_changed == 0:
        c.n_dirty = c.n_reagreed = 0
        c.dirty = c.reagree = np.zeros(n, bool)
        c.n_kept_triangles, c.tri = prev.tri.shape[0], prev.tri
        return c
    c.filter = coarse_filter(old, new, prm, cell, c.changed, mut)
    c.dirty = dirty_mask(old, new, prm, c.changed, mut) & ~c.filter.out
    c.n_dirty = int(c.dirty.sum())
    if chooses_full(c.n_dirty, fraction, n, mut):
        c.mode, c.n_reagreed, c.n_kept_triangles, c.tri = 4, n, 0, cur.tri
        c.reagree = np.ones(n, bool)
        return c
    c.reagree = reagree_mask(c.dirty, prev.stars, cur.stars, n, mut)
    c.n_reagreed = int(c.reagree.sum())
    c.tri, c.n_kept_triangles = patch(prev.tri, prev.stars, cur.stars, c.dirty, c.reagree, new, prm)
    return c
