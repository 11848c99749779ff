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


def changed_mask(old, new):
    """changed(i): i >= n_prev, or any of the seven words differs bitwise (NaN equals itself, -0 differs from +0)."""
    n_prev, n = old[0].shape[0], new[0].shape[0]
    assert n >= n_prev
    out = np.ones(n, bool)
    out[:n_prev] = np.any(words(old) != words(new)[:n_prev], axis=1)
    return out


def _within(q_pos32, q_bound32, pts32):
    """For every q: is some point within its ball, decided as smx_nn decides it (float32 differences, squares, a left-to-
    right sum, against the float32 product)?"""
    hit = np.zeros(q_pos32.shape[0], bool)
    if pts32.shape[0] == 0:
        return hit
    for lo in range(0, q_pos32.shape[0], 512):
        d = q_pos32[lo:lo + 512, None, :] - pts32[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        hit[lo:lo + 512] = np.any(d2 <= q_bound32[lo:lo + 512, None], axis=1)
    return hit


def dirty_mask(old, new, prm, changed=None):
    """D: every changed slot, and every unchanged live slot with a changed slot's current position (if that slot is live
    now) or snapshot position (if it was live then) within f2 r2_q."""
    changed = changed_mask(old, new) if changed is None else changed
    n_prev = old[0].shape[0]
    pos, _, r2 = new
    live_now = mr.live_mask(pos, r2)
    live_then = mr.live_mask(old[0], old[2])
    pts = [pos[changed & live_now], old[0][changed[:n_prev] & live_then]]
    pts32 = np.concatenate(pts).astype(np.float32)
    f2 = np.float32(prm.search_radius_factor) * np.float32(prm.search_radius_factor)
    q = np.nonzero(~changed & live_now)[0]
    with np.errstate(invalid="ignore"):
        hit = _within(pos[q].astype(np.float32), f2 * r2[q].astype(np.float32), pts32)
    out = changed.copy()
    out[q[hit]] = True
    return out


def ring_members(star):
    out = set()
    for e in star:
        out |= e
    return out


def reagree_mask(dirty, old_stars, new_stars, n):
    """A: D and every member of the old and of the new ring of every slot in D (stars as mesh_ref.stars gives them)."""
    out = dirty.copy()
    for p in np.nonzero(dirty)[0]:
        for m in ring_members(old_stars.get(int(p), ())) | ring_members(new_stars.get(int(p), ())):
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
    stars = {p: (new_stars[p] if dirty[p] else old_stars[p]) for p in new_stars}   # (live now; if not in D, live before)
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
