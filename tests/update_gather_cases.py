"""One Integrate call whose neighbour update meets every kind of candidate (test infrastructure, no GPU needed).

The update (oracle/smx_oracle_recon.c, UpdateNeighbors; update_neighbors_body / relink in smx_recon.hip) offers every
visible surfel the supporting surfels of the four pixels around its own as new links.  The HIP kernel gathers records
only for candidates that are a surfel, not the slot itself and not yet one of its links; this scenario makes sure that
one call holds slots for each of

  all_linked      all four adjacent supporting surfels are links already: nothing is gathered, nothing stored
  new_nearer      a new candidate takes the place of a farther link
  self            a candidate is the slot itself
  fills_empty     invalid candidates beside new ones, and empty link slots (infinite distance) that get filled
  too_far         a new candidate fails the distance test
  opposed         a new candidate passes the distance test and fails the normal test

A seventh kind -- the same new candidate at two of the four pixels, the second meeting the first's insertion -- cannot
be built: a surfel supports at most its own pixel and one 4-adjacent pixel (its quadrant neighbour), and no two of the four
pixels around a pixel are 4-adjacent, so the supporting image never offers one slot the same surfel twice.  census()
counts it all the same ("twice"), and the tests assert that it stays at zero.

It is the crafted map of decision_maps.py and its call of frame 9 (which has the opposed normals and the displaced
surfels), with the LINKS of seeded groups of slots rewritten.  Links decide nothing in a call before the neighbour update
-- association, merging and integration never read them -- so a dry run of the same call on the unedited map tells
which candidates every slot will meet, and the links are then written to order.
"""
from types import SimpleNamespace

import numpy as np

import decision_maps as dm
import oracle as orc

INVALID = dm.INVALID
SEED = 771
REL = 1e-3          # census: distance and normal tests count only if this clear of their thresholds
CASES = ("all_linked", "new_nearer", "self", "fills_empty", "too_far", "opposed")


def _run(sc, rows, call):
    """The oracle's snapshot after `call` on the map `rows` (as decision_maps.run_oracle keeps it)."""
    fx, fy, cx, cy = sc.camera
    rec = orc.Recon(sc.capacity, dm.W, dm.H, fx, fy, cx, cy)
    rec.surfels()[:, :rows.shape[1]] = rows
    rec.set_counts(rows.shape[1], sc.merge_count)
    depth = call.depth.copy()
    rec.integrate(call.frame, call.depth_scaling, depth, call.normals, call.radius, call.color, call.pose, call.params)
    n = rec.surfels_size
    snap = SimpleNamespace(rows=rec.surfels()[:, :n].copy(), count=n, merge_count=rec.merge_count, surfel_count=rec.surfel_count,
                           scratch={k: v.copy() for k, v in rec.scratch().items()}, depth=depth, stats=rec.stats())
    rec.close()
    return snap


def lane_tests(rows, frame, pose, camera, params, depth, inv_scaling, radius, supporting, W, H):
    """float32 restatement of the lane tests in front of the gathers (update_neighbors_body, smx_recon.hip), for the
    slots `rows` [25, n] as the integration left them: (reaches the gathers [n], candidates [4, n] u32).  The one
    restatement: tests/tools/update_gather_census.py counts with it too."""
    f32 = np.float32
    fx, fy, cx, cy = (f32(v) for v in camera)
    p = params
    A = rows
    G = np.asarray(pose, np.float32).reshape(3, 4)
    R, t = G[:, :3], G[:, 3]
    loc = R.T @ (A[0:3] - t[:, None])
    z = loc[2]
    ok = dm._is_active(A[18].view(np.uint32), frame, p.surfel_integration_active_window_size) & (z > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * (loc[0] / z) + cx, fy * (loc[1] / z) + cy
        ok &= (u >= 1) & (v >= 1) & (u < W - 1) & (v < H - 1)
        x, y = np.where(ok, u, 1).astype(np.int64), np.where(ok, v, 1).astype(np.int64)
        k = y * W + x
        md = f32(inv_scaling) * depth.ravel().astype(np.float32)[k]
        ok &= ~(z > (f32(1) + f32(p.sensor_noise_factor)) * md)
        ln = R.T @ A[8:11]
        ok &= ~((loc * ln).sum(0) / np.sqrt((loc * loc).sum(0)) > 0)
        ok &= ~(A[7] < 0) & ~(radius.ravel()[k] / A[7] > f32(2.25))
    sup = supporting.ravel()
    cand = np.stack([sup[(y + dy) * W + (x + dx)] for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1))])
    return ok, cand


def _lanes(n, call, after, camera):
    """lane_tests for the first n slots of a snapshot `after` of `call`."""
    return lane_tests(after.rows[:, :n], call.frame, call.pose, camera, call.params, after.depth, 1.0 / call.depth_scaling,
                      call.radius, after.scratch["supporting"], dm.W, dm.H)


def build():
    """The scenario: .rows (edited map), .count, .merge_count, .call, .camera, .pre, .capacity, .snap (the oracle after
    the call), .groups (name -> slots whose links were rewritten)."""
    sc = dm.build()
    call = sc.calls[1]
    assert call.kind == "integrate" and call.frame == 9
    n = sc.count
    dry = _run(sc, sc.rows, call)
    ok, cand = _lanes(n, call, dry, sc.camera)
    idx = np.arange(n, dtype=np.uint32)
    valid = (cand != INVALID) & (cand != idx)
    srt = np.sort(cand, axis=0)
    distinct = (srt[1:] != srt[:-1]).all(0)
    rng = np.random.default_rng(SEED)

    def some(mask, share):
        pool = rng.permutation(np.flatnonzero(mask))
        return np.sort(pool[:int(len(pool) * share)])

    rows = sc.rows.copy()
    links = rows.view(np.uint32)[19:23]
    groups = {}
    free = ok.copy()
    # all four candidates are links already
    groups["all_linked"] = g = some(free & valid.all(0) & distinct, 0.25)
    links[:, g] = cand[:, g]
    free[g] = False
    # links far away: four live slots from other parts of the map
    groups["far_links"] = g = some(free & valid.any(0), 0.1)
    live = np.flatnonzero(rows[7] > 0)
    for j in range(4):
        links[j, g] = live[(np.searchsorted(live, g) + (j + 1) * len(live) // 5) % len(live)]
    free[g] = False
    # invalid candidates beside new ones, every link slot empty
    groups["empty"] = g = some(free & (cand == INVALID).any(0) & valid.any(0), 0.5)
    links[:, g] = INVALID
    free[g] = False
    # two links kept, two emptied
    groups["half_empty"] = g = some(free & valid.any(0), 0.15)
    links[2:, g] = INVALID
    rows.setflags(write=False)
    snap = _run(sc, rows, call)
    # (what the links were written to order for: the candidates are the dry run's)
    assert np.array_equal(snap.scratch["supporting"], dry.scratch["supporting"])
    assert np.array_equal(snap.rows[0:3, :n], dry.rows[0:3, :n]) and np.array_equal(snap.rows[7:11, :n], dry.rows[7:11, :n])
    return SimpleNamespace(rows=rows, count=n, merge_count=sc.merge_count, call=call, camera=sc.camera, pre=sc.pre,
                           capacity=sc.capacity, snap=snap, groups=groups)


def census(us):
    """How many slots of the call fall into each case (CASES), from the map before, the oracle's map after and the
    candidates the lanes meet.  A link that the integration reset (a replaced surfel) counts as empty."""
    n, call, after = us.count, us.call, us.snap
    ok, cand = _lanes(n, call, after, us.camera)
    idx = np.arange(n, dtype=np.uint32)
    before = us.rows.view(np.uint32)[19:23].copy()
    replaced = (after.rows[17, :n].view(np.uint32) == np.uint32(call.frame)) & (us.rows[17].view(np.uint32) != np.uint32(call.frame))
    before[:, replaced] = INVALID
    links = after.rows[19:23, :n].view(np.uint32)
    is_link = np.stack([(cand[d] == before).any(0) for d in range(4)])
    new = (cand != INVALID) & (cand != idx) & ~is_link
    now_link = np.stack([(cand[d] == links).any(0) for d in range(4)])
    changed = (links != before).sum(0)
    out = {}
    out["all_linked"] = int(np.count_nonzero(ok & ((cand != INVALID) & (cand != idx) & is_link).all(0) & (changed == 0)))
    out["new_nearer"] = int(np.count_nonzero(ok & (new & now_link).any(0) & (before != INVALID).all(0) & (changed >= 1)))
    tw = np.zeros(n, bool)
    for a in range(4):
        for b in range(a + 1, 4):
            tw |= new[a] & (cand[a] == cand[b]) & now_link[a] & ((links == cand[a]).sum(0) == 1)
    out["twice"] = int(np.count_nonzero(ok & tw))
    out["self"] = int(np.count_nonzero(ok & (cand == idx).any(0) & new.any(0)))
    out["fills_empty"] = int(np.count_nonzero(ok & (cand == INVALID).any(0) & ((before == INVALID).sum(0) > (links == INVALID).sum(0))))
    # the two tests of a new candidate, in float64 on the rows the integration left behind
    A = after.rows[:, :n].astype(np.float64)
    rf2 = float(call.params.radius_factor_for_regularization_neighbors) ** 2
    too_far, opposed = np.zeros(n, bool), np.zeros(n, bool)
    for d in range(4):
        c = np.where(new[d], cand[d], 0).astype(np.int64)
        d2 = ((A[0:3, c] - A[0:3]) ** 2).sum(0)
        lim = rf2 * A[7]
        nd = (A[8:11, c] * A[8:11]).sum(0)
        too_far |= new[d] & (d2 > lim * (1 + REL)) & ~now_link[d]
        opposed |= new[d] & (d2 < lim * (1 - REL)) & (nd < -REL) & ~now_link[d]
    out["too_far"] = int(np.count_nonzero(ok & too_far))
    out["opposed"] = int(np.count_nonzero(ok & opposed))
    out["lanes"] = int(np.count_nonzero(ok))
    out["lanes_without_new_candidate"] = int(np.count_nonzero(ok & ~new.any(0)))
    return out
