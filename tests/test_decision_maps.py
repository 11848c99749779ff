"""The crafted map of tests/decision_maps.py on the CPU oracle alone: every one of the twelve decisions is reached on
both sides (census), and the oracle does with each edited group what the decision says, against the group's control.
No GPU; the GPU twin is tests/test_gpu_decision_maps.py."""
import numpy as np
import pytest

import decision_maps as dm

INVALID = 0xFFFFFFFF
MIN_CASES = 20


@pytest.fixture(scope="module")
def run():
    sc = dm.build()
    snaps = dm.run_oracle(sc)
    return sc, snaps


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_state_is_one_the_frame_loop_could_have_produced():
    sc = dm.build()
    rows, n, n0 = sc.rows, sc.count, sc.grown_count
    u32 = rows.view(np.uint32)
    assert n % 1024 != 0 and n > n0
    assert np.all(np.isfinite(rows[0:11]))
    live = rows[7] > 0
    assert np.all(live | (rows[7] < 0)) and np.count_nonzero(~live) == sc.merge_count
    norm = np.sqrt((rows[8:11].astype(np.float64) ** 2).sum(0))
    assert np.abs(norm[live] - 1).max() < 1e-6            # rotated, never rescaled
    links = u32[19:23]
    assert np.all((links == INVALID) | (links < n0))      # kept as grown, or none
    assert np.all(u32[19:23, n0:] == INVALID)
    assert u32[17].max() <= 8 and u32[18].max() <= sc.calls[0].frame == 8
    assert np.all(u32[24, live] >> 24 == 0)            # (merged slots keep the flag the merge gave them)
    # disjoint groups, scattered over the slot range: a run of 64 slots holds several kinds
    kind = np.zeros(n, np.int32)
    for j, (name, idx) in enumerate(sorted(sc.groups.items())):
        assert np.all(kind[idx] == 0), name
        kind[idx] = j + 1
    kinds_per_wave = [len(np.unique(kind[a:a + 64])) for a in range(0, 2048, 64)]
    assert min(kinds_per_wave) >= 4
    for seg in dm.BACK_SEGMENTS:
        assert np.all(np.isin(np.flatnonzero(live[seg * 1024:(seg + 1) * 1024]) + seg * 1024, sc.groups["back_segments"]))


def test_census_every_decision_is_taken_both_ways(run):
    """Printed by this test, (rare side, common side) summed over the calls:
      1  :224 (27238, 191061)  :286 (13663, 100111)  :497 (31190, 214963)  :568 (16553, 132799)
      2  :279 (18042, 113774)  :458 (16962, 246153)
      3  :291 (4231, 42812), of which (888, 1391) in the call under the groups' own pose: the tilted group is turned 45
         degrees, past the 40 degree threshold, and lies 1 % behind the surface -- turned 25 degrees, not one of its slots
         fails the test under its own pose, however large the group
      4  :308 (921, 1614)
      5  :509 (4934, 189518)
      6  :554 (120597, 277052)
      7  :557 u<1 39050, u>=W-1 26562, v<1 14505, v>=H-1 13518, inside 202026; :106 (109, 46603): the valid-depth disc
         leaves few surfels for the last column, which is why there are calls at yaw -9, -12 and -15 as well
      8  :589 (1439, 325096), of which (1051, 16026) under the groups' own pose: a quarter of the slots turned +-65
         degrees -- at +-50 the integration pulls the normals back below 45 degrees and 15 cases remain
      9  :660 (914, 12288)   10  :670 (786, 165256)   11  :113 integrate (154, 245999), create (80, 46678)
     12  :775 (1567, 11973)
    """
    sc, snaps = run
    per_call = [dm.census(sn.rows_before, c, sn) for c, sn in zip(sc.calls, snaps)]
    for c, r in zip(sc.calls, per_call):
        print(c.tag, {k: v for k, v in r.items() if isinstance(k, int)})
    tot = dm.total(per_call)
    print("census:", tot)
    assert sorted(tot) == list(range(1, 13))
    for dec, sites in tot.items():
        for site, (rare, common) in sites.items():
            assert rare >= MIN_CASES and common >= MIN_CASES, (dec, site, rare, common)
    # the groups themselves drive their decisions in the call at their own pose, not only the turned calls
    own = per_call[1]
    for dec, site in ((1, ":286"), (2, ":279"), (3, ":291"), (4, ":308"), (8, ":589"), (9, ":660"), (10, ":670"),
                      (11, ":113 create")):
        assert own[dec][site][0] >= MIN_CASES, (dec, site, own[dec][site])


def test_back_facing_and_occluded_groups_are_left_alone(run):
    sc, snaps = run
    first = snaps[1]                              # frame 9 at its own pose
    sup = first.scratch["supporting"]
    for name in ("back", "back_segments", "occluded"):
        idx = sc.groups[name]
        if name == "occluded":
            # ... where the surfel is occluded at both of its pixels (a depth edge may show it to its second pixel)
            idx = idx[_occluded_everywhere(sc, first, idx)]
            assert len(idx) > 0.9 * len(sc.groups[name])
        for row in (0, 1, 2, 6, 18):
            assert np.array_equal(_bits(first.rows[row, idx]), _bits(first.rows_before[row, idx])), (name, row)
        assert not np.isin(sup, idx).any(), name
    for name in ("control", "occluded_control"):
        idx = sc.groups[name]
        stamped = first.rows[18, idx].view(np.uint32) == 9
        assert stamped.mean() > 0.5, (name, stamped.mean())      # (the rest lies outside frame 9 or under its edits)
        assert np.isin(idx, sup).mean() > 0.25, name
    # the two whole back-facing segments stay untouched through every call at a pose near their own
    for c, sn in zip(sc.calls[1:], snaps[1:]):
        if abs(c.pose.astype(np.float64)[:, 2] @ sc.pose9.astype(np.float64)[:, 2]) > 0.9:
            idx = sc.groups["back_segments"]
            idx = idx[sn.rows_before[17, idx].view(np.uint32) <= 8]      # (a conflict may have replaced a slot since)
            assert len(idx) > 1500 and not np.isin(sn.scratch["supporting"], idx).any(), c.tag


def _occluded_everywhere(sc, snap, idx):
    c = sc.calls[1]
    fx, fy, cx, cy = sc.camera
    G = c.pose.astype(np.float64)
    loc = G[:, :3].T @ (snap.rows_before[0:3, idx].astype(np.float64) - G[:, 3:4])
    u, v = fx * loc[0] / loc[2] + cx, fy * loc[1] / loc[2] + cy
    px, py = np.floor(u).astype(int), np.floor(v).astype(int)
    ok = np.ones(len(idx), bool)
    depth = c.depth.astype(np.float64) / c.depth_scaling
    for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        md = depth[np.clip(py + dy, 0, dm.H - 1), np.clip(px + dx, 0, dm.W - 1)]
        ok &= (md == 0) | (loc[2] > 1.06 * md)
    return ok


def test_pairs_25_degrees_apart_both_stay_while_5_degree_pairs_merge(run):
    sc, snaps = run
    first = snaps[1]
    sup = first.scratch["supporting"]
    fx, fy, cx, cy = sc.camera
    G = sc.calls[1].pose.astype(np.float64)
    outcome = {}
    for name in ("pair25", "pair5", "pair5_behind", "tilted_pair", "pair5_occluded"):
        src, cp = sc.groups[name], sc.groups[name + "_copy"]
        loc = G[:, :3].T @ (first.rows_before[0:3, cp].astype(np.float64) - G[:, 3:4])
        px, py = np.floor(fx * loc[0] / loc[2] + cx).astype(int), np.floor(fy * loc[1] / loc[2] + cy).astype(int)
        met = sup[py, px] == src                  # the copy met its original as the supporting surfel of its pixel
        assert met.sum() > 0.25 * len(src), (name, met.sum())   # (elsewhere a lower slot supports the pixel)
        assert np.all(first.rows_before[7, cp] > 0) and np.all(first.rows_before[7, src] > 0)
        outcome[name] = (first.rows[7, src[met]] > 0, first.rows[7, cp[met]] > 0)
    assert outcome["pair25"][0].all() and outcome["pair25"][1].all()        # 25 degrees: both copies stay live
    assert outcome["pair5"][0].all() and not outcome["pair5"][1].any()      # 5 degrees: the copy is merged away
    # a copy just behind the measured surface: merged where its normal is compatible with the measured one, kept where it
    # is 45 degrees off -- although it equals its original's (:291)
    assert outcome["pair5_behind"][0].all() and not outcome["pair5_behind"][1].any()
    assert outcome["tilted_pair"][0].all() and outcome["tilted_pair"][1].all()
    # a copy just outside the noise band behind the surface, its original just inside: occluded, so it stays (:279)
    assert outcome["pair5_occluded"][0].all() and outcome["pair5_occluded"][1].all()
    gone = sc.groups["pair5_copy"][first.rows[7, sc.groups["pair5_copy"]] < 0]
    assert np.all(first.rows[18, gone].view(np.uint32) == 0) and np.all(first.rows[24, gone].view(np.uint32) >> 24 == 1)


def _uv(rows, call, sc):
    fx, fy, cx, cy = sc.camera
    G = call.pose.astype(np.float64)
    loc = G[:, :3].T @ (rows[0:3].astype(np.float64) - G[:, 3:4])
    with np.errstate(divide="ignore", invalid="ignore"):
        return loc[2], fx * loc[0] / loc[2] + cx, fy * loc[1] / loc[2] + cy


def test_new_links_obey_the_gates_of_the_neighbour_update(run):
    """Decisions 1 (:568), 6, 7 (:557) and 8: a surfel seen from behind, behind the camera or projecting into the one
    pixel border finds no new neighbour, and no new link joins opposing normals.  The controls: the links the other
    surfels find, among them those in the first column and row inside the border (the turned calls' images are valid up
    to the edge, or the zero border of a preprocessed depth image would hide :557 behind the occlusion test)."""
    sc, snaps = run
    found = barred = from_behind_camera = seen_from_behind = 0
    found_at = {"x=1": 0, "x=W-2": 0, "y=1": 0, "y=H-2": 0}
    eps = 1e-3
    for c, sn in zip(sc.calls[1:], snaps[1:]):
        n = sn.rows_before.shape[1]
        before, after = sn.rows_before[19:23].view(np.uint32), sn.rows[19:23, :n].view(np.uint32)
        new_link = (after != before) & (after != INVALID)
        gained = new_link.any(0)
        z, u, v = _uv(sn.rows[:, :n], c, sc)
        outside = (z <= 0) | (u < 1 - eps) | (u >= dm.W - 1 + eps) | (v < 1 - eps) | (v >= dm.H - 1 + eps)
        assert not gained[outside].any(), c.tag
        live = sn.rows[7, :n] > 0
        barred += np.count_nonzero(outside & live & (z > 0))
        if sn.stats["n_visible"] > 0:
            from_behind_camera += np.count_nonzero(live & (z <= 0))
        nrm = sn.rows[8:11, :n].astype(np.float64)
        G = c.pose.astype(np.float64)
        view = G[:, :3].T @ (sn.rows[0:3, :n].astype(np.float64) - G[:, 3:4])
        dot_view = ((G[:, :3].T @ nrm) * view).sum(0) / np.sqrt((view * view).sum(0))
        back = dot_view > 1e-4
        assert not gained[back].any(), c.tag
        seen_from_behind += np.count_nonzero(back & live & ~outside)
        for j in range(4):
            i = np.flatnonzero(new_link[j])
            assert np.all((nrm[:, i] * nrm[:, after[j, i]]).sum(0) > 0), (c.tag, j)
        found += np.count_nonzero(new_link)
        inside = ~outside & (z > 0)
        for name, m in (("x=1", (u >= 1 + eps) & (u < 2 - eps)), ("x=W-2", (u >= dm.W - 2 + eps) & (u < dm.W - 1 - eps)),
                        ("y=1", (v >= 1 + eps) & (v < 2 - eps)), ("y=H-2", (v >= dm.H - 2 + eps) & (v < dm.H - 1 - eps))):
            found_at[name] += np.count_nonzero(gained & inside & m)
    print("new links:", found, "in the first rows / columns inside the border:", found_at, "surfels in the border:", barred,
          "behind the camera with supporting surfels in view:", from_behind_camera, "seen from behind:", seen_from_behind)
    assert barred > 10000 and found > 2000 and seen_from_behind > 10000, (barred, found, seen_from_behind)
    assert from_behind_camera > 10000
    assert min(found_at.values()) >= MIN_CASES, found_at


def test_supporting_surfels_project_into_their_pixel_or_next_to_it(run):
    """Decision 7 (:106): the quadrant neighbour never leaves the image row."""
    sc, snaps = run
    seen = 0
    for c, sn in zip(sc.calls[1:], snaps[1:]):
        sup = sn.scratch["supporting"]
        y, x = np.nonzero(sup != INVALID)
        z, u, v = _uv(sn.rows_before[:, sup[y, x]], c, sc)
        du, dv = np.abs(u - (x + 0.5)), np.abs(v - (y + 0.5))
        eps = 1e-3
        assert np.all(z > 0) and np.all(((du <= 0.5 + eps) & (dv <= 1.5 + eps)) | ((du <= 1.5 + eps) & (dv <= 0.5 + eps))), c.tag
        seen += len(x)
        # ... and the min-depth image is set only where a surfel projects into the pixel or next to it
        first = sn.scratch["first_depth"]
        z, u, v = _uv(sn.rows_before, c, sc)
        ok = (z > 0) & (u >= 0) & (v >= 0) & (u < dm.W) & (v < dm.H)
        px, py = np.floor(u[ok]).astype(int), np.floor(v[ok]).astype(int)
        near = np.zeros((dm.H + 2, dm.W + 2), bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                near[py + dy, px + dx] = True
        assert not (np.isfinite(first) & ~near[1:-1, 1:-1]).any(), c.tag
    assert seen > 50000


def test_repeated_frame_index_does_not_integrate_into_its_own_new_surfels(run):
    sc, snaps = run
    k = [i for i, c in enumerate(sc.calls) if "same frame index" in c.tag][0]
    assert sc.calls[k].frame == sc.calls[k - 1].frame
    a, b = snaps[k - 1], snaps[k]
    n_new = a.stats["n_new"]
    assert n_new > 1000
    new = np.arange(a.count - n_new, a.count)
    assert np.all(a.rows[6, new] == 1.0) and np.all(b.rows[6, new] == 1.0)
    assert np.all(b.rows[17, new].view(np.uint32) == sc.calls[k].frame)
    old = np.flatnonzero((a.rows[17, :a.count - n_new].view(np.uint32) < sc.calls[k].frame) & (a.rows[7, :a.count - n_new] > 0))
    grew = b.rows[6, old] > a.rows[6, old]
    assert grew.sum() > 1000                      # the control: older surfels do take the second measurement


def test_a_camera_turned_away_integrates_nothing_and_keeps_the_links(run):
    sc, snaps = run
    k = [c.tag for c in sc.calls].index("yaw 120")
    sn = snaps[k]
    n = sn.rows_before.shape[1]
    assert sn.stats["n_integrated"] == 0 and sn.stats["n_visible"] == 0 and sn.stats["n_merged"] == 0
    assert not (sn.scratch["supporting"] != INVALID).any()
    for row in (0, 1, 2, 6, 7, 8, 9, 10, 17, 18, 24):
        assert np.array_equal(_bits(sn.rows[row, :n]), _bits(sn.rows_before[row, :n])), row
    before, after = sn.rows_before[19:23].view(np.uint32), sn.rows[19:23, :n].view(np.uint32)
    # no link finds a new target; the regulariser that follows may still drop one whose smooth ends drifted apart
    assert np.all((after == before) | (after == INVALID))
    assert (after != before).mean() < 0.01
    assert sn.stats["n_new"] > 5000


def test_new_surfels_on_a_depth_step_have_no_link_across_it(run):
    sc, snaps = run
    c, sn = sc.calls[1], snaps[1]
    new_flags, new_indices = sn.scratch["new_flags"], sn.scratch["new_indices"]
    base = sn.rows_before.shape[1]
    depth = sn.depth.astype(np.float64) / c.depth_scaling
    ys = np.arange(dm.H)[dm.STEP_ROWS]
    links = sn.rows[19:23].view(np.uint32)        # directions: left, right, up, down
    checked = 0
    for y in ys:
        for x in range(dm.STEP_COLS.start + 1, dm.STEP_COLS.stop - 1):
            if new_flags[y, x] != 1:
                continue
            slot = base + new_indices[y, x]
            reach = 2.0 * np.sqrt(c.radius[y, x])
            for d, yy in ((2, y - 1), (3, y + 1)):
                if depth[yy, x] > 0 and abs(depth[yy, x] - depth[y, x]) > 1.1 * reach:   # the step alone is too far
                    assert links[d, slot] == INVALID, (y, x, d)
                    checked += 1
    assert checked > 300
    # new pixels on both sides of a step: rows 7 % and 14 % nearer than the map alternate, no link goes up or down
    checked = level = 0
    across = []
    for y in range(dm.STEP2_ROWS.start + 1, dm.STEP2_ROWS.stop - 1):
        for x in range(dm.STEP2_COLS.start, dm.STEP2_COLS.stop):
            if new_flags[y, x] != 1:
                continue
            slot = base + new_indices[y, x]
            reach = 2.0 * np.sqrt(c.radius[y, x])
            for d, yy, xx in ((2, y - 1, x), (3, y + 1, x), (0, y, x - 1), (1, y, x + 1)):
                if new_flags[yy, xx] != 1:
                    continue
                if abs(depth[yy, xx] - depth[y, x]) > 1.1 * reach:
                    assert d >= 2 and links[d, slot] == INVALID, (y, x, d)
                    checked += 1
                    across.append(slot)
                elif abs(depth[yy, xx] - depth[y, x]) < 0.9 * reach:
                    assert links[d, slot] == base + new_indices[yy, xx], (y, x, d)
                    level += 1
    assert checked > 300 and level > 300, (checked, level)
    # the regulariser that ends the call drops a link that long itself (:740), but not before it has pulled on it: with
    # a link across the step the smooth position moves a whole radius (the step clamp), without one hardly at all
    across = np.unique(across)
    pulled = np.sqrt(((sn.rows[3:6, across].astype(np.float64) - sn.rows[0:3, across]) ** 2).sum(0) / sn.rows[7, across])
    assert np.median(pulled) < 0.1, np.median(pulled)
    # control: new surfels away from the edits link to a neighbour above or below
    yy, xx = np.nonzero(new_flags[60:110, 20:140] == 1)
    slots = base + new_indices[60:110, 20:140][yy, xx]
    assert len(slots) > 50 and ((links[2, slots] != INVALID) | (links[3, slots] != INVALID)).mean() > 0.8


def test_displaced_smooth_positions_move_by_one_radius(run):
    sc, snaps = run
    c, sn = sc.calls[0], snaps[0]
    assert c.kind == "regularize"
    cen = dm.census(sn.rows_before, c, sn)
    moved = np.sqrt(((sn.rows[3:6].astype(np.float64) - sn.rows_before[3:6].astype(np.float64)) ** 2).sum(0))
    radius = np.sqrt(np.maximum(sn.rows_before[7].astype(np.float64), 0))
    grp = sc.groups["clamp"]
    clamped, free = grp[cen["clamped"][grp]], grp[cen["free"][grp]]
    assert len(clamped) > 0.25 * len(grp) and len(free) > 20
    # smooth positions of a few metres: one float32 ulp is 2.4e-7 m per axis, the step adds a rounding of its own
    assert np.abs(moved[clamped] - radius[clamped]).max() < 2e-6
    assert np.all(moved[free] < radius[free])
    ctl = sc.groups["control"]
    assert np.all(moved[ctl] <= radius[ctl] + 2e-6) and np.median(moved[ctl] / radius[ctl]) < 0.5
    for row in (0, 1, 2, 6, 7, 8, 9, 10, 17, 18, 24):
        assert np.array_equal(_bits(sn.rows[row]), _bits(sn.rows_before[row])), row
