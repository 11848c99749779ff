"""The chains of tests/mesh_update_cases.py without a GPU: every step keeps the margin rule of tests/mesh_cases.py; the
update rule holds on every step from the previous step's state (mesh_ref.triangulate is the truth); the coarse filter
leaves out no slot of D; every designed decision is reached (the census); and every one-decision mutant of the model is
noticed at a named step, or listed as unkillable with its reason.  tests/test_gpu_mesh_update_cases.py runs the same
chains on the device against the same model."""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_ref as mr
import mesh_update_cases as uc
import mesh_update_ref as mu

CHAINS = uc.chains()
IDS = [c.name for c in CHAINS]


def _owned(tri, n):
    return np.bincount(tri[:, 0].astype(np.int64), minlength=n)


def test_chains_are_small_float32_valued_and_named_once():
    assert len(set(IDS)) == len(IDS)
    names = [s.name for c in CHAINS for s in c.steps]
    assert len(set(names)) == len(names)
    for c in CHAINS:
        assert c.steps[0].designed["mode"] == 1
        for s in c.steps:
            assert s.n <= 2000 and s.prm is c.prm
            assert 1.0 <= s.prm.search_radius_factor <= 2.0 and (s.fraction is None or 0.0 <= s.fraction <= 1.0)   # (what the call accepts)
            for a in s.map:
                assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64), equal_nan=True)
            # the filter's threshold 0.25f * h * h is exact in float32
            h = np.float32(s.cell)
            assert float(np.float32(0.25) * h * h) == 0.25 * float(h) * float(h)


@pytest.mark.parametrize("ch", CHAINS, ids=IDS)
def test_every_step_keeps_the_margin_rule(ch):
    seen = set()
    for s in ch.steps:
        key = b"".join(a.tobytes() for a in s.map)
        if key in seen:
            continue
        seen.add(key)
        sw = mc.sweep(*s.map, s.prm, s.exempt)
        for kind, (ratio, where, _) in sorted(sw.margins.items()):
            assert ratio >= mc.Case.margin_of(kind), "%s breaks the margin rule: %s is %.3g of its terms at %s" % (s.name, kind, ratio, where)
        # the stars by the definition are the model's
        truth = uc.truths(ch)[ch.steps.index(s)]
        assert set(sw.stars) == set(truth.stars)
        assert all(sw.stars[p] == truth.stars[p] for p in truth.stars), s.name


@pytest.mark.parametrize("ch", CHAINS, ids=IDS)
def test_rule_from_the_previous_steps_state(ch):
    """test_mesh_update_model.py's argument on every step: no star differs outside D, no slot outside A differs in its owned
    triangles or its star-triangle count, and the previous result patched on A is the new triangulation."""
    t = uc.truths(ch)
    for k in range(1, len(ch.steps)):
        old, new, s = t[k - 1], t[k], ch.steps[k]
        n = new.n
        changed = mu.changed_mask(old.map, new.map)
        dirty = mu.dirty_mask(old.map, new.map, s.prm, changed)
        reagree = mu.reagree_mask(dirty, old.stars, new.stars, n)
        assert np.all(dirty[changed]) and np.all(reagree[dirty])
        assert [p for p in range(n) if not dirty[p] and old.stars.get(p, set()) != new.stars.get(p, set())] == [], s.name
        _, old_counted = mu.agree(old.stars, old.map, s.prm)
        _, new_counted = mu.agree(new.stars, new.map, s.prm)
        assert sum(new_counted.values()) == new.stats["n_star_triangles"]
        assert [p for p in np.nonzero(~reagree)[0] if old_counted.get(int(p), 0) != new_counted.get(int(p), 0)] == [], s.name
        keep_old = old.tri[~reagree[old.tri[:, 0].astype(np.int64)]]
        keep_new = new.tri[~reagree[new.tri[:, 0].astype(np.int64)]]
        assert keep_old.tobytes() == keep_new.tobytes(), s.name
        patched, _ = mu.patch(old.tri, old.stars, new.stars, dirty, reagree, new.map, s.prm)
        assert patched.tobytes() == new.tri.tobytes(), s.name


@pytest.mark.parametrize("ch", CHAINS, ids=IDS)
def test_the_filter_leaves_out_no_slot_of_d(ch):
    t = uc.truths(ch)
    for k in range(1, len(ch.steps)):
        s = ch.steps[k]
        dirty = mu.dirty_mask(t[k - 1].map, t[k].map, s.prm)
        for cell in (s.cell, uc.H_UNFILTERED.get(ch.name)):
            if cell is None:
                continue
            out = mu.filtered_out(t[k - 1].map, t[k].map, s.prm, cell)
            assert not np.any(out & dirty), (s.name, cell, np.nonzero(out & dirty)[0])
            if cell != s.cell:      # the second run of the device test: nothing is filtered, so n_dirty is the exact test's alone
                assert not out.any(), (s.name, cell)


def test_the_reallocation_case_is_tied_to_reserve_keeps_formula():
    assert uc.reserve_keep_formula() == uc.RESERVE_KEEP_GROWTH, "DevBuf::reserve_keep allocates by another formula: re-derive chain Wr"
    assert uc.reserve_keep_capacity(16 * uc.WR_N0) == 6424 and uc.reserve_keep_capacity(uc.WR_N0) == 1361
    ch = uc.chain("Wr")
    assert [s.n for s in ch.steps] == [uc.WR_N0, uc.WR_N1, uc.WR_N1]
    assert uc.reallocates(uc.WR_N0, uc.WR_N1) == {"rings": True, "per_slot": True}
    # the other growing chains: G stays inside its first allocation; Wg's ring rows (352 slots of room after 256) are
    # copied once on the way to 512, its per-slot buffers never
    n = [s.n for s in uc.chain("G").steps]
    assert not any(v for m in n for v in uc.reallocates(n[0], m).values())
    n = [s.n for s in uc.chain("Wg").steps]
    assert [uc.reallocates(n[0], m) for m in n[1:3]] == [{"rings": False, "per_slot": False}, {"rings": True, "per_slot": False}]


# ---- the census: what every step reaches -----------------------------------------------------------------------------------
def _wedges_moved(ch, changed):
    g = ch.roles["groups"]
    return [w for ws in g.values() for w in ws if changed[w["c"]]]


def _census(ch, k, t, c):
    """What step k reaches, as a dict of the same keys as the step's `designed`."""
    s, old, new = ch.steps[k], t[k - 1], t[k]
    n, n_prev = new.n, old.n
    out = dict(mode=c.mode, n_changed=c.n_changed, n_ghosts=c.n_ghosts, n_dirty=c.n_dirty)
    d = s.designed
    f = c.filter
    live_then = mr.live_mask(old.map[0], old.map[2])
    live_now = mr.live_mask(new.map[0], new.map[2])
    if "offsets" in d:
        ws = _wedges_moved(ch, c.changed)
        used = set()
        one = 0
        for w in ws:
            via = f.via[w["q"]]
            one += via == [w["o"]]
            used |= set(via)
            assert c.dirty[w["q"]] and not c.changed[w["q"]]
        out["offsets"], out["q_via_one_cell"] = len(used - {(0, 0, 0)}), one
        _, qc = mu.coarse_cell(*[np.array([new.map[0][w["q"]][a] for w in ws]) for a in range(3)], np.float32(1.0) / np.float32(s.cell))
        if "negative_cells" in d:
            out["negative_cells"] = bool(np.all(qc < 0))
        if "across_zero" in d:
            zero = [i for i, w in enumerate(ws) if w in ch.roles["groups"]["zero"]]
            ok = len(zero) == 26
            for i in zero:
                a0 = next(a for a in range(3) if ws[i]["o"][a] != 0)
                ok &= {int(qc[i][a0]), int(qc[i][a0]) + ws[i]["o"][a0]} == {0, -1}
            out["across_zero"] = ok
        if "ghost_only" in d:
            without = mu.dirty_mask(old.map, new.map, s.prm, c.changed, ("no_ghosts",))
            out["ghost_only"] = not any(without[w["q"]] for w in ws)
    for key, mask in (("subject", f.subject if f else None), ("by_radius", f.by_radius if f else None),
                      ("by_cell", f.by_cell if f else None), ("filtered", f.out if f else None)):
        if key in d:
            if key == "filtered":
                out[key] = sorted(int(i) for i in np.nonzero(mask)[0])
                d = dict(d, filtered=sorted(d["filtered"]))
            else:
                out[key] = [i for i in d[key] if mask[i]]
                assert all(c.dirty[i] for i in d[key]), "a slot the filter lets through by design is not in D"
    if "no_filter" in d:
        out["no_filter"] = f.no_filter
    for key in ("in_d", "not_in_d"):
        if key in d:
            out[key] = [i for i in d[key] if c.dirty[i] == (key == "in_d") and not c.changed[i] and f.subject[i] and not f.out[i]]
    if "ghosts_per_block" in d:
        ghost = np.zeros(n, bool)
        ghost[:n_prev] = c.changed[:n_prev] & live_then
        out["ghosts_per_block"] = [int(ghost[b:b + 256].sum()) for b in range(0, n, 256)]
        assert ghost[[255, 256, 511, 512]].all()
    if "one_word" in d:
        wo, wn = mu.words(old.map), mu.words(new.map)
        cols = {"radius": [3], "normal": [4, 5, 6], "minus_zero": [0, 1, 2]}
        ok = {}
        for what, slot in d["one_word"].items():
            diff = np.nonzero(wo[slot] != wn[slot])[0]
            ok[what] = slot if (diff.size == 1 and int(diff[0]) in cols[what] and c.changed[slot]) else None
            if what == "minus_zero":
                ok[what] = slot if (ok[what] is not None and wo[slot][diff[0]] == 0 and wn[slot][diff[0]] == 0x80000000) else None
        out["one_word"] = ok
    if "nan_now" in d:
        i = d["nan_now"]
        out["nan_now"] = i if (np.isnan(new.map[0][i]).any() and live_then[i] and not live_now[i] and c.changed[i]) else None
    if "revived" in d:
        i = d["revived"]
        out["revived"] = i if (old.map[2][i] < 0 and live_now[i] and np.array_equal(old.map[0][i], new.map[0][i]) and c.changed[i]) else None
    if "appended" in d:
        new_slots = np.arange(n_prev, n)
        merged = [i for i in new_slots if new.map[2][i] < 0]
        old_dirty = [i for i in range(n_prev) if c.dirty[i] and not c.changed[i]]
        pos = np.where(live_now[:, None], new.map[0], np.inf)
        alone = [i for i in new_slots if live_now[i] and np.sum(np.sum((pos - pos[i]) ** 2, axis=1) < 1.5 ** 2) == 1]   # (in empty space)
        assert merged and old_dirty and alone and not c.changed[:n_prev].any()
        out["appended"] = n - n_prev
    if "owner_gains" in d:
        slot, _ = d["owner_gains"]
        out["owner_gains"] = (slot, int(_owned(new.tri, n)[slot]) - int(_owned(old.tri, n)[slot]))
    if "shifted_blocks" in d:
        ob, nb_ = _owned(old.tri, n), _owned(new.tri, n)
        off_o = np.concatenate([[0], np.cumsum([ob[b:b + 256].sum() for b in range(0, n, 256)])])
        off_n = np.concatenate([[0], np.cumsum([nb_[b:b + 256].sum() for b in range(0, n, 256)])])
        out["shifted_blocks"] = [b for b in range((n + 255) // 256) if off_o[b] != off_n[b]]
        for b in out["shifted_blocks"]:        # every run of these workgroups is a kept run, and there are some
            assert not c.reagree[256 * b:256 * b + 256].any()
        assert all(ob[256 * b:256 * b + 256].sum() > 0 for b in (1, 2))
    for key in ("new_ring_owners", "old_ring_owners"):
        if key in d:
            ob, nb_ = _owned(old.tri, n), _owned(new.tri, n)
            moved = [p for p in np.nonzero(c.reagree & ~c.dirty)[0] if ob[p] != nb_[p]]
            sign = 1 if key == "new_ring_owners" else -1
            out[key] = bool(moved) and all(sign * (int(nb_[p]) - int(ob[p])) > 0 for p in moved)
    if "new_block" in d:
        b = (n - 1) // 256
        out["new_block"] = b if (256 * b >= n_prev and n - n_prev == 1) else None
    if "reallocates" in d:
        out["reallocates"] = all(uc.reallocates(ch.steps[0].n, n).values()) and not c.changed[:n_prev].any()
    return out, d


@pytest.mark.parametrize("ch", CHAINS, ids=IDS)
def test_census_every_designed_decision_is_reached(ch):
    t, calls = uc.truths(ch), uc.model_calls(ch)
    print("\n%s: %s" % (ch.name, ch.what))
    for k, (s, c) in enumerate(zip(ch.steps, calls)):
        line = "  %-4s %4d slots, mode %d, changed %d, ghosts %d, |D| %d, |A| %d, kept %d of %d triangles" % (
            s.name, s.n, c.mode, c.n_changed, c.n_ghosts, c.n_dirty, c.n_reagreed, c.n_kept_triangles, t[k].tri.shape[0])
        if c.filter is not None:
            f = c.filter
            used = sorted(set(o for v in f.via.values() for o in v))
            line += "; filter: %d left out, %d let through by radius, %d without a cell, %s, %d offsets used" % (
                f.out.sum(), f.by_radius.sum(), f.by_cell.sum(), "OFF" if f.no_filter else "on", len(used))
        print(line)
        if k == 0:
            assert c.mode == 1
            continue
        got, want = _census(ch, k, t, c)
        extra = {key: v for key, v in got.items() if key not in ("mode", "n_changed", "n_ghosts", "n_dirty")}
        if extra:
            print("       reached: %s" % extra)
        print("       (%s)" % s.why)
        for key, v in want.items():
            assert got[key] == v, "%s: designed %s = %s, reached %s" % (s.name, key, v, got[key])
        if c.mode == 0:
            assert c.tri.tobytes() == t[k].tri.tobytes()


def test_census_across_the_chains():
    """The decisions that need more than one step or chain."""
    modes = {s.name: c.mode for ch in CHAINS for s, c in zip(ch.steps, uc.model_calls(ch))}
    assert modes["M1"] == 0 and modes["M2"] == 4 and modes["M3"] == 0
    m = uc.chain("M")
    assert float(np.float32(uc.M_FRACTION)) * m.steps[1].n == 256.0 == uc.model_calls(m)[1].n_dirty
    assert uc.model_calls(m)[2].n_changed < m.steps[2].n / 2
    # slots on both sides of the radius condition in one map, and of the filter
    f = uc.model_calls(uc.chain("F"))[3].filter
    assert f.by_radius.any() and f.subject.any() and f.out.any() and (f.subject & ~f.out).any()
    # the second cell of the F and D chains filters no live slot
    for name, cell in uc.H_UNFILTERED.items():
        ch = uc.chain(name)
        for s, c in zip(ch.steps, uc.model_calls(ch, cell=cell)):
            assert c.filter is None or not c.filter.out[mr.live_mask(s.map[0], s.map[2])].any(), s.name


# ---- mutants ------------------------------------------------------------------------------------------------------------------
# mutant -> the step that has to notice it (n_changed, n_dirty, mode or the patched bytes differ from the model's)
KILLED_AT = {
    "no_ghosts": "F4", "no_current": "F1", "no_old_rings": "W4", "no_new_rings": "W3", "lt_ball": "D1",
    "ignore_radius": "G2", "ignore_normal": "G2", "zero_equal": "G2", "nan_equal": "G2",
    "face7": "F1", "cells19": "F1", "no_mark_ghosts": "F4", "no_radius": "F3", "ge_path": "M1",
}
UNKILLABLE = {
    "trunc": "truncation makes cell 0 twice as wide (-h, h) and shifts the negative cells by one; a ball of radius <= h / 2 "
             "still lies within the 27 cells around its centre's, and marks and probes use the same function: the filter "
             "stays sound and only lets other slots through.  No count and no byte of the call shows it.  It is held to the "
             "header instead: tests/test_mesh_update_kernel_host.py compares coarse_cell with mesh_coarse_cell bit for bit "
             "on negative coordinates.",
    "radius_without_f2": "the call accepts search_radius_factor in [1, 2] only, so r2 <= h^2 / 4 gives f r <= h, and a ball of "
                         "radius h still lies within the 27 cells around its centre's: a condition on r2 alone filters more "
                         "slots and is still sound.  Step Ff1 shows the side of the condition its slot is on in the census.",
}


def _differs_under_the_mutant(mut):
    """Where the unkillable mutant does differ: in what the filter probes or leaves out, which no call reports."""
    if mut == "trunc":
        ch = uc.chain("F")           # the cells of the marks at negative coordinates
        t = uc.truths(ch)
        a = mu.coarse_filter(t[1].map, t[2].map, ch.prm, ch.cell)
        b = mu.coarse_filter(t[1].map, t[2].map, ch.prm, ch.cell, mut=(mut,))
        return not np.array_equal(a.mark_cells, b.mark_cells)
    ch = uc.chain("Ff")              # q is probed instead of let through, and found: the changed point is in the next cell
    t, q = uc.truths(ch), uc.chain("Ff").roles["q"]
    a = mu.coarse_filter(t[0].map, t[1].map, ch.prm, ch.cell)
    b = mu.coarse_filter(t[0].map, t[1].map, ch.prm, ch.cell, mut=(mut,))
    return bool(a.by_radius[q] and not a.subject[q] and b.subject[q] and not b.out[q])


def _noticed(mut):
    """The steps at which the mutant's call differs from the model's, and how."""
    out = {}
    for ch in CHAINS:
        t, calls = uc.truths(ch), uc.model_calls(ch)
        for k in range(1, len(ch.steps)):
            s, c = ch.steps[k], calls[k]
            m = mu.model_call(t[k - 1], t[k], s.cell, s.fraction, (mut,))
            how = [key for key in ("mode", "n_changed", "n_dirty") if getattr(m, key) != getattr(c, key)]
            if m.tri.tobytes() != t[k].tri.tobytes():
                how.append("bytes")
            if how:
                out[s.name] = how
    return out


def test_mutant_list_is_the_models():
    assert set(KILLED_AT) | set(UNKILLABLE) == set(mu.MUTANTS) and not set(KILLED_AT) & set(UNKILLABLE)
    assert len(UNKILLABLE) <= 3


@pytest.mark.parametrize("mut", sorted(KILLED_AT))
def test_a_mutant_of_the_model_is_noticed_at_its_step(mut):
    got = _noticed(mut)
    print("\n%-18s (%s)\n    noticed at %s" % (mut, mu.MUTANTS[mut], ", ".join("%s (%s)" % (k, "/".join(v)) for k, v in got.items()) or "-"))
    assert KILLED_AT[mut] in got, "%s is not noticed at %s" % (mut, KILLED_AT[mut])


@pytest.mark.parametrize("mut", sorted(UNKILLABLE))
def test_an_unkillable_mutant_is_noticed_nowhere_and_says_why(mut):
    """Not a pass for the cases: the list is what the chains cannot show, with the reason.  (If a step does notice it, the
    entry belongs in KILLED_AT.)"""
    got = _noticed(mut)
    print("\n%-18s (%s)\n    unkillable: %s" % (mut, mu.MUTANTS[mut], UNKILLABLE[mut]))
    assert got == {}, got
    assert _differs_under_the_mutant(mut)
