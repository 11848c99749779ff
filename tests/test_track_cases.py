"""The tracking sums bit for bit, without a GPU: the header's own functions walked in the launch's order
(tests/track_host.py) against the exact model (tests/track_exact.py) on the hand-built cases of tests/track_cases.py -- every
case, every stride, without and with colour: the sums of both records of a (stride, 1), (stride, 1) schedule, P, and the end of
the call.  The exact model in turn stays within the derived bound of the float64 restatement, so it cannot drift from the
algorithm.  A census over the exact model's exit codes asserts that the cases take both sides of every decision (`-s` prints
the table of DESIGN.md 5c), and one-decision mutants of the exact model must each change the sums of a named case."""
import ctypes as C

import numpy as np
import pytest

import track_cases as tc
import track_exact as tx
import track_host as th
import track_ref as tr
import track_rgbd_ref as trr
from test_track_kernel_host import _sum_bounds


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return th.host_library(tmp_path_factory.mktemp("track_host"))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_call(c, p, records, result, photo, note, Tf_start=None, depth_scaling=None):
    """What both the host walk and the device are held to: records and result against exact_call with the recorded twists.
    Returns exact_call's dict."""
    D, M, Cm, P = c.model()
    want = tx.exact_call(D, M, c.depth, c.normals, c.intrinsics, c.pred, p, depth_scaling or c.depth_scaling, (P, c.color) if photo else None,
                         [r["x"] for r in records], Tf_start)
    assert len(records) == len(want["records"]), (note, len(records), len(want["records"]))
    for k, (g, w) in enumerate(zip(records, want["records"])):
        assert (g["level"], g["stride"], g["status"]) == (w["level"], w["stride"], w["status"]), (note, k, g["status"], w["status"])
        n = len(g["sums"])
        assert np.array_equal(_bits(g["sums"]), _bits(w["sums"][:n])), (note, k, np.nonzero(_bits(g["sums"]) != _bits(w["sums"][:n]))[0])
        assert np.all(w["sums"][n:] == 0)
        assert np.allclose(g["x"], w["x_ref"], rtol=1e-9, atol=1e-15), (note, k)
    assert th.same_result(result, want) == [], (note, th.same_result(result, want))
    return want


@pytest.mark.parametrize("name", tc.NAMES)
def test_the_walk_gives_the_exact_models_bits(host, name):
    c = tc.by_name(name)
    D, M, Cm, P = c.model()
    got_P = np.full((c.height, c.width, 4), 7.0, np.float32)
    host.host_prepare(c.width, c.height, C.c_float(c.params([(1, 1)]).gradient_max_relative_depth_step), th.ptr(D), th.ptr(Cm), th.ptr(got_P))
    assert np.array_equal(got_P.view(np.uint32), P.view(np.uint32))
    slabs = th.new_slabs()      # one buffer for all the calls, never cleared: a stale slab at the other stride would be read
    for stride in tc.STRIDES:
        n = tx.samples(c.width, stride) * tx.samples(c.height, stride)
        assert host.host_samples(c.width, stride) == tx.samples(c.width, stride)
        assert host.host_grid(n) == tx.grid_of(n)
        for photo in (True, False, True):
            p = c.params([(stride, 1), (stride, 1)])
            records, result, _ = th.walk_call(host, D, M, c.depth, c.normals, c.intrinsics, c.pred, p, c.depth_scaling,
                                              (P, c.color) if photo else None, slabs=slabs)
            want = check_call(c, p, records, result, photo, (name, stride, photo))
            if n == 0:
                assert len(records) == 1 and np.all(records[0]["sums"] == 0) and result["status"] == tr.TOO_FEW_INLIERS
            # the exact model against the float64 restatement, within the derived bound
            for w in want["records"]:
                T = w["Tf"].astype(np.float64)
                if photo:
                    ref, mg = trr.iteration(D, M, P, c.depth, c.normals, c.color, c.intrinsics, T, stride, p, c.depth_scaling)
                    diff, bound = trr.compare_sums(w["sums"], ref, mg, p, _sum_bounds)
                    counts = (tr.S_ASSOCIATED, tr.S_INLIERS, trr.S_PHOTO_INLIERS)
                else:
                    _, _, _, inl, pix, mg = tr.iteration(D, M, c.depth, c.normals, c.intrinsics, T, stride, p.gates(), c.depth_scaling)
                    ref = mg["sums"]
                    bound = _sum_bounds(inl, mg["flagged"], max(mg["p_max"], 1.0), p.max_distance)
                    diff = np.abs(w["sums"][:28] - ref[:28])
                    counts = (tr.S_ASSOCIATED, tr.S_INLIERS)
                assert np.all(diff <= bound), (name, stride, photo, int(np.argmax(diff - bound)))
                assert w["sums"][tr.S_PIXELS] == ref[tr.S_PIXELS]
                for e in counts:
                    assert abs(w["sums"][e] - ref[e]) <= mg["flagged"], (name, stride, e)


def test_the_clamped_grid_and_the_ninth_visit(host):
    """1026 x 512: 525 312 samples at stride 1 -- 257 workgroups by the division, 256 launched, 1024 lanes with a ninth
    sample; 65 workgroups at stride 2.  One iteration per stride, without and with colour."""
    c = tc.clamp_case()
    D, M, Cm, P = c.model()
    assert c.rows.shape[1] > 15000
    p = c.params([(1, 1)])
    grids = {}
    for stride in tc.STRIDES:
        n = tx.samples(c.width, stride) * tx.samples(c.height, stride)
        for photo in (None, (P, c.color)):
            got, grid = th.walk_reduce(host, D, M, c.depth, c.normals, c.intrinsics, tr.IDENTITY, stride, p, c.depth_scaling, photo)
            want, codes = tx.exact_sums(D, M, c.depth, c.normals, c.intrinsics, tr.IDENTITY, stride, p.gates(), c.depth_scaling,
                                        (P, c.color, p) if photo else None)
            assert np.array_equal(_bits(got), _bits(want)), (stride, photo is not None)
            assert grid == tx.grid_of(n) and want[tr.S_INLIERS] > 0.5 * n
            grids[stride] = (n, grid)
    assert grids[1] == (525312, 256) and -(-525312 // 2048) == 257 and 525312 > 8 * 256 * 256
    assert grids[2] == (131328, 65)
    # the order matters at this size: the mutants of the structure that need many slabs
    base, _ = tx.exact_sums(D, M, c.depth, c.normals, c.intrinsics, tr.IDENTITY, 1, p.gates(), c.depth_scaling)
    for mutant in ("clamp255", "slabs_reversed"):
        other, _ = tx.exact_sums(D, M, c.depth, c.normals, c.intrinsics, tr.IDENTITY, 1, p.gates(), c.depth_scaling, mutant=mutant)
        assert not np.array_equal(_bits(base), _bits(other)), mutant
        assert np.array_equal(base[28:], other[28:])


# ---- the census ----------------------------------------------------------------------------------------------------------
def _census():
    """{side: {case name: count}} over every case, stride and both records, from the exact model's exit codes."""
    table = {}

    def add(side, name, k):
        table.setdefault(side, {})
        table[side][name] = table[side].get(name, 0) + int(k)
    for name in tc.NAMES:
        c = tc.by_name(name)
        D, M, Cm, P = c.model()
        for k, v in tc.prepare_census(D, c.params([(1, 1)]).gradient_max_relative_depth_step).items():
            add("track_photo_pixel: " + k, name, v)
        for stride in tc.STRIDES:
            p = c.params([(stride, 1), (stride, 1)])
            r = tx.exact_call(D, M, c.depth, c.normals, c.intrinsics, c.pred, p, c.depth_scaling, (P, c.color))
            for it, rec in enumerate(r["records"]):
                geo, ph = rec["codes"]["geo"], rec["codes"]["photo"]
                for e, text in enumerate(tr.EXITS):
                    add("track_pixel: " + text, name, (geo == e).sum())
                add("track_pixel: depth not 0", name, (geo != tr.EXIT_NO_DEPTH).sum())
                add("track_pixel: pz > 0", name, (geo > tr.EXIT_BEHIND).sum())
                add("track_pixel: inside the image", name, (geo >= tr.EXIT_HOLE).sum())
                add("track_pixel: Dq > 0", name, (geo >= tr.EXIT_DISTANCE).sum())
                add("track_pixel: distance gate passed", name, (geo >= tr.EXIT_ANGLE).sum())
                add("track_pixel: frame normal clamped (nx^2 + ny^2 > 1)", name, rec["codes"]["clamped"].sum())
                add("track_pixel: frame normal not clamped", name, ((geo != tr.EXIT_NO_DEPTH) & ~rec["codes"]["clamped"]).sum())
                add("track_pixel: angle gate failed, photometric inlier", name, ((geo == tr.EXIT_ANGLE) & (ph == 3)).sum())
                for e, text in enumerate(tx.PHOTO_EXITS):
                    add("track_pixel: " + text, name, (ph == e).sum())
                add("track_pixel: P.w = 1", name, (ph >= 1).sum())
                add("track_pixel: gradient at or above min_gradient", name, (ph >= 2).sum())
                if it == 1:
                    for e in (tr.EXIT_LEFT, tr.EXIT_RIGHT, tr.EXIT_TOP, tr.EXIT_BOTTOM):
                        add("after an update: " + tr.EXITS[e], name, (geo == e).sum())
    return table


# a side no case reaches on the device, with the reason; taken by test_the_side_only_the_host_walk_takes
UNREACHED = {"track_pixel: pz <= 0": "T_rel starts at the identity and a frame depth is positive, so pz = z > 0 in the first "
             "iteration; later only an update that turns the camera by more than a right angle could put a point behind it, and "
             "no solvable case here produces one"}


def test_every_side_of_every_decision_is_taken():
    table = _census()
    print("\n%-62s %8s  %s" % ("side", "samples", "cases"))
    for side, by in table.items():
        total = sum(by.values())
        print("%-62s %8d  %s" % (side, total, ", ".join("%s %d" % (n, k) for n, k in by.items() if k) or "-"))
        if side in UNREACHED:
            assert total == 0, side
        else:
            assert total > 0, side
    assert set(UNREACHED) <= set(table)
    # opposite motions: each of the four sides after a real update
    right, left = "corner right 70x37", "corner left 70x37"
    assert table["after an update: uf >= W"][right] > 0 and table["after an update: wf >= H"][right] > 0
    assert table["after an update: uf < 0"][left] > 0 and table["after an update: wf < 0"][left] > 0


def test_the_side_only_the_host_walk_takes(host):
    """pz <= 0: handed a Tf that looks backwards, every sample with depth leaves there (and one that puts a point exactly
    into the camera plane, pz = 0, leaves there too); walk and model agree on the sums, and a whole call from that Tf ends as
    DEGENERATE with nothing associated."""
    c = tc.by_name("corner right 70x37")
    D, M, Cm, P = c.model()
    p = c.params([(2, 1)])
    back = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0]], np.float32)
    plane = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]], np.float32)      # pz = 0 exactly for every sample
    for Tf in (back, plane):
        got, _ = th.walk_reduce(host, D, M, c.depth, c.normals, c.intrinsics, Tf, 2, p, c.depth_scaling, (P, c.color))
        want, codes = tx.exact_sums(D, M, c.depth, c.normals, c.intrinsics, Tf, 2, p.gates(), c.depth_scaling, (P, c.color, p))
        assert np.array_equal(_bits(got), _bits(want))
        assert np.all(codes["geo"][codes["geo"] != tr.EXIT_NO_DEPTH] == tr.EXIT_BEHIND) and want[tr.S_PIXELS] > 0
        assert want[tr.S_ASSOCIATED] == 0 and np.all(want[:28] == 0)
    records, result, _ = th.walk_call(host, D, M, c.depth, c.normals, c.intrinsics, c.pred, p, c.depth_scaling, None, Tf_start=back)
    check_call(c, p, records, result, False, "backwards", Tf_start=back)
    assert result["status"] == tr.DEGENERATE


# ---- mutants -------------------------------------------------------------------------------------------------------------
# mutant -> (case, stride, with colour, record): the named case whose sums it must change
MUTANT_CASES = {
    "distance_lt": ("gates 70x37", 1, False, 0),
    "angle_gt": ("gates 70x37", 1, False, 0),
    "gradient_gt": ("gates 70x37", 1, True, 0),
    "intensity_lt": ("gates 70x37", 1, True, 0),
    "rint": ("corner right 70x37", 2, False, 1),
    "photo_angle": ("corner right 70x37", 1, True, 0),
    "no_half": ("corner left 70x37", 4, True, 1),
    "slab32": ("corner right 70x37", 1, True, 0),
    # (a term is one float widened to double: sums of terms of similar size are exact, and where they are not another order
    # moves the last bit of few sums and of none at the small strides; the photometric rows, with their wider range, show it)
    "waves_reversed": ("corner right 70x37", 2, True, 0),
    "lanes_strided": ("corner right 70x37", 1, True, 0),
}
# (these two need more than two slabs -- two are added commutatively: tests/test_track_cases.py::test_the_clamped_grid_...)
MUTANTS_AT_THE_CLAMP = ("clamp255", "slabs_reversed")


def test_every_mutant_is_detected_by_a_named_case():
    assert set(MUTANT_CASES) | set(MUTANTS_AT_THE_CLAMP) == set(tx.MUTANTS)
    for mutant, (name, stride, photo, k) in MUTANT_CASES.items():
        c = tc.by_name(name)
        D, M, Cm, P = c.model()
        p = c.params([(stride, 1), (stride, 1)])
        r = tx.exact_call(D, M, c.depth, c.normals, c.intrinsics, c.pred, p, c.depth_scaling, (P, c.color) if photo else None)
        Tf = r["records"][k]["Tf"]
        ph = (P, c.color, p) if photo else None
        base, _ = tx.exact_sums(D, M, c.depth, c.normals, c.intrinsics, Tf, stride, p.gates(), c.depth_scaling, ph)
        assert np.array_equal(_bits(base), _bits(r["records"][k]["sums"][:len(base)]))
        other, _ = tx.exact_sums(D, M, c.depth, c.normals, c.intrinsics, Tf, stride, p.gates(), c.depth_scaling, ph, mutant=mutant)
        changed = np.nonzero(_bits(base) != _bits(other))[0]
        print("%-15s %-22s stride %d record %d: %d of %d sums change" % (mutant, name, stride, k, len(changed), len(base)))
        assert len(changed) > 0, (mutant, tx.MUTANTS[mutant])
        if mutant in ("distance_lt", "angle_gt", "gradient_gt", "intensity_lt"):
            # exactly one sample sits on the gate... or a few: the count that drops says how many
            e = tr.S_INLIERS if mutant in ("distance_lt", "angle_gt") else trr.S_PHOTO_INLIERS
            assert 1 <= base[e] - other[e], (mutant, base[e], other[e])


# ---- the end of a call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("photo", [False, True], ids=["plain", "rgbd"])
def test_the_end_of_a_call_on_the_host(host, photo):
    c = tc.by_name("corner right 70x37")
    D, M, Cm, P = c.model()
    ph = (P, c.color) if photo else None

    for name, kw, ds, exact, expect in tc.end_of_call_variants(c, photo):
        p = c.params(**kw)
        records, result, _ = th.walk_call(host, D, M, c.depth, c.normals, c.intrinsics, c.pred, p, ds, ph)
        print(name, [(q["level"], q["status"]) for q in records][:12], result["status"])
        want = check_call(c, p, records, result, photo, name, depth_scaling=ds) if exact else None
        expect(records, result, want)
