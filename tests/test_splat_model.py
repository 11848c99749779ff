"""The exact model of the splat render (tests/splat_ref.py) and the hand-built maps (tests/splat_cases.py), without a GPU:
the census shows that the maps take both sides of every decision of k_render_splat and k_render_resolve, the exact model
agrees with the float64 restatement of tests/viz_ref.py within that restatement's own bounds, and every mutant of the
model -- one flipped decision each -- changes what at least one case gives.  Run with -s for the tables."""
import numpy as np
import pytest

import splat_cases as sc
import splat_ref as sp
import viz_ref as vr


@pytest.fixture(scope="module")
def results():
    return [(name, pname, sp.render(rows, n, **kw)) for name, pname, rows, n, kw in sc.runs()]


# decision -> sides that some case has to take (in every parameter set listed; None = in any)
PLANES = ("cz_below", "cz_equal", "cz_above")
REQUIRED = [
    ("merged", ("radius_squared_negative", "radius_squared_nan", "live"), None),
    ("near plane", PLANES + ("cz_nan",), ("disc library", "disc tracker", "disc factor 2 extent 4", "square h=0")),
    ("far plane", PLANES, ("disc library", "disc tracker", "disc factor 2 extent 4", "square h=2")),
    ("projection guard", ("far_outside", "passes"), None),
    ("disc extent", ("dz_at_or_below_near", "dz_equal_near", "clamped", "unclamped"), ("disc library", "disc factor 2 extent 4")),
    ("disc radius", ("zero", "infinite", "finite_positive"), ("disc library",)),
    ("square rule", ("point",), ("square h=0",)),
    ("square rule", ("integer_half_extent",), ("square h=2",)),
    ("square rule", ("half_integer_half_extent",), ("square h=2.5",)),
    ("square centre", ("on_a_pixel_centre", "on_a_pixel_edge", "elsewhere"), ("square h=0", "square h=2", "square h=2.5")),
    ("rectangle", ("clipped_left", "clipped_right", "clipped_top", "clipped_bottom", "outside_left", "outside_right", "outside_top",
                   "outside_bottom", "one_pixel", "inside_unclipped"), ("square h=2", "disc library")),
    ("rectangle", ("empty_before_the_clip",), ("disc library",)),     # (a disc of radius 0 off the pixel centres)
    ("disc pixel", ("edge_on", "not_edge_on", "t_at_or_below_near", "t_above_near", "inside", "on_the_border", "outside",
                    "inside_radius_zero", "inside_radius_infinite"), ("disc library",)),
    ("disc pixel", ("t_at_or_below_near", "t_equal_near", "inside", "outside"), ("disc factor 2 extent 4",)),
    ("z-test", ("first", "win_by_depth", "loss_by_depth", "tie_lower_slot_earlier", "tie_lower_slot_later"), ("square h=2", "disc library")),
    ("resolve", ("empty", "covered"), tuple(sc.PARAMS)),
]


def test_the_cases_take_both_sides_of_every_decision(results):
    for decision, sides, psets in REQUIRED:
        for pset in psets or (None,):
            for side in sides:
                key = "%s: %s" % (decision, side)
                hits = [(name, r["census"][key]) for name, pname, r in results if pset in (None, pname) and r["census"].get(key, 0) > 0]
                print("%-44s %-24s %s" % (key, pset or "any", "; ".join("%s (%d)" % h for h in hits[:3]) or "NOBODY"))
                assert hits, (key, pset)
    # a NaN never reaches the guard: a NaN position makes cz NaN, which the depth test rejects, and no finite float input
    # overflows fx cx / cz in double precision
    assert all(r["census"]["projection guard: nan"] == 0 for _, _, r in results)
    # the views: neither width a multiple of 64, one below it; neither height a multiple of 4
    assert sorted(v[0] for v in sc.VIEWS.values()) == [33, 70] and all(v[0] % 64 and v[1] % 4 for v in sc.VIEWS.values())
    assert all(p.get("max_extent", 16.0) <= 64 for p in sc.PARAMS.values())


def test_every_slot_has_its_reason():
    for name, rows, n, view, notes in sc.cases():
        assert len(notes) == n and all(notes), name
        assert n <= 400


# Mutants whose images no case can tell from the model's, with the reason.  They have to show in the slot rectangles instead
# (which the host walk compares with the model's as well).
IMAGE_EQUIVALENT = {
    "dz_lt": "at dz == near_z the other branch gives min(max_extent, 2 f_max rho / near_z), still at least twice the disc's "
             "projected half width f rho / near_z: the rectangle shrinks, no covered pixel leaves it",
}


def test_every_mutant_of_the_model_is_caught(results):
    runs = list(sc.runs())
    survivors = []
    for mutant, what in sp.MUTANTS.items():
        by_image = by_rect = None
        for (name, pname, rows, n, kw), (_, _, want) in zip(runs, results):
            got = sp.render(rows, n, mutant=mutant, **kw)
            if by_image is None and not sp.same_images(got, want):
                by_image = "%s / %s" % (name, pname)
            if by_rect is None and not np.array_equal(got["rects"], want["rects"]):
                by_rect = "%s / %s" % (name, pname)
            if by_image:
                break
        print("%-11s %-62s -> %s" % (mutant, what, "images of " + by_image if by_image else
                                     ("rectangles of " + by_rect if by_rect else "SURVIVES")))
        if mutant in IMAGE_EQUIVALENT:
            assert by_image is None and by_rect, mutant
        elif not by_image:
            survivors.append(mutant)
    assert not survivors, survivors


def test_the_exact_model_agrees_with_the_float64_restatement_on_the_oracle_map(orc):
    """tests/test_gpu_render.py's own bounds, model against model: the slot may differ only where viz_ref calls the pixel
    unstable and at no more than 0.5 % of the covered pixels, depths agree to 1e-5 relative elsewhere."""
    rows, n, view = sc.oracle_map()
    for mname, mode in sc.GROWN_MODES.items():
        got = sp.render(rows, n, **view, **mode)
        ref = vr.render(rows, n, **view, **mode)
        cov = ref["index"] != vr.INVALID
        diff = got["index"] != ref["index"]
        unstable = vr.unstable(ref)
        same = ~diff & cov
        rel = np.abs(got["depth"][same].astype(np.float64) - ref["depth"][same]) / ref["depth"][same]
        print("%-11s %d slots, %d covered, %d differ (%d of them stable), %d unstable, depth rel max %.3g" % (
            mname, n, cov.sum(), diff.sum(), (diff & ~unstable).sum(), unstable.sum(), rel.max()))
        assert cov.sum() > 0.1 * cov.size
        assert not (diff & ~unstable).any(), np.argwhere(diff & ~unstable)[:5]
        assert diff.sum() <= 0.005 * cov.sum(), (diff.sum(), cov.sum())
        assert rel.max() <= 1e-5, rel.max()
