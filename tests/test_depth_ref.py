"""The CPU oracle against a float64 statement of each per-pixel stage (tests/depth_ref.py), on the inputs of
tests/depth_inputs.py over the parameter grid the GPU parity module runs.  The HIP kernels are held bit-equal to the
oracle; this is the check that the oracle -- and with it the kernels -- computes the operation it is meant to.

Integer decisions must agree wherever the float64 quantity is farther from its threshold than a stated float32
rounding margin; the pixels inside a margin are excluded, and may be at most 1 % of the valid pixels.  Float results
must lie within a bound derived from the operation count (depth_ref.py has the derivations).  Every test prints its
observed maxima (pytest -s) and carries them in its assertion messages.

Observed (CPU oracle, this grid; the bounds in brackets):
  bilateral   R = 0 .. 9 x three sigma factors x three ignored values, 131x37 and 20x200: largest |oracle - float64|
              1 unit [1]; at most 0.42 % of the valid pixels differ [1 %]; every difference at most 0.018 units from a
              rounding boundary, at most 0.10 of its margin v (T + 8) 2^-23 [1]; no pixel within the margin of the
              region radius
  cull        undecided pixels at most 0.15 % [1 %]; every other decision equal
  normals     undecided at most 0.58 % (640x480, 89 degrees) [1 %]; largest |n - n64| 3.7e-5, at most 0.088 of the
              per-pixel worst-case bound [1]; median error 0.010 of the bound [1 / 8, see TYPICAL_OVER_WORST_CASE]
  radii       undecided clamp decisions at most 0.074 % [1 %]; largest relative error of radius^2 1.7e-4 (near neighbours
              at 10 m: a difference of nearly equal coordinates), at most 0.63 of the per-pixel bound [1]
"""
import numpy as np
import pytest

import depth_inputs as di
import depth_ref as dr
import oracle as orc

MAX_EXCLUDED = 0.01
# The per-pixel bound of the normals is a WORST CASE: it adds every rounding at its largest (u times the largest
# magnitude the term can have) and all of them with the same sign, so it lets a component error of a few 1e-4 pass at
# a single pixel.  The errors of a correct float32 implementation are not like that: the N roundings are independent
# and roughly uniform in +-u, i.e. of r.m.s. u / sqrt(3), and add in quadrature, so the r.m.s. error over many pixels is
# at most bound / sqrt(3 N).  Counting only the roundings that dominate -- six in x and y of each of the four
# neighbour points, N = 24 -- that is bound / 8.5; the median is below the r.m.s.  A median above 1 / 8 of the bound
# therefore means a systematic error, however far below the worst case it stays.
TYPICAL_OVER_WORST_CASE = 1.0 / 8.0
_radii_pairs = di.CLAMP_PAIRS_BRANCHING + di.CLAMP_PAIRS_ONE_SIDED


def _report(name, **kw):
    print("[depth_ref] %s: %s" % (name, ", ".join("%s=%.4g" % kv for kv in kw.items())))


@pytest.mark.parametrize("w,h", di.BILATERAL_SMALL_SIZES)
@pytest.mark.parametrize("vti", di.VALUES_TO_IGNORE)
@pytest.mark.parametrize("radius", list(range(0, 10)))
def test_bilateral_oracle_matches_float64(w, h, vti, radius):
    """Radii 0 .. 8 as the kernels are instantiated, and 9 (the oracle has no radius limit)."""
    sxy, rf = di.BILATERAL_RADIUS_PAIRS.get(radius, di.BILATERAL_REFUSED_PAIRS[0])
    img = di.noisy_steps(w, h, vti, di.BILATERAL_MAX_DEPTH)
    region = di.corner_cutting_radius(w, h)
    worst = dict(share=0.0, dist=0.0, margin_ratio=0.0)
    pairs = [(sxy, rf)] + [p for r, p in di.BILATERAL_EDGE_PAIRS if r == radius]
    for sxy, rf in pairs:
        for svf in di.SIGMA_VALUE_FACTORS:
            out = orc.bilateral_filter_and_cutoff(img, sxy, svf, vti, rf, di.BILATERAL_MAX_DEPTH, region)
            ref = dr.bilateral(img, sxy, svf, vti, rf, di.BILATERAL_MAX_DEPTH, region)
            assert ref["radius"] == radius
            what = "%dx%d R=%d (%g, %g) svf=%g ignore=%d" % (w, h, radius, sxy, rf, svf, vti)
            cmp_valid = ~ref["region_margin"]
            assert ref["region_margin"].mean() <= MAX_EXCLUDED, what
            valid = ref["valid"]
            # validity: an invalid pixel gives value_to_ignore; a valid one never does except by rounding to it
            assert np.all(out[~valid & cmp_valid] == vti), what
            expect = np.floor(np.where(valid, ref["value"], 0.0))
            diff = np.where(valid & cmp_valid, out.astype(np.float64) - expect, 0.0)
            assert np.abs(diff).max() <= 1, "%s: largest difference %g" % (what, np.abs(diff).max())
            differs = diff != 0
            nv = int((valid & cmp_valid).sum())
            share = differs.sum() / nv
            dist = np.abs(ref["value"] - np.rint(ref["value"]))          # distance of mean + 0.5 to the nearest integer
            margin = dr.bilateral_round_margin(ref, img)
            worst["share"] = max(worst["share"], share)
            if differs.any():
                worst["dist"] = max(worst["dist"], float(dist[differs].max()))
                worst["margin_ratio"] = max(worst["margin_ratio"], float((dist[differs] / margin[differs]).max()))
            assert share <= MAX_EXCLUDED, "%s: %d of %d valid pixels differ (%.2f %%)" % (what, differs.sum(), nv, 100 * share)
            assert np.all(dist[differs] <= margin[differs]), "%s: a difference %.4g from a rounding boundary, margin %.4g" % (
                what, dist[differs].max(), margin[differs][dist[differs].argmax()])
    _report("bilateral %dx%d R=%d ignore=%d" % (w, h, radius, vti), differing_share=worst["share"],
            largest_distance_to_boundary=worst["dist"], largest_distance_over_margin=worst["margin_ratio"])


@pytest.mark.parametrize("count", di.CULL_COUNTS)
def test_cull_oracle_matches_float64(count):
    w, h = 160, 120
    s = di.cull_stream(w, h)
    f = di.CULL_FRAME
    ref_depth = s.frame(f)[0]
    others, T = di.perturbed_others(s, f, count)
    cam = (s.fx, s.fy, s.cx, s.cy)
    worst = 0.0
    for tol in di.CULL_TOLERANCES:
        for req in di.cull_required_counts(count):
            out = orc.outlier_depth_map_fusion(ref_depth, others, T, *cam, tol, req)
            keep, certain = dr.outlier_cull(ref_depth, others, T, *cam, tol, req)
            what = "count %d tolerance %g required %d" % (count, tol, req)
            excluded = (~certain).sum() / (ref_depth != 0).sum()
            worst = max(worst, excluded)
            assert excluded <= MAX_EXCLUDED, "%s: %.2f %% undecided" % (what, 100 * excluded)
            bad = ((out != 0) != keep) & certain
            assert not bad.any(), "%s: %d decisions differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])
            assert np.all(out[out != 0] == ref_depth[out != 0])
    _report("cull count %d" % count, largest_undecided_share=worst)


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_erosion_oracle_matches_its_definition(radius):
    for w, h in di.FAN_SIZES[:1] + ((131, 37),):
        d = di.slanted_fan(w, h)
        assert np.array_equal(orc.erode_depth_map(d, radius), dr.erode(d, radius))


@pytest.mark.parametrize("w,h", di.FAN_SIZES)
@pytest.mark.parametrize("ds", di.DEPTH_SCALINGS)
def test_normals_oracle_matches_float64(w, h, ds):
    cam = di.fan_camera(w, h)
    e = orc.erode_depth_map(di.slanted_fan(w, h, ds), 0)
    worst_excl, worst_ratio, worst_err, worst_median = 0.0, 0.0, 0.0, 0.0
    for thr in di.NORMAL_THRESHOLDS_DEG:
        od, on = orc.compute_normals_and_drop_bad_pixels(e, *cam, thr, ds)
        ref = dr.normals(e, *cam, thr, ds)
        t = ref["tested"]
        assert ref["length"][t].min() > 4e-6             # clear of the degenerate-normal branch
        assert not od[~t].any() and not on[~t].any()
        undecided = t & (np.abs(ref["dot"] - ref["thr"]) <= ref["dot_margin"])
        excl = undecided.sum() / t.sum()
        worst_excl = max(worst_excl, excl)
        what = "%dx%d ds=%g threshold %g" % (w, h, ds, thr)
        assert excl <= MAX_EXCLUDED, "%s: %.2f %% of the tested pixels within the margin" % (what, 100 * excl)
        bad = t & ~undecided & ((od != 0) != ref["keep"])
        assert not bad.any(), "%s: %d angle decisions differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])
        assert np.all(od[od != 0] == e[od != 0])
        err = np.abs(on.astype(np.float64) - ref["n"][..., :2])[t].max(axis=-1)
        ratio = float((err / ref["n_bound"][t]).max())
        worst_ratio, worst_err = max(worst_ratio, ratio), max(worst_err, float(err.max()))
        assert ratio <= 1.0, "%s: normal error %.3g of its bound (largest error %.3g)" % (what, ratio, err.max())
        median = float(np.median(err / ref["n_bound"][t]))
        worst_median = max(worst_median, median)
        assert median <= TYPICAL_OVER_WORST_CASE, "%s: median normal error %.3g of its bound" % (what, median)
    _report("normals %dx%d ds=%g" % (w, h, ds), largest_undecided_share=worst_excl, largest_error=worst_err,
            largest_error_over_bound=worst_ratio, largest_median_error_over_bound=worst_median)


@pytest.mark.parametrize("w,h", di.FAN_SIZES)
@pytest.mark.parametrize("ds", di.DEPTH_SCALINGS)
def test_radii_oracle_matches_float64(w, h, ds):
    cam = di.fan_camera(w, h)
    e = orc.erode_depth_map(di.slanted_fan(w, h, ds), 0)
    nd, _ = orc.compute_normals_and_drop_bad_pixels(e, *cam, 85.0, ds)
    worst_excl, worst_ratio, worst_rel = 0.0, 0.0, 0.0
    for ext, cf in _radii_pairs:
        marker = np.full((h, w), -7.0, np.float32)
        od, orad = orc.compute_point_radii_and_remove_isolated_pixels(nd, *cam, ext, cf, ds, radius_init=marker)
        _, orad_inf = orc.compute_point_radii_and_remove_isolated_pixels(nd, *cam, ext, float("inf"), ds, radius_init=marker)
        ref = dr.radii(nd, *cam, ext, cf, ds)
        m = ref["has"]
        what = "%dx%d ds=%g extension %g clamp %g" % (w, h, ds, ext, cf)
        assert np.array_equal(od != 0, ref["keep"]), what
        assert np.all(od[od != 0] == nd[od != 0]) and np.all(orad[~m] == -7.0), what     # untouched where there is no depth
        excl = ref["clamp_margin"].sum() / m.sum()
        worst_excl = max(worst_excl, excl)
        assert excl <= MAX_EXCLUDED, "%s: %.2f %% of the clamp decisions within the margin" % (what, 100 * excl)
        sure = m & ~ref["clamp_margin"] & (ref["count"] > 0)
        clamped_orc = orad != orad_inf                     # found by comparing with the inf run
        bad = sure & (clamped_orc != ref["clamped"])
        # (where clamping leaves the value as it was the two runs cannot differ; those are inside the margin)
        assert not bad.any(), "%s: %d clamp decisions differ, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])
        mm = m & (ref["count"] > 0)
        err = np.abs(orad.astype(np.float64) - ref["r2"])[mm]
        ratio = float((err / ref["r2_bound"][mm]).max())
        worst_ratio = max(worst_ratio, ratio)
        worst_rel = max(worst_rel, float((err / ref["r2"][mm]).max()))
        assert ratio <= 1.0, "%s: radius error %.3g of its bound (largest relative error %.3g)" % (what, ratio, worst_rel)
    _report("radii %dx%d ds=%g" % (w, h, ds), largest_undecided_share=worst_excl, largest_relative_error=worst_rel,
            largest_error_over_bound=worst_ratio)
