"""The inputs of depth_inputs.py make the preprocessing stages decide BOTH ways, for every parameter value of the grid
that tests/test_gpu_preprocess_params.py runs on the GPU.  Asserted on the CPU oracle's output alone, so it is checked
wherever the suite runs: a parity case whose branch is never (or always) taken would pass vacuously.

Each condition: the branch is taken by at least 5 % of the valid pixels and not taken by at least 5 %.
"""
import numpy as np
import pytest

import depth_inputs as di
import oracle as orc

MIN_SHARE = 0.05


def _both_ways(taken, of, what):
    n, k = int(of.sum()), int((taken & of).sum())
    assert n > 0, what
    assert MIN_SHARE * n <= k <= (1 - MIN_SHARE) * n, "%s: branch taken by %d of %d valid pixels (%.1f %%)" % (
        what, k, n, 100.0 * k / n)


def _disc_holds(mask, R):
    """[h,w] bool: a pixel of `mask` lies in the disc of radius R around the pixel (centre excluded)."""
    h, w = mask.shape
    out = np.zeros((h, w), bool)
    p = np.pad(mask, R)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if 0 < dx * dx + dy * dy <= R * R:
                out |= p[R + dy:R + dy + h, R + dx:R + dx + w]
    return out


def test_radius_pairs_reach_every_radius():
    for r, (sxy, rf) in di.BILATERAL_RADIUS_PAIRS.items():
        assert di._radius_of(sxy, rf) == r
    for r, (sxy, rf) in di.BILATERAL_EDGE_PAIRS:
        assert di._radius_of(sxy, rf) == r
    # the edge pairs really are the last float32 inside: one step further gives another radius
    (_, (s, lo1)), (_, (_, hi1)), (_, (s8, lo8)), (_, (_, hi8)) = di.BILATERAL_EDGE_PAIRS
    f32 = np.float32
    assert di._radius_of(s, np.nextafter(f32(lo1), f32(-np.inf))) == 0 and di._radius_of(s, np.nextafter(f32(hi1), f32(np.inf))) == 2
    assert di._radius_of(s8, np.nextafter(f32(lo8), f32(-np.inf))) == 7 and di._radius_of(s8, np.nextafter(f32(hi8), f32(np.inf))) == 9
    assert [di._radius_of(*p) for p in di.BILATERAL_REFUSED_PAIRS] == [9, 9, 12]


def _bilateral_conditions(img, w, h, r, svf, vti):
    sxy, rf = di.BILATERAL_RADIUS_PAIRS[r]
    out = orc.bilateral_filter_and_cutoff(img, sxy, svf, vti, rf, di.BILATERAL_MAX_DEPTH, di.corner_cutting_radius(w, h))
    valid = out != vti
    if vti == 0:
        valid &= img != 0                  # (the filter never fills a hole: centre ignored -> ignored)
    assert 0.4 < valid.mean() < 0.9        # the cutoff, the region radius and the ignored value all cut
    what = "%dx%d R=%d svf=%g ignore=%d" % (w, h, r, svf, vti)
    _both_ways(out != img, valid, what + ": output differs from input")
    _both_ways(_disc_holds(img == vti, r), valid, what + ": ignored value inside the disc")


def _image_conditions(img, w, h, vti):
    assert (img > di.BILATERAL_MAX_DEPTH).mean() > 0.05 and (img == 0).mean() > 0.04
    if vti:
        assert (img == vti).mean() > 0.03
    region = di.corner_cutting_radius(w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    cut = (xs - w // 2) ** 2 + (ys - h // 2) ** 2 > region * region
    assert 0.005 < cut.mean() < 0.2 and cut[0, 0] and cut[-1, -1] and cut[0, -1] and not cut[h // 2, w // 2]


@pytest.mark.parametrize("w,h", di.BILATERAL_SMALL_SIZES)
@pytest.mark.parametrize("vti", di.VALUES_TO_IGNORE)
def test_noisy_steps_makes_the_bilateral_filter_branch(w, h, vti):
    """Every case of test_bilateral_every_kernel (radius 0 returns its input and has an empty disc: nothing to branch on)."""
    img = di.noisy_steps(w, h, vti, di.BILATERAL_MAX_DEPTH)
    _image_conditions(img, w, h, vti)
    for r in range(1, 9):
        for svf in di.SIGMA_VALUE_FACTORS:
            _bilateral_conditions(img, w, h, r, svf, vti)


@pytest.mark.parametrize("radius,w,h", [c for c in di.BILATERAL_LARGE_CASES if c[0] > 0])
def test_noisy_steps_makes_the_bilateral_filter_branch_on_large_images(radius, w, h):
    """Every case of test_bilateral_large, 1280 x 960 included."""
    svf, vti = di.large_case(radius)
    img = di.noisy_steps(w, h, vti, di.BILATERAL_MAX_DEPTH)
    _image_conditions(img, w, h, vti)
    _bilateral_conditions(img, w, h, radius, svf, vti)


@pytest.mark.parametrize("w,h", di.FAN_SIZES)
@pytest.mark.parametrize("ds", di.DEPTH_SCALINGS)
def test_slanted_fan_makes_normals_and_radii_branch(w, h, ds):
    cam = di.fan_camera(w, h)
    d = di.slanted_fan(w, h, ds)
    assert 0.005 < (d == 0).mean() < 0.03
    e = orc.erode_depth_map(d, 0)
    tested = e != 0
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        tested &= np.roll(e, (dy, dx), (0, 1)) != 0       # (the border ring is 0 after the border copy: no wrap-around)
    kept_before = None
    for thr in di.NORMAL_THRESHOLDS_DEG:
        nd, _ = orc.compute_normals_and_drop_bad_pixels(e, *cam, thr, ds)
        assert not (nd != 0)[~tested].any()
        _both_ways(nd == 0, tested, "%dx%d ds=%g threshold %g: dropped by the angle test" % (w, h, ds, thr))
        kept = int((nd != 0).sum())
        assert kept_before is None or kept > kept_before * 1.05, (thr, kept, kept_before)   # every threshold cuts elsewhere
        kept_before = kept
    nd, _ = orc.compute_normals_and_drop_bad_pixels(e, *cam, 85.0, ds)
    m = nd != 0
    for ext, cf in di.CLAMP_PAIRS_BRANCHING:
        _, r_inf = orc.compute_point_radii_and_remove_isolated_pixels(nd, *cam, ext, float("inf"), ds)
        od, r = orc.compute_point_radii_and_remove_isolated_pixels(nd, *cam, ext, cf, ds)
        _both_ways(r != r_inf, m, "%dx%d ds=%g extension %g clamp %g: radius clamped" % (w, h, ds, ext, cf))
        _both_ways(od == 0, m, "isolated-pixel removal")
    for ext, cf in di.CLAMP_PAIRS_ONE_SIDED:                 # what the grid's comment says of them
        _, r_inf = orc.compute_point_radii_and_remove_isolated_pixels(nd, *cam, ext, float("inf"), ds)
        _, r = orc.compute_point_radii_and_remove_isolated_pixels(nd, *cam, ext, cf, ds)
        share = float((r != r_inf)[m].mean())
        assert share < MIN_SHARE or share > 1 - MIN_SHARE, (ext, cf, share)
    assert {p[0] for p in di.CLAMP_PAIRS_BRANCHING} == {1.0, 1.5, 2.5}
    assert {p[1] for p in di.CLAMP_PAIRS_BRANCHING} == {1.5, 2.0, 3.0, 5.0}
    assert len(set(di.CLAMP_PAIRS_BRANCHING + di.CLAMP_PAIRS_ONE_SIDED)) == 15
    for radius in (1, 2, 3):
        er = orc.erode_depth_map(d, radius)
        _both_ways(er == 0, d != 0, "erosion radius %d" % radius)


@pytest.mark.parametrize("w,h", di.CULL_SIZES)
@pytest.mark.parametrize("count", di.CULL_COUNTS)
def test_perturbed_others_make_the_cull_branch(count, w, h):
    s, ref, others, T = di.cull_inputs(w, h, count)
    cam = (s.fx, s.fy, s.cx, s.cy)
    valid = ref != 0
    kept_by_tol = []
    for tol in di.CULL_TOLERANCES:
        for req in di.cull_required_counts(count):
            out = orc.outlier_depth_map_fusion(ref, others, T, *cam, tol, req)
            what = "count %d tolerance %g required %d: rejected" % (count, tol, req)
            if req == 0:                            # "at least 0 agree" holds for every pixel, by definition
                assert np.array_equal(out, ref), what
            else:
                _both_ways(out == 0, valid, what)
        kept_by_tol.append(int((orc.outlier_depth_map_fusion(ref, others, T, *cam, tol, -1) != 0).sum()))
    assert all(b > 1.1 * a for a, b in zip(kept_by_tol, kept_by_tol[1:])), kept_by_tol    # every tolerance cuts elsewhere
    # the two special poses: part of the image leaves the turned neighbour, part lies behind the advanced one
    ys, xs = np.mgrid[0:h, 0:w]
    d = ref.astype(np.float64)
    X = np.stack([d * (xs - (s.cx - 0.5)) / s.fx, d * (ys - (s.cy - 0.5)) / s.fy, d], axis=-1)
    for k, kind in ((count - 2, "outside"), (count - 1, "behind")):
        M = T[k].astype(np.float64)
        o = X @ M[:, :3].T + M[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = s.fx * o[..., 0] / o[..., 2] + s.cx, s.fy * o[..., 1] / o[..., 2] + s.cy
        front = o[..., 2] > 0
        outside = front & ~((u > -1) & (v > -1) & (u < w) & (v < h))
        assert (outside & valid).sum() > 0.05 * valid.sum(), kind
        if kind == "behind":
            assert (~front & valid).sum() > 0.01 * valid.sum()
        assert (front & ~outside & valid).sum() > 0.3 * valid.sum()


@pytest.mark.parametrize("radius", list(range(0, 9)))
def test_fused_cases_branch(radius):
    """Every case of test_bilateral_with_outlier_fusion: the cutoff and the region radius remove part of the frame, and of
    what the filter leaves the cull rejects at least 5 % and keeps at least 5 %.  (Not asked here, because these room
    frames cannot give it: the filter's output equals its input for only 1 .. 5 % of the pixels once R >= 4.)"""
    sxy, rf = di.BILATERAL_RADIUS_PAIRS[radius]
    for w, h in di.fused_sizes(radius):
        for count in di.FUSED_OTHER_COUNTS:
            s, raw, others, T = di.cull_inputs(w, h, count)
            for svf, tol, req in di.fused_cases(radius, w, h, count):
                f_o = orc.bilateral_filter_and_cutoff(raw, sxy, svf, 0, rf, di.fused_max_depth(raw), di.corner_cutting_radius(w, h))
                c_o = orc.outlier_depth_map_fusion(f_o, others, T, s.fx, s.fy, s.cx, s.cy, tol, req)
                what = "%dx%d R=%d %d others svf=%g tolerance %g required %d" % (w, h, radius, count, svf, tol, req)
                _both_ways(f_o == 0, raw != 0, what + ": removed by the cutoff or the region radius")
                _both_ways(c_o == 0, f_o != 0, what + ": rejected by the cull")


def test_reference_pin_cull_cases_branch():
    s, raw, others, T = di.cull_inputs(160, 120, 8)
    for tol, req in di.PIN_CULL_CASES:
        out = orc.outlier_depth_map_fusion(raw, others, T, s.fx, s.fy, s.cx, s.cy, tol, req)
        _both_ways(out == 0, raw != 0, "reference pin, tolerance %g required %d: rejected" % (tol, req))


def test_off_default_parameter_sets_change_the_map():
    """On the oracle alone: the parameter sets of the off-default pipeline tests (test_gpu_preprocess_params.py) do not
    give the default set's map -- otherwise those tests would prove nothing -- and every float field is its own value."""
    import dataclasses
    from surfelmeshing_amd.pipeline import PreprocessParams
    pre, dflt = di.off_default_pre(), PreprocessParams()
    floats = [getattr(pre, f.name) for f in dataclasses.fields(pre) if isinstance(getattr(dflt, f.name), float)]
    assert len(floats) == 10 and len(set(floats)) == len(floats), floats
    for f in dataclasses.fields(pre):
        if f.name not in di.PIPELINE_FIELDS_NOT_VARIED:
            assert getattr(pre, f.name) != getattr(dflt, f.name), f.name
    p_def = di.oracle_pipeline_run("default")[2]
    for which in ("off", "r0"):
        po = di.oracle_pipeline_run(which)[2]
        assert po.recon.surfels_size > 1500 and (po.depth_final != 0).sum() > 1000
        assert not di.same_pipeline_result(po, p_def)
    assert not di.same_pipeline_result(di.oracle_pipeline_run("off")[2], di.oracle_pipeline_run("r0")[2])
    # the radius clamp of the first set decides both ways on these frames, the second set's never clamps
    s, pre, po = di.oracle_pipeline_run("off")
    stages = po.stages
    _, r_inf = orc.compute_point_radii_and_remove_isolated_pixels(stages["normals_depth"], s.fx, s.fy, s.cx, s.cy,
                                                                  pre.point_radius_extension_factor, float("inf"), pre.depth_scaling)
    m = stages["normals_depth"] != 0
    assert 0 < (po.radius[m] != r_inf[m]).sum() < m.sum()


def _fields_that_do_not_matter(pre, base):
    import dataclasses
    from surfelmeshing_amd.pipeline import PreprocessParams
    dflt = PreprocessParams()
    return [f.name for f in dataclasses.fields(pre) if f.name not in di.PIPELINE_FIELDS_NOT_VARIED and
            di.same_pipeline_result(base, di.oracle_pipeline_run_with(dataclasses.replace(pre, **{f.name: getattr(dflt, f.name)})))]


def test_every_off_default_field_decides_the_run():
    """A frame loop that dropped ONE field of the first parameter set (used its default instead) would not give the
    oracle's run: asserted field by field on the oracle.  Likewise for two neighbouring float fields of the native
    driver's config struct swapped.  The second set makes no such claim; what it leaves undecided is listed."""
    import dataclasses
    _, pre, base = di.oracle_pipeline_run("off")
    assert _fields_that_do_not_matter(pre, base) == []
    from surfelmeshing_amd.pipeline import DriverConfig
    import ctypes
    floats = [n for n, t in DriverConfig._fields_ if t is ctypes.c_float and hasattr(pre, n)]
    assert len(floats) == 10
    for a, b in zip(floats, floats[1:]):
        swapped = dataclasses.replace(pre, **{a: getattr(pre, b), b: getattr(pre, a)})
        assert not di.same_pipeline_result(base, di.oracle_pipeline_run_with(swapped)), (a, b)
    _, pre0, base0 = di.oracle_pipeline_run("r0")
    assert _fields_that_do_not_matter(pre0, base0) == list(di.RADIUS_0_INERT_FIELDS)


def test_max_depth_u16_is_the_float32_product():
    """APP/main.cc:1021 multiplies two floats; the native driver does the same.  4500 x 2.87 is 12914.9995 in float32 (u16 12914) and
    12915.000000000002 in float64."""
    from surfelmeshing_amd.pipeline import PreprocessParams
    assert PreprocessParams(depth_scaling=4500.0, max_depth=2.87).max_depth_u16() == 12914
    assert PreprocessParams().max_depth_u16() == 15000
    assert PreprocessParams(max_depth=10.0).max_depth_u16() == 50000
    assert PreprocessParams(max_depth=20.0).max_depth_u16() == 65535
