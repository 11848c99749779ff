"""GPU parity of the preprocessing kernels over their parameter space, on inputs that make them decide.

Every comparison with the CPU oracle is bit-exact.  The inputs come from tests/depth_inputs.py; that each case's branch
is taken both ways is asserted on the oracle in tests/test_depth_inputs.py (non-GPU suite), and that the oracle computes
the operation it is meant to in tests/test_depth_ref.py (against float64).  Radius coverage of the bilateral filter
lives HERE: the second bilateral case of test_gpu_parity.py::test_depth_stage_edge_cases looks like other parameters
but is radius 6 again (2.0 x 3.0), like every other test outside this module.

Which case runs which bilateral kernel (launch_bilateral, csrc/smx_depth.hip; R = (int)(radius_factor * sigma_xy + 0.5f)):
  k_bilateral (generic, R = 0)  test_bilateral_every_kernel[0] (131x37, 20x200), test_bilateral_large[0-640-480];
                                with others (two launches): test_bilateral_with_outlier_fusion[0]
  k_bilateral_p<R, 0>, R = 1..8 test_bilateral_every_kernel[R] (131x37 and 20x200, every sigma_value_factor x
                                value_to_ignore), test_bilateral_large[R-640-480]; R = 1 and 8 also from the four
                                products next to the + 0.5f rounding (BILATERAL_EDGE_PAIRS) and at 1280x960
                                (test_bilateral_large[1-1280-960], [8-1280-960]: more tiles than workgroups);
                                with six others (two launches): test_bilateral_with_outlier_fusion[R]
  k_bilateral_p<R, 8>, R = 1..8 test_bilateral_with_outlier_fusion[R] (eight others: the one-launch route), 160x120 and
                                203x77; R = 1, 4, 8 also at 640x480
  R >= 9                        test_bilateral_radius_above_8_is_refused (SMX_CHECK_ARG; output untouched)
Which case takes which branch both ways (the 5 % conditions are in test_depth_inputs.py):
  bilateral: output differs / equals input, ignored value in the disc / none, over max_depth, outside the region radius
                                test_bilateral_every_kernel[1..8], test_bilateral_large     (noisy_steps)
  cull: rejected / kept, projects outside, behind the camera
                                test_outlier_cull_counts_and_tolerances[2|4|6|8], 160x120 and 203x77 (perturbed_others);
                                after the filter: test_bilateral_with_outlier_fusion (cutoff and cull both ways; the
                                filter's "equals input" side is NOT reached there, see its docstring)
  normals: dropped by the angle test / kept, for 20 .. 89 degrees
                                test_normals_thresholds_and_scalings                          (slanted_fan)
  radii: clamped / not (CLAMP_PAIRS_BRANCHING), isolated pixel removed / kept
                                test_radii_extension_and_clamp, test_fused_erode_normals_radii_parameters
  erosion 0 .. 3                test_fused_erode_normals_radii_parameters
  DriverConfig fields           test_frame_pipeline_off_its_defaults[off], test_native_driver_off_its_defaults[off-*]:
                                every field off its default, every float its own value, and each field decides the
                                oracle's run on its own (test_depth_inputs.py::test_every_off_default_field_decides_the_run);
                                the second set [r0] is there for its routes and leaves five fields undecided
                                (depth_inputs.RADIUS_0_INERT_FIELDS)
"""
import functools

import numpy as np
import pytest

import depth_inputs as di
import oracle as orc
from common import assert_surfels_match
from test_gpu_reference_pin import ref  # noqa: F401  (the fixture that loads oracle/_ref, defined there)

pytestmark = pytest.mark.gpu

MARKER = 12345


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _steps(w, h, vti):
    return di.noisy_steps(w, h, vti, di.BILATERAL_MAX_DEPTH)


def _cull_inputs(w, h, count):
    return di.cull_inputs(w, h, count)


def _run_bilateral(smx, A, B, img, sxy, svf, vti, rf, region):
    A.Upload(img)
    B.Clear(MARKER)
    smx.BilateralFilteringAndDepthCutoffCUDA(None, sxy, svf, vti, rf, di.BILATERAL_MAX_DEPTH, region, A, B)
    got = B.Download()
    exp = orc.bilateral_filter_and_cutoff(img, sxy, svf, vti, rf, di.BILATERAL_MAX_DEPTH, region)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%dx%d sigma_xy %g factor %.9g svf %g ignore %d: %d pixels differ, first (y, x) = %s: %d vs %d" % (
        img.shape[1], img.shape[0], sxy, rf, svf, vti, len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])


# ---- bilateral filter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", list(range(0, 9)))
def test_bilateral_every_kernel(smx, radius):
    """Ragged (131x37) and narrower than a tile plus halo (20x200): every sigma_value_factor x value_to_ignore, a
    max_depth that cuts a band, a region radius that cuts the corners; radii 1 and 8 also from the products next to
    the rounding boundary."""
    pairs = [di.BILATERAL_RADIUS_PAIRS[radius]] + [p for r, p in di.BILATERAL_EDGE_PAIRS if r == radius]
    for w, h in di.BILATERAL_SMALL_SIZES:
        A, B = smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.uint16)
        for vti in di.VALUES_TO_IGNORE:
            img = _steps(w, h, vti)
            for sxy, rf in pairs:
                for svf in di.SIGMA_VALUE_FACTORS:
                    _run_bilateral(smx, A, B, img, sxy, svf, vti, rf, di.corner_cutting_radius(w, h))
        # without the region cut and with max_depth at the top of the range: the band is filtered too
        img = _steps(w, h, 65535)
        A.Upload(img)
        sxy, rf = pairs[0]
        smx.BilateralFilteringAndDepthCutoffCUDA(None, sxy, 0.05, 65535, rf, 65535, 1.0e4, A, B)
        assert np.array_equal(B.Download(), orc.bilateral_filter_and_cutoff(img, sxy, 0.05, 65535, rf, 65535, 1.0e4))


@pytest.mark.parametrize("radius,w,h", di.BILATERAL_LARGE_CASES)
def test_bilateral_large(smx, radius, w, h):
    """640x480: one tile per workgroup; 1280x960: more tiles than workgroups, every workgroup walks the tile loop."""
    sxy, rf = di.BILATERAL_RADIUS_PAIRS[radius]
    svf, vti = di.large_case(radius)
    A, B = smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.uint16)
    _run_bilateral(smx, A, B, _steps(w, h, vti), sxy, svf, vti, rf, di.corner_cutting_radius(w, h))


@pytest.mark.parametrize("radius", list(range(0, 9)))
def test_bilateral_with_outlier_fusion(smx, radius):
    """BilateralFilteringAndOutlierFusionCUDA: eight others is one launch of k_bilateral_p<R, 8> (R >= 1), six others
    and R = 0 take the two launches through the scratch image; both equal the oracle's filter followed by its cull.
    Input: the room frame of cull_stream with perturbed_others.  The cutoff, the region radius and the cull decide both
    ways here (test_depth_inputs.py::test_fused_cases_branch); the filter's 'output equals input' side does not -- on
    these smooth noisy walls it is 1 .. 5 % of the pixels for R >= 4 -- so for the taps of the <R, 8> instantiations
    the evidence is the bit-equality itself on inputs that leave nearly every pixel changed, and the <R, 0> cases on
    noisy_steps, which run the same tap code."""
    sxy, rf = di.BILATERAL_RADIUS_PAIRS[radius]
    for w, h in di.fused_sizes(radius):
        for count in di.FUSED_OTHER_COUNTS:
            s, raw, others, T = _cull_inputs(w, h, count)
            cam = (s.fx, s.fy, s.cx, s.cy)
            region, max_depth = di.corner_cutting_radius(w, h), di.fused_max_depth(raw)
            IN, S, OUT = (smx.CUDABuffer(h, w, np.uint16) for _ in range(3))
            IN.Upload(raw)
            obufs = [smx.CUDABuffer(h, w, np.uint16) for _ in others]
            for b, o in zip(obufs, others):
                b.Upload(o)
            for svf, tol, req in di.fused_cases(radius, w, h, count):
                f_o = orc.bilateral_filter_and_cutoff(raw, sxy, svf, 0, rf, max_depth, region)
                c_o = orc.outlier_depth_map_fusion(f_o, others, T, *cam, tol, req)
                OUT.Clear(MARKER)
                smx.BilateralFilteringAndOutlierFusionCUDA(None, sxy, svf, rf, max_depth, region, IN, tol, *cam, obufs, T, S, OUT,
                                                           required_count=req)
                assert np.array_equal(OUT.Download(), c_o), (w, h, radius, count, svf, tol, req)
                if count != 8 or radius == 0:
                    assert np.array_equal(S.Download(), f_o), "scratch image of the two-launch route"


def test_bilateral_radius_above_8_is_refused(smx):
    """smx.h: radii 0 .. 8 are implemented, a larger one is refused (SMX_ERR_INVALID_ARGUMENT, raised as SmxError)
    before anything is launched -- alone and through the fused entry point, which leaves its scratch image alone too."""
    w, h = 131, 37
    img = _steps(w, h, 0)
    A, B, S = (smx.CUDABuffer(h, w, np.uint16) for _ in range(3))
    A.Upload(img)
    s, raw, others, T = _cull_inputs(w, h, 8)
    obufs = [smx.CUDABuffer(h, w, np.uint16) for _ in others]
    for sxy, rf in di.BILATERAL_REFUSED_PAIRS:
        B.Clear(MARKER)
        S.Clear(MARKER)
        with pytest.raises(smx.SmxError):
            smx.BilateralFilteringAndDepthCutoffCUDA(None, sxy, 0.05, 0, rf, 65535, 1.0e4, A, B)
        with pytest.raises(smx.SmxError):
            smx.BilateralFilteringAndOutlierFusionCUDA(None, sxy, 0.05, rf, 65535, 1.0e4, A, 0.02, s.fx, s.fy, s.cx, s.cy,
                                                       obufs, T, S, B)
        assert np.all(B.Download() == MARKER) and np.all(S.Download() == MARKER)
    # the last product inside the boundary is radius 8 and runs
    sxy, rf = di.BILATERAL_EDGE_PAIRS[3][1]
    smx.BilateralFilteringAndDepthCutoffCUDA(None, sxy, 0.05, 0, rf, 65535, 1.0e4, A, B)
    assert np.array_equal(B.Download(), orc.bilateral_filter_and_cutoff(img, sxy, 0.05, 0, rf, 65535, 1.0e4))


# ---- outlier cull ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", di.CULL_COUNTS)
def test_outlier_cull_counts_and_tolerances(smx, count):
    for w, h in di.CULL_SIZES:
        s, raw, others, T = _cull_inputs(w, h, count)
        cam = (s.fx, s.fy, s.cx, s.cy)
        IN, OUT = smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.uint16)
        IN.Upload(raw)
        obufs = [smx.CUDABuffer(h, w, np.uint16) for _ in others]
        for b, o in zip(obufs, others):
            b.Upload(o)
        for tol in di.CULL_TOLERANCES:
            for req in di.cull_required_counts(count):
                OUT.Clear(MARKER)
                smx.OutlierDepthMapFusionCUDA(None, tol, IN, *cam, obufs, T, OUT, required_count=req)
                exp = orc.outlier_depth_map_fusion(raw, others, T, *cam, tol, req)
                assert np.array_equal(OUT.Download(), exp), (w, h, count, tol, req)


# ---- normals, radii, the fused tail -----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", di.FAN_SIZES)
def test_normals_thresholds_and_scalings(smx, w, h):
    cam = di.fan_camera(w, h)
    A, B, N = smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.float32, 2)
    for ds in di.DEPTH_SCALINGS:
        e = orc.erode_depth_map(di.slanted_fan(w, h, ds), 0)
        A.Upload(e)
        for thr in di.NORMAL_THRESHOLDS_DEG:
            B.Clear(MARKER)
            smx.ComputeNormalsAndDropBadPixelsCUDA(None, thr, ds, *cam, A, B, N)
            od, on = orc.compute_normals_and_drop_bad_pixels(e, *cam, thr, ds)
            assert np.array_equal(B.Download(), od), (w, h, ds, thr)
            assert np.array_equal(_bits(N.Download()), _bits(on)), (w, h, ds, thr)


@pytest.mark.parametrize("w,h", di.FAN_SIZES)
def test_radii_extension_and_clamp(smx, w, h):
    cam = di.fan_camera(w, h)
    A, B, R = smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.float32)
    marker = np.full((h, w), -7.0, np.float32)
    for ds in di.DEPTH_SCALINGS:
        e = orc.erode_depth_map(di.slanted_fan(w, h, ds), 0)
        nd, _ = orc.compute_normals_and_drop_bad_pixels(e, *cam, 85.0, ds)
        A.Upload(nd)
        for ext, cf in di.CLAMP_PAIRS_BRANCHING + di.CLAMP_PAIRS_ONE_SIDED:
            R.Clear(-7.0)
            smx.ComputePointRadiiAndRemoveIsolatedPixelsCUDA(None, ext, cf, ds, *cam, A, R, B)
            od, orad = orc.compute_point_radii_and_remove_isolated_pixels(nd, *cam, ext, cf, ds, radius_init=marker)
            assert np.array_equal(B.Download(), od), (w, h, ds, ext, cf)
            assert np.array_equal(_bits(R.Download()), _bits(orad)), (w, h, ds, ext, cf)      # marker kept where depth is 0


def _fused_cases(full):
    """threshold x erosion radius (all 24 pairs twice on the small image, 12 of them once at 640 x 480), with
    (extension, clamp) and depth_scaling walking through all their values meanwhile."""
    pairs = di.CLAMP_PAIRS_BRANCHING + di.CLAMP_PAIRS_ONE_SIDED
    cases, k = [], 0
    for i, thr in enumerate(di.NORMAL_THRESHOLDS_DEG):
        for radius in ((0, 1, 2, 3) if full else (i % 4, (i + 2) % 4)):
            for _ in range(2 if full else 1):
                ext, cf = pairs[(4 * k) % len(pairs)]                    # (4 and 15 are coprime: all pairs in turn)
                cases.append((radius, thr, ext, cf, di.DEPTH_SCALINGS[(k + k // 2) % 2]))
                k += 1
    return cases


@pytest.mark.parametrize("w,h", di.FAN_SIZES)
def test_fused_erode_normals_radii_parameters(smx, w, h):
    """ErodeNormalsRadiiCUDA equals the oracle's three stages off the defaults: final depth, normals, and the radius
    buffer including the marker it must leave where the depth is dropped."""
    cam = di.fan_camera(w, h)
    A, B = smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.uint16)
    N, R = smx.CUDABuffer(h, w, np.float32, 2), smx.CUDABuffer(h, w, np.float32)
    marker = np.full((h, w), -7.0, np.float32)
    cases = _fused_cases(full=(w, h) != (640, 480))
    assert {c[0] for c in cases} == {0, 1, 2, 3} and {c[1] for c in cases} == set(di.NORMAL_THRESHOLDS_DEG)
    assert {c[3] for c in cases} >= {1.5, 2.0, 3.0, 5.0, float("inf")} and {c[4] for c in cases} == set(di.DEPTH_SCALINGS)
    fans = {ds: di.slanted_fan(w, h, ds) for ds in di.DEPTH_SCALINGS}
    for radius, thr, ext, cf, ds in cases:
        A.Upload(fans[ds])
        R.Clear(-7.0)
        smx.ErodeNormalsRadiiCUDA(None, radius, thr, ext, cf, ds, *cam, A, B, N, R)
        oe = orc.erode_depth_map(fans[ds], radius)
        on_d, on = orc.compute_normals_and_drop_bad_pixels(oe, *cam, thr, ds)
        or_d, orad = orc.compute_point_radii_and_remove_isolated_pixels(on_d, *cam, ext, cf, ds, radius_init=marker)
        what = (w, h, radius, thr, ext, cf, ds)
        assert np.array_equal(B.Download(), or_d), what
        assert np.array_equal(_bits(N.Download()), _bits(on)), what
        assert np.array_equal(_bits(R.Download()), _bits(orad)), what


# ---- whole pipelines off their defaults -----------------------------------------------------------------------------------
FRAMES = di.PIPELINE_FRAMES


def _oracle_run(which):
    """(stream, PreprocessParams, OraclePipeline after FRAMES) of a parameter set of depth_inputs.PIPELINE_PARAMETER_SETS;
    first the condition that makes the comparison worth anything: this set's map is not the default set's."""
    s, pre, po = di.oracle_pipeline_run(which)
    dflt = di.oracle_pipeline_run("default")[2]
    assert po.recon.surfels_size != dflt.recon.surfels_size and not np.array_equal(po.depth_final, dflt.depth_final)
    return s, pre, po


@pytest.mark.parametrize("which", ["off", "r0"])
def test_frame_pipeline_off_its_defaults(smx, which):
    from surfelmeshing_amd.pipeline import FramePipeline
    s, pre, po = _oracle_run(which)
    pg = FramePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, pre)
    for f in range(0, 20):
        pg.upload(f, *s.frame(f))
    n_o = pre.outlier_filtering_frame_count
    for f in FRAMES:
        pg.process(f, s.outlier_frames(f, n_o), s.others_TR_reference(f, n_o), s.pose(f))
    n = po.recon.surfels_size
    assert pg.reconstruction.surfels_size() == n
    assert_surfels_match(pg.reconstruction.debug_download_surfels(n), po.recon.surfels(), n)
    assert np.array_equal(pg.depth_final.Download(), po.depth_final)
    assert np.array_equal(_bits(pg.normals.Download()), _bits(po.normals))
    m = po.depth_final != 0
    assert np.array_equal(_bits(pg.radius.Download())[m], _bits(po.radius)[m])


@pytest.mark.parametrize("which,run_ahead,fused_head,fused_tail,split_pre", [
    ("off", False, False, False, False), ("off", True, False, False, False), ("off", False, True, True, False),
    ("off", False, False, False, True), ("r0", False, True, True, False)])
def test_native_driver_off_its_defaults(smx, which, run_ahead, fused_head, fused_tail, split_pre):
    """The C++ frame loop receives the preprocessing parameters through DriverConfig (pipeline.py) <-> smx_driver_config
    (smx_driver.h), mirrored by hand."""
    from surfelmeshing_amd.pipeline import NativeFramePipeline
    from surfelmeshing_amd._lib import IntegrateParams
    s, pre, po = _oracle_run(which)
    pn = NativeFramePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, pre, IntegrateParams.defaults())
    pn.set_run_ahead(run_ahead)
    pn.set_fused_head(fused_head)
    pn.set_fused_tail(fused_tail)
    pn.set_split_preprocessing(split_pre)
    for f in range(0, 20):
        pn.upload(f, *s.frame(f))
    n_o = pre.outlier_filtering_frame_count
    pn.run([pn.make_step(f, s.outlier_frames(f, n_o), s.others_TR_reference(f, n_o), s.pose(f)) for f in FRAMES])
    n = po.recon.surfels_size
    assert pn.reconstruction.surfels_size() == n
    assert_surfels_match(pn.reconstruction.debug_download_surfels(n), po.recon.surfels(), n)
    d, nrm, rad = pn.download_work()
    assert np.array_equal(d, po.depth_final)
    assert np.array_equal(_bits(nrm), _bits(po.normals))
    m = po.depth_final != 0
    assert np.array_equal(_bits(rad)[m], _bits(po.radius)[m])


# ---- the reference's own kernels off the defaults ----------------------------------------------------------------------
def test_depth_kernels_match_the_reference_off_the_defaults(ref):  # noqa: F811
    """test_gpu_reference_pin.py::test_depth_kernels_match_the_reference at other parameters, on the branching inputs.
    The bilateral criterion is that file's: at most 1 unit, same zero mask, at most max(3, size / 2000) pixels differ
    (the reference is built with fast-math, so no bit parity is defined for the exponential); everything else bit-equal."""
    for w, h in ((131, 37), (160, 120)):
        img = _steps(w, h, 0)
        for radius in (1, 4, 8):
            sxy, rf = di.BILATERAL_RADIUS_PAIRS[radius]
            for svf in (0.05, 0.5):
                args = (sxy, svf, 0, rf, di.BILATERAL_MAX_DEPTH, di.corner_cutting_radius(w, h))
                a_o, a_r = orc.bilateral_filter_and_cutoff(img, *args), ref.bilateral_filter_and_cutoff(img, *args)
                diff = a_o.astype(np.int32) - a_r.astype(np.int32)
                print("[reference pin] bilateral %dx%d R=%d svf=%g: %d of %d pixels differ, largest %d" % (
                    w, h, radius, svf, np.count_nonzero(diff), diff.size, np.abs(diff).max()))
                assert np.abs(diff).max() <= 1 and np.count_nonzero(diff) <= max(3, a_o.size // 2000), (
                    radius, svf, np.count_nonzero(diff), int(np.abs(diff).max()))
                assert np.array_equal(a_o == 0, a_r == 0)
    s, raw, others, T = _cull_inputs(160, 120, 8)
    cam = (s.fx, s.fy, s.cx, s.cy)
    for tol, req in di.PIN_CULL_CASES:                     # (both ways: test_depth_inputs.py::test_fused_cases_branch)
        b_o = orc.outlier_depth_map_fusion(raw, others, T, *cam, tol, req)
        b_r = ref.outlier_depth_map_fusion(raw, others, T, *cam, tol, req)
        assert np.array_equal(b_o, b_r), (tol, req)
    w, h = di.FAN_SIZES[0]
    cam = di.fan_camera(w, h)
    for ds in di.DEPTH_SCALINGS:
        e = orc.erode_depth_map(di.slanted_fan(w, h, ds), 0)
        for thr in (45.0, 75.0):
            n_od, n_on = orc.compute_normals_and_drop_bad_pixels(e, *cam, thr, ds)
            n_rd, n_rn = ref.compute_normals_and_drop_bad_pixels(e, *cam, thr, ds)
            assert np.array_equal(n_od, n_rd) and (n_od != 0).sum() > 500, (ds, thr)
            m = n_od != 0
            assert np.array_equal(_bits(n_on[m]), _bits(n_rn[m])), (ds, thr)
            for ext, cf in ((1.5, 2.0), (2.5, 5.0)):
                r_od, r_or = orc.compute_point_radii_and_remove_isolated_pixels(n_od, *cam, ext, cf, ds)
                r_rd, r_rr = ref.compute_point_radii_and_remove_isolated_pixels(n_od, *cam, ext, cf, ds)
                assert np.array_equal(r_od, r_rd), (ds, thr, ext, cf)
                m = r_od != 0
                assert m.sum() > 300 and np.array_equal(_bits(r_or[m]), _bits(r_rr[m])), (ds, thr, ext, cf)
