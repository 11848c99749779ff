"""smx_recon_track and smx_recon_track_rgbd on the GPU against the exact model of tests/track_exact.py, bit for bit, on the
hand-built cases of tests/track_cases.py: the maps uploaded with debug_upload_surfels, the frames uploaded directly.  Every
case at every stride of {1, 2, 4, 8}, both calls: the model images must be the exact splat model's and the restatement's P,
both records of a (stride, 1), (stride, 1) schedule must carry the exact model's sums as float64 bits -- all 31 or all 33, no
pixel excused, no bound -- the twist must follow from the device's own sums by the restatement's solve (rtol 1e-9: double sin
is not specified to the bit) and the returned result must be, field by field, what tests/track_exact.py::exact_call derives
from the records.  Then the decisions at the end of a call, the clamped grid, and calls of both kinds alternating on one
object.  tests/test_track_cases.py holds the header's functions to the same model on the CPU."""
import numpy as np
import pytest

import track_cases as tc
import track_exact as tx
import track_ref as tr
from test_track_cases import _bits, check_call
from track_host import result_fields

pytestmark = pytest.mark.gpu


def _object(smx, c):
    rec = smx.CUDASurfelReconstruction(c.rows.shape[1] + 1000, smx.PinholeCamera4f(c.width, c.height, c.fx, c.fy, c.cx, c.cy))
    rec.debug_upload_surfels(c.rows)
    return rec


class Frame:
    def __init__(self, smx, c):
        h, w = c.height, c.width
        self.depth, self.normals = smx.CUDABuffer(h, w, np.uint16), smx.CUDABuffer(h, w, np.float32, 2)
        self.color = smx.CUDABuffer(h, w, np.uint8, 3)
        self.depth.Upload(c.depth)
        self.normals.Upload(c.normals)
        self.color.Upload(c.color)
        self.md, self.mn = smx.CUDABuffer(h, w, np.float32), smx.CUDABuffer(h, w, np.float32, 4)
        self.mp = smx.CUDABuffer(h, w, np.float32, 4)


def _lib_params(p, rgbd):
    from surfelmeshing_amd._lib import TrackParams, TrackRGBDParams
    kw = dict(levels=p.levels, max_distance=p.max_distance, max_normal_angle_deg=p.max_normal_angle_deg,
              convergence_rotation=p.convergence_rotation, convergence_translation=p.convergence_translation,
              min_inliers=p.min_inliers, min_inlier_fraction=p.min_inlier_fraction, min_pivot_ratio=p.min_pivot_ratio,
              near_z=p.near_z, far_z=p.far_z, disc_radius_factor=p.disc_radius_factor,
              max_splat_extent_in_pixels=p.max_splat_extent_in_pixels)
    if not rgbd:
        return TrackParams.defaults(**kw)
    return TrackRGBDParams.defaults(photometric_weight=p.photometric_weight, max_intensity_difference=p.max_intensity_difference,
                                    min_gradient=p.min_gradient, gradient_max_relative_depth_step=p.gradient_max_relative_depth_step,
                                    **kw)


def _call(rec, f, c, p, rgbd, depth_scaling=None, images=True):
    """(records, result fields) of one call."""
    ds = depth_scaling or c.depth_scaling
    if rgbd:
        out = rec.TrackRGBD(None, ds, f.depth, f.normals, f.color, c.pred, _lib_params(p, True), f.md if images else None,
                            f.mn if images else None, f.mp if images else None)
        return rec.debug_track_rgbd_iterations(), result_fields(out)
    out = rec.Track(None, ds, f.depth, f.normals, c.pred, _lib_params(p, False), f.md if images else None, f.mn if images else None)
    return rec.debug_track_iterations(), result_fields(out)


def _assert_model_images(f, c, rgbd):
    D, M, Cm, P = c.model()
    assert np.array_equal(f.md.Download().view(np.uint32), D.view(np.uint32))
    assert np.array_equal(f.mn.Download().reshape(M.shape).view(np.uint32), M.view(np.uint32))
    if rgbd:
        assert np.array_equal(f.mp.Download().reshape(P.shape).view(np.uint32), P.view(np.uint32))


# ---- the sums, x and the result ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.NAMES)
def test_both_records_carry_the_exact_models_bits(smx, name):
    c = tc.by_name(name)
    rec, f = _object(smx, c), Frame(smx, c)
    compared = 0
    for stride in tc.STRIDES:
        for rgbd in (False, True):
            p = c.params([(stride, 1), (stride, 1)])
            records, result = _call(rec, f, c, p, rgbd)
            _assert_model_images(f, c, rgbd)
            want = check_call(c, p, records, result, rgbd, (name, stride, rgbd))
            assert len(records[0]["sums"]) == (33 if rgbd else 31) and np.array_equal(want["records"][0]["Tf"], tr.IDENTITY.astype(np.float32))
            compared += sum(len(r["sums"]) for r in records)
            if tx.samples(c.width, stride) * tx.samples(c.height, stride) == 0:
                assert np.all(records[0]["sums"] == 0) and result["status"] == tr.TOO_FEW_INLIERS and len(records) == 1
    print("%s: %d sums compared as float64 bits, all equal" % (name, compared))
    rec.close()


def test_the_clamped_grid_and_the_ninth_visit(smx):
    """1026 x 512 over about 20 000 generated discs: 525 312 samples at stride 1 (257 workgroups clamped to 256, a ninth
    visit), 65 workgroups at stride 2.  One iteration per stride, without and with colour."""
    c = tc.clamp_case()
    rec, f = _object(smx, c), Frame(smx, c)
    D, M, Cm, P = c.model()
    for stride in tc.STRIDES:
        for rgbd in (False, True):
            p = c.params([(stride, 1)])
            records, result = _call(rec, f, c, p, rgbd)
            if stride == 1:
                _assert_model_images(f, c, rgbd)
            want, _ = tx.exact_sums(D, M, c.depth, c.normals, c.intrinsics, tr.IDENTITY, stride, p.gates(), c.depth_scaling,
                                    (P, c.color, p) if rgbd else None)
            assert len(records) == 1 and records[0]["status"] in (tr.OK, tr.CONVERGED)
            assert np.array_equal(_bits(records[0]["sums"]), _bits(want)), (stride, rgbd)
    assert tx.grid_of(525312) == 256 and tx.grid_of(131328) == 65
    rec.close()


# ---- the end of a call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgbd", [False, True], ids=["plain", "rgbd"])
def test_the_decisions_at_the_end_of_a_call(smx, rgbd):
    """min_inlier_fraction just above the last iteration's ratio (TOO_FEW_INLIERS, the pose before the last update to the
    bit) and just below (untouched); a first level that converges early (the rest of it skipped, the next level run, its OK
    the final status); a float product that overflows (NOT_FINITE, the prediction to the bit, x = 0); a 32 + 32 + 32 schedule
    that fills the ring (96 records)."""
    c = tc.by_name("corner right 70x37")
    rec, f = _object(smx, c), Frame(smx, c)
    for name, kw, ds, exact, expect in tc.end_of_call_variants(c, rgbd):
        p = c.params(**kw)
        records, result = _call(rec, f, c, p, rgbd, ds, images=False)
        print(name, [(q["level"], q["status"]) for q in records][:12], result["status"])
        want = check_call(c, p, records, result, rgbd, name, depth_scaling=ds) if exact else None
        expect(records, result, want)
    rec.close()


# ---- alternating calls ---------------------------------------------------------------------------------------------------
def test_alternating_calls_never_read_the_other_calls_slabs(smx):
    """rgbd, plain, rgbd on one object (slabs 40 doubles apart, then 32, then 40; two workgroups at stride 1): every call's
    records equal those of the same call on a fresh object."""
    c = tc.by_name("corner right 70x37")
    rec, f = _object(smx, c), Frame(smx, c)
    p = c.params([(1, 2), (2, 1)])
    for rgbd in (True, False, True):
        got, res = _call(rec, f, c, p, rgbd, images=False)
        fresh = _object(smx, c)
        want, wres = _call(fresh, f, c, p, rgbd, images=False)
        fresh.close()
        assert len(got) == len(want) == 3
        for a, b in zip(got, want):
            assert (a["level"], a["stride"], a["status"]) == (b["level"], b["stride"], b["status"])
            assert np.array_equal(_bits(a["sums"]), _bits(b["sums"])) and np.array_equal(_bits(a["x"]), _bits(b["x"]))
        assert np.array_equal(res["global_T_frame"].view(np.uint32), wres["global_T_frame"].view(np.uint32))
        check_call(c, p, got, res, rgbd, ("alternating", rgbd))
    rec.close()
