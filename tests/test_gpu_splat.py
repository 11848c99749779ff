"""smx_recon_render on the GPU against the exact model of tests/splat_ref.py, bit for bit: the hand-built maps of
tests/splat_cases.py (uploaded with debug_upload_surfels) with every parameter set, and the model images of a tracking call.
No tolerance and no excused pixel: the kernels' geometry is correctly rounded double arithmetic without contraction, which
numpy reproduces (tests/test_splat_kernel_host.py shows the same equality for the kernels' own functions on the host).  The
grown maps of tests/test_gpu_render.py are held to the same equality there, beside the float64 comparison."""
import numpy as np
import pytest

import splat_cases as sc
import splat_ref as sp

pytestmark = pytest.mark.gpu

CASES = {name: (rows, n, view) for name, rows, n, view, _ in sc.cases()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def assert_images_equal(got, want, what):
    for k in sp.IMAGES:
        g, w = bits(got[k]).reshape(bits(want[k]).shape), bits(want[k])
        assert np.array_equal(g, w), (what, k, int((g != w).sum()), np.argwhere(g != w)[:5])


def _uploaded(smx, rows, view):
    rec = smx.CUDASurfelReconstruction(1000, smx.PinholeCamera4f(view["width"], view["height"], view["fx"], view["fy"], view["cx"], view["cy"]))
    rec.debug_upload_surfels(rows)
    return rec


@pytest.mark.parametrize("case", list(CASES))
def test_cases_equal_the_model_bit_for_bit(smx, case):
    from surfelmeshing_amd import render
    rows, n, view = CASES[case]
    rec = _uploaded(smx, rows, view)
    try:
        for pname, p in sc.PARAMS.items():
            kw = dict(view, **p)
            args, opts = sc.api_params(kw)
            got = render.render_view(rec, *args, color=opts.pop("color_flags"), **opts)
            assert_images_equal(got, sp.render(rows, n, **kw), "%s / %s" % (case, pname))
    finally:
        rec.close()


@pytest.mark.parametrize("case", ["cloud 70x37", "ties 70x37", "disc_extent 33x17"])
def test_the_trackers_model_images_equal_the_model(smx, case):
    """What smx_recon_track reads: its model depth and normal images, rendered at its own parameters (near_z 0.05, far_z 20,
    factor 1, extent 16), against the model.  (tests/test_gpu_track.py::test_model_images_are_the_renders ties them to the render.)"""
    from surfelmeshing_amd._lib import TrackParams
    rows, n, view = CASES[case]
    w, h = view["width"], view["height"]
    rec = _uploaded(smx, rows, view)
    try:
        depth = smx.CUDABuffer(h, w, np.uint16)
        depth.Clear(10000)                                             # a wall 2 m in front of the camera
        normals = smx.CUDABuffer(h, w, np.float32, 2)
        normals.Clear(0.0)
        md, mn = smx.CUDABuffer(h, w, np.float32), smx.CUDABuffer(h, w, np.float32, 4)
        p = TrackParams.defaults()
        assert (p.near_z, p.far_z, p.disc_radius_factor, p.max_splat_extent_in_pixels) == (np.float32(0.05), 20.0, 1.0, 16.0)
        rec.Track(None, 5000.0, depth, normals, view["global_T_camera"], p, md, mn)
        want = sp.render(rows, n, **dict(view, **sc.PARAMS["disc tracker"]))
        assert (want["index"] != sp.INVALID).sum() > 20
        D, M = md.Download(), mn.Download().reshape(h, w, 4)
        assert np.array_equal(bits(D), bits(want["depth"])), np.argwhere(bits(D) != bits(want["depth"]))[:5]
        assert np.array_equal(bits(M), bits(want["normal"]))
    finally:
        rec.close()
