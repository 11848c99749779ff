"""The oracle's three input-side image functions against the REFERENCE's own function text:
MedianFilterAndDensifyDepthMap (APP/main.cc:207-252), Image<T>::DownscaleUsingMedianWhileExcluding (VIS/image.h:1003-1053)
and Image<Vec3u8>::DownscaleToHalfSize (VIS/image.h:929-948, the colour pyramid's step).  Bit-exact on random, sparse,
ragged and degenerate images.

The reference's outputs on these images are recorded in tests/golden/ref_image_fns.npz (tests/golden/make_ref_image_golden.py,
from oracle/_ref/libsmx_ref_image.so, which oracle/ref_build.py compiles from the reference's text where the reference
sources are at hand).  The oracle is always compared with the recording; where the library is built, the library is also
run on the recorded inputs and must reproduce the recording."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from common import ROOT

SO = os.path.join(ROOT, "oracle", "_ref", "libsmx_ref_image.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_image_fns.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def ref():
    """The reference's functions, or None where oracle/_ref/libsmx_ref_image.so is not built."""
    return RefImageFns(SO) if os.path.exists(SO) else None


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class RefImageFns:
    def __init__(self, path):
        self.lib = C.CDLL(path)

    def median_filter_and_densify(self, d):
        out = np.empty_like(d)
        self.lib.ref_median_filter_and_densify(C.c_int(d.shape[1]), C.c_int(d.shape[0]), _p(d), _p(out))
        return out

    def downscale_using_median_while_excluding(self, d, ow, oh, ignore):
        out = np.empty((oh, ow), np.uint16)
        self.lib.ref_downscale_using_median_while_excluding(C.c_uint16(ignore), C.c_int(d.shape[1]), C.c_int(d.shape[0]),
                                                            _p(d), C.c_int(ow), C.c_int(oh), _p(out))
        return out

    def downscale_to_half_size_rgb(self, c):
        c = np.ascontiguousarray(c)
        out = np.empty((c.shape[0] // 2, c.shape[1] // 2, 3), np.uint8)
        self.lib.ref_downscale_to_half_size_rgb(C.c_int(c.shape[1]), C.c_int(c.shape[0]), _p(c), _p(out))
        return out


def _depth_images(rng):
    for (h, w, p_zero) in ((48, 64, 0.0), (48, 64, 0.3), (37, 53, 0.7), (5, 3, 0.5), (1, 9, 0.2), (2, 2, 0.0), (60, 80, 0.97)):
        d = rng.integers(300, 9000, (h, w)).astype(np.uint16)
        d[rng.random((h, w)) < p_zero] = 0
        yield d
    flat = np.full((20, 30), 1234, np.uint16)      # ties everywhere: the even-count branch picks by distance to the average
    flat[::3, ::2] = 1236
    yield flat
    yield np.zeros((8, 8), np.uint16)


def _downscale_sizes(h, w):
    return ((max(1, h // 2), max(1, w // 2)), (max(1, h // 3), max(1, w // 4)), (h, w), (1, 1))


def _color_images(rng):
    for (h, w) in ((48, 64), (16, 8), (2, 2), (120, 160)):
        c = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        c[: h // 4] = 255                                   # 4 x 63 = 252: the truncating quarters never reach 255
        yield c


def record(ref):
    """The recording: every input image and the reference's outputs on it (tests/golden/make_ref_image_golden.py)."""
    g = {}
    for i, d in enumerate(_depth_images(np.random.default_rng(5))):
        once = ref.median_filter_and_densify(d)
        g["median_%d_in" % i], g["median_%d_once" % i] = d, once
        g["median_%d_twice" % i] = ref.median_filter_and_densify(once)   # (APP/main.cc:929-939 applies it several times)
    for i, d in enumerate(_depth_images(np.random.default_rng(6))):
        g["down_%d_in" % i] = d
        for (oh, ow) in _downscale_sizes(*d.shape):
            for ignore in (0, 1234):
                g["down_%d_%dx%d_%d" % (i, oh, ow, ignore)] = ref.downscale_using_median_while_excluding(d, ow, oh, ignore)
    for i, c in enumerate(_color_images(np.random.default_rng(7))):
        g["pyr_%d_in" % i] = c
        level, cur = 0, c
        while cur.shape[0] % 2 == 0 and cur.shape[1] % 2 == 0 and level < 3:
            level, cur = level + 1, ref.downscale_to_half_size_rgb(cur)
            g["pyr_%d_%d" % (i, level)] = cur
    return g


def _cases(golden, prefix):
    return sorted(int(k.split("_")[1]) for k in golden if k.startswith(prefix) and k.endswith("_in"))


def test_the_recording_is_what_the_reference_computes(golden, ref):
    assert len(golden) > 100
    if ref is not None:    # (where the reference's text was compiled: the recording must still be its output)
        now = record(ref)
        assert set(now) == set(golden)
        for k, v in golden.items():
            assert np.array_equal(now[k], v), k


def test_median_filter_and_densify_matches_the_reference_text(golden):
    cases = _cases(golden, "median_")
    assert len(cases) == 9
    for i in cases:
        d = golden["median_%d_in" % i]
        assert np.array_equal(orc.median_filter_and_densify(d, 1), golden["median_%d_once" % i]), d.shape
        assert np.array_equal(orc.median_filter_and_densify(d, 2), golden["median_%d_twice" % i]), d.shape


def test_downscale_using_median_matches_the_reference_text(golden):
    cases = _cases(golden, "down_")
    assert len(cases) == 9
    for i in cases:
        d = golden["down_%d_in" % i]
        for (oh, ow) in _downscale_sizes(*d.shape):
            for ignore in (0, 1234):
                mine = orc.downscale_using_median_while_excluding(d, ow, oh, ignore)
                assert np.array_equal(mine, golden["down_%d_%dx%d_%d" % (i, oh, ow, ignore)]), (d.shape, oh, ow, ignore)


def test_color_pyramid_matches_the_reference_text(golden):
    cases = _cases(golden, "pyr_")
    assert len(cases) == 4
    for i in cases:
        c = golden["pyr_%d_in" % i]
        levels = sorted(int(k.rsplit("_", 1)[1]) for k in golden if k.startswith("pyr_%d_" % i) and not k.endswith("_in"))
        assert levels == list(range(1, len(levels) + 1)) and levels, (i, levels)
        for level in levels:
            assert np.array_equal(orc.color_image_pyramid(c, level), golden["pyr_%d_%d" % (i, level)]), (c.shape, level)
