"""The changed-predicate of smx_recon_triangulate_update without a GPU: smx_mesh.hpp holds it as a plain inline function
(k_mesh_diff calls it), so this test compiles it for the host and checks the cases the contract names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import ROOT

SRC = os.path.join(ROOT, "surfelmeshing_amd", "csrc")

HARNESS = r'''
#define SMX_MESH_HOST_ONLY 1
#include "smx_mesh.hpp"
extern "C" int host_slot_changed(unsigned slot, unsigned n_prev, const float* now, const float* kept) {
  return smx::mesh_slot_changed(slot, n_prev, now, kept) ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_update_host")
    src = d / "mesh_update_host.cpp"
    src.write_text(HARNESS)
    lib = d / "libmesh_update_host.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", SRC,
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(str(lib))


def _changed(host, slot, n_prev, now, kept):
    now, kept = np.ascontiguousarray(now, np.float32), np.ascontiguousarray(kept, np.float32)
    assert now.shape == kept.shape == (7,)
    return bool(host.host_slot_changed(C.c_uint32(slot), C.c_uint32(n_prev), now.ctypes.data_as(C.c_void_p),
                                       kept.ctypes.data_as(C.c_void_p)))


def test_changed_predicate(host):
    base = np.array([0.25, -1.5, 3.0, 0.0004, 0.6, 0.0, 0.8], np.float32)
    assert not _changed(host, 3, 10, base, base.copy())                       # equal words
    for t in range(7):                                                        # one differing word, in every position
        other = base.copy()
        other[t] = np.nextafter(other[t], np.float32(10.0))                   # (the smallest difference there is: one bit)
        assert _changed(host, 3, 10, other, base), t
        assert _changed(host, 3, 10, base, other), t
    nan = base.copy()
    nan[1] = np.nan
    nan[3] = np.float32(np.nan)
    assert not _changed(host, 0, 1, nan, nan.copy())                          # a NaN equals the same NaN
    payload = nan.copy()
    payload.view(np.uint32)[1] ^= 1                                           # ... but not a NaN of other bits
    assert _changed(host, 0, 1, payload, nan)
    assert _changed(host, 0, 1, nan, base)
    zero, minus = base.copy(), base.copy()
    zero[5], minus[5] = 0.0, -0.0
    assert _changed(host, 0, 1, minus, zero) and not _changed(host, 0, 1, minus, minus.copy())   # -0 against +0
    assert _changed(host, 10, 10, base, base.copy()) and _changed(host, 11, 10, base, base.copy())   # i >= n_prev
    assert not _changed(host, 9, 10, base, base.copy())
    assert _changed(host, 0, 0, base, base.copy())
