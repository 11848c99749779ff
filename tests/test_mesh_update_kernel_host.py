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
// the two functions of the coarse filter in front of the reverse test; cells[3 i ..] stay as they were where ok[i] is 0
extern "C" void host_coarse_cells(int m, const float* xyz, float inv_h, int* ok, int* cells) {
  for (int i = 0; i < m; ++i)
    ok[i] = smx::mesh_coarse_cell(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], inv_h, cells + 3 * i, cells + 3 * i + 1, cells + 3 * i + 2) ? 1 : 0;
}
extern "C" void host_coarse_bits(int m, const int* cells, unsigned* bits) {
  for (int i = 0; i < m; ++i) bits[i] = smx::mesh_coarse_bit(cells[3 * i], cells[3 * i + 1], cells[3 * i + 2]);
}
extern "C" int host_near_bits_log2() { return smx::kMeshNearBitsLog2; }
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


# ---- the coarse filter's two functions against their numpy restatement in tests/mesh_update_ref.py, bit for bit ----
def _host_cells(host, xyz, inv_h):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    m = xyz.shape[0]
    ok, cells = np.zeros(m, np.int32), np.zeros((m, 3), np.int32)
    host.host_coarse_cells(m, xyz.ctypes.data_as(C.c_void_p), C.c_float(inv_h), ok.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p))
    return ok.astype(bool), cells


def _host_bits(host, cells):
    cells = np.ascontiguousarray(cells, np.int32).reshape(-1, 3)
    bits = np.zeros(cells.shape[0], np.uint32)
    host.host_coarse_bits(cells.shape[0], cells.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p))
    return bits


def _assert_cells_equal(host, xyz, cell):
    import mesh_update_ref as mu
    inv_h = np.float32(1.0) / np.float32(cell)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok_h, cells_h = _host_cells(host, xyz, inv_h)
    ok_m, cells_m = mu.coarse_cell(xyz[:, 0], xyz[:, 1], xyz[:, 2], inv_h)
    assert np.array_equal(ok_h, ok_m)
    assert np.array_equal(cells_h[ok_h], cells_m[ok_m]) and cells_m.dtype == np.int32
    assert np.array_equal(_host_bits(host, cells_h[ok_h]), mu.coarse_bit(*cells_m[ok_m].T))
    return ok_m, cells_m


def test_coarse_cell_and_bit_on_the_cases_coordinates(host):
    import mesh_update_cases as uc
    import mesh_update_ref as mu
    assert host.host_near_bits_log2() == mu.NEAR_BITS_LOG2
    negative = 0
    for ch in uc.chains():
        for s in ch.steps:
            for cell in (s.cell, uc.H_UNFILTERED.get(ch.name, s.cell)):
                ok, cells = _assert_cells_equal(host, s.map[0], cell)
                negative += int((cells[ok] < 0).any(axis=1).sum())
    assert negative > 500          # (where floorf and a truncation differ)
    # chain N: the far slot has no cell, its neighbour half a unit nearer has the last one
    ch = uc.chain("N")
    ok, cells = _assert_cells_equal(host, ch.steps[0].map[0], ch.cell)
    assert not ok[ch.roles["far_q"]] and ok[ch.roles["far_p"]] and cells[ch.roles["far_p"]][0] == 2 ** 20 - 1


def test_coarse_cell_and_bit_on_random_cells_the_limit_and_nan(host):
    import mesh_update_ref as mu
    rng = np.random.default_rng(20)
    cells = np.concatenate([rng.integers(-2 ** 20, 2 ** 20, (8000, 3)), rng.integers(-40, 40, (2000, 3))]).astype(np.int32)
    assert cells.shape[0] == 10000 and (cells < 0).any(axis=1).sum() > 5000
    assert np.array_equal(_host_bits(host, cells), mu.coarse_bit(*cells.T))
    bits = mu.coarse_bit(*cells.T)
    assert bits.dtype == np.uint32 and bits.max() < 2 ** mu.NEAR_BITS_LOG2 and np.unique(bits).size > 9900
    # coordinates inside those cells, for the cells used in the chains (2.5, 2, 0.5, 0.05) and the default
    for cell in (2.5, 2.0, 0.5, 0.05):
        xyz = (cells.astype(np.float64) + rng.uniform(0.0, 1.0, cells.shape)) * cell
        _assert_cells_equal(host, xyz, cell)
    # the limit: |x / h| < 2^20 has a cell, 2^20 and beyond, the infinities and NaN have none (on any axis)
    lim = 2.0 ** 20
    below = np.nextafter(np.float32(lim), np.float32(0.0))
    for axis in range(3):
        for v, want in ((below, True), (-below, True), (lim, False), (-lim, False), (np.nextafter(np.float32(lim), np.float32(np.inf)), False),
                        (3.0e38, False), (np.inf, False), (-np.inf, False), (np.nan, False)):
            p = np.array([[1.5, -2.5, 3.5]], np.float32)
            p[0, axis] = v
            ok, cells1 = _assert_cells_equal(host, p, 1.0)
            assert bool(ok[0]) == want, (axis, v)
            if want:
                assert cells1[0, axis] == (2 ** 20 - 1 if v > 0 else -2 ** 20) and cells1[0, (axis + 1) % 3] == [1, -3, 3][(axis + 1) % 3]
    # floorf, not a truncation: -0.5 lies in cell -1, -0.0 in cell 0
    ok, c = _assert_cells_equal(host, [[-0.5, -0.0, -1.0]], 1.0)
    assert ok[0] and c[0].tolist() == [-1, 0, -1]
