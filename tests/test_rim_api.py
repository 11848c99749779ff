"""smx_recon_mesh_rim without a GPU: the symbol is declared, exported and loadable; header and ctypes mirror agree on
smx_rim_stats; the refusals that need no device come before anything is launched; the shim's MeshRim builds with the plain
host compiler under -Wall -Werror; the Python wrapper refuses what it can before it reaches the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rim_ref as rf
from common import ROOT

STAT_FIELDS = rf.STAT_NAMES


def test_symbol_source_and_header():
    from surfelmeshing_amd import _lib, build, meshing
    assert "smx_recon_mesh_rim" in _lib.EXPORTS and "smx_rim.hip" in build.SOURCES
    for f in ("smx_rim.hip", "smx_rim.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))
    L = _lib.load()
    assert L.smx_recon_mesh_rim is not None
    assert tuple(n for n, _ in _lib.RimStats._fields_) == STAT_FIELDS == meshing.RIM_STAT_NAMES
    assert meshing.RIM_REGIONS == ("A", "B", "AB", "C", "AC", "BC")


def test_struct_matches_the_header(tmp_path):
    from surfelmeshing_amd._lib import RimStats
    src = tmp_path / "rim_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx.h"\n'
                   'typedef int (*rim_fn)(smx_recon, smx_stream, const uint32_t*, uint32_t, int32_t, uint8_t*, smx_rim_stats*);\n'
                   'int main(void) { rim_fn f = &smx_recon_mesh_rim; (void)f;\n'
                   '  printf("%zu", sizeof(smx_rim_stats));\n' +
                   "".join('  printf(" %%zu", offsetof(smx_rim_stats, %s));\n' % f for f in STAT_FIELDS) +
                   '  return 0; }\n')
    exe = tmp_path / "rim_probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(exe) + ".o"], check=True)
    subprocess.run(["gcc", str(exe) + ".o", "-L", os.path.join(ROOT, "surfelmeshing_amd"), "-lsmx", "-Wl,-rpath," + os.path.join(ROOT, "surfelmeshing_amd"),
                    "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(RimStats) == 36
    assert got[1:] == [getattr(RimStats, f).offset for f in STAT_FIELDS] == list(range(0, 36, 4))


def test_refusals_that_need_no_device():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    tri = np.array([[0, 1, 2]], np.uint32)
    rim = np.full(8, 0xA5, np.uint8)
    st = _lib.RimStats()
    sentinel = ctypes.c_void_p(0x1000)           # never dereferenced: every case below is refused before the object is looked at

    def call(r, tin, n_in, out):
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        return L.smx_recon_mesh_rim(r, None, ptr(tin), ctypes.c_uint32(n_in), ctypes.c_int32(0), ptr(out), ctypes.byref(st))
    assert call(None, tri, 1, rim) == -1 and b"r != nullptr" in L.smx_last_error()
    assert call(sentinel, tri, (1 << 28) + 1, rim) == -1 and b"n_in" in L.smx_last_error()
    assert call(sentinel, None, 1, rim) == -1 and call(sentinel, tri, 1, None) == -1
    both = np.zeros(12, np.uint8)
    assert L.smx_recon_mesh_rim(sentinel, None, both.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(1), ctypes.c_int32(0),
                                ctypes.c_void_p(both.ctypes.data + 4), None) == -1 and b"overlaps" in L.smx_last_error()
    assert np.all(rim == 0xA5)


SHIM_PROGRAM = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map and ask which triangles touch the boundary
size_t rim_triangles(cudaStream_t stream, CUDASurfelReconstruction& reconstruction) {
  MeshParams params;
  std::vector<u32> triangles;
  std::vector<uint8_t> rim;
  smx_rim_stats stats;
  reconstruction.Triangulate(stream, params, &triangles);
  reconstruction.MeshRim(stream, triangles, &rim);
  reconstruction.MeshRim(stream, triangles, &rim, &stats);
  return rim.size() + stats.n_rim_triangles;
}
int main() { return 0; }
'''


def test_shim_mesh_rim_compiles_and_links(tmp_path):
    src = tmp_path / "rim_caller.cc"
    src.write_text(SHIM_PROGRAM)
    lib = os.path.join(ROOT, "surfelmeshing_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lsmx",
                        "-Wl,-rpath," + lib, "-o", str(tmp_path / "rim_caller")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_python_wrapper_refuses_before_the_library():
    from surfelmeshing_amd import api, meshing

    class Rec:
        def __getattr__(self, name):
            raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.MeshRim(Rec(), None, np.arange(10, dtype=np.uint32))      # not three per triangle

    class Passes:
        def MeshRim(self, stream, triangles):
            return ("rim", stream, triangles)
    assert meshing.mesh_rim(Passes(), "t", stream="s") == ("rim", "s", "t")
