"""smx_recon_decimate_mesh without a GPU: the two symbols are declared, exported and loadable; header, ctypes mirror and
shim agree on smx_decimate_stats; the shim's DecimateMesh builds with the plain host compiler; bad arguments are refused
before anything is launched and nothing pretends to work without a device; SaveMeshAsOBJ(referenced_only=True) writes only
the vertices the faces use, and the default output is what it was."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_recon_decimate_mesh", "smx_recon_debug_decimate_timings")
FIELDS = ("n_in", "n_not_live", "n_used_vertices", "n_cells", "n_collapsed", "n_duplicates", "n_triangles")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, then two coarser levels of it
size_t levels(cudaStream_t stream, CUDASurfelReconstruction& reconstruction) {
  MeshParams params;
  std::vector<u32> triangles, coarse, coarser, vertex_map;
  smx_decimate_stats stats;
  reconstruction.Triangulate(stream, params, &triangles);
  reconstruction.DecimateMesh(stream, triangles, 0.05f, &coarse);
  reconstruction.DecimateMesh(stream, coarse, 0.2f, &coarser, &vertex_map, &stats);
  return coarser.size() / 3 + vertex_map.size() + stats.n_cells + stats.n_triangles;
}
int main() { return 0; }
'''


def _gxx(src, exe):
    from surfelmeshing_amd import _lib, build
    build.build(verbose=False)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir, "-Wl,--allow-shlib-undefined"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_decimate_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_decimate.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", "smx_decimate.hip"))


def test_signature_and_stats_agree_between_header_ctypes_and_shim(tmp_path):
    from surfelmeshing_amd import meshing
    from surfelmeshing_amd._lib import DECIMATE_PHASES, DecimateStats
    # the header's prototypes are the issue's: a function pointer of exactly that type takes their addresses
    src = tmp_path / "decimate_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*decimate_fn)(smx_recon, smx_stream, float, const uint32_t*, uint32_t, uint32_t*, uint32_t, uint32_t*,\n'
                   '                           int32_t, uint32_t*, smx_decimate_stats*);\n'
                   'typedef int (*timings_fn)(smx_recon, float*, int32_t);\n'
                   'int main() { decimate_fn f = &smx_recon_decimate_mesh; timings_fn g = &smx_recon_debug_decimate_timings;\n'
                   '  printf("%zu %d %d", sizeof(smx_decimate_stats), SMX_DECIMATE_PHASES, f != 0 && g != 0);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_decimate_stats, %s));\n' % f for f in FIELDS) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "decimate_probe")
    got = [int(v) for v in subprocess.run([str(tmp_path / "decimate_probe")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert [n for n, _ in DecimateStats._fields_] == list(FIELDS) == list(meshing.DECIMATE_STAT_NAMES)
    assert got == [ctypes.sizeof(DecimateStats), DECIMATE_PHASES, 1] + [getattr(DecimateStats, f).offset for f in FIELDS]
    assert got == [28, 4, 1, 0, 4, 8, 12, 16, 20, 24]


def test_shim_decimate_mesh_compiles_and_links(tmp_path):
    src = tmp_path / "decimate_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "decimate_caller")


def test_bad_arguments_are_refused_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    n = ctypes.c_uint32(7)
    st = _lib.DecimateStats()
    sentinel = ctypes.c_void_p(16)      # stands for an object: never dereferenced, the arguments are refused before
    tri = np.arange(12, dtype=np.uint32)
    out = np.full(12, 0xA5A5A5A5, np.uint32)

    def call(r, cell, tin=tri, n_in=4, tout=out, capacity=4, count=n):
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        return L.smx_recon_decimate_mesh(r, None, ctypes.c_float(cell), ptr(tin), ctypes.c_uint32(n_in), ptr(tout),
                                         ctypes.c_uint32(capacity), None, ctypes.c_int32(0),
                                         ctypes.byref(count) if count is not None else None, ctypes.byref(st))
    assert call(None, 0.05) == -1
    assert call(sentinel, 0.05, count=None) == -1
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert call(sentinel, cell) == -1 and b"cell_size" in L.smx_last_error()
    assert call(sentinel, 0.05, tin=None) == -1
    assert call(sentinel, 0.05, tout=None) == -1                     # a capacity without an array
    assert call(sentinel, 0.05, tout=tri) == -1 and b"overlap" in L.smx_last_error()
    assert call(sentinel, 0.05, tout=tri[9:], capacity=1) == -1 and b"overlap" in L.smx_last_error()
    assert np.all(out == 0xA5A5A5A5) and np.array_equal(tri, np.arange(12, dtype=np.uint32))
    assert L.smx_recon_debug_decimate_timings(None, None, ctypes.c_int32(4)) == -1
    buf = (ctypes.c_float * 4)()
    assert L.smx_recon_debug_decimate_timings(sentinel, buf, ctypes.c_int32(3)) == -1
    if _lib.device_count() == 0:        # no fall-back: without a device there is no object to decimate on
        with pytest.raises(_lib.SmxError):
            api.CUDASurfelReconstruction(1000, api.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))


def test_save_mesh_as_obj_referenced_only(tmp_path, monkeypatch):
    from surfelmeshing_amd import export
    pos = np.arange(24, dtype=np.float32).reshape(8, 3)
    pos[2] = np.nan                                                  # a merged surfel
    col = (np.arange(24, dtype=np.uint8) * 10).reshape(8, 3)
    monkeypatch.setattr(export, "export_vertices", lambda reconstruction, stream=None: (pos.copy(), col.copy()))
    tri = np.array([[1, 5, 7], [5, 6, 7], [1, 2, 5], [0, 9, 1]], np.uint32)      # (the last two: a merged corner, an index past the map)
    full, part = str(tmp_path / "full.obj"), str(tmp_path / "part.obj")
    assert export.SaveMeshAsOBJ(None, full, triangles=tri)
    assert export.SaveMeshAsOBJ(None, part, triangles=tri, referenced_only=True)
    # the default: every live vertex, faces renumbered past the merged one -- what write_obj gives for exactly that
    live = ~np.isnan(pos[:, 0])
    want = str(tmp_path / "want.obj")
    export.write_obj(want, pos[live], col[live], np.array([[1, 4, 6], [4, 5, 6]]))
    assert open(full, "rb").read() == open(want, "rb").read()
    lines = open(full).read().splitlines()
    assert sum(ln.startswith("v ") for ln in lines) == 7 and lines[-2:] == ["f 2 5 7", "f 5 6 7"]
    # referenced only: the four vertices the two faces use, in slot order, and faces that index nothing else
    export.write_obj(want, pos[[1, 5, 6, 7]], col[[1, 5, 6, 7]], np.array([[0, 1, 3], [1, 2, 3]]))
    assert open(part, "rb").read() == open(want, "rb").read()
    lines = open(part).read().splitlines()
    assert sum(ln.startswith("v ") for ln in lines) == 4 and lines[-2:] == ["f 1 2 4", "f 2 3 4"]
    # no triangles: the flag changes nothing
    export.SaveMeshAsOBJ(None, part, referenced_only=True)
    export.SaveMeshAsOBJ(None, full)
    assert open(part, "rb").read() == open(full, "rb").read()
