"""smx_recon_triangulate_update without a GPU: the three symbols are declared, exported and loadable; header, ctypes mirror
and shim agree on smx_mesh_update_stats; the shim's TriangulateUpdate builds with the plain host compiler; bad arguments
are refused before anything is launched."""
import ctypes
import os
import subprocess

from common import ROOT

SYMBOLS = ("smx_recon_triangulate_update", "smx_recon_triangulate_reset", "smx_recon_debug_mesh_update_timings")
FIELDS = ("mode", "n_changed", "n_dirty", "n_reagreed", "n_kept_triangles")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: follow the map every few frames
size_t follow(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, SurfelNeighborIndex* index) {
  MeshParams params;
  std::vector<u32> triangles;
  smx_mesh_stats stats;
  smx_mesh_update_stats update_stats;
  reconstruction.TriangulateUpdate(stream, params, &triangles);
  reconstruction.TriangulateUpdate(stream, params, &triangles, index ? index->handle() : nullptr, 0.05f, &stats, &update_stats);
  reconstruction.TriangulateUpdate(stream, params, &triangles, nullptr, 0.05f, &stats, &update_stats, 0.5f);
  reconstruction.ResetTriangulation();
  return triangles.size() / 3 + stats.n_live + update_stats.mode + update_stats.n_changed + update_stats.n_dirty +
         update_stats.n_reagreed + update_stats.n_kept_triangles;
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


def test_update_is_declared_and_exported():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name


def test_update_stats_agree_between_header_ctypes_and_shim(tmp_path):
    from surfelmeshing_amd import meshing
    from surfelmeshing_amd._lib import MeshUpdateStats
    src = tmp_path / "update_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'int main() { printf("%zu", sizeof(smx_mesh_update_stats));\n' +
                   "".join('  printf(" %%zu", offsetof(smx_mesh_update_stats, %s));\n' % f for f in FIELDS) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "update_probe")
    got = [int(v) for v in subprocess.run([str(tmp_path / "update_probe")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert [n for n, _ in MeshUpdateStats._fields_] == list(FIELDS) == list(meshing.UPDATE_STAT_NAMES)
    assert got == [ctypes.sizeof(MeshUpdateStats)] + [getattr(MeshUpdateStats, f).offset for f in FIELDS]
    assert got == [20, 0, 4, 8, 12, 16]
    assert len(meshing.UPDATE_MODES) == 5


def test_shim_triangulate_update_compiles_and_links(tmp_path):
    src = tmp_path / "update_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "update_caller")


def test_bad_arguments_are_refused_with_nothing_launched():
    # (no object and no device are needed to see that: the checks come first)
    from surfelmeshing_amd import _lib
    L = _lib.load()
    n = ctypes.c_uint32(7)
    us = _lib.MeshUpdateStats()
    sentinel = ctypes.c_void_p(16)      # stands for an object: never dereferenced, the arguments are refused before

    def call(r, nn, params, fraction, cell=0.05):
        return L.smx_recon_triangulate_update(r, None, nn, ctypes.c_float(cell), ctypes.byref(params), ctypes.c_float(fraction),
                                              None, ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.byref(n), None,
                                              ctypes.byref(us))
    ok = _lib.MeshParams.defaults()
    assert call(None, None, ok, -1.0) == -1
    assert call(sentinel, sentinel, ok, 1.5) == -1
    assert b"full_above_fraction" in L.smx_last_error()
    assert call(sentinel, sentinel, ok, float("nan")) == -1
    assert call(sentinel, sentinel, ok, 0.5, cell=0.0) == -1
    for bad in (dict(max_neighbors=65), dict(max_neighbors=0), dict(search_radius_factor=0.5), dict(search_radius_factor=2.5),
                dict(max_star_degree=8), dict(min_triangle_angle_deg=120.0, max_triangle_angle_deg=60.0),
                dict(max_angle_between_normals_deg=0.0)):
        assert call(sentinel, sentinel, _lib.MeshParams.defaults(**bad), 0.5) == -1, bad
    assert L.smx_recon_triangulate_reset(None) == -1
    assert L.smx_recon_debug_mesh_update_timings(None, None) == -1
