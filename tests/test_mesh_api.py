"""smx_recon_triangulate without a GPU: header, ctypes mirror and shim agree on the structs, the defaults are the
documented ones, the shim's Triangulate builds with the plain host compiler, and bad parameters are refused."""
import ctypes
import os
import subprocess

import pytest

from common import ROOT

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, then write faces
size_t mesh_it(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, SurfelNeighborIndex* index) {
  MeshParams params;                       // the defaults
  params.search_radius_factor = 1.5f;
  params.max_neighbors = 32;
  std::vector<u32> triangles;
  smx_mesh_stats stats;
  reconstruction.Triangulate(stream, params, &triangles);
  reconstruction.Triangulate(stream, params, &triangles, index ? index->handle() : nullptr, 0.05f, &stats);
  return triangles.size() / 3 + stats.n_live;
}
int main() { return 0; }
'''


def test_triangulate_is_declared_and_exported():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("smx_recon_triangulate", "smx_mesh_params_default", "smx_recon_debug_mesh_timings"):
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name


def test_structs_agree_between_header_ctypes_and_shim(tmp_path):
    from surfelmeshing_amd._lib import MeshParams, MeshStats
    src = tmp_path / "mesh_probe.cc"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
        'int main() { vis::MeshParams p;\n'
        '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(smx_mesh_params), sizeof(vis::MeshParams), sizeof(smx_mesh_stats),\n'
        '    offsetof(smx_mesh_params, search_radius_factor), offsetof(smx_mesh_params, max_neighbors),\n'
        '    offsetof(smx_mesh_params, max_star_degree), offsetof(smx_mesh_stats, n_triangles),\n'
        '    offsetof(smx_mesh_stats, truncated_lists));\n'
        '  printf("%g %g %g %g %d %d\\n", p.max_angle_between_normals_deg, p.min_triangle_angle_deg, p.max_triangle_angle_deg,\n'
        '    p.search_radius_factor, p.max_neighbors, p.max_star_degree); return 0; }\n')
    from surfelmeshing_amd import _lib, build
    build.build(verbose=False)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    exe = tmp_path / "mesh_probe"
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir, "-Wl,--allow-shlib-undefined"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    sizes = [int(v) for v in out[0].split()]
    assert sizes == [ctypes.sizeof(MeshParams), ctypes.sizeof(MeshParams), ctypes.sizeof(MeshStats),
                     MeshParams.search_radius_factor.offset, MeshParams.max_neighbors.offset,
                     MeshParams.max_star_degree.offset, MeshStats.n_triangles.offset, MeshStats.truncated_lists.offset]
    assert sizes[0] == 24 and sizes[2] == 20
    assert out[1].split() == ["90", "10", "170", "1", "64", "16"]      # the shim's constructor = the library's defaults


def test_defaults():
    from surfelmeshing_amd import meshing
    from surfelmeshing_amd._lib import MeshParams, MeshStats
    p = MeshParams.defaults()
    assert (p.max_angle_between_normals_deg, p.min_triangle_angle_deg, p.max_triangle_angle_deg) == (90.0, 10.0, 170.0)
    assert p.search_radius_factor == 1.0 and p.max_neighbors == 64 and p.max_star_degree == 16
    assert [n for n, _ in MeshStats._fields_] == list(meshing.STAT_NAMES)
    q = meshing.MeshParams().to_pod()
    assert bytes(q) == bytes(p)
    q = meshing.MeshParams(search_radius_factor=1.5, max_neighbors=16, max_angle_between_normals_deg=30.0).to_pod()
    assert (q.search_radius_factor, q.max_neighbors, q.max_angle_between_normals_deg, q.max_star_degree) == (1.5, 16, 30.0, 16)
    with pytest.raises(AttributeError):
        MeshParams.defaults(no_such_field=1)
    import mesh_ref as mr
    m = mr.Params()
    for name in ("max_angle_between_normals_deg", "min_triangle_angle_deg", "max_triangle_angle_deg", "search_radius_factor",
                 "max_neighbors"):
        assert getattr(m, name) == getattr(p, name), name      # the model's defaults are the library's
    assert mr.MAX_STAR_DEGREE == p.max_star_degree


def test_parameter_validation():
    from surfelmeshing_amd import meshing
    for bad in (dict(max_neighbors=65), dict(max_neighbors=0), dict(search_radius_factor=0.99),
                dict(search_radius_factor=2.01), dict(min_triangle_angle_deg=100.0, max_triangle_angle_deg=90.0),
                dict(max_triangle_angle_deg=181.0), dict(max_angle_between_normals_deg=0.0)):
        with pytest.raises(ValueError):
            meshing.MeshParams(**bad)
    # the library refuses the call before it looks at anything else (no object is needed to see that)
    from surfelmeshing_amd import _lib
    L = _lib.load()
    n = ctypes.c_uint32(7)
    assert L.smx_recon_triangulate(None, None, None, ctypes.c_float(0.05), ctypes.byref(_lib.MeshParams.defaults()), None,
                                   ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.byref(n), None) == -1
    assert L.smx_mesh_params_default(None) == -1


def test_shim_triangulate_compiles_and_links(tmp_path):
    from surfelmeshing_amd import _lib, build
    build.build(verbose=False)
    src = tmp_path / "mesh_caller.cc"
    src.write_text(SHIM_SRC)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(tmp_path / "mesh_caller"), "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir,
                        "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
