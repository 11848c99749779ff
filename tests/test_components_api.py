"""smx_recon_mesh_components without a GPU: the three symbols are declared, exported and loadable; header, ctypes mirror and
numpy record agree on the three structs; the shim's MeshComponents builds with the plain host compiler; the Python
wrappers and tools/run_tum.py refuse bad arguments before anything reaches the library, and the library refuses them
before anything is launched."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_components_params_default", "smx_recon_mesh_components", "smx_recon_debug_components_timings")
STAT_FIELDS = ("n_in", "n_not_live", "n_used_vertices", "n_components", "n_kept_components", "n_largest_triangles", "n_triangles")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, drop the floaters, keep the two largest pieces of a coarser level
size_t cleaned(cudaStream_t stream, CUDASurfelReconstruction& reconstruction) {
  MeshParams params;
  std::vector<u32> triangles, clean, coarse, largest, labels;
  std::vector<smx_mesh_component> pieces;
  smx_components_params p;
  smx_components_stats stats;
  smx_components_params_default(&p);
  p.min_triangles = 20; p.min_diagonal = 0.05f;
  reconstruction.Triangulate(stream, params, &triangles);
  reconstruction.MeshComponents(stream, triangles, p, &clean);
  reconstruction.DecimateMesh(stream, clean, 0.05f, &coarse);
  p.keep_largest = 2;
  reconstruction.MeshComponents(stream, coarse, p, &largest, &labels, &pieces, &stats);
  return largest.size() / 3 + labels.size() + pieces.size() + stats.n_components + (pieces.empty() ? 0 : pieces[0].n_triangles);
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


def test_components_are_declared_exported_and_their_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_components.hip" in build.SOURCES
    for f in ("smx_components.hip", "smx_components.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_structs_agree_between_header_ctypes_and_numpy(tmp_path):
    from surfelmeshing_amd import api, meshing
    from surfelmeshing_amd._lib import COMPONENTS_PHASES, ComponentsParams, ComponentsStats, MeshComponent
    # the header's prototypes are the issue's: a function pointer of exactly that type takes their addresses
    src = tmp_path / "components_probe.cc"
    row = ("label", "n_vertices", "n_triangles", "kept", "lo", "hi")
    par = ("min_triangles", "min_diagonal", "keep_largest")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*components_fn)(smx_recon, smx_stream, const smx_components_params*, const uint32_t*, uint32_t, uint32_t*,\n'
                   '                             uint32_t, uint32_t*, smx_mesh_component*, uint32_t, int32_t, uint32_t*, uint32_t*,\n'
                   '                             smx_components_stats*);\n'
                   'typedef int (*timings_fn)(smx_recon, float*, int32_t);\n'
                   'typedef int (*default_fn)(smx_components_params*);\n'
                   'int main() { components_fn f = &smx_recon_mesh_components; timings_fn g = &smx_recon_debug_components_timings;\n'
                   '  default_fn d = &smx_components_params_default;\n'
                   '  printf("%zu %zu %zu %d %d", sizeof(smx_components_params), sizeof(smx_mesh_component), sizeof(smx_components_stats),\n'
                   '         SMX_COMPONENTS_PHASES, f != 0 && g != 0 && d != 0);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_components_params, %s));\n' % f for f in par) +
                   "".join('  printf(" %%zu", offsetof(smx_mesh_component, %s));\n' % f for f in row) +
                   "".join('  printf(" %%zu", offsetof(smx_components_stats, %s));\n' % f for f in STAT_FIELDS) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "components_probe")
    got = [int(v) for v in subprocess.run([str(tmp_path / "components_probe")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got[:5] == [12, 40, 28, 4, 1]
    assert got[:5] == [ctypes.sizeof(ComponentsParams), ctypes.sizeof(MeshComponent), ctypes.sizeof(ComponentsStats), COMPONENTS_PHASES, 1]
    assert got[5:8] == [getattr(ComponentsParams, f).offset for f in par] == [0, 4, 8]
    assert got[8:14] == [getattr(MeshComponent, f).offset for f in row] == [0, 4, 8, 12, 16, 28]
    assert got[14:] == [getattr(ComponentsStats, f).offset for f in STAT_FIELDS] == [0, 4, 8, 12, 16, 20, 24]
    assert [n for n, _ in ComponentsStats._fields_] == list(STAT_FIELDS) == list(meshing.COMPONENTS_STAT_NAMES)
    # the numpy record MeshComponents returns is the same 40 bytes
    assert api.COMPONENT_DTYPE.itemsize == 40 and list(api.COMPONENT_DTYPE.names) == list(row)
    assert [api.COMPONENT_DTYPE.fields[f][1] for f in row] == [0, 4, 8, 12, 16, 28]
    import components_ref as cr
    assert cr.COMPONENT_DTYPE == api.COMPONENT_DTYPE


def test_shim_mesh_components_compiles_and_links(tmp_path):
    src = tmp_path / "components_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "components_caller")


def test_the_default_parameters_keep_everything():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    p = _lib.ComponentsParams(7, 7.0, 7)
    assert L.smx_components_params_default(ctypes.byref(p)) == 0
    assert (p.min_triangles, p.min_diagonal, p.keep_largest) == (0, 0.0, 0)
    assert L.smx_components_params_default(None) == -1


def test_the_library_refuses_bad_arguments_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    n, nc = ctypes.c_uint32(7), ctypes.c_uint32(7)
    st = _lib.ComponentsStats()
    sentinel = ctypes.c_void_p(16)      # stands for an object: never dereferenced, the arguments are refused before
    tri = np.arange(12, dtype=np.uint32)
    out = np.full(12, 0xA5A5A5A5, np.uint32)
    good = _lib.ComponentsParams(0, 0.0, 0)

    def call(r, p=good, tin=tri, n_in=4, tout=out, capacity=4, count=n, pieces=nc):
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        ref = lambda v: None if v is None else ctypes.byref(v)                        # noqa: E731
        return L.smx_recon_mesh_components(r, None, ref(p), ptr(tin), ctypes.c_uint32(n_in), ptr(tout), ctypes.c_uint32(capacity),
                                           None, None, ctypes.c_uint32(0), ctypes.c_int32(0), ref(count), ref(pieces), ctypes.byref(st))
    assert call(None) == -1
    assert call(sentinel, p=None) == -1
    assert call(sentinel, count=None) == -1 and call(sentinel, pieces=None) == -1
    for d in (-1.0, -1e-30, float("nan"), float("inf")):
        assert call(sentinel, p=_lib.ComponentsParams(0, d, 0)) == -1 and b"min_diagonal" in L.smx_last_error()
    assert call(sentinel, tin=None) == -1
    assert call(sentinel, tout=None) == -1                           # a capacity without an array
    assert call(sentinel, tout=tri) == -1 and b"overlap" in L.smx_last_error()
    assert call(sentinel, tout=tri[9:], capacity=1) == -1 and b"overlap" in L.smx_last_error()
    assert np.all(out == 0xA5A5A5A5) and np.array_equal(tri, np.arange(12, dtype=np.uint32))
    assert L.smx_recon_debug_components_timings(None, None, ctypes.c_int32(4)) == -1
    buf = (ctypes.c_float * 4)()
    assert L.smx_recon_debug_components_timings(sentinel, buf, ctypes.c_int32(3)) == -1
    if _lib.device_count() == 0:        # no fall-back: without a device there is no object to label a mesh on
        with pytest.raises(_lib.SmxError):
            api.CUDASurfelReconstruction(1000, api.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))


class _Untouchable:
    """Stands for a reconstruction: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)


def test_the_python_wrappers_refuse_bad_arguments_before_the_library():
    from surfelmeshing_amd import api, meshing
    rec, tri = _Untouchable(), np.arange(12, dtype=np.uint32).reshape(4, 3)
    p = api.components_params(3, 0.25, 2)
    assert (p.min_triangles, p.min_diagonal, p.keep_largest) == (3, 0.25, 2)
    bad = [dict(min_triangles=-1), dict(min_triangles=2 ** 32), dict(min_triangles=1.5), dict(min_diagonal=-0.1),
           dict(min_diagonal=float("nan")), dict(min_diagonal=float("inf")), dict(keep_largest=-2), dict(keep_largest=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            api.components_params(**kw)
        with pytest.raises(ValueError):
            api.CUDASurfelReconstruction.MeshComponents(rec, None, tri, **kw)
        with pytest.raises(ValueError):
            meshing.clean_map_mesh(rec, tri, **kw)
        with pytest.raises(ValueError):
            meshing.clean_options(kw)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.MeshComponents(rec, None, np.arange(10, dtype=np.uint32))      # not three per triangle
    with pytest.raises(ValueError):
        meshing.clean_options(dict(min_triangle=3))                                                  # a misspelt key
    assert meshing.clean_options(None) is None and meshing.clean_options(dict(keep_largest=1)) == dict(keep_largest=1)


def test_run_tum_cleaning_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    a = run_tum.parse_args(["d", "--mesh", "--mesh_min_component", "20", "--mesh_min_extent", "0.05", "--mesh_keep_largest", "3"])
    assert a.mesh_clean == dict(min_triangles=20, min_diagonal=0.05, keep_largest=3)
    a = run_tum.parse_args(["d", "--mesh_every", "5", "--mesh_keep_largest", "1", "--mesh_decimate", "0.1"])
    assert a.mesh_clean == dict(min_triangles=0, min_diagonal=0.0, keep_largest=1) and a.mesh_decimate == 0.1
    assert run_tum.parse_args(["d", "--mesh"]).mesh_clean is None
    for argv in (["d", "--mesh_min_component", "20"], ["d", "--mesh_min_extent", "0.1"], ["d", "--mesh_keep_largest", "1"],
                 ["d", "--mesh", "--mesh_min_component", "-1"], ["d", "--mesh", "--mesh_min_extent", "-0.5"],
                 ["d", "--mesh", "--mesh_min_extent", "nan"], ["d", "--mesh", "--mesh_min_extent", "inf"],
                 ["d", "--mesh", "--mesh_keep_largest", "0"]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
