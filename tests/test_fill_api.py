"""smx_recon_fill_holes without a GPU: the three symbols are declared, exported and loadable; header, ctypes mirror and numpy
record agree on the three structs; the shim's FillHoles builds with the plain host compiler; the Python wrappers,
MapMesher.update(fill=...) and tools/run_tum.py refuse bad arguments before anything reaches the library, and the library
refuses them before anything is launched."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_fill_params_default", "smx_recon_fill_holes", "smx_recon_debug_fill_timings")
STAT_FIELDS = ("n_in", "n_not_live", "n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_pinched_vertices", "n_listed_loops",
               "n_filled_loops", "n_rejected_diagonal", "n_rejected_filter", "n_new_triangles", "n_triangles")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, drop the floaters, close the small holes, make a coarser level
size_t filled(cudaStream_t stream, CUDASurfelReconstruction& reconstruction) {
  MeshParams params;
  std::vector<u32> triangles, clean, whole, coarse;
  std::vector<smx_mesh_hole> holes;
  smx_components_params c;
  smx_fill_params p;
  smx_fill_stats stats;
  u32 kept = 0;
  smx_components_params_default(&c);
  smx_fill_params_default(&p);
  p.max_hole_edges = SMX_FILL_MAX_HOLE_EDGES;
  reconstruction.Triangulate(stream, params, &triangles);
  reconstruction.MeshComponents(stream, triangles, c, &clean);
  reconstruction.FillHoles(stream, clean, p, &whole);
  reconstruction.FillHoles(stream, clean, p, &whole, &kept, &holes, &stats);
  reconstruction.DecimateMesh(stream, whole, 0.05f, &coarse);
  return coarse.size() / 3 + kept + holes.size() + stats.n_filled_loops + (holes.empty() ? 0 : holes[0].status == SMX_HOLE_FILLED);
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


def test_fill_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_fill.hip" in build.SOURCES
    for f in ("smx_fill.hip", "smx_fill.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_structs_agree_between_header_ctypes_and_numpy(tmp_path):
    from surfelmeshing_amd import api, meshing
    from surfelmeshing_amd._lib import FILL_MAX_HOLE_EDGES, FILL_PHASES, FillParams, FillStats, MeshHole
    src = tmp_path / "fill_probe.cc"
    row = ("label", "n_edges", "status")
    par = ("max_hole_edges", "min_triangle_angle_deg", "max_triangle_angle_deg")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*fill_fn)(smx_recon, smx_stream, const smx_fill_params*, const uint32_t*, uint32_t, uint32_t*, uint32_t,\n'
                   '                       smx_mesh_hole*, uint32_t, int32_t, uint32_t*, uint32_t*, uint32_t*, smx_fill_stats*);\n'
                   'typedef int (*timings_fn)(smx_recon, float*, int32_t);\n'
                   'typedef int (*default_fn)(smx_fill_params*);\n'
                   'int main() { fill_fn f = &smx_recon_fill_holes; timings_fn g = &smx_recon_debug_fill_timings;\n'
                   '  default_fn d = &smx_fill_params_default;\n'
                   '  printf("%zu %zu %zu %d %d %d %d %d %d", sizeof(smx_fill_params), sizeof(smx_mesh_hole), sizeof(smx_fill_stats),\n'
                   '         SMX_FILL_PHASES, SMX_FILL_MAX_HOLE_EDGES, SMX_HOLE_FILLED, SMX_HOLE_DIAGONAL, SMX_HOLE_FILTER, f != 0 && g != 0 && d != 0);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_fill_params, %s));\n' % f for f in par) +
                   "".join('  printf(" %%zu", offsetof(smx_mesh_hole, %s));\n' % f for f in row) +
                   "".join('  printf(" %%zu", offsetof(smx_fill_stats, %s));\n' % f for f in STAT_FIELDS) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "fill_probe")
    got = [int(v) for v in subprocess.run([str(tmp_path / "fill_probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:9] == [12, 12, 48, 4, 32, 1, 2, 3, 1]
    assert got[:5] == [ctypes.sizeof(FillParams), ctypes.sizeof(MeshHole), ctypes.sizeof(FillStats), FILL_PHASES, FILL_MAX_HOLE_EDGES]
    assert got[5:8] == [api.SMX_HOLE_FILLED, api.SMX_HOLE_DIAGONAL, api.SMX_HOLE_FILTER]
    assert got[9:12] == [getattr(FillParams, f).offset for f in par] == [0, 4, 8]
    assert got[12:15] == [getattr(MeshHole, f).offset for f in row] == [0, 4, 8]
    assert got[15:] == [getattr(FillStats, f).offset for f in STAT_FIELDS] == list(range(0, 48, 4))
    assert [n for n, _ in FillStats._fields_] == list(STAT_FIELDS) == list(meshing.FILL_STAT_NAMES)
    assert list(meshing.FILL_KEYS) == list(par)
    assert api.HOLE_DTYPE.itemsize == 12 and list(api.HOLE_DTYPE.names) == list(row)
    import fill_ref as fr
    assert fr.HOLE_DTYPE == api.HOLE_DTYPE and tuple(fr.STAT_NAMES) == STAT_FIELDS and fr.MAX_HOLE_EDGES == FILL_MAX_HOLE_EDGES
    assert (fr.FILLED, fr.DIAGONAL, fr.FILTER) == (1, 2, 3)


def test_shim_fill_holes_compiles_and_links(tmp_path):
    src = tmp_path / "fill_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "fill_caller")


def test_the_default_parameters():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    p = _lib.FillParams(7, 7.0, 7.0)
    assert L.smx_fill_params_default(ctypes.byref(p)) == 0
    assert (p.max_hole_edges, p.min_triangle_angle_deg, p.max_triangle_angle_deg) == (8, 10.0, 170.0)
    assert L.smx_fill_params_default(None) == -1


def test_the_library_refuses_bad_arguments_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    n, kept, nh = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    st = _lib.FillStats()
    sentinel = ctypes.c_void_p(16)      # stands for an object: never dereferenced, the arguments are refused before
    tri = np.arange(12, dtype=np.uint32)
    out = np.full(12, 0xA5A5A5A5, np.uint32)
    good = _lib.FillParams(8, 10.0, 170.0)

    def call(r, p=good, tin=tri, n_in=4, tout=out, capacity=4, count=n, split=kept, listed=nh):
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        ref = lambda v: None if v is None else ctypes.byref(v)                        # noqa: E731
        return L.smx_recon_fill_holes(r, None, ref(p), ptr(tin), ctypes.c_uint32(n_in), ptr(tout), ctypes.c_uint32(capacity), None,
                                      ctypes.c_uint32(0), ctypes.c_int32(0), ref(count), ref(split), ref(listed), ctypes.byref(st))
    assert call(None) == -1
    assert call(sentinel, p=None) == -1
    assert call(sentinel, count=None) == -1 and call(sentinel, split=None) == -1 and call(sentinel, listed=None) == -1
    for edges in (0, 2, 33, 0xFFFFFFFF):
        assert call(sentinel, p=_lib.FillParams(edges, 10.0, 170.0)) == -1 and b"max_hole_edges" in L.smx_last_error()
    for lo, hi in ((-1.0, 170.0), (10.0, 181.0), (20.0, 20.0), (30.0, 20.0), (float("nan"), 170.0), (10.0, float("nan")),
                   (10.0, float("inf")), (float("-inf"), 170.0)):
        assert call(sentinel, p=_lib.FillParams(8, lo, hi)) == -1 and b"triangle_angle_deg" in L.smx_last_error()
    assert call(sentinel, n_in=(1 << 28) + 1) == -1
    assert call(sentinel, tin=None) == -1
    assert call(sentinel, tout=None) == -1                           # a capacity without an array
    assert call(sentinel, tout=tri) == -1 and b"overlap" in L.smx_last_error()
    assert call(sentinel, tout=tri[9:], capacity=1) == -1 and b"overlap" in L.smx_last_error()
    assert np.all(out == 0xA5A5A5A5) and np.array_equal(tri, np.arange(12, dtype=np.uint32))
    assert L.smx_recon_debug_fill_timings(None, None, ctypes.c_int32(4)) == -1
    buf = (ctypes.c_float * 4)()
    assert L.smx_recon_debug_fill_timings(sentinel, buf, ctypes.c_int32(3)) == -1
    if _lib.device_count() == 0:        # no fall-back: without a device there is no object to fill a mesh on
        with pytest.raises(_lib.SmxError):
            api.CUDASurfelReconstruction(1000, api.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))


class _Untouchable:
    """Stands for a reconstruction: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)


BAD = [dict(max_hole_edges=2), dict(max_hole_edges=33), dict(max_hole_edges=4.5), dict(max_hole_edges=True), dict(max_hole_edges=-1),
       dict(min_triangle_angle_deg=-0.5), dict(max_triangle_angle_deg=180.5), dict(min_triangle_angle_deg=30.0, max_triangle_angle_deg=30.0),
       dict(min_triangle_angle_deg=float("nan")), dict(max_triangle_angle_deg=float("nan")), dict(max_triangle_angle_deg=float("inf"))]


def test_the_python_wrappers_refuse_bad_arguments_before_the_library():
    from surfelmeshing_amd import api, meshing
    rec, tri = _Untouchable(), np.arange(12, dtype=np.uint32).reshape(4, 3)
    p = api.fill_params(32, 0.0, 180.0)
    assert (p.max_hole_edges, p.min_triangle_angle_deg, p.max_triangle_angle_deg) == (32, 0.0, 180.0)
    p = api.fill_params()
    assert (p.max_hole_edges, p.min_triangle_angle_deg, p.max_triangle_angle_deg) == (8, 10.0, 170.0)
    for kw in BAD:
        with pytest.raises(ValueError):
            api.fill_params(**kw)
        with pytest.raises(ValueError):
            api.CUDASurfelReconstruction.FillHoles(rec, None, tri, **kw)
        with pytest.raises(ValueError):
            meshing.fill_map_mesh(rec, tri, **kw)
        with pytest.raises(ValueError):
            meshing.fill_options(kw)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.FillHoles(rec, None, np.arange(10, dtype=np.uint32))      # not three per triangle
    with pytest.raises(ValueError):
        meshing.fill_options(dict(max_hole_edge=8))                                             # a misspelt key
    assert meshing.fill_options(None) is None and meshing.fill_options(dict(max_hole_edges=5)) == dict(max_hole_edges=5)


class _Recorder:
    """Stands for a reconstruction under MapMesher: records the order of the mesh services and what each was given."""
    _device_id = 0

    def __init__(self):
        self.calls = []

    def TriangulateUpdate(self, stream, pod, index=None, cell_size=None, full_above_fraction=None):
        self.calls.append(("triangulate", None))
        return "T", {"n_triangles": 1}, {"mode": 0}

    def MeshComponents(self, stream, triangles, **kw):
        self.calls.append(("clean", triangles))
        return "C", {"clean": 1}

    def FillHoles(self, stream, triangles, **kw):
        self.calls.append(("fill", triangles, kw))
        return "F", {"fill": 1}

    def DecimateMesh(self, stream, triangles, cell_size):
        self.calls.append(("decimate", triangles))
        return "D", {"decimate": 1}


def test_map_mesher_checks_the_keys_first_and_runs_clean_fill_decimate(monkeypatch):
    from surfelmeshing_amd import api, meshing

    class _Index:
        def __init__(self, device):
            pass

        def close(self):
            pass
    monkeypatch.setattr(api, "SurfelNeighborIndex", _Index)
    rec = _Recorder()
    m = meshing.MapMesher(rec)
    for fill in (dict(max_holes=8), dict(max_hole_edges=2), dict(max_hole_edges=8, min_triangle_angle_deg=float("nan"))):
        with pytest.raises(ValueError):
            m.update(fill=fill)
    with pytest.raises(ValueError):
        m.update(clean=dict(min_triangles=1), fill=dict(edges=3))
    assert rec.calls == []                                         # refused before anything ran
    assert m.update() == ("T", {"n_triangles": 1}, {"mode": 0}) and m.filled is None and m.fill_stats is None
    rec.calls.clear()
    out = m.update(fill=dict(max_hole_edges=5))
    assert out[3] == "F" and m.filled == "F" and m.fill_stats == {"fill": 1}
    assert rec.calls == [("triangulate", None), ("fill", "T", dict(max_hole_edges=5))]
    rec.calls.clear()
    out = m.update(cell_size=0.1, clean=dict(min_triangles=3), fill=dict(max_hole_edges=8, max_triangle_angle_deg=160.0))
    assert [c[:2] for c in rec.calls] == [("triangulate", None), ("clean", "T"), ("fill", "C"), ("decimate", "F")]
    assert out[3] == "D" and (m.cleaned, m.filled, m.decimated) == ("C", "F", "D")
    rec.calls.clear()
    out = m.update(clean=dict(min_triangles=3))
    assert out[3] == "C" and m.filled is None and [c[0] for c in rec.calls] == ["triangulate", "clean"]
    assert "clean -> fill -> decimate" in meshing.MapMesher.update.__doc__ and "clean -> fill -> decimate" in meshing.__doc__


def test_run_tum_fill_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    a = run_tum.parse_args(["d", "--mesh", "--mesh_fill_holes", "8"])
    assert a.mesh_fill == dict(max_hole_edges=8, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0)
    a = run_tum.parse_args(["d", "--mesh_every", "5", "--mesh_fill_holes", "32", "--mesh_fill_min_angle", "5", "--mesh_fill_max_angle", "175",
                            "--mesh_decimate", "0.1", "--mesh_keep_largest", "1"])
    assert a.mesh_fill == dict(max_hole_edges=32, min_triangle_angle_deg=5.0, max_triangle_angle_deg=175.0)
    assert a.mesh_decimate == 0.1 and a.mesh_clean is not None
    assert run_tum.parse_args(["d", "--mesh"]).mesh_fill is None
    assert run_tum.parse_args(["d", "--mesh", "--mesh_fill_holes", "0"]).mesh_fill is None
    assert run_tum.parse_args(["d", "--mesh_fill_holes", "0"]).mesh_fill is None      # 0 = off needs no mesh
    for argv in (["d", "--mesh_fill_holes", "8"], ["d", "--mesh", "--mesh_fill_holes", "2"], ["d", "--mesh", "--mesh_fill_holes", "33"],
                 ["d", "--mesh", "--mesh_fill_holes", "-1"], ["d", "--mesh", "--mesh_fill_min_angle", "5"],
                 ["d", "--mesh", "--mesh_fill_holes", "0", "--mesh_fill_max_angle", "170"],
                 ["d", "--mesh", "--mesh_fill_holes", "8", "--mesh_fill_min_angle", "-1"],
                 ["d", "--mesh", "--mesh_fill_holes", "8", "--mesh_fill_max_angle", "181"],
                 ["d", "--mesh", "--mesh_fill_holes", "8", "--mesh_fill_min_angle", "20", "--mesh_fill_max_angle", "20"],
                 ["d", "--mesh", "--mesh_fill_holes", "8", "--mesh_fill_min_angle", "nan"]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
