"""smx_recon_import_points at the boundary, without a device: the parameter defaults, the struct sizes against the header, and
every refusal that looks at no object (the library checks the parameters before it touches the map)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import ROOT
from surfelmeshing_amd import _lib, api, meshing

THIRD = float(np.float32(1.0 / 3.0))


def test_parameter_defaults():
    p = _lib.ImportParams.defaults()
    assert (p.cell_size, p.search_radius, p.k, p.min_neighbors) == (np.float32(0.05), np.float32(0.1), 16, 6)
    assert (p.max_surface_variation, p.radius_rank, p.radius_scale_squared, p.confidence) == (THIRD, 8, 2.0, 1.0)
    assert (p.default_color, p.frame_index, p.orient, list(p.view_point)) == (0, 1, 0, [0.0, 0.0, 0.0])
    assert bytes(api.import_params()) == bytes(p)
    q = api.import_params(orient="origins", k=64, min_neighbors=64, radius_rank=63, view_point=(1, 2, 3), default_color=0xFFFFFFFF, frame_index=12,
                          max_surface_variation=0.0)
    assert (q.orient, q.k, q.min_neighbors, q.radius_rank, list(q.view_point), q.default_color, q.frame_index) == (2, 64, 64, 63, [1.0, 2.0, 3.0],
                                                                                                                  0xFFFFFFFF, 12)
    assert _lib.load().smx_import_params_default(None) != 0
    with pytest.raises(AttributeError):
        _lib.ImportParams.defaults(no_such_field=1)


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "import_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(smx_import_params), sizeof(smx_import_stats),\n'
                   '  offsetof(smx_import_params, view_point), offsetof(smx_import_params, radius_rank), offsetof(smx_import_stats, new_size),\n'
                   '  SMX_IMPORT_ORIENT_NONE, SMX_IMPORT_ORIENT_VIEW_POINT, SMX_IMPORT_ORIENT_ORIGINS, SMX_IMPORT_PHASES, SMX_IMPORT_JACOBI_SWEEPS);\n'
                   '  return 0; }\n')
    exe = tmp_path / "import_probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.ImportParams), C.sizeof(_lib.ImportStats), _lib.ImportParams.view_point.offset, _lib.ImportParams.radius_rank.offset,
                   _lib.ImportStats.new_size.offset, _lib.IMPORT_ORIENTS["none"], _lib.IMPORT_ORIENTS["view_point"], _lib.IMPORT_ORIENTS["origins"],
                   _lib.IMPORT_PHASES, 6]
    assert got[:2] == [56, 36] and len(_lib.IMPORT_PHASE_NAMES) == _lib.IMPORT_PHASES + 1
    assert [n for n, _ in _lib.ImportStats._fields_] == ["n_points", "n_bad", "n_sparse", "n_degenerate", "n_rough", "n_imported", "n_saturated",
                                                         "old_size", "new_size"]


def _call(r, nn, points, origins, n, p, p2s=None, capacity=0):
    st = _lib.ImportStats()
    return _lib.load().smx_recon_import_points(r, None, nn, points, None, origins, C.c_uint32(n), C.c_int32(0), p, p2s, C.c_uint32(capacity),
                                               C.c_int32(0), C.byref(st))


def test_refusals_that_need_no_device():
    """NULL pointers and bad parameters are refused before the object is looked at: the handles here are never read."""
    a, b = (C.create_string_buffer(1 << 16) for _ in range(2))     # stand-ins for a map and an index
    R, NN = (C.cast(x, C.c_void_p) for x in (a, b))
    pts = (C.c_float * 12)()
    good = _lib.ImportParams.defaults()
    INVALID = -1
    for args in ((None, NN, pts, None, 4, C.byref(good)), (R, None, pts, None, 4, C.byref(good)), (R, NN, None, None, 4, C.byref(good)),
                 (R, NN, pts, None, 4, None)):
        assert _call(*args) == INVALID
    nan, inf = float("nan"), float("inf")
    bad = [dict(k=3), dict(k=65), dict(min_neighbors=2), dict(min_neighbors=17), dict(frame_index=0), dict(cell_size=0.0), dict(cell_size=-1.0),
           dict(cell_size=nan), dict(search_radius=0.0), dict(search_radius=nan), dict(radius_scale_squared=0.0), dict(radius_scale_squared=nan),
           dict(max_surface_variation=-0.01), dict(max_surface_variation=0.34), dict(max_surface_variation=nan), dict(radius_rank=0),
           dict(radius_rank=64), dict(confidence=nan), dict(confidence=inf), dict(orient=3), dict(orient=-1), dict(view_point=(0.0, nan, 0.0)),
           dict(view_point=(inf, 0.0, 0.0))]
    for kw in bad:
        assert _call(R, NN, pts, None, 4, C.byref(_lib.ImportParams.defaults(**kw))) == INVALID, kw
        assert b"invalid argument" in _lib.load().smx_last_error()
    assert _call(R, NN, pts, None, 4, C.byref(_lib.ImportParams.defaults(orient=2))) == INVALID      # ORIGINS without origins
    small = (C.c_uint32 * 3)()
    assert _call(R, NN, pts, None, 4, C.byref(good), small, 3) == INVALID and not any(small)           # a point_to_slot that is too small
    assert _lib.load().smx_recon_debug_import_timings(None, (C.c_float * 8)(), 8) == INVALID
    assert _lib.load().smx_recon_debug_import_timings(R, None, 8) == INVALID


def test_python_layer_refuses_what_the_library_would():
    for kw in (dict(k=3), dict(k=65), dict(min_neighbors=2), dict(min_neighbors=17), dict(frame_index=0), dict(cell_size=0.0), dict(search_radius=-1.0),
               dict(radius_scale_squared=0.0), dict(max_surface_variation=0.5), dict(radius_rank=0), dict(radius_rank=64), dict(orient="outwards"),
               dict(orient=3), dict(confidence=float("nan")), dict(view_point=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            api.import_params(**kw)
    assert api.import_stats_dict(_lib.ImportStats(*range(9)))["new_size"] == 8
    assert meshing.pack_colors([[1, 2, 3], [255, 0, 128]]).tolist() == [0x00030201, 0x008000FF]
    with pytest.raises(ValueError):
        api._cloud_arg(np.zeros(7, np.float32), 3, np.float32, "points")


SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// another sensor's scan becomes a map of its own, and that map goes into the session's under the pose a registration found
u32 scan_into_session(cudaStream_t stream, CUDASurfelReconstruction& session, CUDASurfelReconstruction& scan_map, const std::vector<float>& xyz,
                      const std::vector<float>& sensor_origins, const float* session_T_scan) {
  smx_import_params ip;
  smx_import_params_default(&ip);
  ip.orient = SMX_IMPORT_ORIENT_ORIGINS;
  std::vector<u32> point_to_slot;
  smx_import_stats ist;
  scan_map.ImportPoints(stream, xyz.data(), nullptr, sensor_origins.data(), (u32)(xyz.size() / 3), ip, &point_to_slot, nullptr, &ist);
  scan_map.ImportPoints(stream, xyz.data(), nullptr, sensor_origins.data(), (u32)(xyz.size() / 3), ip);   // (without the map)
  smx_merge_params mp;
  smx_merge_params_default(&mp);
  session.MergeMap(stream, scan_map, session_T_scan, mp);
  return ist.n_imported;
}
int main() { return 0; }
'''


def test_shim_import_compiles_and_links(tmp_path):
    from surfelmeshing_amd import build
    build.build(verbose=False)
    src = tmp_path / "import_caller.cc"
    src.write_text(SHIM_SRC)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(tmp_path / "import_caller"), "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir,
                        "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_mesh_ply_flags():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mesh_ply
    a = mesh_ply.parse_args(["in.ply", "--export_mesh", "out.obj", "--search_radius", "0.2", "--k", "24", "--radius_rank", "12", "--view_point", "1,2,3",
                             "--mesh_min_component", "50", "--mesh_fill_holes", "8", "--mesh_decimate", "0.05"])
    assert (a.search_radius, a.k, a.radius_rank, a.view_point, a.mesh_min_component, a.mesh_fill_holes, a.mesh_decimate) == (
        0.2, 24, 12, (1.0, 2.0, 3.0), 50, 8, 0.05)
    d = mesh_ply.parse_args(["in.ply", "--export_mesh", "out.obj"])
    assert (d.search_radius, d.k, d.radius_rank, d.view_point, d.mesh_min_component, d.mesh_fill_holes, d.mesh_decimate) == (0.1, 16, 8, None, None, 0, None)
    for bad in (["--view_point", "1,2"], ["--k", "3"], ["--mesh_fill_holes", "2"], ["--mesh_decimate", "0"], ["--radius_rank", "64"]):
        with pytest.raises(SystemExit):
            mesh_ply.parse_args(["in.ply", "--export_mesh", "out.obj"] + bad)
    with pytest.raises(SystemExit):
        mesh_ply.parse_args(["in.ply"])
    line = mesh_ply.format_stats_line({"n_points": 10, "n_bad": 1, "n_sparse": 2, "n_degenerate": 0, "n_rough": 0, "n_imported": 7, "n_saturated": 3,
                                       "old_size": 0, "new_size": 7})
    assert line == "imported 7 of 10 points (bad 1, sparse 2, degenerate 0, rough 0; 3 lists full)"
