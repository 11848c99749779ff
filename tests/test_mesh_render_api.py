"""smx_recon_render_mesh without a GPU: the symbols are declared, exported and loadable; header, ctypes mirror and shim
agree on the two PODs; the shim's RenderMesh builds with the plain host compiler; bad arguments are refused before anything
is launched; tools/run_tum.py refuses --render_source mesh without a mesh option."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_mesh_render_params_default", "smx_recon_render_mesh", "smx_recon_debug_mesh_render_timings")
PARAM_FIELDS = ("width", "height", "fx", "fy", "cx", "cy", "global_T_camera", "near_z", "far_z", "color_flags", "frame_index",
                "surfel_integration_active_window_size", "cull_back_faces", "normal_mode")
STAT_FIELDS = ("n_in", "n_out_of_range", "n_not_live", "n_clipped", "n_degenerate", "n_culled", "n_drawn", "n_large",
               "n_covered_pixels")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, decimate it, look at both
u32 preview(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, const smx_mesh_render_params& params,
            CUDABuffer<float>* depth, CUDABuffer<RenderColor>* color) {
  MeshParams mesh_params;
  std::vector<u32> triangles, coarse;
  smx_mesh_render_stats stats;
  reconstruction.Triangulate(stream, mesh_params, &triangles);
  reconstruction.RenderMesh(stream, params, triangles, depth, nullptr, nullptr, color);
  reconstruction.DecimateMesh(stream, triangles, 0.05f, &coarse);
  reconstruction.RenderMesh(stream, params, coarse, depth, nullptr, nullptr, nullptr, &stats);
  return stats.n_drawn + stats.n_large + stats.n_covered_pixels;
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


def test_mesh_render_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_mesh_raster.hip" in build.SOURCES
    for f in ("smx_mesh_raster.hip", "smx_mesh_raster.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_pods_agree_between_header_ctypes_and_shim(tmp_path):
    from surfelmeshing_amd import api
    from surfelmeshing_amd._lib import MeshRenderParams, MeshRenderStats
    src = tmp_path / "mesh_render_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*render_fn)(smx_recon, smx_stream, const smx_mesh_render_params*, const uint32_t*, uint32_t, int32_t,\n'
                   '                         const smx_buffer_desc*, const smx_buffer_desc*, const smx_buffer_desc*, const smx_buffer_desc*,\n'
                   '                         smx_mesh_render_stats*);\n'
                   'typedef int (*default_fn)(smx_mesh_render_params*);\n'
                   'int main() { render_fn f = &smx_recon_render_mesh; default_fn g = &smx_mesh_render_params_default;\n'
                   '  printf("%zu %zu %d %d %d %d", sizeof(smx_mesh_render_params), sizeof(smx_mesh_render_stats), f != 0 && g != 0,\n'
                   '         SMX_MESH_NORMAL_VERTEX, SMX_MESH_NORMAL_FACE, SMX_MESH_RENDER_LARGE_PIXELS);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_mesh_render_params, %s));\n' % f for f in PARAM_FIELDS) +
                   "".join('  printf(" %%zu", offsetof(smx_mesh_render_stats, %s));\n' % f for f in STAT_FIELDS) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "mesh_render_probe")
    got = [int(v) for v in subprocess.run([str(tmp_path / "mesh_render_probe")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert [n for n, _ in MeshRenderParams._fields_] == list(PARAM_FIELDS)
    assert [n for n, _ in MeshRenderStats._fields_] == list(STAT_FIELDS)
    assert got == ([ctypes.sizeof(MeshRenderParams), ctypes.sizeof(MeshRenderStats), 1, api.SMX_MESH_NORMAL_VERTEX,
                    api.SMX_MESH_NORMAL_FACE, api.SMX_MESH_RENDER_LARGE_PIXELS] +
                   [getattr(MeshRenderParams, f).offset for f in PARAM_FIELDS] + [getattr(MeshRenderStats, f).offset for f in STAT_FIELDS])
    assert got[:6] == [100, 36, 1, 0, 1, 256]


def test_shim_render_mesh_compiles_and_links(tmp_path):
    src = tmp_path / "mesh_render_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "mesh_render_caller")


def test_defaults_and_make_params():
    from surfelmeshing_amd import api
    from surfelmeshing_amd._lib import MeshRenderParams
    p = MeshRenderParams.defaults()
    assert (p.width, p.height, p.color_flags, p.cull_back_faces, p.normal_mode) == (0, 0, 0, 0, api.SMX_MESH_NORMAL_VERTEX)
    assert list(p.global_T_camera) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and p.near_z == np.float32(0.05) and p.far_z == 1000.0
    with pytest.raises(AttributeError):
        MeshRenderParams.defaults(splat_mode=1)
    pose = np.arange(12, dtype=np.float32).reshape(3, 4)
    q = api.make_mesh_render_params(64, 48, 50.0, 51.0, 32.0, 24.0, pose, color_flags=api.SMX_VIS_RADII, cull_back_faces=True,
                                    normal_mode=api.SMX_MESH_NORMAL_FACE, frame_index=7)
    assert (q.width, q.height, q.fx, q.fy, q.cx, q.cy) == (64, 48, 50.0, 51.0, 32.0, 24.0)
    assert list(q.global_T_camera) == list(range(12)) and (q.color_flags, q.frame_index, q.cull_back_faces, q.normal_mode) == (4, 7, 1, 1)
    assert q.near_z == p.near_z and q.far_z == p.far_z


def test_bad_arguments_are_refused_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    sentinel = ctypes.c_void_p(16)      # stands for an object: never dereferenced, the arguments are refused before
    tri = np.arange(12, dtype=np.uint32)
    image = np.full((48, 64), 0xA5A5A5A5, np.uint32)
    good = dict(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0)

    def desc(elem=4, **kw):
        d = dict(address=image.ctypes.data, height=48, width=64, pitch=64 * elem)
        d.update(kw)
        return _lib.BufferDesc(d["address"], d["height"], d["width"], d["pitch"])

    def call(r=sentinel, tin=tri, n_in=4, depth=None, normal=None, params=True, **fields):
        p = _lib.MeshRenderParams.defaults(**dict(good, **fields))
        return L.smx_recon_render_mesh(r, None, ctypes.byref(p) if params else None,
                                       tin.ctypes.data_as(ctypes.c_void_p) if tin is not None else None, ctypes.c_uint32(n_in),
                                       ctypes.c_int32(0), ctypes.byref(depth) if depth is not None else None, None,
                                       ctypes.byref(normal) if normal is not None else None, None, None)
    assert L.smx_mesh_render_params_default(None) == -1
    assert call(r=None) == -1 and call(params=False) == -1
    for bad in (dict(width=0), dict(height=-1), dict(width=16385), dict(fx=0.0), dict(fy=float("nan")), dict(cx=float("inf")),
                dict(near_z=0.0), dict(far_z=0.01), dict(color_flags=16), dict(cull_back_faces=2), dict(cull_back_faces=-1),
                dict(normal_mode=2), dict(normal_mode=-1)):
        assert call(**bad) == -1, bad
    nan_pose = (ctypes.c_float * 12)(*([1.0] * 11 + [float("nan")]))
    assert call(global_T_camera=nan_pose) == -1
    assert call(tin=None) == -1 and b"triangles" in L.smx_last_error()
    for bad in (desc(width=63), desc(height=47), desc(pitch=64 * 4 - 4), desc(pitch=64 * 4 + 2), desc(address=image.ctypes.data + 2),
                desc(address=0)):
        assert call(depth=bad) == -1
    assert call(normal=desc()) == -1                                 # a pitch too short for float4
    assert np.all(image == 0xA5A5A5A5)
    assert L.smx_recon_debug_mesh_render_timings(None, None) == -1
    if _lib.device_count() == 0:        # no fall-back: without a device there is no object to draw from
        with pytest.raises(_lib.SmxError):
            api.CUDASurfelReconstruction(1000, api.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))


def test_run_tum_refuses_a_mesh_render_without_a_mesh(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    with pytest.raises(SystemExit) as e:
        run_tum.parse_args(["folder", "--render_dir", "out", "--render_every", "2", "--render_source", "mesh"])
    assert e.value.code == 2 and "--render_source mesh needs a mesh" in capsys.readouterr().err
    assert run_tum.parse_args(["folder", "--render_dir", "out"]).render_source == "splats"
    for mesh in (["--mesh"], ["--mesh_every", "4"], ["--mesh", "--mesh_decimate", "0.05"]):
        assert run_tum.parse_args(["folder", "--render_source", "mesh"] + mesh).render_source == "mesh"
