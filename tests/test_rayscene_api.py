"""smx_rayscene without a GPU: the six symbols are declared, exported and loadable and the new source is listed; header and
ctypes mirror agree on the three structs; the shim's RayScene builds with the plain host compiler; the defaults; the library
refuses bad arguments before anything is launched and the Python wrappers before anything reaches the library;
tools/run_tum.py --mesh_eval_rays_frames."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_rayscene_create", "smx_rayscene_destroy", "smx_rayscene_params_default", "smx_recon_build_rayscene", "smx_rayscene_cast",
           "smx_rayscene_debug_timings")
PARAMS = ("cell_size", "occupancy")
BUILD = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_wide", "n_entries", "n_cells", "cell_size_used", "occupancy_log2",
         "n_blocks_set", "occupancy_bytes", "device_bytes")
CAST = ("n_rays", "n_bad_rays", "n_hit", "n_front_hits", "max_t_bits", "reserved", "n_layers", "n_bit_tests", "n_lookups", "n_lookup_misses",
        "n_pair_tests")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, build one scene of it, cast from camera after camera
size_t cast(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, const std::vector<std::vector<float>>& cameras) {
  MeshParams params;
  std::vector<u32> triangles, hit;
  std::vector<float> t, uv;
  smx_raycast_params p;
  smx_rayscene_cast_stats stats;
  smx_raycast_params_default(&p);
  p.t_max = 1.0f;
  reconstruction.Triangulate(stream, params, &triangles);
  RayScene scene;
  reconstruction.BuildRayScene(stream, triangles, &scene);
  reconstruction.BuildRayScene(stream, triangles, &scene, 0.05f, 4);
  size_t sum = scene.stats().n_entries + (size_t)scene.stats().device_bytes + (scene.handle() != nullptr);
  for (const std::vector<float>& rays : cameras) {
    scene.Cast(stream, rays, p, &hit, &t);
    scene.Cast(stream, rays, p, &hit, &t, &uv, &stats);
    sum += hit.size() + uv.size() + stats.n_hit + (size_t)stats.n_bit_tests;
  }
  return sum;
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


def test_rayscene_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_rayscene.hip" in build.SOURCES
    for f in ("smx_rayscene.hip", "smx_rayscene.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_structs_agree_between_header_and_ctypes(tmp_path):
    from surfelmeshing_amd import _lib
    from surfelmeshing_amd._lib import RaySceneCastStats, RaySceneParams, RaySceneStats
    src = tmp_path / "rayscene_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*build_fn)(smx_recon, smx_stream, smx_rayscene, const smx_rayscene_params*, const uint32_t*, uint32_t, int32_t,\n'
                   '                        smx_rayscene_stats*);\n'
                   'typedef int (*cast_fn)(smx_rayscene, smx_stream, const smx_raycast_params*, const float*, uint32_t, uint32_t*, float*, float*,\n'
                   '                       int32_t, smx_rayscene_cast_stats*);\n'
                   'typedef int (*create_fn)(int32_t, smx_rayscene*);\n'
                   'typedef int (*destroy_fn)(smx_rayscene);\n'
                   'typedef int (*timings_fn)(smx_rayscene, float*, int32_t);\n'
                   'typedef int (*default_fn)(smx_rayscene_params*);\n'
                   'int main() { build_fn b = &smx_recon_build_rayscene; cast_fn c = &smx_rayscene_cast; create_fn n = &smx_rayscene_create;\n'
                   '  destroy_fn x = &smx_rayscene_destroy; timings_fn g = &smx_rayscene_debug_timings; default_fn d = &smx_rayscene_params_default;\n'
                   '  printf("%zu %zu %zu %d %d", sizeof(smx_rayscene_params), sizeof(smx_rayscene_stats), sizeof(smx_rayscene_cast_stats),\n'
                   '         SMX_RAYSCENE_PHASES, b != 0 && c != 0 && n != 0 && x != 0 && g != 0 && d != 0);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_rayscene_params, %s));\n' % f for f in PARAMS) +
                   "".join('  printf(" %%zu", offsetof(smx_rayscene_stats, %s));\n' % f for f in BUILD) +
                   "".join('  printf(" %%zu", offsetof(smx_rayscene_cast_stats, %s));\n' % f for f in CAST) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "rayscene_probe")
    out = [int(v) for v in subprocess.run([str(tmp_path / "rayscene_probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:5] == [8, 56, 64, 5, 1]
    assert out[:4] == [ctypes.sizeof(RaySceneParams), ctypes.sizeof(RaySceneStats), ctypes.sizeof(RaySceneCastStats), _lib.RAYSCENE_PHASES]
    offs = out[5:]
    assert offs[:2] == [getattr(RaySceneParams, f).offset for f in PARAMS] == [0, 4]
    assert offs[2:14] == [getattr(RaySceneStats, f).offset for f in BUILD] == list(range(0, 40, 4)) + [40, 48]
    assert offs[14:] == [getattr(RaySceneCastStats, f).offset for f in CAST] == list(range(0, 24, 4)) + [24, 32, 40, 48, 56]
    assert [n for n, _ in RaySceneStats._fields_] == list(BUILD) and [n for n, _ in RaySceneCastStats._fields_] == list(CAST)
    assert [n for n, _ in RaySceneParams._fields_] == list(PARAMS)


def test_shim_ray_scene_compiles_and_links(tmp_path):
    src = tmp_path / "rayscene_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "rayscene_caller")


def test_the_default_parameters():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    p = _lib.RaySceneParams(7.0, 7)
    assert L.smx_rayscene_params_default(ctypes.byref(p)) == 0
    assert (p.cell_size, p.occupancy) == (0.0, 0)
    assert L.smx_rayscene_params_default(None) == -1
    assert _lib.RAYSCENE_MAX_LOG2 == 6


def test_the_library_refuses_bad_arguments_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    st, bst = _lib.RaySceneCastStats(), _lib.RaySceneStats()
    good, rays = _lib.RaycastParams(0.0, 1.0, 0.0, 0), np.zeros(24, np.float32)
    GUARD = 0xA5A5A5A5
    hit, t = np.full(4, GUARD, np.uint32), np.full(4, GUARD, np.uint32).view(np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    # without a scene nothing is looked at
    assert L.smx_rayscene_cast(None, None, ctypes.byref(good), ptr(rays), ctypes.c_uint32(4), ptr(hit), ptr(t), None, ctypes.c_int32(0),
                               ctypes.byref(st)) == -1
    assert L.smx_recon_build_rayscene(ctypes.c_void_p(16), None, None, ctypes.byref(_lib.RaySceneParams(0.0, 0)), None, ctypes.c_uint32(0),
                                      ctypes.c_int32(0), ctypes.byref(bst)) == -1
    assert L.smx_rayscene_create(ctypes.c_int32(-1), None) == -1 and L.smx_rayscene_destroy(None) == 0
    assert L.smx_rayscene_debug_timings(None, None, ctypes.c_int32(5)) == -1
    assert np.all(hit == GUARD) and np.all(t.view(np.uint32) == GUARD)
    if _lib.device_count() == 0:        # no fall-back: without a device there is no scene
        with pytest.raises(_lib.SmxError):
            api.RayScene()


class _Untouchable:
    """Stands for a reconstruction or a scene: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)


BAD_BUILD = [dict(cell_size=-0.1), dict(cell_size=float("nan")), dict(cell_size=float("inf")), dict(occupancy=-2), dict(occupancy=8),
             dict(occupancy=True), dict(occupancy=1.5)]
BAD_CAST = [dict(t_min=-0.5), dict(t_min=2.0, t_max=1.0), dict(t_max=2.0 ** 21), dict(t_min=float("nan")), dict(t_max=float("inf")),
            dict(cull=3), dict(cull=-1), dict(cull=True)]


def test_the_python_wrappers_refuse_bad_arguments_before_the_library():
    from surfelmeshing_amd import api, meshing
    rec, tri = _Untouchable(), np.arange(12, dtype=np.uint32).reshape(4, 3)
    p = api.rayscene_params(0.5, 4)
    assert (p.cell_size, p.occupancy) == (0.5, 4)
    p = api.rayscene_params()
    assert (p.cell_size, p.occupancy) == (0.0, 0)
    assert api.rayscene_params(0.0, -1).occupancy == -1 and api.rayscene_params(0.0, 7).occupancy == 7
    for kw in BAD_BUILD:
        with pytest.raises(ValueError):
            api.rayscene_params(**kw)
        with pytest.raises(ValueError):
            api.CUDASurfelReconstruction.BuildRayScene(rec, None, tri, **kw)
        with pytest.raises(ValueError):
            meshing.build_ray_scene(rec, tri, **kw)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.BuildRayScene(rec, None, np.arange(10, dtype=np.uint32), scene=_Untouchable())      # not three per triangle
    scene, rays = _Untouchable(), np.zeros((5, 6), np.float32)
    for kw in BAD_CAST:
        with pytest.raises(ValueError):
            api.RayScene.Cast(scene, None, rays, **kw)
        with pytest.raises(ValueError):
            meshing.cast_rays(rec, tri, rays[:, :3], rays[:, 3:], scene=scene, **kw)
    with pytest.raises(TypeError):
        api.RayScene.Cast(scene, None, rays, cell_size=0.05)            # a cast has no cell size: the scene's is fixed at the build
    closed = api.RayScene.__new__(api.RayScene)
    closed._h, closed.stats = None, None
    with pytest.raises(ValueError):
        closed.Cast(None, np.zeros(7, np.float32))                      # a closed scene; and not six per ray
    with pytest.raises(ValueError):
        closed.Cast(None, rays)
    closed.close()


def test_run_tum_mesh_eval_rays_frames_flag_and_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval_rays_frames", "3"]).mesh_eval_rays_frames == 3
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh_every", "4", "--mesh_eval_rays_frames", "2"]).mesh_eval_rays_frames == 2
    a = run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval_rays"])
    assert a.mesh_eval_rays_frames == 0 and a.mesh_eval_rays is True
    for argv in (["d", "--mesh", "--mesh_eval_rays_frames", "3"],                            # no ground truth
                 ["d", "--synthetic", "8", "--mesh_eval_rays_frames", "3"],                   # no mesh
                 ["d", "--synthetic", "8", "--mesh", "--mesh_eval_rays_frames", "-1"]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
    d = np.float32([[0, 0, 2], [0, 0, 4], [3, 0, 4]])
    hit, t = np.uint32([5, 0xFFFFFFFF, 7]), np.float32([1.001, np.inf, 0.998])
    assert run_tum.format_ray_eval(hit, t, d, 6, "scene rays") == "scene rays of frame 6: 2 of 3 rays hit the mesh (66.7 %): mean 6.00 mm, rms 7.21 mm"
    assert run_tum.format_ray_eval(hit, t, d, 6) == "surface error along the rays of frame 6: 2 of 3 rays hit the mesh (66.7 %): mean 6.00 mm, rms 7.21 mm"
