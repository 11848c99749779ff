"""smx_distscene without a GPU: the seven symbols are declared, exported and loadable and the new source is listed; header and
ctypes mirror agree on the two structs; the shim's DistanceScene builds with the plain host compiler; the defaults; the library
refuses bad arguments before anything is launched and the Python wrappers before anything reaches the library;
tools/run_tum.py --mesh_eval_frames."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_distscene_create", "smx_distscene_destroy", "smx_distscene_params_default", "smx_recon_build_distscene", "smx_distscene_query",
           "smx_recon_compare_to_distscene", "smx_distscene_debug_timings")
PARAMS = ("max_distance", "cell_size")
BUILD = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_wide", "n_entries", "n_cells", "cell_size_used", "max_distance", "device_bytes")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, build one scene of it, measure point set after point set, then a coarser mesh against it
size_t measure(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, const std::vector<std::vector<float>>& clouds) {
  MeshParams params;
  std::vector<u32> triangles, coarse, nearest;
  std::vector<float> distance, closest;
  smx_distance_params p;
  smx_distance_stats stats;
  smx_compare_side side;
  smx_distance_params_default(&p);
  p.max_distance = 0.01f;
  reconstruction.Triangulate(stream, params, &triangles);
  DistanceScene scene;
  reconstruction.BuildDistanceScene(stream, triangles, &scene, 0.05f);
  reconstruction.BuildDistanceScene(stream, triangles, &scene, 0.05f, 0.1f);
  size_t sum = scene.stats().n_entries + (size_t)scene.stats().device_bytes + (scene.handle() != nullptr) + (scene.stats().max_distance > 0.0f);
  for (const std::vector<float>& points : clouds) {
    scene.Query(stream, points, p, &nearest, &distance);
    scene.Query(stream, points, p, &nearest, &distance, &closest, &stats);
    sum += nearest.size() + closest.size() + stats.n_matched;
  }
  reconstruction.DecimateMesh(stream, triangles, 0.05f, &coarse);
  reconstruction.CompareToDistanceScene(stream, coarse, scene, 0.05f, 1000, 7, &side);
  return sum + (size_t)side.sum_d + side.distance.n_matched;
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


def test_distscene_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_distscene.hip" in build.SOURCES
    for f in ("smx_distscene.hip", "smx_distscene.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_structs_agree_between_header_and_ctypes(tmp_path):
    from surfelmeshing_amd import _lib
    from surfelmeshing_amd._lib import DistSceneParams, DistSceneStats
    src = tmp_path / "distscene_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*build_fn)(smx_recon, smx_stream, smx_distscene, const smx_distscene_params*, const uint32_t*, uint32_t, int32_t,\n'
                   '                        smx_distscene_stats*);\n'
                   'typedef int (*query_fn)(smx_distscene, smx_stream, const smx_distance_params*, const float*, uint32_t, uint32_t*, float*, float*,\n'
                   '                        int32_t, smx_distance_stats*);\n'
                   'typedef int (*compare_fn)(smx_recon, smx_stream, smx_distscene, float, uint32_t, uint32_t, const uint32_t*, uint32_t, int32_t,\n'
                   '                          smx_compare_side*);\n'
                   'typedef int (*create_fn)(int32_t, smx_distscene*);\n'
                   'typedef int (*destroy_fn)(smx_distscene);\n'
                   'typedef int (*timings_fn)(smx_distscene, float*, int32_t);\n'
                   'typedef int (*default_fn)(smx_distscene_params*);\n'
                   'int main() { build_fn b = &smx_recon_build_distscene; query_fn q = &smx_distscene_query; create_fn n = &smx_distscene_create;\n'
                   '  destroy_fn x = &smx_distscene_destroy; timings_fn g = &smx_distscene_debug_timings; default_fn d = &smx_distscene_params_default;\n'
                   '  compare_fn c = &smx_recon_compare_to_distscene;\n'
                   '  printf("%zu %zu %d %d", sizeof(smx_distscene_params), sizeof(smx_distscene_stats), SMX_DISTSCENE_PHASES,\n'
                   '         b != 0 && q != 0 && n != 0 && x != 0 && g != 0 && d != 0 && c != 0);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_distscene_params, %s));\n' % f for f in PARAMS) +
                   "".join('  printf(" %%zu", offsetof(smx_distscene_stats, %s));\n' % f for f in BUILD) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "distscene_probe")
    out = [int(v) for v in subprocess.run([str(tmp_path / "distscene_probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:4] == [8, 48, 5, 1]
    assert out[:3] == [ctypes.sizeof(DistSceneParams), ctypes.sizeof(DistSceneStats), _lib.DISTSCENE_PHASES]
    offs = out[4:]
    assert offs[:2] == [getattr(DistSceneParams, f).offset for f in PARAMS] == [0, 4]
    assert offs[2:] == [getattr(DistSceneStats, f).offset for f in BUILD] == list(range(0, 36, 4)) + [40]
    assert [n for n, _ in DistSceneStats._fields_] == list(BUILD) and [n for n, _ in DistSceneParams._fields_] == list(PARAMS)


def test_shim_distance_scene_compiles_and_links(tmp_path):
    src = tmp_path / "distscene_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "distscene_caller")


def test_the_default_parameters():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    p = _lib.DistSceneParams(7.0, 7.0)
    assert L.smx_distscene_params_default(ctypes.byref(p)) == 0
    assert (p.max_distance, p.cell_size) == (float(np.float32(0.05)), 0.0)
    assert L.smx_distscene_params_default(None) == -1


def test_the_library_refuses_bad_arguments_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    st, bst, side = _lib.DistanceStats(), _lib.DistSceneStats(), _lib.CompareSide()
    good, pts = _lib.DistanceParams(0.02, 0.0, 0), np.zeros(12, np.float32)
    GUARD = 0xA5A5A5A5
    nearest, distance = np.full(4, GUARD, np.uint32), np.full(4, GUARD, np.uint32).view(np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    fake = ctypes.c_void_p(16)            # stands for an object: a refusal comes before anything looks at it

    def query(sc, prm):
        return L.smx_distscene_query(sc, None, ctypes.byref(prm) if prm is not None else None, ptr(pts), ctypes.c_uint32(4), ptr(nearest),
                                     ptr(distance), None, ctypes.c_int32(0), ctypes.byref(st))

    def build(r, sc, prm, tri=None, n_in=0):
        return L.smx_recon_build_distscene(r, None, sc, ctypes.byref(prm) if prm is not None else None, tri, ctypes.c_uint32(n_in),
                                           ctypes.c_int32(0), ctypes.byref(bst))
    # a query on NULL, without parameters, with a cell size, outside 1e-3 .. 16
    assert query(None, good) == -1 and query(fake, None) == -1
    for bad in (_lib.DistanceParams(0.02, 0.05, 0), _lib.DistanceParams(0.0005, 0.0, 0), _lib.DistanceParams(17.0, 0.0, 0),
                _lib.DistanceParams(float("nan"), 0.0, 0), _lib.DistanceParams(0.02, 0.0, 2)):
        assert query(fake, bad) == -1
    assert np.all(nearest == GUARD) and np.all(distance.view(np.uint32) == GUARD)
    # a build without a scene looks at nothing
    assert build(fake, None, _lib.DistSceneParams(0.05, 0.0)) == -1
    assert L.smx_distscene_create(ctypes.c_int32(-1), None) == -1 and L.smx_distscene_destroy(None) == 0
    assert L.smx_distscene_debug_timings(None, None, ctypes.c_int32(5)) == -1
    assert L.smx_recon_compare_to_distscene(None, None, None, ctypes.c_float(0.05), ctypes.c_uint32(10), ctypes.c_uint32(0), None, ctypes.c_uint32(0),
                                            ctypes.c_int32(0), ctypes.byref(side)) == -1
    assert L.smx_recon_compare_to_distscene(fake, None, fake, ctypes.c_float(0.05), ctypes.c_uint32(10), ctypes.c_uint32(0), None, ctypes.c_uint32(0),
                                            ctypes.c_int32(0), None) == -1
    if _lib.device_count() == 0:        # no fall-back: without a device there is no scene
        with pytest.raises(_lib.SmxError):
            api.DistanceScene()
        return
    # with a scene: the build's own refusals come before the object is looked at
    with api.DistanceScene() as sc:
        tri = np.zeros(3, np.uint32)
        assert build(None, sc._h, _lib.DistSceneParams(0.05, 0.0)) == -1 and build(fake, sc._h, None) == -1
        for bad in (_lib.DistSceneParams(0.0005, 0.0), _lib.DistSceneParams(16.5, 0.0), _lib.DistSceneParams(float("nan"), 0.0),
                    _lib.DistSceneParams(0.05, -0.1), _lib.DistSceneParams(0.05, float("nan")), _lib.DistSceneParams(0.05, float("inf"))):
            assert build(fake, sc._h, bad) == -1
        ok = _lib.DistSceneParams(0.05, 0.0)
        assert build(fake, sc._h, ok, ptr(tri), 2 ** 28 + 1) == -1 and build(fake, sc._h, ok, None, 1) == -1
        assert query(sc._h, good) == -1                                   # never built: empty
        assert np.all(nearest == GUARD) and np.all(distance.view(np.uint32) == GUARD)


class _Untouchable:
    """Stands for a reconstruction or a scene: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)


BAD_BUILD = [dict(max_distance=0.0005), dict(max_distance=17.0), dict(max_distance=float("nan")), dict(max_distance=float("inf")),
             dict(max_distance=0.05, cell_size=-0.1), dict(max_distance=0.05, cell_size=float("nan")), dict(max_distance=0.05, cell_size=float("inf"))]
BAD_QUERY = [dict(max_distance=0.0005), dict(max_distance=17.0), dict(max_distance=float("nan")), dict(max_distance=0.02, signed=2)]


def test_the_python_wrappers_refuse_bad_arguments_before_the_library():
    from surfelmeshing_amd import api, meshing
    rec, tri = _Untouchable(), np.arange(12, dtype=np.uint32).reshape(4, 3)
    p = api.distscene_params(0.5, 0.75)
    assert (p.max_distance, p.cell_size) == (0.5, 0.75)
    assert api.distscene_params(0.05).cell_size == 0.0
    for kw in BAD_BUILD:
        with pytest.raises(ValueError):
            api.distscene_params(**kw)
        with pytest.raises(ValueError):
            api.CUDASurfelReconstruction.BuildDistanceScene(rec, None, tri, **kw)
        with pytest.raises(ValueError):
            meshing.build_distance_scene(rec, tri, **kw)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.BuildDistanceScene(rec, None, np.arange(10, dtype=np.uint32), 0.05, scene=_Untouchable())   # not three per triangle
    scene, pts = _Untouchable(), np.zeros((5, 3), np.float32)
    for kw in BAD_QUERY:
        with pytest.raises(ValueError):
            api.DistanceScene.Query(scene, None, pts, **kw)
        with pytest.raises(ValueError):
            meshing.mesh_distance(rec, tri, pts, scene=scene, **kw)
        if "signed" not in kw:
            with pytest.raises(ValueError):
                api.CUDASurfelReconstruction.CompareToDistanceScene(rec, None, tri, scene, kw["max_distance"], 10)
    with pytest.raises(TypeError):
        api.DistanceScene.Query(scene, None, pts, 0.02, cell_size=0.05)    # a query has no cell size: the scene's is fixed at the build
    for n_samples, seed in ((-1, 0), (2 ** 28 + 1, 0), (1.5, 0), (10, 2 ** 32)):
        with pytest.raises(ValueError):
            api.CUDASurfelReconstruction.CompareToDistanceScene(rec, None, tri, scene, 0.05, n_samples, seed)
    # a scene built for 0.02 m refuses 0.05 m; a closed scene and a scene without a build refuse everything
    built = api.DistanceScene.__new__(api.DistanceScene)
    built._h, built.stats = _Untouchable(), dict(max_distance=float(np.float32(0.02)), device_bytes=123)
    assert built.device_bytes == 123
    with pytest.raises(ValueError):
        built.Query(None, pts, 0.05)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.CompareToDistanceScene(rec, None, tri, built, 0.05, 10)
    with pytest.raises(ValueError):
        meshing.compare_meshes(rec, tri, tri, 0.05, 10, directions=1, scene_b=built)
    with pytest.raises(ValueError):
        built.Query(None, np.zeros(7, np.float32), 0.02)                   # not three per point
    built._h = None
    closed = api.DistanceScene.__new__(api.DistanceScene)
    closed._h, closed.stats = None, None
    assert closed.device_bytes == 0
    for sc in (closed, built):
        with pytest.raises(ValueError):
            sc.Query(None, pts, 0.02)
    with pytest.raises(ValueError):
        closed.Query(None, pts)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.CompareToDistanceScene(rec, None, tri, closed, 0.05, 10)
    closed.close()


def test_run_tum_mesh_eval_frames_flag_and_lines():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval", "0.05", "--mesh_eval_frames", "3"]).mesh_eval_frames == 3
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh_every", "4", "--mesh_eval", "0.05", "--mesh_eval_frames", "2"]).mesh_eval_frames == 2
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval", "0.05"]).mesh_eval_frames == 0
    for argv in (["d", "--synthetic", "8", "--mesh", "--mesh_eval_frames", "3"],                                      # no --mesh_eval
                 ["d", "--mesh", "--mesh_decimate", "0.05", "--mesh_eval", "0.05", "--mesh_eval_frames", "3"],       # no ground truth
                 ["d", "--synthetic", "8", "--mesh_eval", "0.05", "--mesh_eval_frames", "3"],                        # no mesh
                 ["d", "--synthetic", "8", "--mesh", "--mesh_eval", "0.05", "--mesh_eval_frames", "-1"]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
    from surfelmeshing_amd import meshing
    hist = [0] * 32
    a = dict(n_points=3, n_bad_points=0, n_matched=2, max_dist2_bits=5, histogram=hist[:1] + [2] + hist[2:], max_distance=0.05, n_in=9)
    b = dict(n_points=2, n_bad_points=1, n_matched=1, max_dist2_bits=9, histogram=[1] + hist[1:], max_distance=0.05, n_in=9)
    m = run_tum.merge_distance_stats([a, b])
    assert (m["n_points"], m["n_bad_points"], m["n_matched"], m["max_dist2_bits"], m["n_in"]) == (5, 1, 3, 9, 9)
    assert m["histogram"][:3] == [1, 2, 0] and m["max_distance"] == 0.05
    d = np.float32([0.002, np.inf, 0.003, 0.001, np.inf])
    line = run_tum.format_point_eval(meshing.distance_summary(d, m), "2 frames")
    assert line == "scene points of 2 frames: " + meshing.format_distance_summary(meshing.distance_summary(d, m))
    assert line.startswith("scene points of 2 frames: 3 of 5 points matched (60.0 %): mean 2.00 mm")
    assert run_tum.format_point_eval(meshing.distance_summary(d[:3], a), "frame 6").startswith("scene points of frame 6: 2 of 3 points matched")
