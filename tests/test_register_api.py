"""smx_distscene_register without a GPU: the four symbols are declared, exported and loadable and the new source is listed;
header and ctypes mirror agree on the three structs; the shim's DistanceScene::Register builds with the plain host compiler;
the defaults; the library refuses bad arguments before it looks at the scene and the Python wrappers before anything reaches
the library; tools/run_tum.py --mesh_eval_register."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_register_params_default", "smx_distscene_register", "smx_distscene_debug_register_iterations", "smx_distscene_debug_register_timings")
PARAMS = ("level_stride", "level_iterations", "level_max_distance", "max_normal_angle_deg", "convergence_rotation", "convergence_translation",
          "min_inliers", "min_inlier_fraction", "min_pivot_ratio")
RESULT = ("scene_T_points", "status", "iterations_run", "inliers", "points_used", "rms_residual", "last_update_rotation", "last_update_translation",
          "information")
ITERATION = ("level", "stride", "status", "reserved", "Tf", "sums", "x")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, build one scene of it, align scan after scan to it
float align(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, const std::vector<std::vector<float>>& scans,
            const std::vector<float>& normals) {
  MeshParams params;
  std::vector<u32> triangles;
  reconstruction.Triangulate(stream, params, &triangles);
  DistanceScene scene;
  reconstruction.BuildDistanceScene(stream, triangles, &scene, 0.05f);
  smx_register_params p;
  smx_register_params_default(&p);
  p.level_max_distance[2] = 0.01f;
  const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  smx_register_result result;
  float sum = 0.0f;
  for (const std::vector<float>& points : scans) {
    scene.Register(stream, points, nullptr, p, identity, &result);
    scene.Register(stream, points, &normals, p, result.scene_T_points, &result);
    sum += result.rms_residual + (float)result.inliers + (result.status == SMX_TRACK_CONVERGED ? 1.0f : 0.0f);
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


def test_register_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_register.hip" in build.SOURCES
    for f in ("smx_register.hip", "smx_register.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_structs_agree_between_header_and_ctypes(tmp_path):
    from surfelmeshing_amd import _lib
    from surfelmeshing_amd._lib import RegisterIteration, RegisterParams, RegisterResult
    src = tmp_path / "register_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*reg_fn)(smx_distscene, smx_stream, const smx_register_params*, const float*, const float*, uint32_t, int32_t,\n'
                   '                      const float*, smx_register_result*, int32_t);\n'
                   'typedef int (*its_fn)(smx_distscene, smx_stream, smx_register_iteration*, int32_t, int32_t*);\n'
                   'typedef int (*timings_fn)(smx_distscene, float*, int32_t);\n'
                   'typedef int (*default_fn)(smx_register_params*);\n'
                   'int main() { reg_fn r = &smx_distscene_register; its_fn i = &smx_distscene_debug_register_iterations;\n'
                   '  timings_fn g = &smx_distscene_debug_register_timings; default_fn d = &smx_register_params_default;\n'
                   '  printf("%zu %zu %zu %d %d %d", sizeof(smx_register_params), sizeof(smx_register_result), sizeof(smx_register_iteration),\n'
                   '         SMX_REGISTER_SUMS, SMX_REGISTER_PHASES, r != 0 && i != 0 && g != 0 && d != 0);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_register_params, %s));\n' % f for f in PARAMS) +
                   "".join('  printf(" %%zu", offsetof(smx_register_result, %s));\n' % f for f in RESULT) +
                   "".join('  printf(" %%zu", offsetof(smx_register_iteration, %s));\n' % f for f in ITERATION) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "register_probe")
    out = [int(v) for v in subprocess.run([str(tmp_path / "register_probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:6] == [60, 220, 360, 31, 5, 1]
    assert out[:5] == [ctypes.sizeof(RegisterParams), ctypes.sizeof(RegisterResult), ctypes.sizeof(RegisterIteration), _lib.REGISTER_SUMS, _lib.REGISTER_PHASES]
    offs = out[6:]
    assert offs[:9] == [getattr(RegisterParams, f).offset for f in PARAMS] == [0, 12, 24, 36, 40, 44, 48, 52, 56]
    assert offs[9:18] == [getattr(RegisterResult, f).offset for f in RESULT] == [0, 48, 52, 56, 60, 64, 68, 72, 76]
    assert offs[18:] == [getattr(RegisterIteration, f).offset for f in ITERATION] == [0, 4, 8, 12, 16, 64, 312]
    assert [n for n, _ in RegisterParams._fields_] == list(PARAMS) and [n for n, _ in RegisterResult._fields_] == list(RESULT)
    assert [n for n, _ in RegisterIteration._fields_] == list(ITERATION)


def test_shim_register_compiles_and_links(tmp_path):
    src = tmp_path / "register_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "register_caller")


def test_the_default_parameters():
    from surfelmeshing_amd import _lib, meshing
    L = _lib.load()
    p = _lib.RegisterParams()
    ctypes.memset(ctypes.byref(p), 0x5A, ctypes.sizeof(p))
    assert L.smx_register_params_default(ctypes.byref(p)) == 0
    f = lambda v: float(np.float32(v))                                   # noqa: E731
    assert (list(p.level_stride), list(p.level_iterations), list(p.level_max_distance)) == ([4, 2, 1], [4, 5, 10], [0.0, 0.0, 0.0])
    assert (p.max_normal_angle_deg, p.convergence_rotation, p.convergence_translation) == (30.0, f(1e-5), f(1e-5))
    assert (p.min_inliers, p.min_inlier_fraction, p.min_pivot_ratio) == (50, f(0.1), f(1e-6))
    assert L.smx_register_params_default(None) == -1
    # the tracker's thresholds
    t = _lib.TrackParams.defaults()
    for k in ("max_normal_angle_deg", "convergence_rotation", "convergence_translation", "min_inliers", "min_inlier_fraction", "min_pivot_ratio"):
        assert getattr(p, k) == getattr(t, k), k
    assert (list(t.level_stride), list(t.level_iterations)) == (list(p.level_stride), list(p.level_iterations))
    # the helper: the defaults, levels with and without a distance, fields by name
    assert bytes(meshing.register_params()) == bytes(p)
    q = meshing.register_params(levels=[(8, 3), (1, 7, 0.01)], min_inliers=5, max_normal_angle_deg=45.0)
    assert (list(q.level_stride), list(q.level_iterations), list(q.level_max_distance)) == ([8, 1, 1], [3, 7, 0], [0.0, f(0.01), 0.0])
    assert (q.min_inliers, q.max_normal_angle_deg) == (5, 45.0)
    assert list(meshing.register_params(level_stride=(5, 6, 7)).level_stride) == [5, 6, 7]
    with pytest.raises(AttributeError):
        meshing.register_params(max_distance=0.1)
    with pytest.raises(ValueError):
        meshing.register_params(levels=[(1, 2)] * 4)
    with pytest.raises(ValueError):
        meshing.register_params(levels=[(1,)])


def _call(L, sc, prm, pts, n, T, out, nrm=None):
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    return L.smx_distscene_register(sc, None, ctypes.byref(prm) if prm is not None else None, ptr(pts), ptr(nrm), ctypes.c_uint32(n),
                                    ctypes.c_int32(0), ptr(T), ctypes.byref(out) if out is not None else None, ctypes.c_int32(0))


def _bad_params():
    from surfelmeshing_amd._lib import RegisterParams as P
    d = P.defaults
    yield "no level with iterations", d(levels=[(1, 0)])
    yield "33 iterations", d(levels=[(1, 33)])
    yield "negative iterations", d(level_iterations=(-1, 1, 1))
    yield "stride 0", d(levels=[(0, 1)])
    yield "stride 65537", d(levels=[(65537, 1)])
    yield "negative stride", d(levels=[(-4, 1)])
    yield "distance below 1e-3", d(levels=[(1, 1, 0.0005)])
    yield "negative distance", d(levels=[(1, 1, -0.01)])
    yield "distance NaN", d(levels=[(1, 1, float("nan"))])
    yield "distance inf", d(levels=[(1, 1, float("inf"))])
    yield "distance above 16", d(levels=[(1, 1, 17.0)])
    yield "angle 0", d(max_normal_angle_deg=0.0)
    yield "angle negative", d(max_normal_angle_deg=-30.0)
    yield "angle above 180", d(max_normal_angle_deg=181.0)
    yield "angle NaN", d(max_normal_angle_deg=float("nan"))
    yield "negative convergence rotation", d(convergence_rotation=-1e-5)
    yield "negative convergence translation", d(convergence_translation=-1e-5)
    yield "negative min_inliers", d(min_inliers=-1)
    yield "fraction above 1", d(min_inlier_fraction=1.5)
    yield "negative fraction", d(min_inlier_fraction=-0.1)
    yield "negative pivot ratio", d(min_pivot_ratio=-1e-6)


def test_the_library_refuses_bad_arguments_before_it_looks_at_the_scene():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    good = _lib.RegisterParams.defaults()
    pts, T = np.zeros((4, 3), np.float32), np.eye(3, 4, dtype=np.float32)
    out = _lib.RegisterResult()
    ctypes.memset(ctypes.byref(out), 0xA5, ctypes.sizeof(out))
    untouched = lambda: bytes(out) == b"\xa5" * ctypes.sizeof(out)                 # noqa: E731
    fake = ctypes.c_void_p(16)            # stands for a scene: a refusal comes before anything looks at it
    assert _call(L, None, good, pts, 4, T, out) == -1 and _call(L, fake, None, pts, 4, T, out) == -1
    assert _call(L, fake, good, pts, 4, None, out) == -1 and _call(L, fake, good, pts, 4, T, None) == -1
    assert _call(L, fake, good, None, 4, T, out) == -1                              # points == NULL with n > 0
    assert _call(L, fake, good, pts, 2 ** 28 + 1, T, out) == -1
    for k in range(12):
        for v in (np.nan, np.inf, -np.inf):
            bad = T.copy()
            bad.reshape(-1)[k] = v
            assert _call(L, fake, good, pts, 4, bad, out) == -1, (k, v)
    for what, prm in _bad_params():
        assert _call(L, fake, prm, pts, 4, T, out) == -1, what
        assert b"invalid argument" in L.smx_last_error(), what
    assert untouched()
    # an unused level may hold anything
    loose = _lib.RegisterParams.defaults(levels=[(1, 1)], level_stride=(1, 0, -7), level_max_distance=(0.0, -1.0, float("nan")))
    recs, count = (_lib.RegisterIteration * 2)(), ctypes.c_int32(7)
    assert L.smx_distscene_debug_register_iterations(None, None, recs, ctypes.c_int32(2), ctypes.byref(count)) == -1
    assert L.smx_distscene_debug_register_iterations(fake, None, None, ctypes.c_int32(2), ctypes.byref(count)) == -1
    assert L.smx_distscene_debug_register_iterations(fake, None, recs, ctypes.c_int32(-1), ctypes.byref(count)) == -1
    assert L.smx_distscene_debug_register_iterations(fake, None, recs, ctypes.c_int32(2), None) == -1
    ms = (ctypes.c_float * 5)()
    assert L.smx_distscene_debug_register_timings(None, ms, ctypes.c_int32(5)) == -1
    assert L.smx_distscene_debug_register_timings(fake, None, ctypes.c_int32(5)) == -1
    assert L.smx_distscene_debug_register_timings(fake, ms, ctypes.c_int32(4)) == -1
    if _lib.device_count() == 0:
        return
    with api.DistanceScene() as sc:       # a scene without a build: empty, refused; its loose level is not what is wrong
        assert _call(L, sc._h, loose, pts, 4, T, out) == -1 and b"empty scene" in L.smx_last_error() and untouched()
        assert L.smx_distscene_debug_register_iterations(sc._h, None, recs, ctypes.c_int32(2), ctypes.byref(count)) == 0 and count.value == 0
        assert L.smx_distscene_debug_register_timings(sc._h, ms, ctypes.c_int32(5)) == 0 and list(ms) == [0.0] * 5


class _Untouchable:
    """Stands for a scene's handle: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)


def test_the_python_wrappers_refuse_bad_arguments_before_the_library():
    from surfelmeshing_amd import api, meshing
    pts = np.zeros((5, 3), np.float32)
    built = api.DistanceScene.__new__(api.DistanceScene)
    built._h, built.stats = _Untouchable(), dict(max_distance=float(np.float32(0.02)), device_bytes=1)
    for what, prm in _bad_params():
        with pytest.raises(ValueError):
            built.Register(None, pts, params=prm)
        with pytest.raises(ValueError):
            meshing.register_points(built, pts, params=prm)
    with pytest.raises(ValueError):       # a gate above the bound of the build
        built.Register(None, pts, params=meshing.register_params(levels=[(1, 1, 0.05)]))
    api.register_check_params(meshing.register_params(levels=[(1, 1, 0.02)]), built.stats["max_distance"])
    api.register_check_params(meshing.register_params(levels=[(1, 1)], level_stride=(1, 0, -7)), 0.02)        # an unused level may hold anything
    for bad_T in (np.zeros(11), np.full((3, 4), np.nan), np.eye(4)):
        with pytest.raises(ValueError):
            built.Register(None, pts, T_init=bad_T)
    with pytest.raises(ValueError):
        built.Register(None, np.zeros(7, np.float32))                     # not three per point
    with pytest.raises(ValueError):
        built.Register(None, pts, normals=np.zeros((4, 3), np.float32))   # not one normal per point
    built._h = None
    closed = api.DistanceScene.__new__(api.DistanceScene)
    closed._h, closed.stats = None, None
    for sc in (closed, built):
        with pytest.raises(ValueError):
            sc.Register(None, pts)
    unbuilt = api.DistanceScene.__new__(api.DistanceScene)
    unbuilt._h, unbuilt.stats = _Untouchable(), None
    with pytest.raises(ValueError):
        meshing.register_points(unbuilt, pts)
    unbuilt._h = None
    # the result as a dict
    from surfelmeshing_amd._lib import RegisterResult
    r = RegisterResult()
    r.scene_T_points[:] = list(range(12))
    r.status, r.inliers, r.information[7] = 1, 9, 2.5
    d = api.register_result_dict(r)
    assert d["scene_T_points"].shape == (3, 4) and d["scene_T_points"][1, 0] == 4 and d["status"] == 1 and d["inliers"] == 9
    assert d["information"].shape == (6, 6) and d["information"][1, 1] == 2.5 and set(d) == set(RESULT)


def test_run_tum_mesh_eval_register_flag_and_lines():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval", "0.05", "--mesh_eval_register"]).mesh_eval_register
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh_every", "4", "--mesh_eval", "0.05", "--mesh_eval_frames", "2", "--mesh_eval_register"]).mesh_eval_register
    assert not run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval", "0.05"]).mesh_eval_register
    for argv in (["d", "--synthetic", "8", "--mesh", "--mesh_eval_register"],                                      # no --mesh_eval
                 ["d", "--mesh", "--mesh_decimate", "0.05", "--mesh_eval", "0.05", "--mesh_eval_register"],       # no ground truth
                 ["d", "--synthetic", "8", "--mesh_eval", "0.05", "--mesh_eval_register"]):                       # no mesh
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
    T = np.eye(3, 4)
    c, s = np.cos(0.002), np.sin(0.002)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:, 3] = [0.003, 0.0, -0.004]
    res = dict(scene_T_points=T.astype(np.float32), status=1, iterations_run=7)
    fig = run_tum.register_figures(res, dict(mean=0.004, rms=0.005), dict(mean=0.001, rms=None))
    assert abs(fig["mrad"] - 2.0) < 1e-3 and abs(fig["mm"] - 5.0) < 1e-3 and fig["mean"] == (4.0, 1.0) and fig["rms"] == (5.0, 0.0)
    line = run_tum.format_register_line(6, fig)
    assert line.startswith("registered frame 6: status 1 after 7 iterations, 2.000 mrad and 5.000 mm from the identity; surface error 4.000 -> 1.000 mm mean")
    lost = dict(fig, status=3)
    assert run_tum.format_register_total([fig, lost]).startswith("registered 2 frames: 1 solved, mean 2.000 mrad and 5.000 mm from the identity; surface error 4.000 -> 1.000 mm mean")
    assert run_tum.format_register_total([]).startswith("registered 0 frames: 0 solved")
