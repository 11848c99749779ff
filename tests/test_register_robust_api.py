"""smx_distscene_register_robust, smx_recon_build_distscene_rim and smx_recon_register_mesh without a GPU: the symbols are
declared, exported and loadable; header and ctypes mirror agree on smx_register_robust_params; the defaults; every refusal that
needs no device comes before the scene is looked at, as in the plain call; the shim's methods build with the plain host compiler
under -Wall -Werror; the Python helpers refuse what they can before they reach the library; new keywords default to what the
helpers did before."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_recon_build_distscene_rim", "smx_register_robust_params_default", "smx_distscene_register_robust",
           "smx_distscene_debug_register_robust_counts", "smx_recon_register_mesh")


def test_symbols_and_struct(tmp_path):
    from surfelmeshing_amd import _lib
    L = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTS and getattr(L, s) is not None
    src = tmp_path / "robust_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu", sizeof(smx_register_robust_params), offsetof(smx_register_robust_params, kernel),\n'
                   '  offsetof(smx_register_robust_params, level_scale), offsetof(smx_register_robust_params, reject_rim)); return 0; }\n')
    exe = tmp_path / "robust_probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _lib.RegisterRobustParams
    assert got == [ctypes.sizeof(P), P.kernel.offset, P.level_scale.offset, P.reject_rim.offset] == [20, 0, 4, 16]


def test_the_defaults():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    p = _lib.RegisterRobustParams(7, (ctypes.c_float * 3)(7, 7, 7), 7)
    assert L.smx_register_robust_params_default(ctypes.byref(p)) == 0
    assert (p.kernel, list(p.level_scale), p.reject_rim) == (0, [0.0, 0.0, 0.0], 0)
    assert L.smx_register_robust_params_default(None) == -1
    q = api.register_robust_params()
    assert bytes(q) == bytes(p)
    q = api.register_robust_params("tukey", 0.004, True)
    assert (q.kernel, q.reject_rim) == (2, 1) and np.allclose(list(q.level_scale), 0.004)
    q = api.register_robust_params(kernel=1, scale=(0.01, 0.0, 0.002))
    assert q.kernel == 1 and np.allclose(list(q.level_scale), [0.01, 0.0, 0.002]) and q.reject_rim == 0


def test_refusals_come_before_the_scene_is_looked_at():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    sentinel = ctypes.c_void_p(0x1000)           # never dereferenced: every case below is refused before the scene is looked at
    prm = _lib.RegisterParams.defaults()
    pts = np.zeros((4, 3), np.float32)
    T = np.eye(3, 4, dtype=np.float32)
    out = _lib.RegisterResult()

    def call(rp, params=prm, points=pts, n=4, T_=T, sc=sentinel):
        return L.smx_distscene_register_robust(sc, None, ctypes.byref(params), None if rp is None else ctypes.byref(rp),
                                               None if points is None else points.ctypes.data_as(ctypes.c_void_p), None, ctypes.c_uint32(n), ctypes.c_int32(0),
                                               T_.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out), ctypes.c_int32(0))
    R = _lib.RegisterRobustParams
    three = lambda v: (ctypes.c_float * 3)(v, v, v)                                    # noqa: E731
    assert call(None) == -1 and b"rp" in L.smx_last_error()
    assert call(R(0, three(0), 0), sc=None) == -1
    for kernel in (-1, 3, 100):
        assert call(R(kernel, three(0.01), 0)) == -1 and b"kernel" in L.smx_last_error()
    for rim in (-1, 2):
        assert call(R(0, three(0), rim)) == -1 and b"reject_rim" in L.smx_last_error()
    for c in (-0.001, 1e-7, 16.5, float("nan"), float("inf")):
        for kernel in (1, 2):
            assert call(R(kernel, three(c), 0)) == -1, (kernel, c)
    # what the plain call refuses, before the robust part is looked at or after it: still before the scene
    assert call(R(1, three(0.01), 0), n=(1 << 28) + 1) == -1
    assert call(R(1, three(0.01), 0), points=None) == -1
    bad = T.copy()
    bad[1, 2] = np.nan
    assert call(R(1, three(0.01), 0), T_=bad) == -1
    assert call(R(1, three(0.01), 0), params=_lib.RegisterParams.defaults(levels=[(0, 3)])) == -1
    # the counts, and the mesh call
    n = ctypes.c_int32(5)
    assert L.smx_distscene_debug_register_robust_counts(None, None, None, ctypes.c_int32(0), ctypes.byref(n)) == -1
    assert L.smx_distscene_debug_register_robust_counts(sentinel, None, None, ctypes.c_int32(4), ctypes.byref(n)) == -1
    rp = R(0, three(0), 0)
    mesh = lambda r, sc, n_in, n_samples, rp_: L.smx_recon_register_mesh(r, None, sc, None, ctypes.c_uint32(n_in), ctypes.c_int32(0),      # noqa: E731
                                                                         ctypes.c_uint32(n_samples), ctypes.c_uint32(0), ctypes.byref(prm),
                                                                         None if rp_ is None else ctypes.byref(rp_), T.ctypes.data_as(ctypes.c_void_p),
                                                                         ctypes.byref(out), ctypes.c_int32(0))
    assert mesh(None, sentinel, 0, 10, rp) == -1 and mesh(sentinel, None, 0, 10, rp) == -1 and mesh(sentinel, sentinel, 0, 10, None) == -1
    assert L.smx_recon_build_distscene_rim(sentinel, None, None, None, None, ctypes.c_uint32(0), ctypes.c_int32(0), None, None) == -1


SHIM_PROGRAM = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: a scene with a rim of one mesh, another mesh registered to it in one call, a point set with weights
int aligned(cudaStream_t stream, CUDASurfelReconstruction& target, CUDASurfelReconstruction& source, const std::vector<float>& points) {
  MeshParams params;
  std::vector<u32> target_mesh, source_mesh;
  target.Triangulate(stream, params, &target_mesh);
  source.Triangulate(stream, params, &source_mesh);
  DistanceScene scene;
  target.BuildDistanceSceneRim(stream, target_mesh, &scene, 0.05f);
  smx_register_params p;
  smx_register_robust_params rp;
  smx_register_params_default(&p);
  smx_register_robust_params_default(&rp);
  rp.kernel = 2; rp.level_scale[0] = 0.02f; rp.level_scale[1] = 0.01f; rp.level_scale[2] = 0.005f; rp.reject_rim = 1;
  const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  smx_register_result a, b;
  source.RegisterMesh(stream, scene, source_mesh, 100000, 1, p, rp, identity, &a);
  scene.RegisterRobust(stream, points, nullptr, p, rp, a.scene_T_points, &b);
  return a.status + b.status + (int)scene.rim_stats().n_rim_edges;
}
int main() { return 0; }
'''


def test_the_shim_compiles_and_links(tmp_path):
    src = tmp_path / "robust_caller.cc"
    src.write_text(SHIM_PROGRAM)
    lib = os.path.join(ROOT, "surfelmeshing_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lsmx",
                        "-Wl,-rpath," + lib, "-o", str(tmp_path / "robust_caller")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_python_helpers_refuse_before_the_library_and_default_to_the_plain_call():
    from surfelmeshing_amd import api, meshing
    for kw in (dict(kernel="cauchy"), dict(kernel=3), dict(kernel=-1), dict(kernel=True), dict(kernel=1.5), dict(scale=-1.0), dict(scale=17.0),
               dict(scale=float("nan")), dict(scale=1e-7), dict(scale=(0.1, 0.1)), dict(reject_rim=2), dict(reject_rim="yes")):
        with pytest.raises(ValueError):
            meshing.register_robust_params(**kw)

    class Scene:                       # records how the helpers call it
        _h, stats, has_rim = 1, dict(max_distance=0.05), False

        def Register(self, *a, **kw):
            return ("Register", a, kw)
    sc = Scene()
    prm = meshing.register_params()
    assert meshing.register_points(sc, "p", params=prm) == ("Register", (None, "p", None, None, prm), {})          # as before
    rp = meshing.register_robust_params(kernel="huber", scale=0.01)
    assert meshing.register_points(sc, "p", params=prm, robust=rp) == ("Register", (None, "p", None, None, prm), dict(robust=rp))

    class Rec:
        def BuildDistanceScene(self, *a, **kw):
            return ("Build", a, kw)

        def RegisterMesh(self, *a):
            return ("Mesh", a)
    assert meshing.build_distance_scene(Rec(), "t", 0.05) == ("Build", (None, "t", 0.05, 0.0), {})                 # as before
    assert meshing.build_distance_scene(Rec(), "t", 0.05, rim=True) == ("Build", (None, "t", 0.05, 0.0), dict(rim=True))
    assert meshing.register_mesh(Rec(), sc, "t", 100, seed=3, params=prm, robust=rp) == ("Mesh", (None, sc, "t", 100, 3, None, prm, rp))
    # the wrapper itself: reject_rim on a scene without a rim, a robust that is no struct
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        api.DistanceScene.Register(sc, None, pts, robust=meshing.register_robust_params(reject_rim=True))
    with pytest.raises(ValueError):
        api.DistanceScene.Register(sc, None, pts, robust=dict(kernel=1))

    class Closed:
        _h, stats, has_rim = None, None, False
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.RegisterMesh(object(), None, Closed(), np.zeros((1, 3), np.uint32), 10)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.RegisterMesh(object(), None, sc, np.zeros((1, 3), np.uint32), -1)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.RegisterMesh(object(), None, sc, np.zeros((1, 3), np.uint32), 10, robust=meshing.register_robust_params(reject_rim=True))


def test_run_tum_flags():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_tum
    base = ["d", "--synthetic", "6", "--mesh", "--mesh_eval", "0.05", "--mesh_eval_register"]
    assert run_tum.parse_args(base).mesh_eval_register_robust is None
    a = run_tum.parse_args(base + ["--mesh_eval_register_reject_rim"])
    assert a.mesh_eval_register_robust == dict(kernel="none", scale=0.0, reject_rim=True)
    a = run_tum.parse_args(base + ["--mesh_eval_register_kernel", "tukey", "--mesh_eval_register_scale", "0.004", "--mesh_eval_register_reject_rim"])
    assert a.mesh_eval_register_robust == dict(kernel="tukey", scale=0.004, reject_rim=True)
    a = run_tum.parse_args(base + ["--mesh_eval_register_kernel", "huber", "--mesh_eval_register_scale", "0.002"])
    assert a.mesh_eval_register_robust == dict(kernel="huber", scale=0.002, reject_rim=False)
    for argv in (base[:-1] + ["--mesh_eval_register_reject_rim"], base + ["--mesh_eval_register_kernel", "huber"],
                 base + ["--mesh_eval_register_scale", "0.1"], base + ["--mesh_eval_register_kernel", "cauchy", "--mesh_eval_register_scale", "0.1"],
                 base + ["--mesh_eval_register_kernel", "tukey", "--mesh_eval_register_scale", "17"],
                 base + ["--mesh_eval_register_kernel", "tukey", "--mesh_eval_register_scale", "0"]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
    fig = dict(status=1, iterations=5, mrad=0.5, mm=0.25, mean=(1.0, 0.5), rms=(2.0, 1.0))
    line = run_tum.format_robust_register_line(3, fig, (12, 7))
    assert line.startswith("robustly registered frame 3: status 1 after 5 iterations") and line.endswith("last iteration: 12 on the rim, 7 weighted or rejected")
