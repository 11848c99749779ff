"""smx_recon_raycast_mesh without a GPU: the three symbols are declared, exported and loadable; header and ctypes mirror agree on
the two structs; the shim's RaycastMesh builds with the plain host compiler; the defaults; the Python wrappers refuse bad
arguments before anything reaches the library, and the library refuses them before anything is launched; camera_rays against a
2 x 2 case computed by hand; tools/run_tum.py --mesh_eval_rays."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_raycast_params_default", "smx_recon_raycast_mesh", "smx_recon_debug_raycast_timings")
HEAD = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_rays", "n_bad_rays", "n_hit", "n_front_hits", "max_t_bits", "n_wide",
        "n_entries", "n_cells", "cell_size_used", "reserved")
TAIL = ("n_layers", "n_lookups", "n_pair_tests")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, make a coarser level, ask what a handful of rays hit first on it
size_t cast(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, const std::vector<float>& rays) {
  MeshParams params;
  std::vector<u32> triangles, coarse, hit;
  std::vector<float> t, uv;
  smx_raycast_params p;
  smx_raycast_stats stats;
  smx_raycast_params_default(&p);
  p.t_max = 1.0f;
  p.cull = 1;
  reconstruction.Triangulate(stream, params, &triangles);
  reconstruction.DecimateMesh(stream, triangles, 0.05f, &coarse);
  reconstruction.RaycastMesh(stream, coarse, rays, p, &hit, &t);
  reconstruction.RaycastMesh(stream, coarse, rays, p, &hit, &t, &uv, &stats);
  return hit.size() + uv.size() + stats.n_hit + (size_t)stats.n_pair_tests;
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


def test_raycast_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_raycast.hip" in build.SOURCES
    for f in ("smx_raycast.hip", "smx_raycast.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_structs_agree_between_header_and_ctypes(tmp_path):
    from surfelmeshing_amd import _lib
    from surfelmeshing_amd._lib import RaycastParams, RaycastStats
    import raycast_ref as rr
    par = ("t_min", "t_max", "cell_size", "cull")
    src = tmp_path / "raycast_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*cast_fn)(smx_recon, smx_stream, const smx_raycast_params*, const uint32_t*, uint32_t, const float*, uint32_t,\n'
                   '                       uint32_t*, float*, float*, int32_t, smx_raycast_stats*);\n'
                   'typedef int (*timings_fn)(smx_recon, float*, int32_t);\n'
                   'typedef int (*default_fn)(smx_raycast_params*);\n'
                   'int main() { cast_fn f = &smx_recon_raycast_mesh; timings_fn g = &smx_recon_debug_raycast_timings;\n'
                   '  default_fn d = &smx_raycast_params_default;\n'
                   '  printf("%zu %zu %d %d", sizeof(smx_raycast_params), sizeof(smx_raycast_stats), SMX_RAY_PHASES, f != 0 && g != 0 && d != 0);\n'
                   '  printf(" %.9g %.9g %.9g %.9g %.9g", (double)SMX_RAY_MAX_DIR, (double)SMX_RAY_MIN_DIR, (double)SMX_RAY_MAX_T,\n'
                   '         (double)SMX_RAY_BOX_SLACK, (double)SMX_RAY_MIN_CELL);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_raycast_params, %s));\n' % f for f in par) +
                   "".join('  printf(" %%zu", offsetof(smx_raycast_stats, %s));\n' % f for f in HEAD + TAIL) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "raycast_probe")
    out = subprocess.run([str(tmp_path / "raycast_probe")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:4]] == [16, 80, 4, 1]
    assert [int(out[0]), int(out[1]), int(out[2])] == [ctypes.sizeof(RaycastParams), ctypes.sizeof(RaycastStats), _lib.RAY_PHASES]
    consts = [float(v) for v in out[4:9]]
    assert consts == [_lib.RAY_MAX_DIR, _lib.RAY_MIN_DIR, _lib.RAY_MAX_T, _lib.RAY_BOX_SLACK, _lib.RAY_MIN_CELL] == [1024.0, 2.0 ** -10, 2.0 ** 20, 2.0 ** -12, 2.0 ** -9]
    assert consts == [float(rr.MAX_DIR), float(rr.MIN_DIR), float(rr.MAX_T), float(rr.SLACK), float(rr.MIN_CELL)]
    offs = [int(v) for v in out[9:]]
    assert offs[:4] == [getattr(RaycastParams, f).offset for f in par] == [0, 4, 8, 12]
    assert offs[4:] == [getattr(RaycastStats, f).offset for f in HEAD + TAIL] == list(range(0, 56, 4)) + [56, 64, 72]
    assert [n for n, _ in RaycastStats._fields_] == list(HEAD + TAIL)
    assert tuple(rr.STAT_NAMES) == HEAD[:9] and tuple(rr.WORK_NAMES) == TAIL and rr.WIDE_CELLS == _lib.DIST_WIDE_CELLS


def test_shim_raycast_mesh_compiles_and_links(tmp_path):
    src = tmp_path / "raycast_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "raycast_caller")


def test_the_default_parameters():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    p = _lib.RaycastParams(7.0, 7.0, 7.0, 7)
    assert L.smx_raycast_params_default(ctypes.byref(p)) == 0
    assert (p.t_min, p.t_max, p.cell_size, p.cull) == (0.0, 2.0 ** 20, 0.0, 0)
    assert L.smx_raycast_params_default(None) == -1


def test_the_library_refuses_bad_arguments_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    st = _lib.RaycastStats()
    sentinel = ctypes.c_void_p(16)      # stands for an object: never dereferenced, the arguments are refused before
    both = np.arange(36, dtype=np.uint32)
    tri, rays = both[:12], np.zeros(24, np.float32)
    GUARD = 0xA5A5A5A5
    hit, t, uv = np.full(4, GUARD, np.uint32), np.full(4, GUARD, np.uint32).view(np.float32), np.full(8, GUARD, np.uint32).view(np.float32)
    good = _lib.RaycastParams(0.0, 1.0, 0.0, 0)

    def call(r, p=good, tin=tri, n_in=4, rin=rays, n_rays=4, o0=hit, o1=t, o2=uv):
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        return L.smx_recon_raycast_mesh(r, None, None if p is None else ctypes.byref(p), ptr(tin), ctypes.c_uint32(n_in), ptr(rin),
                                        ctypes.c_uint32(n_rays), ptr(o0), ptr(o1), ptr(o2), ctypes.c_int32(0), ctypes.byref(st))
    assert call(None) == -1
    assert call(sentinel, p=None) == -1
    nan, inf = float("nan"), float("inf")
    for t0, t1 in ((-1.0, 1.0), (2.0, 1.0), (0.0, 2.0 ** 20 + 1.0), (nan, 1.0), (0.0, nan), (0.0, inf), (-inf, 1.0)):
        assert call(sentinel, p=_lib.RaycastParams(t0, t1, 0.0, 0)) == -1 and b"t_m" in L.smx_last_error(), (t0, t1)
    for c in (-1.0, nan, inf, -0.001):
        assert call(sentinel, p=_lib.RaycastParams(0.0, 1.0, c, 0)) == -1 and b"cell_size" in L.smx_last_error()
    for s in (3, -1):
        assert call(sentinel, p=_lib.RaycastParams(0.0, 1.0, 0.0, s)) == -1 and b"cull" in L.smx_last_error()
    assert call(sentinel, n_in=(1 << 28) + 1) == -1 and call(sentinel, n_rays=(1 << 28) + 1) == -1
    assert call(sentinel, tin=None) == -1 and call(sentinel, rin=None) == -1
    assert call(sentinel, o0=None) == -1 and call(sentinel, o1=None) == -1
    # an output over an input, whole or by one element
    for kw in (dict(o0=tri), dict(o1=rays), dict(o2=rays), dict(o0=both[11:]), dict(o2=both.view(np.float32)[11:])):
        assert call(sentinel, **kw) == -1 and b"overlaps" in L.smx_last_error(), kw
    assert np.all(hit == GUARD) and np.all(t.view(np.uint32) == GUARD) and np.all(uv.view(np.uint32) == GUARD)
    assert np.array_equal(both, np.arange(36, dtype=np.uint32))
    assert L.smx_recon_debug_raycast_timings(None, None, ctypes.c_int32(4)) == -1
    buf = (ctypes.c_float * 4)()
    assert L.smx_recon_debug_raycast_timings(sentinel, buf, ctypes.c_int32(3)) == -1
    if _lib.device_count() == 0:        # no fall-back: without a device there is no object to cast on
        with pytest.raises(_lib.SmxError):
            api.CUDASurfelReconstruction(1000, api.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))


class _Untouchable:
    """Stands for a reconstruction: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)


BAD = [dict(t_min=-0.5), dict(t_min=2.0, t_max=1.0), dict(t_max=2.0 ** 21), dict(t_min=float("nan")), dict(t_max=float("inf")),
       dict(cell_size=-0.1), dict(cell_size=float("nan")), dict(cell_size=float("inf")), dict(cull=3), dict(cull=-1), dict(cull=True)]


def test_the_python_wrappers_refuse_bad_arguments_before_the_library():
    from surfelmeshing_amd import api, meshing
    rec, tri = _Untouchable(), np.arange(12, dtype=np.uint32).reshape(4, 3)
    o, d = np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32)
    p = api.raycast_params(0.25, 16.0, 0.5, 2)
    assert (p.t_min, p.t_max, p.cell_size, p.cull) == (0.25, 16.0, 0.5, 2)
    p = api.raycast_params()
    assert (p.t_min, p.t_max, p.cell_size, p.cull) == (0.0, 2.0 ** 20, 0.0, 0)
    for kw in BAD:
        with pytest.raises(ValueError):
            api.raycast_params(**kw)
        with pytest.raises(ValueError):
            api.CUDASurfelReconstruction.RaycastMesh(rec, None, tri, np.concatenate([o, d], axis=1), **kw)
        with pytest.raises(ValueError):
            meshing.cast_rays(rec, tri, o, d, **kw)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.RaycastMesh(rec, None, np.arange(10, dtype=np.uint32), np.zeros((5, 6), np.float32))      # not three per triangle
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.RaycastMesh(rec, None, tri, np.zeros(7, np.float32))                                      # not six per ray
    with pytest.raises(ValueError):
        meshing.cast_rays(rec, tri, o, d[:4])                                                                                   # not one direction per origin
    with pytest.raises(ValueError):
        meshing.camera_rays(10.0, 10.0, 1.0, 1.0, 0, 2, np.eye(4)[:3])


def test_camera_rays_against_a_2_x_2_case_computed_by_hand():
    from surfelmeshing_amd import meshing
    # the camera at (1, 2, 3), turned a quarter about y: its x axis is the world's -z, its z axis the world's +x
    T = np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 2.0], [-1.0, 0.0, 0.0, 3.0]])
    o, d = meshing.camera_rays(2.0, 4.0, 1.0, 1.0, 2, 2, T)
    assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == (4, 3) and d.shape == (4, 3)
    assert np.array_equal(o, np.tile(np.float32([1.0, 2.0, 3.0]), (4, 1)))
    # pixel (x, y): local = ((x + 0.5 - 1) / 2, (y + 0.5 - 1) / 4, 1) = (-+0.25, -+0.125, 1); world = (local_z, local_y, -local_x); row by row
    want = np.float32([[1.0, -0.125, 0.25], [1.0, -0.125, -0.25], [1.0, 0.125, 0.25], [1.0, 0.125, -0.25]])
    assert np.array_equal(d, want)
    # with the identity pose the z component is 1: t is the camera depth
    o, d = meshing.camera_rays(525.0, 525.0, 320.0, 240.0, 640, 480, np.eye(4)[:3])
    assert d.shape == (640 * 480, 3) and np.all(d[:, 2] == 1.0) and np.all(o == 0.0)
    assert d[0, 0] == np.float32((0.5 - 320.0) / 525.0) and d[641, 1] == np.float32((1.5 - 240.0) / 525.0)


def test_run_tum_mesh_eval_rays_flag_and_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval_rays"]).mesh_eval_rays is True
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh_every", "4", "--mesh_eval_rays"]).mesh_eval_rays is True
    assert run_tum.parse_args(["d", "--synthetic", "8", "--mesh"]).mesh_eval_rays is False
    for argv in (["d", "--mesh", "--mesh_eval_rays"],                           # no ground truth
                 ["d", "--synthetic", "8", "--mesh_eval_rays"]):                  # no mesh
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
    d = np.float32([[0, 0, 2], [0, 0, 4], [3, 0, 4]])
    line = run_tum.format_ray_eval(np.uint32([5, 0xFFFFFFFF, 7]), np.float32([1.001, np.inf, 0.998]), d, 6)
    assert line == "surface error along the rays of frame 6: 2 of 3 rays hit the mesh (66.7 %): mean 6.00 mm, rms 7.21 mm"
    assert run_tum.format_ray_eval(np.uint32([0xFFFFFFFF]), np.float32([np.inf]), d[:1], 6).endswith("0 of 1 rays hit the mesh")
