"""smx_recon_mesh_distance without a GPU: the three symbols are declared, exported and loadable; header and ctypes mirror agree on
the two structs; the shim's MeshDistance builds with the plain host compiler; the Python wrappers refuse bad arguments before
anything reaches the library, and the library refuses them before anything is launched; distance_summary on a made-up array;
SyntheticStream.surface_points; tools/run_tum.py --mesh_eval."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

SYMBOLS = ("smx_distance_params_default", "smx_recon_mesh_distance", "smx_recon_debug_distance_timings")
HEAD = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_points", "n_bad_points", "n_matched", "max_dist2_bits")
TAIL = ("n_wide", "n_entries", "n_cells", "cell_size_used")

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a caller's side: mesh the map, make a coarser level, ask how far the fine vertices lie from it
size_t measured(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, const std::vector<float>& points) {
  MeshParams params;
  std::vector<u32> triangles, coarse, nearest;
  std::vector<float> distance, closest;
  smx_distance_params p;
  smx_distance_stats stats;
  smx_distance_params_default(&p);
  p.max_distance = 0.1f;
  p.signed_distance = 1;
  reconstruction.Triangulate(stream, params, &triangles);
  reconstruction.DecimateMesh(stream, triangles, 0.05f, &coarse);
  reconstruction.MeshDistance(stream, coarse, points, p, &nearest, &distance);
  reconstruction.MeshDistance(stream, coarse, points, p, &nearest, &distance, &closest, &stats);
  return nearest.size() + closest.size() + stats.n_matched + stats.histogram[SMX_DIST_BINS - 1];
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


def test_distance_is_declared_exported_and_its_source_listed():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in SYMBOLS:
        assert name in _declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "smx_distance.hip" in build.SOURCES
    for f in ("smx_distance.hip", "smx_distance.hpp"):
        assert os.path.exists(os.path.join(ROOT, "surfelmeshing_amd", "csrc", f))


def test_structs_agree_between_header_and_ctypes(tmp_path):
    from surfelmeshing_amd import _lib
    from surfelmeshing_amd._lib import DIST_BINS, DIST_MAX_COORD, DIST_PHASES, DIST_WIDE_CELLS, DistanceParams, DistanceStats
    import distance_ref as dr
    par = ("max_distance", "cell_size", "signed_distance")
    src = tmp_path / "distance_probe.cc"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx_shim.hpp"\n'
                   'typedef int (*dist_fn)(smx_recon, smx_stream, const smx_distance_params*, const uint32_t*, uint32_t, const float*, uint32_t,\n'
                   '                       uint32_t*, float*, float*, int32_t, smx_distance_stats*);\n'
                   'typedef int (*timings_fn)(smx_recon, float*, int32_t);\n'
                   'typedef int (*default_fn)(smx_distance_params*);\n'
                   'int main() { dist_fn f = &smx_recon_mesh_distance; timings_fn g = &smx_recon_debug_distance_timings;\n'
                   '  default_fn d = &smx_distance_params_default;\n'
                   '  printf("%zu %zu %d %d %d %d %d", sizeof(smx_distance_params), sizeof(smx_distance_stats), SMX_DIST_PHASES, SMX_DIST_BINS,\n'
                   '         SMX_DIST_WIDE_CELLS, (int)SMX_DIST_MAX_COORD, f != 0 && g != 0 && d != 0);\n' +
                   "".join('  printf(" %%zu", offsetof(smx_distance_params, %s));\n' % f for f in par) +
                   "".join('  printf(" %%zu", offsetof(smx_distance_stats, %s));\n' % f for f in HEAD + ("histogram",) + TAIL) +
                   '  printf("\\n"); return 0; }\n')
    _gxx(src, tmp_path / "distance_probe")
    got = [int(v) for v in subprocess.run([str(tmp_path / "distance_probe")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:7] == [12, 176, 4, 32, 64, 64, 1]
    assert got[:6] == [ctypes.sizeof(DistanceParams), ctypes.sizeof(DistanceStats), DIST_PHASES, DIST_BINS, DIST_WIDE_CELLS, int(DIST_MAX_COORD)]
    assert got[7:10] == [getattr(DistanceParams, f).offset for f in par] == [0, 4, 8]
    assert got[10:] == [getattr(DistanceStats, f).offset for f in HEAD + ("histogram",) + TAIL] == list(range(0, 36, 4)) + [160, 164, 168, 172]
    assert [n for n, _ in DistanceStats._fields_] == list(HEAD + ("histogram",) + TAIL)
    assert tuple(dr.STAT_NAMES) == HEAD and dr.BINS == DIST_BINS and dr.WIDE_CELLS == DIST_WIDE_CELLS and float(dr.MAX_COORD) == DIST_MAX_COORD
    assert _lib.DIST_PHASES == 4


def test_shim_mesh_distance_compiles_and_links(tmp_path):
    src = tmp_path / "distance_caller.cc"
    src.write_text(SHIM_SRC)
    _gxx(src, tmp_path / "distance_caller")


def test_the_default_parameters():
    from surfelmeshing_amd import _lib
    L = _lib.load()
    p = _lib.DistanceParams(7.0, 7.0, 7)
    assert L.smx_distance_params_default(ctypes.byref(p)) == 0
    assert (p.max_distance, p.cell_size, p.signed_distance) == (float(np.float32(0.05)), 0.0, 0)
    assert L.smx_distance_params_default(None) == -1


def test_the_library_refuses_bad_arguments_and_no_device_is_loud():
    from surfelmeshing_amd import _lib, api
    L = _lib.load()
    st = _lib.DistanceStats()
    sentinel = ctypes.c_void_p(16)      # stands for an object: never dereferenced, the arguments are refused before
    both = np.arange(24, dtype=np.uint32)
    tri, pts = both[:12], np.zeros(12, np.float32)
    GUARD = 0xA5A5A5A5
    nearest, distance, closest = np.full(4, GUARD, np.uint32), np.full(4, GUARD, np.uint32).view(np.float32), np.full(12, GUARD, np.uint32).view(np.float32)
    good = _lib.DistanceParams(0.05, 0.0, 0)

    def call(r, p=good, tin=tri, n_in=4, pin=pts, n_points=4, o0=nearest, o1=distance, o2=closest):
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        return L.smx_recon_mesh_distance(r, None, None if p is None else ctypes.byref(p), ptr(tin), ctypes.c_uint32(n_in), ptr(pin),
                                         ctypes.c_uint32(n_points), ptr(o0), ptr(o1), ptr(o2), ctypes.c_int32(0), ctypes.byref(st))
    assert call(None) == -1
    assert call(sentinel, p=None) == -1
    for m in (0.0, 0.0009, 16.5, -1.0, float("nan"), float("inf")):
        assert call(sentinel, p=_lib.DistanceParams(m, 0.0, 0)) == -1 and b"max_distance" in L.smx_last_error()
    for c in (-1.0, float("nan"), float("inf"), -0.001):
        assert call(sentinel, p=_lib.DistanceParams(0.05, c, 0)) == -1 and b"cell_size" in L.smx_last_error()
    for s in (2, -1):
        assert call(sentinel, p=_lib.DistanceParams(0.05, 0.0, s)) == -1 and b"signed_distance" in L.smx_last_error()
    assert call(sentinel, n_in=(1 << 28) + 1) == -1 and call(sentinel, n_points=(1 << 28) + 1) == -1
    assert call(sentinel, tin=None) == -1 and call(sentinel, pin=None) == -1
    assert call(sentinel, o0=None) == -1 and call(sentinel, o1=None) == -1
    # an output over an input, whole or by one element
    for kw in (dict(o0=tri), dict(o1=pts), dict(o2=pts), dict(o0=both[11:]), dict(o2=both.view(np.float32)[11:])):
        assert call(sentinel, **kw) == -1 and b"overlaps" in L.smx_last_error(), kw
    assert np.all(nearest == GUARD) and np.all(distance.view(np.uint32) == GUARD) and np.all(closest.view(np.uint32) == GUARD)
    assert np.array_equal(both, np.arange(24, dtype=np.uint32))
    assert L.smx_recon_debug_distance_timings(None, None, ctypes.c_int32(4)) == -1
    buf = (ctypes.c_float * 4)()
    assert L.smx_recon_debug_distance_timings(sentinel, buf, ctypes.c_int32(3)) == -1
    if _lib.device_count() == 0:        # no fall-back: without a device there is no object to measure on
        with pytest.raises(_lib.SmxError):
            api.CUDASurfelReconstruction(1000, api.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))


class _Untouchable:
    """Stands for a reconstruction: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the wrapper reached for .%s before it had checked its arguments" % name)


BAD = [dict(max_distance=0.0), dict(max_distance=0.0005), dict(max_distance=17.0), dict(max_distance=float("nan")), dict(max_distance=float("inf")),
       dict(max_distance=0.05, cell_size=-0.1), dict(max_distance=0.05, cell_size=float("nan")), dict(max_distance=0.05, cell_size=float("inf")),
       dict(max_distance=0.05, signed=2)]


def test_the_python_wrappers_refuse_bad_arguments_before_the_library():
    from surfelmeshing_amd import api, meshing
    rec, tri, pts = _Untouchable(), np.arange(12, dtype=np.uint32).reshape(4, 3), np.zeros((5, 3), np.float32)
    p = api.distance_params(16.0, 0.25, True)
    assert (p.max_distance, p.cell_size, p.signed_distance) == (16.0, 0.25, 1)
    p = api.distance_params(1e-3)
    assert (p.max_distance, p.cell_size, p.signed_distance) == (float(np.float32(1e-3)), 0.0, 0)
    for kw in BAD:
        with pytest.raises(ValueError):
            api.distance_params(**kw)
        with pytest.raises(ValueError):
            api.CUDASurfelReconstruction.MeshDistance(rec, None, tri, pts, **kw)
        with pytest.raises(ValueError):
            meshing.mesh_distance(rec, tri, pts, **kw)
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.MeshDistance(rec, None, np.arange(10, dtype=np.uint32), pts, 0.05)      # not three per triangle
    with pytest.raises(ValueError):
        api.CUDASurfelReconstruction.MeshDistance(rec, None, tri, np.zeros(7, np.float32), 0.05)             # not three per point


def test_distance_summary_on_a_made_up_array():
    from surfelmeshing_amd import meshing
    from surfelmeshing_amd._lib import DIST_BINS
    max_distance = 0.032                                   # a bin per millimetre
    d = np.full(200, np.inf, np.float32)
    d[:100] = (np.arange(100) % 10 + 0.5) * 1e-3           # ten points in each of the bins 0 .. 9
    d[1:100:2] *= -1.0                                     # signed: the summary is over magnitudes
    hist = [10] * 10 + [0] * (DIST_BINS - 10)
    stats = dict(n_points=200, n_matched=100, histogram=hist, max_distance=max_distance)
    s = meshing.distance_summary(d, stats)
    m = np.abs(d[:100].astype(np.float64))
    assert s["n_points"] == 200 and s["n_matched"] == 100 and s["matched_fraction"] == 0.5
    assert s["mean"] == float(m.mean()) and s["rms"] == float(np.sqrt((m * m).mean())) and s["max"] == float(m.max())
    assert (s["bin50"], s["bin90"], s["bin99"]) == (4, 8, 9)
    assert s["p50_below"] == pytest.approx(0.005) and s["p90_below"] == pytest.approx(0.009) and s["p99_below"] == pytest.approx(0.010)
    line = meshing.format_distance_summary(s)
    assert "100 of 200 points matched (50.0 %)" in line and "mean 5.00 mm" in line and "5.00 mm / 9.00 mm / 10.00 mm" in line
    none = meshing.distance_summary(np.full(3, np.inf, np.float32), dict(n_points=3, n_matched=0, histogram=[0] * DIST_BINS, max_distance=0.1))
    assert none["mean"] is None and none["bin50"] is None and meshing.format_distance_summary(none) == "0 of 3 points matched"
    with pytest.raises(ValueError):
        meshing.distance_summary(d, dict(stats, n_matched=99))        # not of one call


def test_surface_points_are_the_noise_free_hits():
    from common import small_stream
    s = small_stream()
    z, hit = s._raycast(3)
    pts = s.surface_points(3, 8)
    assert pts.dtype == np.float32 and pts.shape == (int(np.isfinite(z[::8, ::8]).sum()), 3) and pts.shape[0] == 20 * 15
    assert np.array_equal(pts, hit[::8, ::8][np.isfinite(z[::8, ::8])].astype(np.float32))
    assert s.surface_points(3).shape[0] == 160 * 120
    # on the room's surface: within the relief and its offset of a wall
    from surfelmeshing_amd import synth
    gap = np.min(np.abs(synth.ROOM_HALF[None, :] - np.abs(pts.astype(np.float64))), axis=1)
    assert np.all(gap < 0.03 + synth.RELIEF_AMPLITUDE + 1e-6)


def test_run_tum_mesh_eval_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    a = run_tum.parse_args(["d", "--synthetic", "8", "--mesh", "--mesh_eval", "0.05"])
    assert a.mesh_eval == 0.05
    a = run_tum.parse_args(["d", "--mesh", "--mesh_decimate", "0.1", "--mesh_eval", "0.2"])
    assert a.mesh_eval == 0.2 and a.mesh_decimate == 0.1
    assert run_tum.parse_args(["d", "--mesh"]).mesh_eval is None
    for argv in (["d", "--mesh", "--mesh_eval", "0.05"],                       # neither --synthetic nor --mesh_decimate
                 ["d", "--synthetic", "8", "--mesh_eval", "0.05"],                  # no mesh
                 ["d", "--synthetic", "8", "--mesh", "--mesh_eval", "0.0005"], ["d", "--synthetic", "8", "--mesh", "--mesh_eval", "17"],
                 ["d", "--synthetic", "8", "--mesh", "--mesh_eval", "nan"]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(argv)
