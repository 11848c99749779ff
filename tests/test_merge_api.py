"""smx_recon_merge_map at the boundary, without a device: the parameter defaults, the struct sizes against the header, and every
refusal that looks at no object (the library checks the parameters before it touches either map)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import ROOT
from surfelmeshing_amd import _lib, api, meshing

FLT_MAX = float(np.finfo(np.float32).max)


def test_parameter_defaults():
    p = _lib.MergeParams.defaults()
    assert (p.cell_size, p.radius_factor_squared, p.max_normal_angle_deg) == (np.float32(0.05), 1.0, 30.0)
    assert (p.k, p.mode, p.frame_index) == (8, 0, 1) and p.confidence_cap == FLT_MAX
    q = api.merge_params()
    assert bytes(q) == bytes(p)
    q = api.merge_params(mode="blend", k=64, confidence_cap=7.5, frame_index=12, max_normal_angle_deg=180.0)
    assert (q.mode, q.k, q.confidence_cap, q.frame_index, q.max_normal_angle_deg) == (1, 64, 7.5, 12, 180.0)
    assert _lib.load().smx_merge_params_default(None) != 0
    with pytest.raises(AttributeError):
        _lib.MergeParams.defaults(no_such_field=1)


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "merge_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(smx_merge_params), sizeof(smx_merge_stats),\n'
                   '  offsetof(smx_merge_params, frame_index), offsetof(smx_merge_stats, new_size), SMX_MERGE_KEEP_DST, SMX_MERGE_BLEND,\n'
                   '  SMX_MERGE_PHASES); return 0; }\n')
    exe = tmp_path / "merge_probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.MergeParams), C.sizeof(_lib.MergeStats), _lib.MergeParams.frame_index.offset, _lib.MergeStats.new_size.offset,
                   _lib.MERGE_MODES["keep"], _lib.MERGE_MODES["blend"], _lib.MERGE_PHASES]
    assert got[:2] == [28, 40] and len(_lib.MERGE_PHASE_NAMES) == _lib.MERGE_PHASES + 1
    assert [n for n, _ in _lib.MergeStats._fields_] == ["n_src_slots", "n_src_live", "n_bad", "n_matched", "n_appended", "n_blended_dst",
                                                        "n_saturated", "links_dropped", "old_size", "new_size"]


def _call(dst, nn, src, T, p):
    st = _lib.MergeStats()
    return _lib.load().smx_recon_merge_map(dst, None, nn, src, T, p, None, C.c_uint32(0), C.c_int32(0), C.byref(st))


def test_refusals_that_need_no_device():
    """NULL pointers and bad parameters are refused before either object is looked at: the handles here are never read."""
    a, b, n = (C.create_string_buffer(1 << 16) for _ in range(3))     # stand-ins for two maps and an index
    A, B, NN = (C.cast(x, C.c_void_p) for x in (a, b, n))
    T = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    good = _lib.MergeParams.defaults()
    INVALID = -1
    for args in ((None, NN, B, T, C.byref(good)), (A, None, B, T, C.byref(good)), (A, NN, None, T, C.byref(good)), (A, NN, B, None, C.byref(good)),
                 (A, NN, B, T, None)):
        assert _call(*args) == INVALID
    bad = [dict(k=0), dict(k=65), dict(frame_index=0), dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=float("nan")),
           dict(radius_factor_squared=0.0), dict(radius_factor_squared=float("nan")), dict(max_normal_angle_deg=-1.0),
           dict(max_normal_angle_deg=180.5), dict(max_normal_angle_deg=float("nan")), dict(mode=2), dict(mode=-1),
           dict(confidence_cap=float("nan"))]
    for kw in bad:
        assert _call(A, NN, B, T, C.byref(_lib.MergeParams.defaults(**kw))) == INVALID, kw
        assert b"invalid argument" in _lib.load().smx_last_error()
    for k, v in ((3, float("nan")), (0, float("inf")), (11, -float("inf"))):
        Tb = (C.c_float * 12)(*T)
        Tb[k] = v
        assert _call(A, NN, B, Tb, C.byref(good)) == INVALID
    assert _call(A, NN, A, T, C.byref(good)) == INVALID               # src == dst
    assert _lib.load().smx_recon_debug_merge_timings(None, (C.c_float * 8)(), 8) == INVALID
    assert _lib.load().smx_recon_debug_merge_timings(A, None, 8) == INVALID
    assert _lib.load().smx_recon_debug_set_merge_chunk(None, 4) == INVALID


def test_python_layer_refuses_what_the_library_would():
    for kw in (dict(k=0), dict(k=65), dict(frame_index=0), dict(cell_size=0.0), dict(radius_factor_squared=-1.0), dict(max_normal_angle_deg=181.0),
               dict(mode="average"), dict(mode=2), dict(confidence_cap=float("nan"))):
        with pytest.raises(ValueError):
            api.merge_params(**kw)
    assert api.merge_stats_dict(_lib.MergeStats(*range(10)))["new_size"] == 9
    with pytest.raises(ValueError):
        meshing.remap_triangles([[0, 1, 5]], np.zeros(3, np.uint32))
    assert meshing.remap_triangles(np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32)).shape == (0, 3)


SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a second session into the first under the pose a registration found; the second session's mesh follows through the map
size_t merge_and_remap(cudaStream_t stream, CUDASurfelReconstruction& first, CUDASurfelReconstruction& second, const float* first_T_second,
                       std::vector<u32>* triangles) {
  smx_merge_params p;
  smx_merge_params_default(&p);
  p.mode = SMX_MERGE_BLEND;
  p.frame_index = 100;
  std::vector<u32> src_to_dst;
  smx_merge_stats stats;
  first.MergeMap(stream, second, first_T_second, p, &src_to_dst, nullptr, &stats);
  std::vector<u32> kept;
  for (size_t t = 0; t + 2 < triangles->size(); t += 3) {
    u32 v[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const u32 i = (*triangles)[t + k];
      v[k] = i < src_to_dst.size() ? src_to_dst[i] : 0xFFFFFFFFu;
      ok = ok && v[k] != 0xFFFFFFFFu;
    }
    if (ok) kept.insert(kept.end(), v, v + 3);
  }
  triangles->swap(kept);
  first.MergeMap(stream, second, first_T_second, p);   // (without the map)
  return stats.n_appended;
}
int main() { return 0; }
'''


def test_shim_merge_compiles_and_links(tmp_path):
    from surfelmeshing_amd import build
    build.build(verbose=False)
    src = tmp_path / "merge_caller.cc"
    src.write_text(SHIM_SRC)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(tmp_path / "merge_caller"), "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir,
                        "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_run_tum_merge_flags_and_lines():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import run_tum
    a = run_tum.parse_args(["folder", "--synthetic", "40", "--merge_split", "20", "--merge_mode", "blend", "--mesh", "--mesh_eval", "0.05"])
    assert (a.merge_split, a.merge_mode) == (20, "blend")
    assert run_tum.parse_args(["folder"]).merge_split == 0 and run_tum.parse_args(["folder"]).merge_mode == "keep"
    for bad in (["--merge_split", "-1"], ["--merge_split", "5", "--track"], ["--merge_split", "5", "--mesh_every", "3"], ["--merge_mode", "average"]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(["folder"] + bad)
    res = {"scene_T_points": np.eye(4, dtype=np.float32)[:3], "status": 0, "iterations_run": 7, "inliers": 1234}
    assert run_tum.format_merge_register_line(res).endswith("0.000 mrad and 0.000 mm from the identity")
    names = ("whole", "build", "move", "query_select", "number", "append", "blend", "finish")
    line = run_tum.format_merge_line("keep", {"n_matched": 5, "n_appended": 7}, 1.25, dict.fromkeys(names, 0.5))
    assert line.startswith("merged (keep) in 1.2 ms") or line.startswith("merged (keep) in 1.3 ms")
    assert line.endswith("n_matched 5, n_appended 7")
