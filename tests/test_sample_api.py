"""The Python layer of SampleMesh and CompareMeshes without a GPU: parameter refusals, the PODs against the C header, the
summary of a comparison from hand-made words, and the flags of tools/run_tum.py."""
import ctypes
import os
import subprocess
import sys

import pytest

from common import ROOT


def test_parameters_are_refused_in_python():
    from surfelmeshing_amd import api
    assert api.sample_params(0) == (0, 0) and api.sample_params(1 << 28, 0xFFFFFFFF) == (1 << 28, 0xFFFFFFFF)
    for n, seed in ((-1, 0), ((1 << 28) + 1, 0), (1.5, 0), (True, 0), (10, -1), (10, 1 << 32), (10, 0.5), (10, True)):
        with pytest.raises(ValueError):
            api.sample_params(n, seed)
    p = api.compare_params(0.05, 1000, 7, 0.01, 2)
    assert abs(p.max_distance - 0.05) < 1e-8 and abs(p.cell_size - 0.01) < 1e-8 and (p.n_samples, p.seed, p.directions) == (1000, 7, 2)
    assert api.compare_params(0.001, 0).directions == 3
    for kw in (dict(max_distance=0.0), dict(max_distance=17.0), dict(max_distance=float("nan")), dict(cell_size=-1.0),
               dict(cell_size=float("inf")), dict(n_samples=(1 << 28) + 1), dict(n_samples=-1), dict(seed=1 << 32), dict(directions=0),
               dict(directions=4), dict(directions=True), dict(directions=1.5)):
        args = dict(max_distance=0.05, n_samples=100, seed=0, cell_size=0.0, directions=3)
        args.update(kw)
        with pytest.raises(ValueError):
            api.compare_params(**args)

    class Refuses:                       # the meshing helpers refuse before they touch the object
        def __getattr__(self, name):
            raise AssertionError("the object was reached: " + name)
    from surfelmeshing_amd import meshing
    with pytest.raises(ValueError):
        meshing.sample_mesh(Refuses(), None, -1)
    with pytest.raises(ValueError):
        meshing.compare_meshes(Refuses(), None, None, 0.0, 100)


def test_pod_sizes_match_the_header(tmp_path):
    src = tmp_path / "sample_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(smx_sample_stats), sizeof(smx_compare_params),\n'
                   '  sizeof(smx_compare_side), sizeof(smx_compare_stats), offsetof(smx_sample_stats, total_weight),\n'
                   '  offsetof(smx_compare_side, distance), offsetof(smx_compare_side, sum_d), SMX_SAMPLE_PHASES, SMX_COMPARE_PHASES);\n'
                   '  return 0; }\n')
    exe = tmp_path / "sample_probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    from surfelmeshing_amd._lib import COMPARE_PHASES, SAMPLE_PHASES, CompareParams, CompareSide, CompareStats, SampleStats
    assert got == [ctypes.sizeof(SampleStats), ctypes.sizeof(CompareParams), ctypes.sizeof(CompareSide), ctypes.sizeof(CompareStats),
                   SampleStats.total_weight.offset, CompareSide.distance.offset, CompareSide.sum_d.offset, SAMPLE_PHASES, COMPARE_PHASES]
    assert got[:4] == [48, 20, 248, 496]


def _side(n_samples, n_none, hist, max_bits, sum_d, sq_lo, sq_hi, max_distance=0.032):
    distance = dict(n_matched=sum(hist), histogram=hist, max_dist2_bits=max_bits, max_distance=max_distance, n_points=n_samples,
                    n_bad_points=n_none)
    return dict(sample=dict(n_samples=n_samples, n_none=n_none, n_in=12), distance=distance, sum_d=sum_d, sum_sq_lo=sq_lo, sum_sq_hi=sq_hi)


def test_comparison_summary_on_hand_made_words():
    import struct
    from surfelmeshing_amd import meshing
    bits = lambda v: struct.unpack("<I", struct.pack("<f", v))[0]                      # noqa: E731
    unit = 2.0 ** -20
    # four matched samples at 1, 1, 2 and 4 units of 2^-20 m in bins 0, 0, 0 and 3
    a = _side(4, 0, [3, 0, 0, 1] + [0] * 28, bits((4 * unit) ** 2), 8, 22, 0)
    # a square sum above 2^64: 2^28 samples at 2^24 units (16 m), one sample unmatched
    n = 1 << 28
    b = _side(n + 1, 1, [0] * 31 + [n], bits(256.0), n << 24, 0, n << 16, max_distance=16.0)
    assert (n << 16) << 32 > 1 << 64
    s = meshing.comparison_summary(dict(a_to_b=a, b_to_a=b))
    sa, sb = s["a_to_b"], s["b_to_a"]
    assert sa["matched_fraction"] == 1.0 and sa["mean"] == 2 * unit and sa["rms"] == (22 / 4) ** 0.5 * unit and sa["max"] == 4 * unit
    assert (sa["bin50"], sa["bin90"], sa["bin99"]) == (0, 3, 3) and sa["p50_below"] == 0.001 and sa["p99_below"] == 0.004
    assert sb["n_matched"] == n and sb["mean"] == 16.0 and sb["rms"] == 16.0 and sb["max"] == 16.0 and sb["p50_below"] == 16.0
    assert s["hausdorff"] == 16.0 and s["hausdorff_is_lower_bound"] is True
    # the bin edges are distance_summary's
    import numpy as np
    d = np.array([1, 1, 2, 4], np.float64) * unit
    ds = meshing.distance_summary(d, dict(a["distance"], n_points=4))
    assert all(sa[k] == ds[k] for k in ("bin50", "bin90", "bin99", "p50_below", "p90_below", "p99_below"))
    # every sample matched on both sides: the Hausdorff distance itself; a side not asked for is None
    zero = dict(sample=dict(n_samples=0, n_none=0, n_in=0), distance=dict(n_matched=0, histogram=[0] * 32, max_dist2_bits=0, max_distance=0.032),
                sum_d=0, sum_sq_lo=0, sum_sq_hi=0)
    s = meshing.comparison_summary(dict(a_to_b=a, b_to_a=zero))
    assert s["b_to_a"] is None and s["hausdorff"] == 4 * unit and s["hausdorff_is_lower_bound"] is False
    text = meshing.format_mesh_comparison(s, ("fine", "coarse"))
    assert "fine -> coarse: 4 of 4 samples matched" in text and "Hausdorff distance = 0.004 mm" in text and "coarse -> fine" not in text
    none = _side(5, 5, [0] * 32, 0, 0, 0, 0)
    s = meshing.comparison_summary(dict(a_to_b=none, b_to_a=a))
    assert s["a_to_b"]["mean"] is None and s["hausdorff"] == 4 * unit and s["hausdorff_is_lower_bound"] is True
    assert "0 of 5 samples matched" in meshing.format_mesh_comparison(s) and "Hausdorff distance >= " in meshing.format_mesh_comparison(s)


def test_run_tum_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_tum
    finally:
        sys.path.pop(0)
    a = run_tum.parse_args(["d", "--mesh", "--mesh_decimate", "0.05", "--mesh_compare_samples", "1000"])
    assert a.mesh_compare_samples == 1000 and a.mesh_compare_distance == 0.05
    a = run_tum.parse_args(["d", "--mesh_every", "4", "--mesh_fill_holes", "8", "--mesh_compare_samples", "10", "--mesh_compare_distance", "0.5"])
    assert a.mesh_compare_distance == 0.5
    a = run_tum.parse_args(["d", "--mesh", "--export_mesh_samples", "x.ply", "--mesh_samples", "5000"])
    assert a.export_mesh_samples == "x.ply" and a.mesh_samples == 5000 and a.mesh_compare_samples == 0
    for bad in (["d", "--mesh", "--mesh_compare_samples", "1000"],                              # no stage to compare across
                ["d", "--mesh_decimate", "0.05", "--mesh_compare_samples", "1000"],             # no mesh
                ["d", "--mesh", "--mesh_decimate", "0.05", "--mesh_compare_samples", "-1"],
                ["d", "--mesh", "--mesh_min_component", "5", "--mesh_compare_samples", "10", "--mesh_compare_distance", "0"],
                ["d", "--mesh", "--export_mesh_samples", "x.ply"], ["d", "--mesh", "--mesh_samples", "10"],
                ["d", "--export_mesh_samples", "x.ply", "--mesh_samples", "10"],
                ["d", "--mesh", "--export_mesh_samples", "x.ply", "--mesh_samples", str((1 << 28) + 1)]):
        with pytest.raises(SystemExit):
            run_tum.parse_args(bad)
