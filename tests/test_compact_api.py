"""Map compaction without a GPU: smx_recon_compact is declared and exported, the shim's Compact builds with the plain
host compiler, and the numpy model of compaction the GPU tests rely on (tests/compact_ref.py) is checked on the
oracle: a run continued on a compacted state equals the uncompacted run relabelled, once the merged slots' links are
cleared (with them, compaction is allowed to differ: see links_dropped in include/smx.h)."""
import ctypes
import os
import subprocess

import numpy as np

import compact_ref as cr
from common import RESULT_ROWS, ROOT, small_pre, small_stream
from oracle_pipeline import OraclePipeline

SHIM_SRC = r'''
#include <vector>
#include "smx_shim.hpp"
using namespace vis;

// a mesher's side of a compaction: its triangles (slot indices) go through the map, removed vertices drop the triangle
size_t compact_and_remap(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, std::vector<u32>* triangles) {
  std::vector<u32> old_to_new;
  u32 links_dropped = 0;
  reconstruction.Compact(stream, &old_to_new, &links_dropped);
  std::vector<u32> kept;
  for (size_t t = 0; t + 2 < triangles->size(); t += 3) {
    u32 v[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const u32 i = (*triangles)[t + k];
      v[k] = i < old_to_new.size() ? old_to_new[i] : 0xFFFFFFFFu;
      ok = ok && v[k] != 0xFFFFFFFFu;
    }
    if (ok) kept.insert(kept.end(), v, v + 3);
  }
  triangles->swap(kept);
  reconstruction.Compact(stream);   // (without the map)
  return links_dropped;
}
int main() { return 0; }
'''


def test_compact_is_declared_and_exported():
    from surfelmeshing_amd import _lib, build
    from test_abi import _declared_symbols
    assert "smx_recon_compact" in _declared_symbols()
    assert "smx_recon_compact" in _lib.EXPORTS
    build.build(verbose=False)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "smx_recon_compact")


def test_shim_compact_compiles_and_links(tmp_path):
    from surfelmeshing_amd import _lib, build
    build.build(verbose=False)
    src = tmp_path / "compact_caller.cc"
    src.write_text(SHIM_SRC)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(tmp_path / "compact_caller"), "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir,
                        "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_numpy_compaction_model():
    rows = np.zeros((25, 6), np.float32)
    rows[7] = [1, -1, 2, np.nan, -1, 3]
    links = np.full((4, 6), cr.INVALID, np.uint32)
    links[0] = [1, 2, 4, 5, 0, cr.INVALID]    # slots 0, 2 point into removed slots; removed 1 and 4 hold a link each
    links[1, 2] = 3
    rows[19:23] = links.view(np.float32)
    new, old_to_new, dropped = cr.compact_rows(rows, 6)
    assert list(old_to_new) == [0, cr.INVALID, 1, 2, cr.INVALID, 3]   # (NaN is not < 0: kept)
    assert dropped == 4
    got = new[19:23].view(np.uint32)
    assert list(got[0]) == [cr.INVALID, cr.INVALID, 3, cr.INVALID] and got[1, 1] == 2


def test_oracle_continuation_on_a_compacted_state_is_a_relabelling():
    s = small_stream(obstacle_until=10, yaw_deg_per_frame=2.0)
    pre = small_pre(s.width)
    a, b = (OraclePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, pre) for _ in range(2))
    for f in range(0, 52):
        d, c = s.frame(f)
        a.upload(f, d, c)
        b.upload(f, d, c)
    for f in range(4, 18):
        for p in (a, b):
            p.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    n_old = a.recon.surfels_size
    assert a.recon.merge_count > 0
    for p in (a, b):
        cr.clear_zombie_links(p.recon.surfels(), n_old)
    old_to_new, dropped = cr.compact_oracle(b.recon)
    assert dropped == 0 and b.recon.surfels_size == n_old - a.recon.merge_count and b.recon.merge_count == 0
    for f in range(18, 48):
        for p in (a, b):
            p.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    n = a.recon.surfels_size
    want = cr.relabel(a.recon.surfels(), n, old_to_new, n_old)
    got = b.recon.surfels()[:, :b.recon.surfels_size]
    assert got.shape == want.shape and a.recon.merge_count > b.recon.merge_count > 0
    for r in RESULT_ROWS:
        assert np.array_equal(got[r].view(np.uint32), want[r].view(np.uint32)), r
