"""smx_recon_triangulate at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, the map
tools/compact_bench.py grows).

    python tools/mesh_bench.py [--reps 5] [--target 5000000] [--json OUT]

Times whole calls with device events around them (the call is synchronous: the window includes its host round trips)
and, from the library's own timed events (smx_recon_debug_mesh_timings), the index build, the list query, the star
kernel and agreement + scan + write separately.  Prints ms per call, surfels/s, triangles, the statistics, and bytes by
the traffic model below.  No threshold: there is no earlier time to compare with."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--target", type=int, default=5_000_000)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.argv = [sys.argv[0]]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import bench  # noqa: E402
from surfelmeshing_amd import _lib, api  # noqa: E402

PHASES = ("index_build", "list_query", "star", "agree_write")


def traffic_bytes(n, live, k, triangles):
    """HBM bytes of the mesh kernels proper for n slots (list query and index build not included): the [n][k] index
    lists read once; per live slot its own S and N records and up to k gathered S and N records (mostly cache hits:
    neighbours share bricks, counted once per slot here as a lower bound); rings written once and read about three
    times (own row plus the rows of the two other corners of every star triangle, largely from L2); counts, meta words,
    offsets; the output written twice (unordered, then the slot's own entries reordered in cache) -- counted once."""
    lists = 4 * n * k + 4 * n
    records = 32 * n + 32 * live
    rings = (64 + 4) * n * (1 + 3)
    scan = 4 * n * 2 + 8 * (n // 256 + 1)
    return lists + records + rings + scan + 12 * triangles


def main():
    _lib.require_gpu()
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    print("# grown in %.1f s: %d slots, %d merged" % (time.time() - t0, n, n - live), flush=True)
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    ms, phases = [], []
    tri = stats = None
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tri, stats = rec.Triangulate(None, p, index=nn)       # (two calls inside: the count, then the write)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        phases.append(rec.debug_mesh_timings())               # (of the second call)
    ms, phases = ms[1:], phases[1:]                           # (the first call allocates the workspace)
    med = float(np.median(ms))
    ph = {k: float(np.median([q[k] for q in phases])) for k in PHASES}
    one = sum(ph.values())
    b = traffic_bytes(n, live, p.max_neighbors, tri.shape[0])
    kern = ph["star"] + ph["agree_write"]
    print("triangulate: %d slots (%d live) -> %d triangles; count + write pair of calls: median %.2f ms (min %.2f, max %.2f) "
          "over %d" % (n, live, tri.shape[0], med, min(ms), max(ms), len(ms)), flush=True)
    print("one call by the library's events: %.2f ms = index build %.2f + list query %.2f + star %.2f + agreement, scan, "
          "write %.2f; %.1f M surfels/s" % (one, ph["index_build"], ph["list_query"], ph["star"], ph["agree_write"],
                                            live / (one * 1e-3) / 1e6), flush=True)
    print("statistics: %s" % stats, flush=True)
    print("traffic model of the star and agreement kernels: %.2f GB in %.2f ms -> %.2f TB/s" % (
        b / 1e9, kern, b / (kern * 1e-3) / 1e12), flush=True)
    res = {"metric": "triangulate_ms", "value": one, "pair_of_calls_ms": med, "slots": n, "live": live,
           "triangles": int(tri.shape[0]), "reps": len(ms), "phases_ms": ph, "stats": stats, "traffic_model_bytes": b,
           "surfels_per_s": live / (one * 1e-3)}
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    nn.close()


if __name__ == "__main__":
    main()
