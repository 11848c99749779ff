"""smx_recon_import_points at size: about 5 M points of the room's surfaces (synth.room_surface_points, config C5) on the device.

    python tools/import_bench.py [--reps 5] [--points 5000000] [--k 16] [--radius_spacings 3.0] [--txt OUT.txt] [--json OUT.json]

The cloud is uploaded once; the search radius is --radius_spacings times the cloud's own spacing (the default of 0.1 m would hold
hundreds of points of a 5 M cloud), the index cell equals it.  Every repetition imports into an emptied object.  Reported:
* milliseconds per call (a host clock around the synchronous call) and per phase by the library's own events
  (smx_recon_debug_import_timings), medians;
* the counts, and the fit kernel's bytes by a traffic model (lists n k 8 B, neighbour records n k 16 B before cache hits, 100 B
  written per imported slot by fit + write) against the HBM peak;
* beside it, in the same process: smx_nn_build and smx_nn_query_self of the same points with device pointers, by device
  events -- the expectation to check is "the call is the build plus the query plus a remainder"."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--points", type=int, default=5_000_000)
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--radius_spacings", type=float, default=3.0)
ap.add_argument("--txt", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from surfelmeshing_amd import _lib, api, synth  # noqa: E402

HBM_PEAK = 8.0e12      # bytes per second, MI355X
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def main():
    _lib.require_gpu()
    pts, spacing = synth.room_surface_points(args.points)
    n, k = pts.shape[0], args.k
    radius = float(np.float32(args.radius_spacings * spacing))
    say("# %d points, spacing %.4f m, search radius %.4f m, k = %d" % (n, spacing, radius, k))
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    torch.cuda.synchronize()
    rec = api.CUDASurfelReconstruction(n + 1024, api.PinholeCamera4f(640, 480, 525.0, 525.0, 320.0, 240.0))
    nn = api.SurfelNeighborIndex()
    pod = api.import_params(cell_size=radius, search_radius=radius, k=k, orient="view_point", view_point=(0.0, 0.0, 0.0))
    empty = np.zeros((25, 0), np.float32)
    calls, phases, stats = [], [], None
    for _ in range(args.reps + 1):
        rec.debug_upload_surfels(empty, 0)
        api.StreamSynchronize(None)
        t1 = time.perf_counter()
        stats = rec.ImportPoints(None, d_pts, index=nn, params=pod)      # (synchronous)
        calls.append(1e3 * (time.perf_counter() - t1))
        phases.append(rec.debug_import_timings())
    calls, phases = calls[1:], phases[1:]                                # (the first call allocates the workspace)
    med = {name: float(np.median([p[name] for p in phases])) for name in phases[0]}
    say("import: %s" % ", ".join("%s %d" % kv for kv in stats.items()))
    say("  call %.2f ms median by the host clock (min %.2f, max %.2f, %d calls); by the library's events %.2f ms: %s" % (
        float(np.median(calls)), min(calls), max(calls), len(calls), med["whole"], ", ".join("%s %.2f" % (a, b) for a, b in med.items() if a != "whole")))
    model = {"lists": n * k * 8, "records": n * k * 16, "written": stats["n_imported"] * 100}
    total = sum(model.values())
    say("  traffic model of fit + write: lists %.0f MB, neighbour records %.0f MB before cache hits, written %.0f MB; %.0f MB = %.3f ms at the HBM "
        "peak of %.1f TB/s; fit + write took %.2f ms (%.0f %% of the peak by this model)" % (
            model["lists"] / 1e6, model["records"] / 1e6, model["written"] / 1e6, total / 1e6, 1e3 * total / HBM_PEAK, HBM_PEAK / 1e12,
            med["fit"] + med["write"], 100.0 * (1e3 * total / HBM_PEAK) / max(med["fit"] + med["write"], 1e-9)))

    # ---- beside it: the index build and the self query of the same points
    rows = d_pts.t().contiguous()
    didx = torch.empty(n * k, dtype=torch.int32, device="cuda")
    dd2 = torch.empty(n * k, dtype=torch.float32, device="cuda")
    dcnt = torch.empty(n, dtype=torch.int32, device="cuda")
    L = _lib.load()
    build_ms, query_ms = [], []
    p = rows.data_ptr()
    for _ in range(args.reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        _lib.check(L.smx_nn_build(nn._h, None, C.c_void_p(p), C.c_void_p(p + 4 * n), C.c_void_p(p + 8 * n), C.c_uint32(n), C.c_float(radius), C.c_int32(1)))
        ev[1].record()
        _lib.check(L.smx_nn_query_self(nn._h, None, None, C.c_float(np.float32(radius) * np.float32(radius)), C.c_int32(k), None, C.c_uint8(0),
                                       C.c_void_p(didx.data_ptr()), C.c_void_p(dd2.data_ptr()), C.c_void_p(dcnt.data_ptr())))
        ev[2].record()
        ev[2].synchronize()
        build_ms.append(ev[0].elapsed_time(ev[1]))
        query_ms.append(ev[1].elapsed_time(ev[2]))
    build_ms, query_ms = float(np.median(build_ms[1:])), float(np.median(query_ms[1:]))
    mean_m = float(dcnt.sum().item()) / n
    rest = med["whole"] - build_ms - query_ms
    say("beside it: smx_nn_build %.2f ms median, smx_nn_query_self (k = %d, %.2f entries per point) %.2f ms median; sum %.2f ms" % (
        build_ms, k, mean_m, query_ms, build_ms + query_ms))
    say("import: the call's %.2f ms = build %.2f + query %.2f + %.2f ms remainder (%.0f %% of the call)" % (
        med["whole"], build_ms, query_ms, rest, 100.0 * rest / med["whole"]))
    result = {"points": n, "spacing": spacing, "search_radius": radius, "k": k, "reps": args.reps, "stats": stats,
              "call_ms_median": float(np.median(calls)), "call_ms_min": min(calls), "call_ms_max": max(calls), "phase_ms_median": med,
              "traffic_model_bytes": model, "build_ms_median": build_ms, "query_ms_median": query_ms, "mean_entries": mean_m, "remainder_ms": rest}
    print(json.dumps({"metric": "import_ms", "value": med["whole"]}), flush=True)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(LINES) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    nn.close()
    rec.close()


if __name__ == "__main__":
    main()
