"""smx_recon_triangulate at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, the map
tools/compact_bench.py grows).

    python tools/mesh_bench.py [--reps 5] [--target 5000000] [--json OUT]
    python tools/mesh_bench.py --update [--target 5000000] [--json OUT] [--txt OUT]

Times whole calls with device events around them (the call is synchronous: the window includes its host round trips)
and, from the library's own timed events (smx_recon_debug_mesh_timings), the index build, the list query, the star
kernel and agreement + scan + write separately.  Prints ms per call, surfels/s, triangles, the statistics, and bytes by
the traffic model below.  No threshold: there is no earlier time to compare with.

--update measures (medians of --reps rounds) smx_recon_triangulate_update on the same map, each figure against the full call in the
same process: one update after 1, 4 and 16 more integrated frames, then a sweep in which 1, 2, 5, 10, 20 and 40 % of the
live slots change (the surfels of the most recent creation frames are moved by 1 mm through
smx_recon_deform_by_creation_frame: a coherent part of the map, as a frame's changes are).  The update is timed as the
application calls it: one call with a device buffer that is large enough.  Every update is compared with the full call's
bytes.  The sweep runs with full_above_fraction = 1, so that the incremental path is what is measured at every point."""
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
ap.add_argument("--update", action="store_true")
ap.add_argument("--txt", default=None)
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


UPDATE_PHASES = ("diff", "index_builds", "reverse_test", "subset_lists", "stars", "agree_merge")


def update_main():
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 5, 0x5EED0001, 0.0)
    t0 = time.time()
    g, _ = wl.grow(False)                               # g: the next frame of the trajectory
    rec = wl.pipe.reconstruction
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, rec.surfels_size(), rec.surfel_count()))
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * rec.surfels_size()                        # triangles: about two per live slot
    dbuf = [api.CUDABuffer(1, 3 * cap, np.uint32) for _ in range(2)]

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def full():
        n, st = C.c_uint32(0), _lib.MeshStats()
        _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dbuf[0].ToCUDA().address),
                                           C.c_uint32(cap), C.c_int32(1), C.byref(n), C.byref(st)))
        return n.value, bytes(st)

    def update(fraction):
        n, st, us = C.c_uint32(0), _lib.MeshStats(), _lib.MeshUpdateStats()
        _lib.check(L.smx_recon_triangulate_update(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_float(fraction),
                                                  C.c_void_p(dbuf[1].ToCUDA().address), C.c_uint32(cap), C.c_int32(1),
                                                  C.byref(n), C.byref(st), C.byref(us)))
        return n.value, bytes(st), {k: int(getattr(us, k)) for k, _ in _lib.MeshUpdateStats._fields_}

    def same(T):
        x, y = dbuf[0].Download()[0][:3 * T], dbuf[1].Download()[0][:3 * T]
        return bool(np.array_equal(x, y))

    def one(label, fraction, change):
        """args.reps times: the change, the update (from the kept state), then the full call on the same map; the full call
        drops the kept state, so a second update (mode 1) restores it for the next round.  Medians; the counts are the
        last round's."""
        ok, t_u, t_f, phs, fphs = True, [], [], [], []
        for _ in range(max(1, args.reps)):
            change()
            ms_u, (Tu, su, us) = timed(lambda: update(fraction))
            phs.append(rec.debug_mesh_update_timings())
            ms_f, (Tf, sf) = timed(full)
            fphs.append(rec.debug_mesh_timings())
            ok = ok and Tu == Tf and su == sf and same(Tf)
            update(fraction)
            t_u.append(ms_u)
            t_f.append(ms_f)
        ms_u, ms_f = float(np.median(t_u)), float(np.median(t_f))
        ph = {k: float(np.median([q[k] for q in phs])) for k in UPDATE_PHASES}
        fph = {k: float(np.median([q[k] for q in fphs])) for k in PHASES}
        n = rec.surfels_size()
        rowd = {"label": label, "reps": len(t_u), "update_ms_all": t_u, "full_ms_all": t_f, "slots": n, "triangles": Tf, "equal_to_full": ok, "update_ms": ms_u, "full_ms": ms_f,
                "ratio": ms_u / ms_f, "update_stats": us, "dirty_fraction": us["n_dirty"] / float(n),
                "update_phases_ms": ph, "full_phases_ms": fph}
        say("%-22s mode %d changed %8d dirty %8d (%.3f of %d) reagreed %8d kept %9d | update %7.2f ms  full %7.2f ms  ratio %.3f "
            "| %s%s" % (label, us["mode"], us["n_changed"], us["n_dirty"], rowd["dirty_fraction"], n, us["n_reagreed"],
                        us["n_kept_triangles"], ms_u, ms_f, rowd["ratio"],
                        " ".join("%s %.2f" % (k, ph[k]) for k in UPDATE_PHASES), "" if ok else "  DIFFERS FROM THE FULL CALL"))
        return rowd
    rows = []
    full()                                              # (allocates the full call's workspace)
    update(-1.0)                                        # the kept state
    rows.append(one("no change", -1.0, lambda: None))
    state = {"g": g}

    def integrate(k):
        for _ in range(k):
            g = state["g"]
            for f in range(g - 4, g + 5):
                wl.render(f, f)
            wl.pipe.run_array(*wl.steps([wl.plan(g, g)]))
            wl.pipe.release(g - 4)
            state["g"] = g + 1
    for k in (1, 4, 16):
        rows.append(one("%d frames, default" % k, -1.0, lambda: integrate(k)))
    # the sweep: the most recent creation frames that hold x % of the live slots move by 1 mm
    table = rec.debug_download_surfels()
    created = table[17].view(np.uint32)[table[7] >= 0].astype(np.int64)
    live = created.size
    del table
    per_frame = np.bincount(created)
    newest_first = np.cumsum(per_frame[::-1])
    for pct in (1, 2, 5, 10, 20, 40):
        k = int(np.searchsorted(newest_first, pct * 0.01 * live)) + 1
        T = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (per_frame.size, 1))
        T[per_frame.size - k:, 3] = 1e-3
        rows.append(one("%d %% moved" % pct, 1.0, lambda: rec.DeformByCreationFrame(None, T)))
    ok = all(r["equal_to_full"] for r in rows)
    say("every update equal to the full call: %s" % ok)
    res = {"metric": "triangulate_update_ms", "rows": rows, "all_equal": ok}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")
    nn.close()
    sys.exit(0 if ok else 1)


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
    update_main() if args.update else main()
