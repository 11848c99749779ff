"""smx_recon_merge_map at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, as bench.py does).

    python tools/merge_bench.py [--reps 5] [--surfels 5000000] [--txt OUT.txt] [--json OUT.json]

Two half-overlapping maps are cut from the grown one: dst = its first two thirds of the slots, src = its last two thirds (slots are
created along the camera's sweep, so the middle third is surface both sessions saw), each uploaded into an object of its own, the
links of src re-based.  The merge runs under the identity, in both modes, --reps repetitions each, dst restored by an upload
between them (outside the window).  Reported:
* milliseconds per call (a host clock around the synchronous call) and per phase by the library's own events
  (smx_recon_debug_merge_timings), medians;
* the counts, and the bytes of a traffic model of the call's own kernels (the neighbour search is not modelled);
* beside it, in the same process: smx_recon_build_neighbor_index over dst and a plain smx_nn_query_batch of the same moved
  points with device pointers, by device events -- the expectation to check is "the call is the build plus the query plus a
  small remainder"."""
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
ap.add_argument("--surfels", type=int, default=5_000_000)
ap.add_argument("--txt", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.argv = [sys.argv[0]]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import bench  # noqa: E402
from surfelmeshing_amd import _lib, api  # noqa: E402

INVALID = np.uint32(0xFFFFFFFF)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def traffic_bytes(st, k, mode, pitch, mean_candidates):
    """HBM bytes of the call's own kernels and resets by phase, from the counts (a model: what they read and write once)."""
    n, live, app, matched, blended = st["n_src_slots"], st["n_src_live"], st["n_appended"], st["n_matched"], st["n_blended_dst"]
    b = {"move": n * (48 + 16 + 48 + 1),
         "select": n * 1 + live * (16 + 4 + 4 * k) + int(live * mean_candidates * 16) + matched * 5,
         "number": 2 * n + 4 * n + (matched * 12 if mode == "blend" else 0),
         "append": n * 1 + app * (4 + 48 + 32 + 96 + 4 * 5),
         "blend": 0,
         "finish": 16 * pitch + 2 * pitch + pitch + st["new_size"] * 16}
    if mode == "blend":
        passes = max(1, ((max(st["old_size"], 2) - 1).bit_length() + 7) // 8)
        b["blend"] = passes * matched * 12 * 2 + matched * (12 + 48 + 4) + blended * (64 + 52)
    return b


def main():
    _lib.require_gpu()
    cap = args.surfels + args.surfels // 10
    wl = bench.Workload(api, 640, 480, args.surfels, cap, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n_all = rec.surfels_size()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n_all, rec.surfel_count()))
    rows = rec.debug_download_surfels(n_all)
    third = n_all // 3
    rows_dst = np.ascontiguousarray(rows[:, :2 * third])
    rows_src = np.ascontiguousarray(rows[:, third:])
    links = rows_src[19:23].view(np.uint32)
    links[...] = np.where((links == INVALID) | (links < third), INVALID, links - np.uint32(third))
    n_dst, n_src = rows_dst.shape[1], rows_src.shape[1]
    cam = api.PinholeCamera4f(640, 480, 525.0, 525.0, 320.0, 240.0)
    dst, src = api.CUDASurfelReconstruction(cap, cam), api.CUDASurfelReconstruction(n_src, cam)
    src.debug_upload_surfels(rows_src)
    nn = api.SurfelNeighborIndex()
    T = np.eye(4, dtype=np.float32)[:3]
    result = {"slots_dst": n_dst, "slots_src": n_src, "reps": args.reps, "modes": {}}

    for mode in ("keep", "blend"):
        pod = api.merge_params(mode=mode, frame_index=1000)
        calls, phases, stats = [], [], None
        for _ in range(args.reps + 1):
            dst.debug_upload_surfels(rows_dst)
            api.StreamSynchronize(None)
            t1 = time.perf_counter()
            stats = dst.MergeMap(None, src, T, index=nn, params=pod)      # (synchronous)
            calls.append(1e3 * (time.perf_counter() - t1))
            phases.append(dst.debug_merge_timings())
        calls, phases = calls[1:], phases[1:]                                # (the first call allocates the workspace)
        med = {k: float(np.median([p[k] for p in phases])) for k in phases[0]}
        model = traffic_bytes(stats, pod.k, mode, (cap + 63) // 64 * 64, float(pod.k))   # (upper bound: every list full)
        say("merge (%s): %d slots into %d: %s" % (mode, n_src, n_dst, ", ".join("%s %d" % kv for kv in stats.items())))
        say("  call %.2f ms median by the host clock (min %.2f, max %.2f, %d calls); by the library's events %.2f ms: %s" % (
            float(np.median(calls)), min(calls), max(calls), len(calls), med["whole"],
            ", ".join("%s %.2f" % (k, v) for k, v in med.items() if k != "whole")))
        say("  traffic model of the call's own kernels (candidate gathers as if every list were full): %s; total %.1f MB" % (
            ", ".join("%s %.1f MB" % (k, v / 1e6) for k, v in model.items()), sum(model.values()) / 1e6))
        result["modes"][mode] = {"stats": stats, "call_ms_median": float(np.median(calls)), "call_ms_min": min(calls), "call_ms_max": max(calls),
                                 "phase_ms_median": med, "traffic_model_bytes": model}

    # ---- beside it: the index build and a plain query of the same moved points (identity: the smooth positions as they are)
    dst.debug_upload_surfels(rows_dst)
    live = ~(rows_src[7] < 0)
    q = np.zeros((4, n_src), np.float32)
    q[0:3, live] = rows_src[3:6, live]
    q[3] = np.where(live, rows_src[7], np.float32(-1.0))
    dq = torch.from_numpy(q).cuda()
    k = 8
    didx = torch.empty(n_src * k, dtype=torch.int32, device="cuda")
    dd2 = torch.empty(n_src * k, dtype=torch.float32, device="cuda")
    dcnt = torch.empty(n_src, dtype=torch.int32, device="cuda")
    L = _lib.load()
    build_ms, query_ms = [], []
    for _ in range(args.reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        nn.BuildFromReconstruction(dst, 0.05)
        ev[1].record()
        p = dq.data_ptr()
        _lib.check(L.smx_nn_query_batch(nn._h, None, C.c_uint32(n_src), C.c_void_p(p), C.c_void_p(p + 4 * n_src), C.c_void_p(p + 8 * n_src),
                                        C.c_void_p(p + 12 * n_src), C.c_int32(k), None, C.c_uint8(0), C.c_int32(1), C.c_void_p(didx.data_ptr()),
                                        C.c_void_p(dd2.data_ptr()), C.c_void_p(dcnt.data_ptr()), C.c_int32(1)))
        ev[2].record()
        ev[2].synchronize()
        build_ms.append(ev[0].elapsed_time(ev[1]))
        query_ms.append(ev[1].elapsed_time(ev[2]))
    build_ms, query_ms = build_ms[1:], query_ms[1:]
    mean_cand = float(dcnt.sum().item()) / max(1, int(live.sum()))
    say("beside it: smx_recon_build_neighbor_index over dst %.2f ms median, plain smx_nn_query_batch of the %d moved points (k = %d, %.2f "
        "candidates per live point) %.2f ms median; sum %.2f ms" % (float(np.median(build_ms)), n_src, k, mean_cand, float(np.median(query_ms)),
                                                                    float(np.median(build_ms)) + float(np.median(query_ms))))
    result.update(build_ms_median=float(np.median(build_ms)), query_ms_median=float(np.median(query_ms)), mean_candidates=mean_cand)
    for mode in ("keep", "blend"):
        r = result["modes"][mode]
        rest = r["phase_ms_median"]["whole"] - result["build_ms_median"] - result["query_ms_median"]
        say("merge (%s): the call's %.2f ms = build %.2f + query %.2f + %.2f ms remainder (%.0f %% of the call)" % (
            mode, r["phase_ms_median"]["whole"], result["build_ms_median"], result["query_ms_median"], rest, 100.0 * rest / r["phase_ms_median"]["whole"]))
        r["remainder_ms"] = rest
    print(json.dumps({"metric": "merge_ms", "value": result["modes"]["keep"]["phase_ms_median"]["whole"]}), flush=True)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(LINES) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
