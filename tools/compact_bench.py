"""smx_recon_compact at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, as bench.py does).

    python tools/compact_bench.py [--reps 20] [--frames 100] [--json OUT]

* the compaction itself: timed with device events around the call (which is synchronous: the window includes its two
  host round trips -- the size read at the start and the result read at the end), --reps repetitions, the state
  restored by an upload between them (outside the window); bytes moved by the traffic model below, and the fraction
  of the HBM peak (8.0 TB/s spec, MI355X);
* the frame loop: --frames frames on the uncompacted map against the same frames on the compacted one, both started
  from the same uploaded state, in the same process."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.argv = [sys.argv[0]]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import bench  # noqa: E402
from surfelmeshing_amd import _lib, api  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s (MI355X_MICROARCH.md: spec; ~6.3 TB/s measured with a float4 copy)


def traffic_bytes(n, k, pitch):
    """HBM bytes of one compaction of n slots of which k are kept (what the kernels and resets read and write)."""
    count_map = 16 * n + n // 4 + n // 4 + 4 * n            # N records; keep bits written / read; old_to_new written
    records = 4 * (4 * n + 16 * k + 16 * k)                   # P, S, N, C: map read, kept records read, staged
    records += 4 * n + 16 * n + 16 * k                        # T: map, every record (removed slots' links counted), staged
    copy_back = 5 * (16 * k + 16 * k)
    resets = 16 * pitch + 2 * pitch + pitch + n              # grad_acc, both flag tables, merge_flag, flag rebuild reads
    return count_map + records + copy_back + resets


def main():
    _lib.require_gpu()
    wl = bench.Workload(api, 640, 480, 5_000_000, 5_500_000, 0x5EED0001, 0.0)
    t0 = time.time()
    g_end, _ = wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    merged = n - live
    print("# grown in %.1f s: %d slots, %d merged (%.2f %%)" % (time.time() - t0, n, merged, 100.0 * merged / n), flush=True)
    rows = rec.debug_download_surfels(n)
    pitch = (wl.pipe.reconstruction.max_surfel_count + 63) // 64 * 64

    # ---- the compaction itself
    ms = []
    for _ in range(args.reps + 1):
        rec.debug_upload_surfels(rows, merged)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, k, dropped = rec.Compact(None, return_map=False)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]   # (the first call allocates the map buffers)
    assert k == live, (k, live)
    b = traffic_bytes(n, k, pitch)
    med = float(np.median(ms))
    print("compaction: %d -> %d slots, %d links dropped; median %.1f us (min %.1f, max %.1f) over %d; traffic model %.2f GB "
          "-> %.2f TB/s = %.0f %% of the 8.0 TB/s HBM peak" % (n, k, dropped, med * 1e3, min(ms) * 1e3, max(ms) * 1e3, len(ms),
                                                                b / 1e9, b / (med * 1e-3) / 1e12, 100.0 * b / (med * 1e-3) / HBM_PEAK),
          flush=True)

    # ---- the frame loop on the uncompacted and on the compacted map, from the same state
    first = g_end + 10
    warm = 10
    total = warm + args.frames
    for j in range(-4, total + 5):
        wl.render(first + j, 4 + j)
    plan = [wl.plan(first + j, 4 + j) for j in range(total)]
    fps = {}
    for name in ("uncompacted", "compacted"):
        rec.debug_upload_surfels(rows, merged)
        if name == "compacted":
            rec.Compact(None, return_map=False)
        wl.pipe.run_array(*wl.steps(plan[:warm]))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        wl.pipe.run_array(*wl.steps(plan[warm:]))
        e1.record()
        e1.synchronize()
        fps[name] = args.frames / (e0.elapsed_time(e1) * 1e-3)
        print("%s map: %d frames %.1f frames/s (slots at the end %d)" % (name, args.frames, fps[name], rec.surfels_size()), flush=True)
    res = {"metric": "compaction_us", "value": med * 1e3, "slots": n, "kept": k, "links_dropped": dropped, "reps": len(ms),
           "us_min": min(ms) * 1e3, "us_max": max(ms) * 1e3, "traffic_model_bytes": b,
           "frames_per_s_uncompacted": fps["uncompacted"], "frames_per_s_compacted": fps["compacted"], "frames": args.frames}
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
