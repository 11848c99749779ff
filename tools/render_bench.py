"""smx_recon_render at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, as bench.py does).

    python tools/render_bench.py [--reps 20] [--frames 100] [--json OUT]

* one render at 640 x 480 (all four images), timed with device events around the call, --reps repetitions: from the
  pose of the last captured frame and from an overview pose (outside the room's corner, looking at its centre), in
  both splat modes; the scan's bytes (S and N records, 32 B per slot) against the HBM peak for scale;
* the frame loop: --frames frames in 10-frame slices, once with a render (disc, capture pose) after every slice and
  once without, from the same uploaded state, in the same process."""
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
from surfelmeshing_amd import _lib, api, render  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s (MI355X_MICROARCH.md: spec)


def main():
    _lib.require_gpu()
    wl = bench.Workload(api, 640, 480, 5_000_000, 5_500_000, 0x5EED0001, 0.0)
    t0 = time.time()
    g_end, _ = wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    print("# grown in %.1f s: %d slots, %d merged" % (time.time() - t0, n, n - live), flush=True)
    W, H = 640, 480
    bufs = {"depth": api.CUDABuffer(H, W, np.float32), "index": api.CUDABuffer(H, W, np.uint32),
            "normal": api.CUDABuffer(H, W, np.float32, 4), "color": api.CUDABuffer(H, W, np.uint8, 4)}
    capture = wl.plan(g_end + 10, 4)[3]   # (the pose of the first frame the loop below integrates)
    overview = render.look_at([2.6, -1.2, 2.6], [0.0, 0.0, 0.0])
    res = {"metric": "render_ms", "slots": n, "live": live, "width": W, "height": H, "reps": args.reps}
    for pose_name, T in (("capture", capture), ("overview", overview)):
        for mode_name, mode in (("square", api.SMX_SPLAT_SQUARE), ("disc", api.SMX_SPLAT_DISC)):
            p = api.make_render_params(W, H, wl.fx, wl.fy, wl.cx, wl.cy, T, splat_mode=mode)
            ms = []
            for _ in range(args.reps + 1):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rec.Render(None, p, **bufs)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            ms = ms[1:]   # (the first call allocates the z-buffer)
            idx = bufs["index"].Download()
            covered = float((idx != 0xFFFFFFFF).mean())
            med = float(np.median(ms))
            key = "%s_%s" % (pose_name, mode_name)
            res[key + "_ms"] = med
            res[key + "_ms_min"] = float(min(ms))
            res[key + "_covered"] = covered
            print("%-16s median %.3f ms (min %.3f, max %.3f) over %d; %.1f %% of the pixels covered; scan of %.0f MB = "
                  "%.1f us at the HBM peak" % (key, med, min(ms), max(ms), len(ms), 100 * covered, 32e-6 * n,
                                               32.0 * n / HBM_PEAK * 1e6), flush=True)
    res["value"] = res["capture_disc_ms"]

    # ---- the frame loop with and without a render every 10 frames
    rows = rec.debug_download_surfels(n)
    first = g_end + 10
    warm, slice_ = 10, 10
    total = warm + args.frames
    for j in range(-4, total + 5):
        wl.render(first + j, 4 + j)
    plan = [wl.plan(first + j, 4 + j) for j in range(total)]
    fps = {}
    for name in ("no_render", "render_every_10"):
        rec.debug_upload_surfels(rows, n - live)
        wl.pipe.run_array(*wl.steps(plan[:warm]))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for a in range(warm, total, slice_):
            wl.pipe.run_array(*wl.steps(plan[a:a + slice_]))
            if name == "render_every_10":
                last = plan[min(a + slice_, total) - 1]
                rec.Render(None, api.make_render_params(W, H, wl.fx, wl.fy, wl.cx, wl.cy, last[3],
                                                        splat_mode=api.SMX_SPLAT_DISC), **bufs)
        e1.record()
        e1.synchronize()
        fps[name] = args.frames / (e0.elapsed_time(e1) * 1e-3)
        print("%s: %d frames %.1f frames/s" % (name, args.frames, fps[name]), flush=True)
    res["frames_per_s_no_render"] = fps["no_render"]
    res["frames_per_s_render_every_10"] = fps["render_every_10"]
    res["frames"] = args.frames
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
