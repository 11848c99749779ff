"""smx_recon_track at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, as bench.py does).

    python tools/track_bench.py [--reps 20] [--frames 100] [--json OUT]

* one call at 640 x 480 with the result left on the device, timed with device events around the call on an otherwise
  idle stream, --reps repetitions: the default schedule, each of its levels alone, and the render alone (the same
  parameters through smx_recon_render), with the inlier counts of the last iteration; a prediction one frame old;
* yardsticks: the launch count x an idle-chip launch boundary (2.3 us) and the algorithmic
  bytes of an iteration (30 B per sampled pixel) at the HBM peak;
* the frame loop: --frames frames one by one, once with a track call in front of every Integrate and once without,
  from the same uploaded state, in the same process."""
import argparse
import ctypes
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
from surfelmeshing_amd._lib import TrackParams, TrackResult  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s (MI355X_MICROARCH.md: spec)
LAUNCH_US = 2.3        # idle-chip launch boundary


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms[1:]     # (the first call allocates)


def main():
    _lib.require_gpu()
    wl = bench.Workload(api, 640, 480, 5_000_000, 5_500_000, 0x5EED0001, 0.0)
    t0 = time.time()
    g_end, _ = wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    print("# grown in %.1f s: %d slots, %d merged" % (time.time() - t0, n, n - live), flush=True)
    W, H = 640, 480
    first = g_end + 10
    # the preprocessed images of one frame (the driver's work images after it), tracked from the previous frame's pose
    for j in range(-4, 6):
        wl.render(first + j, 4 + j)
    rows = rec.debug_download_surfels(n)
    wl.pipe.run_array(*wl.steps([wl.plan(first, 4)]))
    api.StreamSynchronize(None)
    d, nrm, _ = wl.pipe.download_work()
    rec.debug_upload_surfels(rows, n - live)
    depth, normals = api.CUDABuffer(H, W, np.uint16), api.CUDABuffer(H, W, np.float32, 2)
    depth.Upload(d)
    normals.Upload(nrm)
    pred, truth = wl.plan(first - 1, 3)[3], wl.plan(first, 4)[3]
    result = api.CUDABuffer(1, 64, np.float32)
    assert ctypes.sizeof(TrackResult) <= 256
    res = {"metric": "track_ms", "slots": n, "live": live, "width": W, "height": H, "reps": args.reps}

    def read_result():
        raw = result.Download().tobytes()[:ctypes.sizeof(TrackResult)]
        return api.TrackOutcome(TrackResult.from_buffer_copy(raw))

    default = TrackParams.defaults()
    rp = api.make_render_params(W, H, wl.fx, wl.fy, wl.cx, wl.cy, pred, near_z=default.near_z, far_z=default.far_z,
                                splat_mode=api.SMX_SPLAT_DISC, disc_radius_factor=default.disc_radius_factor,
                                max_splat_extent_in_pixels=default.max_splat_extent_in_pixels)
    md, mn = api.CUDABuffer(H, W, np.float32), api.CUDABuffer(H, W, np.float32, 4)
    ms = timed(lambda: rec.Render(None, rp, depth=md, normal=mn), args.reps)
    render_ms = float(np.median(ms))
    res["render_ms"] = render_ms
    print("render alone (disc, depth + normal) median %.3f ms (min %.3f, max %.3f)" % (render_ms, min(ms), max(ms)), flush=True)
    schedules = [("default", [(4, 4), (2, 5), (1, 10)]), ("stride4_x4", [(4, 4)]), ("stride2_x5", [(2, 5)]),
                 ("stride1_x10", [(1, 10)])]
    for name, levels in schedules:
        # (convergence off: every scheduled iteration runs, so that the time belongs to the launch count)
        p = TrackParams.defaults(levels=levels, convergence_rotation=0.0, convergence_translation=0.0)
        ms = timed(lambda: rec.TrackAsync(None, wl.pre.depth_scaling, depth, normals, pred, p, result), args.reps)
        out = read_result()
        recs = rec.debug_track_iterations()
        iters = sum(k for _, k in levels)
        launches = 3 + 1 + 2 * iters
        sampled = sum(k * ((W - s // 2 + s - 1) // s) * ((H - s // 2 + s - 1) // s) for s, k in levels)
        med = float(np.median(ms))
        dt = np.linalg.norm(out.global_T_frame[:, 3].astype(np.float64) - np.asarray(truth, np.float64).reshape(3, 4)[:, 3])
        res[name + "_ms"] = med
        res[name + "_iterations_ms"] = med - render_ms
        res[name + "_inliers"] = out.inliers
        print("%-12s median %.3f ms (min %.3f, max %.3f): render %.3f + iterations %.3f = %.1f us per iteration; %s, %d "
              "iterations, inliers %d / %d, rms %.2f mm, %.2f mm from the generated pose; %d launches x %.1f us = %.3f ms; "
              "%.1f MB of pixel terms = %.1f us at the HBM peak" % (
                  name, med, min(ms), max(ms), render_ms, med - render_ms, 1e3 * (med - render_ms) / iters, out.status_name,
                  len(recs), out.inliers, out.pixels_with_depth, out.rms_residual * 1e3, dt * 1e3, launches, LAUNCH_US,
                  launches * LAUNCH_US * 1e-3, 30e-6 * sampled, 30.0 * sampled / HBM_PEAK * 1e6), flush=True)
    res["value"] = res["default_ms"]

    # ---- the frame loop with and without a track call in front of every Integrate
    warm = 10
    total = warm + args.frames
    for j in range(-4, total + 5):
        wl.render(first + j, 4 + j)
    plan = [wl.plan(first + j, 4 + j) for j in range(total)]
    fps = {}
    for name in ("no_track", "track_every_frame"):
        rec.debug_upload_surfels(rows, n - live)
        wl.pipe.run_array(*wl.steps(plan[:warm]))
        steps = [wl.steps(plan[a:a + 1]) for a in range(warm, total)]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k, a in enumerate(range(warm, total)):
            if name == "track_every_frame":
                rec.TrackAsync(None, wl.pre.depth_scaling, depth, normals, plan[a - 1][3], default, result)
            wl.pipe.run_array(*steps[k])
        e1.record()
        e1.synchronize()
        fps[name] = args.frames / (e0.elapsed_time(e1) * 1e-3)
        print("%s: %d frames %.1f frames/s" % (name, args.frames, fps[name]), flush=True)
    res["frames_per_s_no_track"] = fps["no_track"]
    res["frames_per_s_track_every_frame"] = fps["track_every_frame"]
    res["frames"] = args.frames
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
