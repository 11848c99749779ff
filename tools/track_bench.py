"""smx_recon_track at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, as bench.py does).

    python tools/track_bench.py [--reps 20] [--frames 100] [--rgbd] [--json OUT]

* one call at 640 x 480 with the result left on the device, timed with device events around the call on an otherwise
  idle stream, --reps repetitions: the default schedule, each of its levels alone, and the render alone (the same
  parameters through smx_recon_render), with the inlier counts of the last iteration; a prediction one frame old;
* yardsticks: the launch count x an idle-chip launch boundary (2.3 us) and the algorithmic
  bytes of an iteration (30 B per sampled pixel) at the HBM peak;
* the frame loop: --frames frames one by one, once with a track call in front of every Integrate and once without,
  from the same uploaded state, in the same process;
* --rgbd: smx_recon_track_rgbd with the frame's colour image beside every one of these in the same run, split the same
  way (its render also resolves colour; one prepare launch and 19 B more per associated sampled pixel and iteration),
  and the ratio of the two."""
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
ap.add_argument("--rgbd", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.argv = [sys.argv[0]]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import bench  # noqa: E402
from surfelmeshing_amd import _lib, api  # noqa: E402
from surfelmeshing_amd._lib import TrackParams, TrackResult, TrackRGBDParams, TrackRGBDResult  # noqa: E402

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
    assert ctypes.sizeof(TrackResult) <= ctypes.sizeof(TrackRGBDResult) <= 256
    if args.rgbd:
        color = api.CUDABuffer(H, W, np.uint8, 3)
        color.Upload(wl.pipe.download_frame(first)[1])
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
    if args.rgbd:
        mc = api.CUDABuffer(H, W, np.uint8, 4)
        ms = timed(lambda: rec.Render(None, rp, depth=md, normal=mn, color=mc), args.reps)
        res["rgbd_render_ms"] = float(np.median(ms))
        print("render alone (disc, depth + normal + colour) median %.3f ms (min %.3f, max %.3f)" % (
            res["rgbd_render_ms"], min(ms), max(ms)), flush=True)
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
        if not args.rgbd:
            continue
        q = TrackRGBDParams.defaults(levels=levels, convergence_rotation=0.0, convergence_translation=0.0)
        ms = timed(lambda: rec.TrackRGBDAsync(None, wl.pre.depth_scaling, depth, normals, color, pred, q, result), args.reps)
        raw = result.Download().tobytes()[:ctypes.sizeof(TrackRGBDResult)]
        out2 = api.TrackRGBDOutcome(TrackRGBDResult.from_buffer_copy(raw))
        recs2 = rec.debug_track_rgbd_iterations()
        med2, rr = float(np.median(ms)), res["rgbd_render_ms"]
        assoc = sum(r["sums"][30] for r in recs2)
        dt2 = np.linalg.norm(out2.global_T_frame[:, 3].astype(np.float64) - np.asarray(truth, np.float64).reshape(3, 4)[:, 3])
        res["rgbd_" + name + "_ms"] = med2
        res["rgbd_" + name + "_iterations_ms"] = med2 - rr
        res["rgbd_" + name + "_ratio"] = med2 / med
        res["rgbd_" + name + "_photometric_inliers"] = out2.photometric_inliers
        print("%-12s rgbd median %.3f ms (min %.3f, max %.3f) = %.2f x the geometric call: render %.3f + prepare and iterations "
              "%.3f = %.1f us per iteration; %s, %d iterations, inliers %d, photometric %d (rms %.4f), %.2f mm from the generated "
              "pose; %d launches; prepare %.1f MB + %.1f MB of photometric pixel terms = %.1f us at the HBM peak" % (
                  name, med2, min(ms), max(ms), med2 / med, rr, med2 - rr, 1e3 * (med2 - rr) / iters, out2.status_name,
                  len(recs2), out2.inliers, out2.photometric_inliers, out2.rms_intensity_residual, dt2 * 1e3, launches + 1,
                  36e-6 * W * H, 19e-6 * assoc, (36.0 * W * H + 19.0 * assoc) / HBM_PEAK * 1e6), flush=True)
    res["value"] = res["default_ms"]

    # ---- the frame loop with and without a track call in front of every Integrate
    warm = 10
    total = warm + args.frames
    for j in range(-4, total + 5):
        wl.render(first + j, 4 + j)
    plan = [wl.plan(first + j, 4 + j) for j in range(total)]
    fps = {}
    default_rgbd = TrackRGBDParams.defaults()
    for name in ("no_track", "track_every_frame") + (("track_rgbd_every_frame",) if args.rgbd else ()):
        rec.debug_upload_surfels(rows, n - live)
        wl.pipe.run_array(*wl.steps(plan[:warm]))
        steps = [wl.steps(plan[a:a + 1]) for a in range(warm, total)]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k, a in enumerate(range(warm, total)):
            if name == "track_every_frame":
                rec.TrackAsync(None, wl.pre.depth_scaling, depth, normals, plan[a - 1][3], default, result)
            elif name == "track_rgbd_every_frame":
                rec.TrackRGBDAsync(None, wl.pre.depth_scaling, depth, normals, color, plan[a - 1][3], default_rgbd, result)
            wl.pipe.run_array(*steps[k])
        e1.record()
        e1.synchronize()
        fps[name] = args.frames / (e0.elapsed_time(e1) * 1e-3)
        print("%s: %d frames %.1f frames/s" % (name, args.frames, fps[name]), flush=True)
    res["frames_per_s_no_track"] = fps["no_track"]
    res["frames_per_s_track_every_frame"] = fps["track_every_frame"]
    if args.rgbd:
        res["frames_per_s_track_rgbd_every_frame"] = fps["track_rgbd_every_frame"]
    res["frames"] = args.frames
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
