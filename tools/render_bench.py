"""smx_recon_render at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, as bench.py does).

    python tools/render_bench.py [--reps 20] [--frames 100] [--json OUT]
    python tools/render_bench.py --mesh [--decimate CELL] [--reps 20] [--json OUT] [--txt OUT]

* one render at 640 x 480 (all four images), timed with device events around the call, --reps repetitions: from the
  pose of the last captured frame and from an overview pose (outside the room's corner, looking at its centre), in
  both splat modes; the scan's bytes (S and N records, 32 B per slot) against the HBM peak for scale;
* the frame loop: --frames frames in 10-frame slices, once with a render (disc, capture pose) after every slice and
  once without, from the same uploaded state, in the same process.

With --mesh it measures smx_recon_render_mesh instead: the C2 map is triangulated on the device (and decimated at CELL metres
with --decimate), the triangle array stays on the device, and from the capture pose and the overview pose it times the mesh
render per call (device events around the call) and per kernel (the library's own events: smx_recon_debug_mesh_render_timings),
with the disc and the square splat render of the same pose re-measured beside it in the same process; it prints the triangles
given, drawn and large, and the bytes of a traffic model (12 B of indices and three 32-byte S + N gathers per triangle; 8 B of
z-buffer cleared and 8 B read per pixel, 28 B of images written) against the HBM peak."""
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
ap.add_argument("--txt", default=None, help="--mesh: also write the printed lines to this file")
ap.add_argument("--mesh", action="store_true", help="measure smx_recon_render_mesh beside the splat renders")
ap.add_argument("--decimate", type=float, default=None, metavar="CELL", help="--mesh: also the mesh decimated at CELL metres")
args = ap.parse_args()
sys.argv = [sys.argv[0]]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import bench  # noqa: E402
from surfelmeshing_amd import _lib, api, render  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s (MI355X_MICROARCH.md: spec)


def timed(call, reps):
    """Milliseconds of `call` by device events around it, one warm-up call first; the list of the repetitions."""
    ms = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms[1:]


def mesh_main():
    _lib.require_gpu()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    wl = bench.Workload(api, 640, 480, 5_000_000, 5_500_000, 0x5EED0001, 0.0)
    t0 = time.time()
    g_end, _ = wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d merged" % (time.time() - t0, n, n - live))
    t0 = time.time()
    tri, _ = rec.Triangulate(None)
    say("# triangulated in %.1f s: %d triangles" % (time.time() - t0, tri.shape[0]))
    meshes = [("full", tri)]
    if args.decimate is not None:
        t0 = time.time()
        coarse, dst = rec.DecimateMesh(None, tri, args.decimate)
        say("# decimated at %g m in %.1f s: %d triangles" % (args.decimate, time.time() - t0, coarse.shape[0]))
        meshes.append(("decimated_%g" % args.decimate, coarse))
    W, H = 640, 480
    bufs = {"depth": api.CUDABuffer(H, W, np.float32), "index": api.CUDABuffer(H, W, np.uint32),
            "normal": api.CUDABuffer(H, W, np.float32, 4), "color": api.CUDABuffer(H, W, np.uint8, 4)}
    capture = wl.plan(g_end + 10, 4)[3]
    overview = render.look_at([2.6, -1.2, 2.6], [0.0, 0.0, 0.0])
    res = {"metric": "mesh_render_ms", "slots": n, "live": live, "width": W, "height": H, "reps": args.reps}
    for pose_name, T in (("capture", capture), ("overview", overview)):
        for mode_name, mode in (("square", api.SMX_SPLAT_SQUARE), ("disc", api.SMX_SPLAT_DISC)):
            p = api.make_render_params(W, H, wl.fx, wl.fy, wl.cx, wl.cy, T, splat_mode=mode)
            ms = timed(lambda: rec.Render(None, p, **bufs), args.reps)
            covered = float((bufs["index"].Download() != 0xFFFFFFFF).mean())
            key = "%s_%s" % (pose_name, mode_name)
            res[key + "_ms"], res[key + "_covered"] = float(np.median(ms)), covered
            say("%-32s median %.3f ms (min %.3f, max %.3f) over %d; %.1f %% of the pixels covered" % (
                key + " splats", np.median(ms), min(ms), max(ms), len(ms), 100 * covered))
        for mesh_name, t in meshes:
            dev = api.CUDABuffer(1, max(t.size, 1), np.uint32)
            if t.size:
                dev.Upload(t.reshape(1, -1))
            where = (dev.ToCUDA().address, t.shape[0])
            p = api.make_mesh_render_params(W, H, wl.fx, wl.fy, wl.cx, wl.cy, T)
            st = rec.RenderMesh(None, p, where, return_stats=True, **bufs)
            kernels = {"small": [], "large": [], "resolve": []}

            def call():
                rec.RenderMesh(None, p, where, **bufs)
            ms = timed(call, args.reps)
            for _ in range(args.reps):            # (once more, reading the library's own stamps after each call)
                call()
                for k, v in rec.debug_mesh_render_timings().items():
                    kernels[k].append(v)
            model = t.shape[0] * (12 + 3 * 32) + W * H * (8 + 8 + 28)
            key = "%s_mesh_%s" % (pose_name, mesh_name)
            res[key + "_ms"] = float(np.median(ms))
            res[key + "_kernels_ms"] = {k: float(np.median(v)) for k, v in kernels.items()}
            res[key + "_stats"] = st
            res[key + "_model_bytes"] = model
            say("%-32s median %.3f ms (min %.3f, max %.3f) over %d; kernels small %.3f large %.3f resolve %.3f ms; %d triangles "
                "in, %d drawn, %d large, %d clipped; %.1f %% of the pixels covered; model traffic %.0f MB = %.1f us at the HBM peak" % (
                    key, np.median(ms), min(ms), max(ms), len(ms), np.median(kernels["small"]), np.median(kernels["large"]),
                    np.median(kernels["resolve"]), st["n_in"], st["n_drawn"], st["n_large"], st["n_clipped"],
                    100.0 * st["n_covered_pixels"] / (W * H), 1e-6 * model, model / HBM_PEAK * 1e6))
            dev.close()
    res["value"] = res["capture_mesh_full_ms"]
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


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
    mesh_main() if args.mesh else main()
