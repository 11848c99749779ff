"""smx_recon_triangulate at the benchmark's C2 state (the synthetic stream grown to >= 5 M live surfels, the map
tools/compact_bench.py grows).

    python tools/mesh_bench.py [--reps 5] [--target 5000000] [--json OUT]
    python tools/mesh_bench.py --update [--target 5000000] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --decimate CELL[,CELL...] [--target 5000000] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --components [--decimate CELL[,CELL...]] [--compare_json OTHER.json] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --fill [EDGES] [--decimate CELL[,CELL...]] [--small_target N] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --distance METRES[,METRES...] [--decimate CELL[,CELL...]] [--points N] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --distance METRES[,METRES...] --scene [--decimate METRES] [--compare N] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --raycast WxH [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --raycast WxH --scene [--decimate METRES] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --register POINTS [--register_robust] [--distance METRES[,METRES...]] [--decimate METRES] [--json OUT] [--txt OUT]
    python tools/mesh_bench.py --register_global K[,M] [--distance METRES] [--decimate METRES] [--json OUT] [--txt OUT]

Times whole calls with device events around them (the call is synchronous: the window includes its host round trips)
and, from the library's own timed events (smx_recon_debug_mesh_timings), the index build, the list query, the star
kernel and agreement + scan + write separately.  Prints ms per call, surfels/s, triangles, the statistics, and bytes by
the traffic model below.  No threshold: there is no earlier time to compare with.

--update measures (medians of --reps rounds) smx_recon_triangulate_update on the same map, each figure against the full call in the
same process: one update after 1, 4 and 16 more integrated frames, then a sweep in which 1, 2, 5, 10, 20 and 40 % of the
live slots change (the surfels of the most recent creation frames are moved by 1 mm through
smx_recon_deform_by_creation_frame: a coherent part of the map, as a frame's changes are).  The update is timed as the
application calls it: one call with a device buffer that is large enough.  Every update is compared with the full call's
bytes.  The sweep runs with full_above_fraction = 1, so that the incremental path is what is measured at every point.

--decimate measures smx_recon_decimate_mesh on the same map's full mesh for every cell size given (metres):
medians of --reps calls with device arrays that are large enough, whole calls by device events and the four phases by the
library's own (smx_recon_debug_decimate_timings), triangles and vertices in and out, bytes by decimate_traffic_bytes below
against the HBM peak, and the full triangulation re-measured in the same process beside it.

--components measures smx_recon_mesh_components on the same map's full mesh and, with --decimate, on each
decimated mesh: medians of --reps calls with device arrays that are large enough, once with the default parameters (labels
and table only, everything kept) and once with min_triangles = 10; whole calls by device events and the four phases by the
library's own (smx_recon_debug_components_timings); bytes by components_traffic_bytes below against the HBM peak; the
histogram of component sizes (1, 2-9, 10-99, ..., and the largest); the full triangulation re-measured beside it.  Writes
profiles/components_bench.{txt,json} unless --txt / --json say otherwise.  --compare_json names the JSON another build of
the library wrote with the same command on the same box (SMX_LIB_PATH, tools/build_variant.sh): its per-phase times are
printed beside this build's, row by row -- the A/B of the measure phase with and without wave aggregation.

--fill [EDGES] measures smx_recon_fill_holes with max_hole_edges = EDGES (default 8) on the same map's full mesh
and, with --decimate, on each decimated mesh, then on the full mesh of a second, small map (the same stream at 160 x 120 grown
to --small_target live surfels, where the mesh has far more holes per triangle): medians of --reps calls with device arrays
that are large enough, whole calls by device events and the four phases by the library's own (smx_recon_debug_fill_timings);
every count of smx_fill_stats; the histogram of the listed loops' lengths; bytes by fill_traffic_bytes below against the HBM
peak; the full triangulation re-measured beside it.  Writes profiles/fill_bench.{txt,json} unless --txt / --json say
otherwise.

--distance METRES[,METRES...] measures smx_recon_mesh_distance for every max_distance given: --points (default
1 M) points of synth.room_surface_points (the C5 points: on the room's nominal walls with the relief, 30 mm BEHIND the surface
the stream shows, whose raycast offsets the relief inward by 0.03 m -- so the distances measure that offset, a query load with
a known answer, not a reconstruction error; run_tum.py --mesh_eval measures the error) against the same map's full mesh and, with --decimate, against each decimated mesh: medians of --reps calls with device
arrays, whole calls by device events and the four phases by the library's own (smx_recon_debug_distance_timings); points/s;
every count of smx_distance_stats and the summary line of meshing.distance_summary; bytes by distance_traffic_bytes below
against the HBM peak, the query phase's share on its own; the full triangulation re-measured beside it.  Writes
profiles/distance_bench.{txt,json} unless --txt / --json say otherwise.

--distance METRES[,METRES...] --scene measures smx_distscene on the same points and the same two meshes (the
decimated one at the first --decimate cell, 0.05 m by default), everything in one process, for every max_distance given as the
scene's bound: smx_recon_mesh_distance re-measured first (its call and its four phases, each as the median, min and max of --reps
calls: the spread every comparison allows); the scene's build by phase (mark, index, first: smx_distscene_debug_timings, over
--reps rebuilds in place), its structure and its device memory; a query at the bound and at a fifth of it (whole calls by device
events and the phases query and stats by the library's own); the bytes and statistics of the query at the bound are compared with
the call's.  With --compare N one side of a comparison, the decimated mesh's N samples against the full mesh within
--compare_distance, through meshing.compare_meshes(scene_b=) against the plain call.  Writes profiles/distscene_bench.{txt,json}
unless --txt / --json say otherwise.

--raycast WxH measures smx_recon_raycast_mesh: the W x H camera rays (meshing.camera_rays) of the bench pose --
the pose of the first frame after the growth, render_bench.py's capture pose -- against the same map's full mesh and against the
mesh decimated at 0.05 m: medians of --reps calls with device arrays, whole calls by device events and the four phases by the
library's own (smx_recon_debug_raycast_timings); rays/s; every count of smx_raycast_stats; layers, look-ups and pair tests per
ray; the index rebuild's share (mark + index) of the call; and smx_recon_render_mesh of the same pose, size and mesh measured
beside it, with the share of pixels whose index equals the rasteriser's.  Writes profiles/raycast_bench.{txt,json} unless --txt
/ --json say otherwise.

--register POINTS measures smx_distscene_register: POINTS points of synth.room_surface_points (on the device, with
the walls' normals) registered from the identity to a distance scene of the full mesh and of the decimated one (--decimate,
default 0.05 m), built for every bound of --distance (default 0.01,0.05), with the default schedule; per call the whole time and
the move, query, reduce and solve of the last iteration by the library's events, and beside them, in the same process, the
scene's plain query of the same points at the bound.  Writes profiles/register_bench.{txt,json} unless --txt / --json say otherwise.
--register POINTS --register_robust measures smx_distscene_register_robust and smx_recon_build_distscene_rim beside
the plain call and the plain build in the same process: the rim build against the scene build it extends, the robust call (rim
rejection and Tukey weights at bound, bound / 2, bound / 4) against the plain call of the same points, the robust reduce kernel
against the plain one in the last iteration.  Writes profiles/register_robust_bench.{txt,json}.
--register_global K[,M] measures smx_distscene_register_global: 4096 area samples of the full mesh, put into a frame
100 degrees and 0.44 m away, are searched for with the lattice of order K on one anchor and M starts (8), against a scene of the
full mesh and of the decimated one: the score phase and its move, query and score kernel by the library's events, the scene's
plain query of the identical P m moved points in the same process, the whole call with select, refine and rescore, and how far the
winner lies from the truth.  Writes profiles/register_global_bench.{txt,json}.

--raycast WxH --scene measures smx_rayscene on the same rays and the same two meshes (the decimated one at the
first --decimate cell, 0.05 m by default), everything in one process: smx_recon_raycast_mesh re-measured first (its call, its
phases, and the min and max of its cast + stats over the repetitions: the spread every comparison allows); then for occupancy
-1, 0 and every explicit block size that fits: the build by phase (smx_rayscene_debug_timings, medians of --reps rebuilds), the
grid's size and set bits, the scene's device memory, cast + stats as the median, min and max of --reps casts with device
arrays, and the five work counters per ray; the bytes of every cast are compared with the call's.  The last two lines say whether
a cast without a grid stays within the call's cast + stats plus the spread, and whether the smallest grid that fits pays by the
rule of DESIGN.md 5m.  Writes profiles/rayscene_bench.{txt,json} unless --txt / --json say otherwise.

--sample N[,N...] measures smx_recon_sample_mesh on the full mesh of the same map and on its decimation at each
--decimate cell size, for every sample count given; --compare N measures smx_recon_compare_meshes, the full mesh against each
decimated one with N samples per side within --compare_distance.  Per call and per phase by the library's events; a traffic
model against the HBM peak; the full triangulation re-measured beside it.  Writes profiles/sample_bench.{txt,json} unless --txt /
--json say otherwise."""
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
ap.add_argument("--decimate", default=None, help="comma-separated cell sizes in metres")
ap.add_argument("--components", action="store_true")
ap.add_argument("--compare_json", default=None, help="with --components: the JSON of another build's run, printed beside this one")
ap.add_argument("--fill", type=int, nargs="?", const=8, default=None, metavar="EDGES", help="measure smx_recon_fill_holes with this max_hole_edges")
ap.add_argument("--small_target", type=int, default=50_000, help="with --fill: live surfels of the second, 160 x 120 map (0 = none)")
ap.add_argument("--distance", default=None, metavar="METRES[,METRES...]", help="measure smx_recon_mesh_distance at these max_distance values")
ap.add_argument("--points", type=int, default=1_000_000, help="with --distance: query points on the analytic room surface")
ap.add_argument("--sample", default=None, metavar="N[,N...]", help="measure smx_recon_sample_mesh at these sample counts")
ap.add_argument("--compare", type=int, default=0, metavar="N", help="measure smx_recon_compare_meshes, full mesh against each --decimate mesh, N samples per side")
ap.add_argument("--compare_distance", type=float, default=0.05, metavar="METRES", help="with --compare: max_distance")
ap.add_argument("--raycast", default=None, metavar="WxH", help="measure smx_recon_raycast_mesh with the camera rays of the bench pose")
ap.add_argument("--scene", action="store_true", help="with --raycast: measure smx_rayscene (build by phase, cast for every occupancy setting) "
                                                      "beside smx_recon_raycast_mesh, on the full mesh and the one decimated at the first --decimate cell; "
                                                      "with --distance: measure smx_distscene (build by phase, queries) beside smx_recon_mesh_distance")
ap.add_argument("--register", type=int, default=0, metavar="POINTS", help="measure smx_distscene_register of this many room-surface points "
                                                                           "against the full and the decimated mesh at the --distance bounds")
ap.add_argument("--register_robust", action="store_true", help="with --register: the robust call (rim rejection and Tukey weights) and the rim build, "
                                                               "timed beside the plain call and the plain build")
ap.add_argument("--register_global", default=None, metavar="K[,M]", help="measure smx_distscene_register_global: the lattice of order K, M starts (8), "
                                                                          "against the full and the decimated mesh at the first --distance bound (0.05)")
ap.add_argument("--label", default="this build", help="with --components: the name of the build under test in the output")
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


HBM_PEAK = 8.0e12   # bytes/s (MI355X spec)
DECIMATE_PHASES = ("cluster", "remap_dedupe", "survivors", "order")


def _table_size(entries):
    s = 64
    while s < 2 * entries:
        s *= 2
    return s


def decimate_traffic_bytes(n, st):
    """HBM bytes of one smx_recon_decimate_mesh call over n slots, by phase, from its statistics.  Gathers are counted once
    per distinct target (a lower bound: neighbouring triangles share corners and mostly hit in cache), an atomic as a read
    and a write of its entry; the host round trips between the phases move a few words."""
    n_in, used, T = st["n_in"], st["n_used_vertices"], st["n_triangles"]
    alive = T + st["n_duplicates"]
    bits = max(1, int(n - 1).bit_length())
    cluster = (4 * n + 16 * _table_size(min(n, 3 * n_in))      # vmap and the cell table reset
               + 12 * n_in + 32 * used + 4 * used               # mark: the input, S and N records of the corners, U
               + 4 * n + 16 * used + 2 * 32 * used + 4 * used   # insert: vmap, S records, CAS + min on a 16-byte entry, vmap
               + 4 * n + 16 * used + 4 * used)                  # look up
    remap = (4 * _table_size(n_in) + 12 * n_in + 4 * used + 12 * n_in        # reset; the input, vmap gathers, canonical triples
             + 12 * n_in + 8 * alive + 12 * st["n_duplicates"] + 4 * n_in)  # duplicates: triples, the entry, the resident's triple, own
    survivors = 2 * (4 * n_in + 4 * alive) + 8 * (n_in // 256 + 1) + 12 * T + 12 * T
    passes = -(-2 * bits // 8) + -(-bits // 8)
    order = passes * 32 * T + (4 + 12 + 12) * T + (4 + 12 + 12) * T          # per pass: keys twice, values, both written
    return dict(zip(DECIMATE_PHASES, (cluster, remap, survivors, order)))


def decimate_main():
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    cells = [float(c) for c in args.decimate.split(",")]
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    rows = rec.debug_download_surfels()
    spacing = float(np.median(np.sqrt(rows[7][rows[7] >= 0])))
    del rows
    say("# grown in %.1f s: %d slots, %d live; median surfel radius %.4f m" % (time.time() - t0, n, live, spacing))
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, dout, dmap = api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, n, np.uint32)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def full():
        T, st = C.c_uint32(0), _lib.MeshStats()
        _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address),
                                           C.c_uint32(cap), C.c_int32(1), C.byref(T), C.byref(st)))
        return T.value

    def decimate(cell, n_in):
        T, st = C.c_uint32(0), _lib.DecimateStats()
        _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(n_in),
                                             C.c_void_p(dout.ToCUDA().address), C.c_uint32(cap), C.c_void_p(dmap.ToCUDA().address),
                                             C.c_int32(1), C.byref(T), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in _lib.DecimateStats._fields_}
    t_full, ph_full = [], []
    for _ in range(args.reps + 1):
        ms, T_in = timed(full)
        t_full.append(ms)
        ph_full.append(sum(rec.debug_mesh_timings().values()))
    full_ms, full_events_ms = float(np.median(t_full[1:])), float(np.median(ph_full[1:]))
    say("full triangulation, re-measured here: %d triangles, one call %.2f ms (%.2f ms by the library's events)" % (T_in, full_ms, full_events_ms))
    out_rows = []
    for cell in cells:
        t, phs, st, first = [], [], None, None
        for _ in range(args.reps + 1):
            ms, st = timed(lambda: decimate(cell, T_in))
            t.append(ms)
            phs.append(rec.debug_decimate_timings())
            head = dout.Download()[0][:3 * min(st["n_triangles"], 100000)].tobytes()
            first = head if first is None else first
            assert head == first, "two calls gave different bytes"
        med = float(np.median(t[1:]))                       # (the first call allocates the workspace)
        ph = {k: float(np.median([q[k] for q in phs[1:]])) for k in DECIMATE_PHASES}
        b = decimate_traffic_bytes(n, st)
        tot = sum(b.values())
        say("cell %.4f m (%.1f radii): %d -> %d triangles, %d -> %d vertices (%d collapsed, %d duplicates) | call %.2f ms (min %.2f, "
            "max %.2f) = %.2f x the full triangulation | %s | model %.2f GB -> %.2f TB/s = %.0f %% of the %.1f TB/s HBM peak (%s)" % (
                cell, cell / spacing, st["n_in"], st["n_triangles"], st["n_used_vertices"], st["n_cells"], st["n_collapsed"],
                st["n_duplicates"], med, min(t[1:]), max(t[1:]), med / full_ms,
                " ".join("%s %.2f" % (k, ph[k]) for k in DECIMATE_PHASES), tot / 1e9, tot / (med * 1e-3) / 1e12,
                100.0 * tot / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12,
                " ".join("%s %.0f %%" % (k, 100.0 * b[k] / (max(ph[k], 1e-6) * 1e-3) / HBM_PEAK) for k in DECIMATE_PHASES)))
        out_rows.append({"cell_size": cell, "cell_in_median_radii": cell / spacing, "reps": len(t) - 1, "call_ms": med, "call_ms_all": t[1:],
                         "phases_ms": ph, "stats": st, "traffic_model_bytes": b, "fraction_of_hbm_peak": tot / (med * 1e-3) / HBM_PEAK,
                         "ratio_to_full_triangulation": med / full_ms})
    res = {"metric": "decimate_mesh_ms", "slots": n, "live": live, "median_surfel_radius_m": spacing, "triangles_in": T_in,
           "full_triangulation_ms": full_ms, "full_triangulation_events_ms": full_events_ms, "rows": out_rows}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")
    for b in (dtri, dout, dmap):
        b.close()
    nn.close()


COMPONENTS_PHASES = ("mark_link", "flatten_number", "measure", "write")


def components_traffic_bytes(n, st, labels_out=True, table_out=True):
    """HBM bytes of one smx_recon_mesh_components call over n slots, by phase, from its statistics.  Gathers are counted once
    per distinct target (a lower bound: neighbouring triangles share corners and mostly hit in cache); a find is counted as
    two loads of parent per corner (the word and its parent: a lower bound, the trees are shallow once halved), a hook or a
    halving as a read and a write of one word; the aggregated atomics of the measure phase are a few words per wavefront and
    not counted.  The two reads of the counters move a few words."""
    n_in, used, C, T = st["n_in"], st["n_used_vertices"], st["n_components"], st["n_triangles"]
    rem = n_in - st["n_not_live"]
    mark_link = (4 * n + 12 * n_in + 32 * used + 4 * used + 4 * n_in       # reset; mark: the input, S and N of the corners, roots, tcomp
                 + 12 * n_in + 4 * n_in + 2 * 4 * 3 * rem + 8 * used)      # link: the input, tcomp, the finds, one hook per slot
    flatten = 4 * n + 2 * 4 * used + 4 * n + 8 * (n // 256 + 1) + 4 * n + 4 * C   # flatten: parent, finds, label; scan; number: label, roots
    measure = (4 * n + 4 * used + 16 * used                                # vertices: label, dense number, S record
               + 4 * n_in + 4 * rem + 4 * rem + 4 * rem + 4 * rem          # triangles: tcomp, first corner, its label, dense number, tcomp
               + 32 * C + 32 * C + 40 * C)                                 # accumulators reset and read, the table
    write = (2 * (4 * n_in + 4 * rem) + 8 * (n_in // 256 + 1) + 12 * T + 12 * T   # count and write: tcomp, kept; the triangles in and out
             + (8 * n if labels_out else 0) + (80 * C if table_out else 0))
    return dict(zip(COMPONENTS_PHASES, (mark_link, flatten, measure, write)))


def size_histogram(n_triangles):
    """Component sizes in triangles: how many components in 1, 2-9, 10-99, ..., and the largest."""
    sizes = np.asarray(n_triangles, np.int64)
    rows, lo = [], 1
    if sizes.size:
        rows.append(("1", int(np.sum(sizes == 1)), int(sizes[sizes == 1].sum())))
        lo = 2
        while lo <= int(sizes.max()):
            hi = 10 if lo == 2 else lo * 10
            sel = (sizes >= lo) & (sizes < hi)
            rows.append(("%d-%d" % (lo, hi - 1), int(sel.sum()), int(sizes[sel].sum())))
            lo = hi
    return rows, int(sizes.max()) if sizes.size else 0


def components_main():
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    cells = [float(c) for c in args.decimate.split(",")] if args.decimate else []
    other = json.load(open(args.compare_json)) if args.compare_json else None
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# %s; grown in %.1f s: %d slots, %d live" % (args.label, time.time() - t0, n, live))
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, ddec, dout, dlab = (api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32),
                              api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, n, np.uint32))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def full():
        T, st = C.c_uint32(0), _lib.MeshStats()
        _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address),
                                           C.c_uint32(cap), C.c_int32(1), C.byref(T), C.byref(st)))
        return T.value

    def components(src, n_in, prm, dtab, tab_cap):
        T, nc, st = C.c_uint32(0), C.c_uint32(0), _lib.ComponentsStats()
        rc = L.smx_recon_mesh_components(rec._h, None, C.byref(prm), C.c_void_p(src.ToCUDA().address), C.c_uint32(n_in),
                                         C.c_void_p(dout.ToCUDA().address), C.c_uint32(cap), C.c_void_p(dlab.ToCUDA().address),
                                         C.c_void_p(dtab.ToCUDA().address) if dtab is not None else None, C.c_uint32(tab_cap),
                                         C.c_int32(1), C.byref(T), C.byref(nc), C.byref(st))
        _lib.check(rc)
        return {k: int(getattr(st, k)) for k, _ in _lib.ComponentsStats._fields_}
    t_full = []
    for _ in range(args.reps + 1):
        ms, T_in = timed(full)
        t_full.append(ms)
    full_ms = float(np.median(t_full[1:]))
    say("full triangulation, re-measured here: %d triangles, one call %.2f ms" % (T_in, full_ms))
    inputs = [("full mesh", dtri, T_in)]
    out_rows = []
    for cell in cells:
        T, st = C.c_uint32(0), _lib.DecimateStats()
        _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                             C.c_void_p(ddec.ToCUDA().address), C.c_uint32(cap), None, C.c_int32(1), C.byref(T), C.byref(st)))
        coarse = api.CUDABuffer(1, 3 * max(T.value, 1), np.uint32)           # (an array of its own: ddec is reused by the next cell)
        coarse.Upload(np.ascontiguousarray(ddec.Download()[:, :3 * max(T.value, 1)]))
        inputs.append(("decimated at %g m" % cell, coarse, T.value))
    for what, src, n_in in inputs:
        first = components(src, n_in, _lib.ComponentsParams(0, 0.0, 0), None, 0)          # (allocates; tells the table's size)
        Cn = first["n_components"]
        dtab = api.CUDABuffer(1, 10 * max(Cn, 1), np.uint32)
        for prm_name, prm in (("default", _lib.ComponentsParams(0, 0.0, 0)), ("min_triangles 10", _lib.ComponentsParams(10, 0.0, 0))):
            t, phs, st, head0 = [], [], None, None
            for _ in range(args.reps + 1):
                ms, st = timed(lambda: components(src, n_in, prm, dtab, Cn))
                t.append(ms)
                phs.append(rec.debug_components_timings())
                head = dout.Download()[0][:3 * min(st["n_triangles"], 100000)].tobytes() + dtab.Download()[0].tobytes()
                head0 = head if head0 is None else head0
                assert head == head0, "two calls gave different bytes"
            med = float(np.median(t[1:]))
            ph = {k: float(np.median([q[k] for q in phs[1:]])) for k in COMPONENTS_PHASES}
            b = components_traffic_bytes(n, st)
            tot = sum(b.values())
            say("%s, %s: %d -> %d triangles, %d used vertices, %d components (%d kept, the largest has %d triangles) | call %.2f ms "
                "(min %.2f, max %.2f) = %.3f x the full triangulation | %s | model %.2f GB -> %.2f TB/s = %.0f %% of the %.1f TB/s "
                "HBM peak (%s)" % (
                    what, prm_name, st["n_in"], st["n_triangles"], st["n_used_vertices"], st["n_components"], st["n_kept_components"],
                    st["n_largest_triangles"], med, min(t[1:]), max(t[1:]), med / full_ms,
                    " ".join("%s %.3f" % (k, ph[k]) for k in COMPONENTS_PHASES), tot / 1e9, tot / (med * 1e-3) / 1e12,
                    100.0 * tot / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12,
                    " ".join("%s %.0f %%" % (k, 100.0 * b[k] / (max(ph[k], 1e-6) * 1e-3) / HBM_PEAK) for k in COMPONENTS_PHASES)))
            row = {"input": what, "params": prm_name, "reps": len(t) - 1, "call_ms": med, "call_ms_all": t[1:], "phases_ms": ph,
                   "phases_ms_all": phs[1:], "stats": st, "traffic_model_bytes": b, "fraction_of_hbm_peak": tot / (med * 1e-3) / HBM_PEAK,
                   "ratio_to_full_triangulation": med / full_ms}
            if other is not None:
                theirs = [r for r in other["rows"] if r["input"] == what and r["params"] == prm_name]
                if theirs and theirs[0]["stats"] == st:
                    o = theirs[0]
                    say("    %s on the same box: call %.2f ms | %s | measure phase %.3f ms here against %.3f ms there (all: %s | %s)" % (
                        other["label"], o["call_ms"], " ".join("%s %.3f" % (k, o["phases_ms"][k]) for k in COMPONENTS_PHASES),
                        ph["measure"], o["phases_ms"]["measure"], " ".join("%.3f" % q["measure"] for q in phs[1:]),
                        " ".join("%.3f" % q["measure"] for q in o["phases_ms_all"])))
                    row["compared_with"] = {"label": other["label"], "call_ms": o["call_ms"], "phases_ms": o["phases_ms"],
                                            "phases_ms_all": o["phases_ms_all"]}
                else:
                    say("    %s: no row with the same input and statistics" % other["label"])
            if prm_name == "default":
                table = dtab.Download()[0][:10 * Cn].view(api.COMPONENT_DTYPE)
                hist, largest = size_histogram(table["n_triangles"])
                say("    component sizes in triangles (components / their triangles): %s; the largest has %d = %.2f %% of the mesh" % (
                    ", ".join("%s: %d / %d" % h for h in hist), largest, 100.0 * largest / max(st["n_in"] - st["n_not_live"], 1)))
                row["size_histogram"] = [{"triangles": h[0], "components": h[1], "triangles_in_them": h[2]} for h in hist]
                row["largest_component_triangles"] = largest
            out_rows.append(row)
        dtab.close()
    res = {"metric": "mesh_components_ms", "label": args.label, "slots": n, "live": live, "triangles_in": T_in,
           "full_triangulation_ms": full_ms, "rows": out_rows}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(args.json or os.path.join(ROOT, "profiles", "components_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "components_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    for what, src, _ in inputs[1:]:
        src.close()
    for b in (dtri, ddec, dout, dlab):
        b.close()
    nn.close()


FILL_PHASES = ("edges", "loops", "fill", "write")


def fill_traffic_bytes(n, st, max_hole_edges):
    """HBM bytes of one smx_recon_fill_holes call over n slots, by phase, from its statistics.  Gathers are counted once per
    distinct target (a lower bound), an insert as a read and a write of the 16-byte entry it ends at (the probes before it are
    not counted), an atomic on out / in as a read and a write of its word; the two reads of the counters move a few words."""
    n_in, T = st["n_in"], st["n_triangles"]
    rem = n_in - st["n_not_live"]
    used = st["n_edges"] * 2 // 3 + 1                      # about the vertices of a mesh with that many edges (V ~ E / 3 ... E / 1.5)
    entries = _table_size(3 * n_in)
    edges = (16 * entries + 8 * n                          # the table and out / in reset
             + 12 * n_in + 32 * used + 4 * n_in            # the input, S and N of the corners, the keep flags
             + 2 * 16 * 3 * rem                            # three inserts per triangle of R
             + 8 * (n_in // 256 + 1)                       # the scan
             + 16 * entries + (8 + 8 + 4) * st["n_boundary_edges"])   # classify: every entry read; out, in, next of a boundary pair
    loops = 8 * n + 4 * n + (8 + 4) * st["n_boundary_edges"] + 8 * (n // 256 + 1) + 4 * n + 12 * st["n_listed_loops"]
    new = st["n_new_triangles"]
    bits = max(1, int(n - 1).bit_length())
    passes = -(-2 * bits // 8) + -(-bits // 8)
    fill = st["n_listed_loops"] * (12 + max_hole_edges * (4 + 32) + 16 * max_hole_edges + 4) + 12 * new + passes * 32 * new + 2 * 28 * new
    write = 2 * 4 * n_in + 12 * rem + 12 * rem + 12 * new + 12 * new + 12 * st["n_listed_loops"]
    return dict(zip(FILL_PHASES, (edges, loops, fill, write)))


def fill_main():
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines, out_rows, maps = [], [], []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    cells = [float(c) for c in args.decimate.split(",")] if args.decimate else []
    prm = api.fill_params(args.fill)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def one_map(name, width, height, target, cells):
        wl = bench.Workload(api, width, height, target, target + target // 10 + 20000, 0x5EED0001, 0.0)
        t0 = time.time()
        wl.grow(False)
        rec = wl.pipe.reconstruction
        n, live = rec.surfels_size(), rec.surfel_count()
        say("# %s: %d x %d, grown in %.1f s: %d slots, %d live" % (name, width, height, time.time() - t0, n, live))
        nn = api.SurfelNeighborIndex()
        p = _lib.MeshParams.defaults()
        cap = 3 * n
        dtri, ddec, dout = (api.CUDABuffer(1, 3 * cap, np.uint32) for _ in range(3))

        def full():
            T, st = C.c_uint32(0), _lib.MeshStats()
            _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address),
                                               C.c_uint32(cap), C.c_int32(1), C.byref(T), C.byref(st)))
            return T.value

        def fill(src, n_in, dtab, tab_cap):
            T, kept, nh, st = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), _lib.FillStats()
            _lib.check(L.smx_recon_fill_holes(rec._h, None, C.byref(prm), C.c_void_p(src.ToCUDA().address), C.c_uint32(n_in),
                                              C.c_void_p(dout.ToCUDA().address), C.c_uint32(cap),
                                              C.c_void_p(dtab.ToCUDA().address) if dtab is not None else None, C.c_uint32(tab_cap),
                                              C.c_int32(1), C.byref(T), C.byref(kept), C.byref(nh), C.byref(st)))
            return {k: int(getattr(st, k)) for k, _ in _lib.FillStats._fields_}
        t_full = []
        for _ in range(args.reps + 1):
            ms, T_in = timed(full)
            t_full.append(ms)
        full_ms = float(np.median(t_full[1:]))
        say("%s: full triangulation, re-measured here: %d triangles, one call %.2f ms" % (name, T_in, full_ms))
        inputs = [("full mesh", dtri, T_in)]
        for cell in cells:
            T, st = C.c_uint32(0), _lib.DecimateStats()
            _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                                 C.c_void_p(ddec.ToCUDA().address), C.c_uint32(cap), None, C.c_int32(1), C.byref(T), C.byref(st)))
            coarse = api.CUDABuffer(1, 3 * max(T.value, 1), np.uint32)
            coarse.Upload(np.ascontiguousarray(ddec.Download()[:, :3 * max(T.value, 1)]))
            inputs.append(("decimated at %g m" % cell, coarse, T.value))
        for what, src, n_in in inputs:
            H = fill(src, n_in, None, 0)["n_listed_loops"]             # (allocates; tells the table's size)
            dtab = api.CUDABuffer(1, 3 * max(H, 1), np.uint32)
            t, phs, st, head0 = [], [], None, None
            for _ in range(args.reps + 1):
                ms, st = timed(lambda: fill(src, n_in, dtab, H))
                t.append(ms)
                phs.append(rec.debug_fill_timings())
                new = dout.Download()[0][3 * (st["n_triangles"] - st["n_new_triangles"]):3 * st["n_triangles"]]
                head = new[:300000].tobytes() + dtab.Download()[0].tobytes()
                head0 = head if head0 is None else head0
                assert head == head0, "two calls gave different bytes"
            med = float(np.median(t[1:]))
            ph = {k: float(np.median([q[k] for q in phs[1:]])) for k in FILL_PHASES}
            b = fill_traffic_bytes(n, st, args.fill)
            tot = sum(b.values())
            say("%s, %s, max_hole_edges %d: %s | call %.2f ms (min %.2f, max %.2f) = %.3f x the full triangulation | %s | model %.2f GB -> "
                "%.2f TB/s = %.0f %% of the %.1f TB/s HBM peak (%s)" % (
                    name, what, args.fill, " ".join("%s %d" % (k, st[k]) for k, _ in _lib.FillStats._fields_), med, min(t[1:]), max(t[1:]),
                    med / full_ms, " ".join("%s %.3f" % (k, ph[k]) for k in FILL_PHASES), tot / 1e9, tot / (med * 1e-3) / 1e12,
                    100.0 * tot / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12,
                    " ".join("%s %.0f %%" % (k, 100.0 * b[k] / (max(ph[k], 1e-6) * 1e-3) / HBM_PEAK) for k in FILL_PHASES)))
            table = dtab.Download()[0][:3 * H].view(api.HOLE_DTYPE)
            hist = np.bincount(table["n_edges"], minlength=args.fill + 1)[3:].tolist()
            by_status = np.bincount(table["status"], minlength=4)[1:4].tolist()
            say("    listed loops by length 3 .. %d: %s; filled / diagonal / filter: %s; boundary edges left %d of %d" % (
                args.fill, hist, by_status, st["n_boundary_edges"] - int(table["n_edges"][table["status"] == 1].sum()), st["n_boundary_edges"]))
            out_rows.append({"map": name, "input": what, "max_hole_edges": args.fill, "reps": len(t) - 1, "call_ms": med, "call_ms_all": t[1:],
                             "phases_ms": ph, "phases_ms_all": phs[1:], "stats": st, "loop_length_histogram_from_3": hist,
                             "loops_filled_diagonal_filter": by_status, "traffic_model_bytes": b,
                             "fraction_of_hbm_peak": tot / (med * 1e-3) / HBM_PEAK, "ratio_to_full_triangulation": med / full_ms})
            dtab.close()
        maps.append({"map": name, "width": width, "height": height, "slots": n, "live": live, "triangles_in": T_in, "full_triangulation_ms": full_ms})
        for _, src, _ in inputs[1:]:
            src.close()
        for buf in (dtri, ddec, dout):
            buf.close()
        nn.close()
    one_map("C2", 640, 480, args.target, cells)
    if args.small_target > 0:
        one_map("small", 160, 120, args.small_target, [])
    res = {"metric": "mesh_fill_holes_ms", "label": args.label, "maps": maps, "rows": out_rows}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(args.json or os.path.join(ROOT, "profiles", "fill_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "fill_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


UPDATE_PHASES = ("diff", "index_builds", "reverse_test", "subset_lists", "stars", "agree_merge")


DIST_PHASES = ("mark", "index", "query", "stats")


def distance_traffic_bytes(n, n_in, n_points, st):
    """HBM bytes of one smx_recon_mesh_distance call, by phase, from its statistics: a lower bound.  Gathers are counted once per
    distinct target, a sort pass as its keys and values read twice and written once, an atomic as a read and a write of its
    entry; the query as every record and every occupied table entry read ONCE (lanes of one cell share them, neighbouring cells
    mostly hit in cache) plus the points and the outputs; the wide list once per wavefront."""
    E, Wd, P = st["n_entries"], st["n_wide"], n_points
    corners = min(n, 3 * n_in)
    mark = 2 * 12 * n_in + 2 * 32 * corners + 2 * 4 * n_in + 4 * Wd + 8 * (n_in // 256 + 1)
    index = (12 * n_in + 16 * corners + 12 * E                     # entries: the input, S records, keys and values
             + 8 * 36 * E                                          # eight sort passes
             + 4 * E + 12 * E + 16 * corners + 48 * (E + Wd)       # records
             + 16 * _table_size(E) + 8 * E + 32 * st["n_cells"])   # the table: reset, keys read, head and tail claims
    query = (12 * P + 12 * P + 8 * 36 * P                          # the points' keys and their sort
             + 4 * P + 12 * P + 16 * st["n_cells"] + 48 * E + 48 * Wd * (P // 64 + 1)
             + 36 * st["n_matched"] + 28 * P)                      # the winner's corners; key, nearest, distance, closest
    stats = 12 * P + 8 * P
    return dict(zip(DIST_PHASES, (mark, index, query, stats)))


def distance_main():
    import ctypes as C
    from surfelmeshing_amd import meshing, synth
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    maxes = [float(c) for c in args.distance.split(",")]
    cells = [float(c) for c in args.decimate.split(",")] if args.decimate else []
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n, live))
    pts = np.ascontiguousarray(synth.room_surface_points(args.points)[0], np.float32)
    P = pts.shape[0]
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, dout = api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32)
    dpts, dnear, ddist = api.CUDABuffer(1, 3 * P, np.float32), api.CUDABuffer(1, P, np.uint32), api.CUDABuffer(1, P, np.float32)
    dpts.Upload(pts.reshape(1, -1))
    say("# %d query points of synth.room_surface_points: the nominal walls, 30 mm behind the surface the stream shows" % P)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def full():
        T, st = C.c_uint32(0), _lib.MeshStats()
        _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address),
                                           C.c_uint32(cap), C.c_int32(1), C.byref(T), C.byref(st)))
        return T.value

    def distance(src, n_in, max_distance):
        prm, st = api.distance_params(max_distance), _lib.DistanceStats()
        _lib.check(L.smx_recon_mesh_distance(rec._h, None, C.byref(prm), C.c_void_p(src.ToCUDA().address), C.c_uint32(n_in),
                                             C.c_void_p(dpts.ToCUDA().address), C.c_uint32(P), C.c_void_p(dnear.ToCUDA().address),
                                             C.c_void_p(ddist.ToCUDA().address), None, C.c_int32(1), C.byref(st)))
        return api.distance_stats_dict(st)
    t_full = []
    for _ in range(args.reps + 1):
        ms, T_in = timed(full)
        t_full.append(ms)
    full_ms = float(np.median(t_full[1:]))
    say("full triangulation, re-measured here: %d triangles, one call %.2f ms" % (T_in, full_ms))
    inputs = [("full mesh", dtri, T_in)]
    for cell in cells:
        T, st = C.c_uint32(0), _lib.DecimateStats()
        buf = api.CUDABuffer(1, 3 * max(1, T_in), np.uint32) if len(inputs) > 1 else dout
        _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                             C.c_void_p(buf.ToCUDA().address), C.c_uint32(T_in), None, C.c_int32(1), C.byref(T), C.byref(st)))
        inputs.append(("decimated at %g m" % cell, buf, T.value))
    out_rows = []
    for what, src, n_in in inputs:
        for md in maxes:
            t, phs, st, first = [], [], None, None
            for _ in range(args.reps + 1):
                ms, st = timed(lambda: distance(src, n_in, md))
                t.append(ms)
                phs.append(rec.debug_distance_timings())
                head = dnear.Download()[0][:100000].tobytes() + ddist.Download()[0][:100000].tobytes()
                first = head if first is None else first
                assert head == first, "two calls gave different bytes"
            med = float(np.median(t[1:]))                       # (the first call allocates the workspace)
            ph = {k: float(np.median([q[k] for q in phs[1:]])) for k in DIST_PHASES}
            b = distance_traffic_bytes(n, n_in, P, st)
            tot = sum(b.values())
            st["max_distance"] = md
            summary = meshing.distance_summary(ddist.Download()[0], st)
            say("%s, max_distance %g m: %d triangles (%d not live, %d repeated, %d out of range), cell %.4f m, %d entries in %d cells, %d wide | "
                "call %.2f ms (min %.2f, max %.2f) = %.2f x the full triangulation, %.2f M points/s | %s | model %.2f GB -> %.0f %% of the "
                "%.1f TB/s HBM peak (%s) | %s" % (
                    what, md, n_in, st["n_not_live"], st["n_repeated"], st["n_out_of_range"], st["cell_size_used"], st["n_entries"], st["n_cells"],
                    st["n_wide"], med, min(t[1:]), max(t[1:]), med / full_ms, P / (med * 1e-3) / 1e6,
                    " ".join("%s %.2f" % (k, ph[k]) for k in DIST_PHASES), tot / 1e9, 100.0 * tot / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12,
                    " ".join("%s %.0f %%" % (k, 100.0 * b[k] / (max(ph[k], 1e-6) * 1e-3) / HBM_PEAK) for k in DIST_PHASES),
                    meshing.format_distance_summary(summary)))
            out_rows.append({"input": what, "max_distance": md, "triangles_in": n_in, "points": P, "reps": len(t) - 1, "call_ms": med,
                             "call_ms_all": t[1:], "phases_ms": ph, "points_per_s": P / (med * 1e-3), "stats": st, "summary": summary,
                             "traffic_model_bytes": b, "fraction_of_hbm_peak": tot / (med * 1e-3) / HBM_PEAK,
                             "query_fraction_of_hbm_peak": b["query"] / (max(ph["query"], 1e-6) * 1e-3) / HBM_PEAK,
                             "ratio_to_full_triangulation": med / full_ms})
    res = {"metric": "mesh_distance_ms", "slots": n, "live": live, "triangles_in": T_in, "full_triangulation_ms": full_ms, "rows": out_rows}
    with open(args.json or os.path.join(ROOT, "profiles", "distance_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "distance_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nn.close()


DISTSCENE_BUILD_PHASES = ("mark", "index", "first")
DISTSCENE_QUERY_PHASES = ("query", "stats")


def distscene_main():
    """--distance METRES[,METRES...] --scene: smx_distscene beside smx_recon_mesh_distance in one process."""
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    maxes = [float(c) for c in args.distance.split(",")]
    cell = float(args.decimate.split(",")[0]) if args.decimate else 0.05
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n, live))
    from surfelmeshing_amd import meshing, synth
    pts = np.ascontiguousarray(synth.room_surface_points(args.points)[0], np.float32)
    P = pts.shape[0]
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, dout = api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32)
    dpts, dnear, ddist = api.CUDABuffer(1, 3 * P, np.float32), api.CUDABuffer(1, P, np.uint32), api.CUDABuffer(1, P, np.float32)
    dpts.Upload(pts.reshape(1, -1))
    say("# %d query points of synth.room_surface_points; medians of %d repetitions after one that allocates" % (P, args.reps))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def spread(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

    def show(s):
        return "%.3f ms (min %.3f, max %.3f)" % (s["median"], s["min"], s["max"])

    def answer():
        return dnear.Download()[0][:100000].tobytes() + ddist.Download()[0][:100000].tobytes()
    T, mst = C.c_uint32(0), _lib.MeshStats()
    _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(cap),
                                       C.c_int32(1), C.byref(T), C.byref(mst)))
    T_in = T.value
    Tc, dst = C.c_uint32(0), _lib.DecimateStats()
    _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                         C.c_void_p(dout.ToCUDA().address), C.c_uint32(T_in), None, C.c_int32(1), C.byref(Tc), C.byref(dst)))
    inputs = [("full mesh", dtri, T_in), ("decimated at %g m" % cell, dout, Tc.value)]
    out_rows = []
    for what, src, n_in in inputs:
        tri = _DeviceArray(src, 3 * n_in)
        for md in maxes:
            # ---- the call, re-measured beside the rest
            prm, st = api.distance_params(md), _lib.DistanceStats()
            whole, phs = [], []
            for _ in range(args.reps + 1):
                whole.append(timed(lambda: _lib.check(L.smx_recon_mesh_distance(
                    rec._h, None, C.byref(prm), C.c_void_p(src.ToCUDA().address), C.c_uint32(n_in), C.c_void_p(dpts.ToCUDA().address), C.c_uint32(P),
                    C.c_void_p(dnear.ToCUDA().address), C.c_void_p(ddist.ToCUDA().address), None, C.c_int32(1), C.byref(st))))[0])
                phs.append(rec.debug_distance_timings())
            want = answer()
            call = {"call": spread(whole[1:]), "phases": {k: spread([q[k] for q in phs[1:]]) for k in DIST_PHASES}}
            cst = api.distance_stats_dict(st)
            say("%s, max_distance %g m, %d triangles: smx_recon_mesh_distance %s | %s" % (
                what, md, n_in, show(call["call"]), " | ".join("%s %s" % (k, show(call["phases"][k])) for k in DIST_PHASES)))
            # ---- the scene's build
            scene = rec.BuildDistanceScene(None, tri, md)
            builds = []
            for _ in range(args.reps):
                rec.BuildDistanceScene(None, tri, md, scene=scene)
                builds.append(scene.debug_timings())
            build = {k: spread([q[k] for q in builds]) for k in DISTSCENE_BUILD_PHASES}
            bst = scene.stats
            assert all(bst[k] == cst[k] for k in ("n_wide", "n_entries", "n_cells", "cell_size_used")), "the scene's structure differs from the call's"
            say("  scene build: %s | sum of medians %.3f ms against the call's mark + index %.3f ms; cell %.4f m, %d entries in %d cells, %d wide, "
                "%.1f MiB on the device (first_rec %.1f MiB)" % (
                    " | ".join("%s %s" % (k, show(build[k])) for k in DISTSCENE_BUILD_PHASES), sum(build[k]["median"] for k in DISTSCENE_BUILD_PHASES),
                    call["phases"]["mark"]["median"] + call["phases"]["index"]["median"], bst["cell_size_used"], bst["n_entries"], bst["n_cells"],
                    bst["n_wide"], bst["device_bytes"] / 2.0 ** 20, 4.0 * n_in / 2.0 ** 20))
            # ---- queries at the bound and at a fifth of it
            queries = {}
            for q in [md] + ([md / 5.0] if md / 5.0 >= 1e-3 else []):
                qp, qst = api.distance_params(q), _lib.DistanceStats()
                whole, phs = [], []
                for _ in range(args.reps + 1):
                    whole.append(timed(lambda: _lib.check(L.smx_distscene_query(
                        scene._h, None, C.byref(qp), C.c_void_p(dpts.ToCUDA().address), C.c_uint32(P), C.c_void_p(dnear.ToCUDA().address),
                        C.c_void_p(ddist.ToCUDA().address), None, C.c_int32(1), C.byref(qst))))[0])
                    phs.append(scene.debug_timings())
                if q == md:
                    assert answer() == want, "the scene's bytes differ from smx_recon_mesh_distance's"
                    assert api.distance_stats_dict(qst) == cst, "the scene's statistics differ from smx_recon_mesh_distance's"
                row = {"whole": spread(whole[1:]), "phases": {k: spread([v[k] for v in phs[1:]]) for k in DISTSCENE_QUERY_PHASES},
                       "n_matched": int(qst.n_matched)}
                queries["%g" % q] = row
                say("  scene query at %g m: %s = %.2f M points/s | %s | %d of %d matched" % (
                    q, show(row["whole"]), P / (row["whole"]["median"] * 1e-3) / 1e6,
                    " | ".join("%s %s" % (k, show(row["phases"][k])) for k in DISTSCENE_QUERY_PHASES), row["n_matched"], P))
            at = queries["%g" % md]
            say("  query + stats of the scene %.3f ms against the call's %.3f ms; the whole query is %.2f x the whole call" % (
                sum(at["phases"][k]["median"] for k in DISTSCENE_QUERY_PHASES), call["phases"]["query"]["median"] + call["phases"]["stats"]["median"],
                at["whole"]["median"] / call["call"]["median"]))
            out_rows.append({"input": what, "max_distance": md, "triangles_in": n_in, "points": P, "reps": args.reps, "call": call, "stats": cst,
                             "build_phases_ms": build, "scene_stats": bst, "first_rec_bytes": 4 * n_in, "queries": queries})
            scene.close()
    res = {"metric": "distscene_query_ms", "slots": n, "live": live, "triangles_in": T_in, "rows": out_rows}
    # ---- one side of a comparison through scene_b= against the plain comparison
    if args.compare:
        a, b, md = _DeviceArray(dout, 3 * Tc.value), _DeviceArray(dtri, 3 * T_in), args.compare_distance
        plain, through, got, want = [], [], None, None
        with meshing.build_distance_scene(rec, b, md) as scene:
            for _ in range(args.reps + 1):
                ms, want = timed(lambda: meshing.compare_meshes(rec, a, b, md, args.compare, 1, scene.stats["cell_size_used"], directions=1))
                plain.append(ms)
                ms, got = timed(lambda: meshing.compare_meshes(rec, a, b, md, args.compare, 1, directions=1, scene_b=scene))
                through.append(ms)
            assert got == want, "the comparison through the scene differs from smx_recon_compare_meshes"
            build_ms = sum(scene.debug_timings()[k] for k in DISTSCENE_BUILD_PHASES)
        res["compare"] = {"samples": args.compare, "max_distance": md, "plain_ms": spread(plain[1:]), "scene_b_ms": spread(through[1:]),
                          "scene_build_ms": build_ms, "matched": got["a_to_b"]["distance"]["n_matched"]}
        say("decimated -> full, %d samples within %g m: smx_recon_compare_meshes (directions 1) %s | through scene_b %s, the scene built once in "
            "%.3f ms | the same words, %d matched" % (args.compare, md, show(res["compare"]["plain_ms"]), show(res["compare"]["scene_b_ms"]), build_ms,
                                                     res["compare"]["matched"]))
    with open(args.json or os.path.join(ROOT, "profiles", "distscene_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "distscene_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nn.close()


REGISTER_PHASES = ("move", "query", "reduce", "solve")


def register_robust_main():
    """--register POINTS --register_robust: the rim build beside the scene build, the robust call beside the plain one."""
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    maxes = [float(c) for c in (args.distance or "0.01,0.05").split(",")]
    cell = float(args.decimate.split(",")[0]) if args.decimate else 0.05
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n, live))
    from surfelmeshing_amd import meshing, synth
    pts = synth.room_surface_points(args.register + args.register // 50 + 64)[0]
    if pts.shape[0] > args.register:
        pts = pts[np.sort(np.random.default_rng(7).permutation(pts.shape[0])[:args.register])]
    pts = np.ascontiguousarray(pts, np.float32)
    P = pts.shape[0]
    tp = torch.from_numpy(pts).cuda()
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, dout = api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32)
    dres = api.CUDABuffer(1, C.sizeof(_lib.RegisterResult) // 4 + 4, np.uint32)
    drim = api.CUDABuffer(1, cap, np.uint8)
    say("# %d points of synth.room_surface_points, no normals, on the device; the default schedule from the identity; robust = rim rejection and "
        "Tukey weights at bound, bound / 2, bound / 4; medians of %d repetitions after one that allocates" % (P, args.reps))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def spread(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

    def show(s):
        return "%.3f ms (min %.3f, max %.3f)" % (s["median"], s["min"], s["max"])
    T, mst = C.c_uint32(0), _lib.MeshStats()
    _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(cap),
                                       C.c_int32(1), C.byref(T), C.byref(mst)))
    T_in = T.value
    Tc, dst = C.c_uint32(0), _lib.DecimateStats()
    _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                         C.c_void_p(dout.ToCUDA().address), C.c_uint32(T_in), None, C.c_int32(1), C.byref(Tc), C.byref(dst)))
    prm = meshing.register_params()
    out_rows = []
    for what, src, n_in in (("full mesh", dtri, T_in), ("decimated at %g m" % cell, dout, Tc.value)):
        tri = _DeviceArray(src, 3 * n_in)
        # ---- the rim alone
        rim_ms, rim_st = [], _lib.RimStats()
        for _ in range(args.reps + 1):
            rim_ms.append(timed(lambda: _lib.check(L.smx_recon_mesh_rim(rec._h, None, C.c_void_p(src.ToCUDA().address), C.c_uint32(n_in), C.c_int32(1),
                                                                        C.c_void_p(drim.ToCUDA().address), C.byref(rim_st))))[0])
        rst = {k: int(getattr(rim_st, k)) for k, _ in _lib.RimStats._fields_}
        for md in maxes:
            builds = {"plain": [], "with rim": []}
            scene = api.DistanceScene()
            for _ in range(args.reps + 1):
                builds["plain"].append(timed(lambda: rec.BuildDistanceScene(None, tri, md, scene=scene))[0])
                builds["with rim"].append(timed(lambda: rec.BuildDistanceScene(None, tri, md, scene=scene, rim=True))[0])
            robust = meshing.register_robust_params(kernel="tukey", scale=(md, md / 2, md / 4), reject_rim=True)
            rows = {}
            for name, rp in (("plain", None), ("robust", robust)):
                whole, phs, first = [], [], None
                for _ in range(args.reps + 1):
                    ms, _ = timed(lambda: scene.Register(None, tp, None, None, prm, result_buffer=dres, robust=rp))
                    whole.append(ms)
                    phs.append(scene.debug_register_timings())
                    got = dres.Download()[0].tobytes()
                    first = got if first is None else first
                    assert got == first, "two calls gave different bytes"
                res = api.register_result_dict(_lib.RegisterResult.from_buffer_copy(first[:C.sizeof(_lib.RegisterResult)]))
                counts = scene.RegisterRobustCounts()
                ph = {k: spread([q[k] for q in phs[1:]]) for k in ("call",) + REGISTER_PHASES}
                rows[name] = {"call_ms": spread(whole[1:]), "phases_ms": ph, "status": int(res["status"]), "iterations_run": int(res["iterations_run"]),
                              "inliers": int(res["inliers"]), "points_used": int(res["points_used"]), "rms_residual": float(res["rms_residual"]),
                              "last_counts": [int(v) for v in counts[-1]] if len(counts) else [0, 0]}
                say("%s, bound %g m, %d triangles, %s call: %s | last iteration: %s | status %d after %d iterations, %d inliers of %d used, rms %.2f mm, "
                    "%d on the rim, %d rejected by Tukey" % (
                        what, md, n_in, name, show(rows[name]["call_ms"]), " | ".join("%s %s" % (k, show(ph[k])) for k in REGISTER_PHASES), res["status"],
                        res["iterations_run"], res["inliers"], res["points_used"], 1e3 * res["rms_residual"], *rows[name]["last_counts"]))
            say("%s, bound %g m, %d triangles: scene build %s, with the rim %s; the rim alone %s (%d edges, %d of them rim, %d rim triangles); robust reduce "
                "%.3f ms against %.3f ms plain and a query of %.3f ms in the last iteration" % (
                    what, md, n_in, show(spread(builds["plain"][1:])), show(spread(builds["with rim"][1:])), show(spread(rim_ms[1:])), rst["n_edges"],
                    rst["n_rim_edges"], rst["n_rim_triangles"], rows["robust"]["phases_ms"]["reduce"]["median"], rows["plain"]["phases_ms"]["reduce"]["median"],
                    rows["robust"]["phases_ms"]["query"]["median"]))
            out_rows.append({"input": what, "bound": md, "triangles_in": n_in, "points": P, "reps": args.reps, "rim_ms": spread(rim_ms[1:]),
                             "rim_stats": rst, "build_ms": {k: spread(v[1:]) for k, v in builds.items()}, "register": rows})
            scene.close()
    res = {"metric": "register_robust_call_ms", "slots": n, "live": live, "triangles_in": T_in, "rows": out_rows}
    with open(args.json or os.path.join(ROOT, "profiles", "register_robust_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "register_robust_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nn.close()


def register_main():
    """--register POINTS: smx_distscene_register beside the scene's plain query of the same points in one process."""
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    maxes = [float(c) for c in (args.distance or "0.01,0.05").split(",")]
    cell = float(args.decimate.split(",")[0]) if args.decimate else 0.05
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n, live))
    from surfelmeshing_amd import meshing, synth
    pts = synth.room_surface_points(args.register + args.register // 50 + 64)[0]        # (about that many: a few more, thinned to the count)
    if pts.shape[0] > args.register:
        pts = pts[np.sort(np.random.default_rng(7).permutation(pts.shape[0])[:args.register])]
    pts = np.ascontiguousarray(pts, np.float32)
    P = pts.shape[0]
    # the wall a point lies on is the axis along which it is nearest to the room's half extent; its normal looks into the room
    wall = np.argmax(np.abs(pts) / np.asarray(synth.ROOM_HALF, np.float32), axis=1)
    nrm = np.zeros_like(pts)
    nrm[np.arange(P), wall] = -np.sign(pts[np.arange(P), wall])
    tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, dout = api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32)
    dnear, ddist = api.CUDABuffer(1, P, np.uint32), api.CUDABuffer(1, P, np.float32)
    dres = api.CUDABuffer(1, C.sizeof(_lib.RegisterResult) // 4 + 4, np.uint32)
    say("# %d points of synth.room_surface_points with their normals, on the device; the default schedule (strides 4, 2, 1; 4 + 5 + 10 iterations, "
        "every level gated at the scene's bound) from the identity; medians of %d repetitions after one that allocates" % (P, args.reps))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def spread(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

    def show(s):
        return "%.3f ms (min %.3f, max %.3f)" % (s["median"], s["min"], s["max"])
    T, mst = C.c_uint32(0), _lib.MeshStats()
    _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(cap),
                                       C.c_int32(1), C.byref(T), C.byref(mst)))
    T_in = T.value
    Tc, dst = C.c_uint32(0), _lib.DecimateStats()
    _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                         C.c_void_p(dout.ToCUDA().address), C.c_uint32(T_in), None, C.c_int32(1), C.byref(Tc), C.byref(dst)))
    prm = meshing.register_params()
    out_rows = []
    for what, src, n_in in (("full mesh", dtri, T_in), ("decimated at %g m" % cell, dout, Tc.value)):
        tri = _DeviceArray(src, 3 * n_in)
        for md in maxes:
            with rec.BuildDistanceScene(None, tri, md) as scene:
                # ---- the scene's plain query of the same points at the bound
                qp, qst = api.distance_params(md), _lib.DistanceStats()
                qs, qph = [], []
                for _ in range(args.reps + 1):
                    qs.append(timed(lambda: _lib.check(L.smx_distscene_query(
                        scene._h, None, C.byref(qp), C.c_void_p(tp.data_ptr()), C.c_uint32(P), C.c_void_p(dnear.ToCUDA().address),
                        C.c_void_p(ddist.ToCUDA().address), None, C.c_int32(1), C.byref(qst))))[0])
                    qph.append(scene.debug_timings()["query"])
                # ---- the registration, with and without normals; the result stays on the device, so the call itself does not wait
                rows = {}
                for name, normals in (("with normals", tn), ("without normals", None)):
                    whole, host, phs, first = [], [], [], None
                    for _ in range(args.reps + 1):
                        t1 = time.perf_counter()
                        ms, _ = timed(lambda: scene.Register(None, tp, normals, None, prm, result_buffer=dres))
                        whole.append(ms)
                        host.append(1e3 * (time.perf_counter() - t1))
                        phs.append(scene.debug_register_timings())
                        got = dres.Download()[0].tobytes()
                        first = got if first is None else first
                        assert got == first, "two calls gave different bytes"
                    res = api.register_result_dict(_lib.RegisterResult.from_buffer_copy(first[:C.sizeof(_lib.RegisterResult)]))
                    its = scene.RegisterIterations()
                    ph = {k: spread([q[k] for q in phs[1:]]) for k in ("call",) + REGISTER_PHASES}
                    own = sum(ph[k]["median"] for k in ("move", "reduce", "solve"))
                    rows[name] = {"call_ms": spread(whole[1:]), "phases_ms": ph, "status": int(res["status"]), "iterations_run": int(res["iterations_run"]),
                                  "inliers": int(res["inliers"]), "points_used": int(res["points_used"]), "rms_residual": float(res["rms_residual"]),
                                  "matched_last": float(its[-1]["sums"][30]) if its else 0.0, "own_kernels_ms": own,
                                  "own_over_plain_query": own / max(float(np.median(qph[1:])), 1e-9)}
                    say("%s, bound %g m, %d triangles, %s: call %s, by the library's events %s | last iteration: %s | move + reduce + solve %.3f ms = "
                        "%.2f x the scene's plain query phase of the same points (%.3f ms; the whole plain query %s) | status %d after %d iterations, %d "
                        "inliers of %d used (%d matched), rms %.2f mm" % (
                            what, md, n_in, name, show(rows[name]["call_ms"]), show(ph["call"]), " | ".join("%s %s" % (k, show(ph[k])) for k in REGISTER_PHASES),
                            own, rows[name]["own_over_plain_query"], float(np.median(qph[1:])), show(spread(qs[1:])), res["status"], res["iterations_run"],
                            res["inliers"], res["points_used"], rows[name]["matched_last"], 1e3 * res["rms_residual"]))
                out_rows.append({"input": what, "bound": md, "triangles_in": n_in, "points": P, "reps": args.reps, "plain_query_ms": spread(qs[1:]),
                                 "plain_query_phase_ms": spread(qph[1:]), "plain_query_matched": int(qst.n_matched), "register": rows,
                                 "cell_size_used": scene.stats["cell_size_used"]})
    res = {"metric": "register_call_ms", "slots": n, "live": live, "triangles_in": T_in, "rows": out_rows}
    with open(args.json or os.path.join(ROOT, "profiles", "register_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "register_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nn.close()


GLOBAL_PHASES = ("score", "move", "query", "score_kernel", "select", "refine", "rescore")


def register_global_main():
    """--register_global K[,M]: smx_distscene_register_global beside the scene's plain query of the identical moved points in one
    process."""
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    spec = [int(v) for v in args.register_global.split(",")]
    k, n_starts = spec[0], spec[1] if len(spec) > 1 else 8
    md = float(args.distance.split(",")[0]) if args.distance else 0.05
    cell = float(args.decimate.split(",")[0]) if args.decimate else 0.05
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n, live))
    from surfelmeshing_amd import meshing, synth
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, dout = api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32)
    T, mst = C.c_uint32(0), _lib.MeshStats()
    _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(cap),
                                       C.c_int32(1), C.byref(T), C.byref(mst)))
    T_in = T.value
    Tc, dst = C.c_uint32(0), _lib.DecimateStats()
    _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                         C.c_void_p(dout.ToCUDA().address), C.c_uint32(T_in), None, C.c_int32(1), C.byref(Tc), C.byref(dst)))
    # 4096 area samples of the full mesh (the part of the room the map holds), seen from a frame 100 degrees and 0.44 m away
    room = meshing.sample_mesh(rec, _DeviceArray(dtri, 3 * T_in), 4096, 7)[0].cpu().numpy().astype(np.float64)
    room = np.ascontiguousarray(room[np.all(np.isfinite(room), axis=1)])
    axis = np.array([0.48, -0.6, 0.64])
    a = np.deg2rad(100.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R_true = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    t_true = np.array([0.3, -0.2, 0.25])
    pts = np.ascontiguousarray((room - t_true) @ R_true, np.float32)             # (R^T (p - t) row by row)
    m = pts.shape[0]
    centre = pts.astype(np.float64).mean(axis=0)
    anchors = (R_true @ centre + t_true).reshape(1, 3)                           # (the position is known roughly: one anchor)
    poses = api.pose_lattice(k, centre, anchors)
    P = poses.shape[0]
    tp = torch.from_numpy(pts).cuda()
    # the identical P m moved points for the plain query, by the move's own float32 expression
    Tt = torch.from_numpy(poses).cuda()
    x, y, z = (tp[None, :, c] for c in range(3))
    moved = torch.stack([((Tt[:, r, 0, None] * x + Tt[:, r, 1, None] * y) + Tt[:, r, 2, None] * z) + Tt[:, r, 3, None] for r in range(3)], dim=2).reshape(-1, 3).contiguous()
    dnear, ddist = api.CUDABuffer(1, P * m, np.uint32), api.CUDABuffer(1, P * m, np.float32)
    say("# %d area samples of the full mesh in a frame 100 degrees and 0.44 m away, the k = %d lattice (%d poses) on one anchor, %d starts, gate %g m, "
        "the default schedule; P m = %d moved points; medians of %d repetitions after one that allocates" % (m, k, P, n_starts, md, P * m, args.reps))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def spread(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

    def show(s):
        return "%.3f ms (min %.3f, max %.3f)" % (s["median"], s["min"], s["max"])
    prm = meshing.register_params()
    out_rows = []
    for what, src, n_in in (("full mesh", dtri, T_in), ("decimated at %g m" % cell, dout, Tc.value)):
        tri = _DeviceArray(src, 3 * n_in)
        with rec.BuildDistanceScene(None, tri, md) as scene:
            # ---- the scene's plain query of the identical moved points at the gate
            qp, qst = api.distance_params(md), _lib.DistanceStats()
            qs, qph = [], []
            for _ in range(args.reps + 1):
                qs.append(timed(lambda: _lib.check(L.smx_distscene_query(
                    scene._h, None, C.byref(qp), C.c_void_p(moved.data_ptr()), C.c_uint32(P * m), C.c_void_p(dnear.ToCUDA().address),
                    C.c_void_p(ddist.ToCUDA().address), None, C.c_int32(1), C.byref(qst))))[0])
                qph.append(scene.debug_timings()["query"])
            # ---- the scores alone, then the whole search
            sc_ms, sc_ph, first = [], [], None
            for _ in range(args.reps + 1):
                ms, got = timed(lambda: scene.ScorePoses(None, tp, poses, api.score_params(1, md)))
                sc_ms.append(ms)
                sc_ph.append(scene.debug_global_timings())
                first = got if first is None else first
                assert got.tobytes() == first.tobytes(), "two calls gave different bytes"
            whole, phs, res = [], [], None
            for _ in range(args.reps + 1):
                ms, res = timed(lambda: scene.RegisterGlobal(None, tp, None, poses, prm, score=api.score_params(1, md), n_starts=n_starts))
                whole.append(ms)
                phs.append(scene.debug_global_timings())
            ph = {key: spread([q[key] for q in phs[1:]]) for key in GLOBAL_PHASES}
            sph = {key: spread([q[key] for q in sc_ph[1:]]) for key in GLOBAL_PHASES[:4]}
            own = sph["move"]["median"] + sph["score_kernel"]["median"]
            plain = float(np.median(qph[1:]))
            Tw = res["result"]["scene_T_points"].astype(np.float64)
            angle = float(np.degrees(np.arccos(np.clip((np.trace(Tw[:, :3].T @ R_true) - 1) / 2, -1, 1))))
            shift = float(np.linalg.norm(Tw[:, 3] - t_true))
            costs = sorted(s["cost_after"] for s in res["starts"])
            row = {"input": what, "triangles_in": n_in, "points": m, "poses": P, "moved_points": P * m, "n_starts": n_starts, "gate": md, "reps": args.reps,
                   "plain_query_ms": spread(qs[1:]), "plain_query_phase_ms": spread(qph[1:]), "plain_query_matched": int(qst.n_matched),
                   "score_call_ms": spread(sc_ms[1:]), "score_phases_ms": sph, "own_kernels_ms": own, "score_phase_over_plain_query_plus_own": sph["score"]["median"] / max(plain + own, 1e-9),
                   "call_ms": spread(whole[1:]), "phases_ms": ph, "found": res["found"], "winner_rank": res["winner_rank"],
                   "winner_status": res["result"]["status"], "angle_from_truth_deg": angle, "shift_from_truth_m": shift,
                   "cost_after_winner": costs[0], "cost_after_runner_up": costs[1] if len(costs) > 1 else None, "starts": res["starts"],
                   "cell_size_used": scene.stats["cell_size_used"]}
            out_rows.append(row)
            say("%s, gate %g m, %d triangles: score call %s | score phase by the library's events %s = move %s + query %s + score kernel %s | the scene's plain "
                "query phase of the identical %d points %.3f ms (the whole plain query %s, %d matched): the score phase is %.2f x (plain query + move + score "
                "kernel = %.3f ms) | whole search %s: select %s, refine %s, rescore %s | found %d, winner rank %d (status %d), %.4f degrees and %.3f mm from the "
                "truth, cost after %d against the runner-up's %s" % (
                    what, md, n_in, show(spread(sc_ms[1:])), show(sph["score"]), show(sph["move"]), show(sph["query"]), show(sph["score_kernel"]), P * m, plain,
                    show(spread(qs[1:])), int(qst.n_matched), row["score_phase_over_plain_query_plus_own"], plain + own, show(spread(whole[1:])), show(ph["select"]),
                    show(ph["refine"]), show(ph["rescore"]), res["found"], res["winner_rank"], res["result"]["status"], angle, 1e3 * shift, costs[0],
                    costs[1] if len(costs) > 1 else "-"))
    res = {"metric": "register_global_call_ms", "slots": n, "live": live, "triangles_in": T_in, "rows": out_rows}
    with open(args.json or os.path.join(ROOT, "profiles", "register_global_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "register_global_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nn.close()


SAMPLE_PHASES = ("weights", "scan", "draw")
COMPARE_PHASES = ("a_to_b.sample", "a_to_b.distance", "a_to_b.sums", "b_to_a.sample", "b_to_a.distance", "b_to_a.sums")


def sample_traffic_bytes(n, n_in, n_samples, st, bary=True, normals=True):
    """HBM bytes of one smx_recon_sample_mesh call, by phase, from its statistics: a lower bound.  Gathers are counted once per
    distinct target (the S and the N record of a corner in the weights, the S record in the draw); the draw reads the blocks'
    offsets once, one 64-byte line of the in-block sums and the index triple per triangle hit, and writes the outputs."""
    nb = n_in // 256 + 1
    weights = 12 * n_in + 32 * min(n, 3 * n_in) + 8 * n_in + 8 * nb
    scan = 16 * nb
    hit = st["n_triangles_hit"]
    draw = 8 * nb + (64 + 12) * hit + 16 * min(n, 3 * hit) + (12 + 4 + (8 if bary else 0) + (12 if normals else 0)) * n_samples
    return dict(zip(SAMPLE_PHASES, (weights, scan, draw)))


def sample_main():
    import ctypes as C
    from surfelmeshing_amd import meshing
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    counts = [int(c) for c in args.sample.split(",")] if args.sample else []
    cells = [float(c) for c in args.decimate.split(",")] if args.decimate else []
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n, live))
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri = api.CUDABuffer(1, 3 * cap, np.uint32)
    P = max(counts + [1])
    dpts, dti, dbary, dnrm = (api.CUDABuffer(1, k * P, np.float32 if k != 1 else np.uint32) for k in (3, 1, 2, 3))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def full():
        T, st = C.c_uint32(0), _lib.MeshStats()
        _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address),
                                           C.c_uint32(cap), C.c_int32(1), C.byref(T), C.byref(st)))
        return T.value

    def sample(src, n_in, count):
        st = _lib.SampleStats()
        _lib.check(L.smx_recon_sample_mesh(rec._h, None, C.c_void_p(src.ToCUDA().address), C.c_uint32(n_in), C.c_uint32(count), C.c_uint32(0),
                                           C.c_void_p(dpts.ToCUDA().address), C.c_void_p(dti.ToCUDA().address), C.c_void_p(dbary.ToCUDA().address),
                                           C.c_void_p(dnrm.ToCUDA().address), C.c_int32(1), C.byref(st)))
        return api.sample_stats_dict(st)

    def compare(a, n_a, b, n_b):
        prm, st = api.compare_params(args.compare_distance, args.compare), _lib.CompareStats()
        _lib.check(L.smx_recon_compare_meshes(rec._h, None, C.byref(prm), C.c_void_p(a.ToCUDA().address), C.c_uint32(n_a),
                                              C.c_void_p(b.ToCUDA().address), C.c_uint32(n_b), C.c_int32(1), C.byref(st)))
        return api.compare_stats_dict(st, args.compare_distance)
    t_full = []
    for _ in range(args.reps + 1):
        ms, T_in = timed(full)
        t_full.append(ms)
    full_ms = float(np.median(t_full[1:]))
    say("full triangulation, re-measured here: %d triangles, one call %.2f ms" % (T_in, full_ms))
    inputs = [("full mesh", dtri, T_in)]
    for cell in cells:
        T, st = C.c_uint32(0), _lib.DecimateStats()
        buf = api.CUDABuffer(1, 3 * max(1, T_in), np.uint32)
        _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                             C.c_void_p(buf.ToCUDA().address), C.c_uint32(T_in), None, C.c_int32(1), C.byref(T), C.byref(st)))
        inputs.append(("decimated at %g m" % cell, buf, T.value))
    sample_rows, compare_rows = [], []
    for what, src, n_in in inputs:
        for count in counts:
            t, phs, st, first = [], [], None, None
            for _ in range(args.reps + 1):
                ms, st = timed(lambda: sample(src, n_in, count))
                t.append(ms)
                phs.append(rec.debug_sample_timings())
                head = dpts.Download()[0][:100000].tobytes() + dti.Download()[0][:100000].tobytes()
                first = head if first is None else first
                assert head == first, "two calls gave different bytes"
            med = float(np.median(t[1:]))                       # (the first call allocates the workspace)
            ph = {k: float(np.median([q[k] for q in phs[1:]])) for k in SAMPLE_PHASES}
            b = sample_traffic_bytes(n, n_in, count, st)
            tot = sum(b.values())
            say("sample %s, %d samples: %d triangles (%d not live, %d repeated, %d out of range, %d of zero weight), W 2^%.2f, %d none, %d "
                "triangles hit | call %.2f ms (min %.2f, max %.2f) = %.3f x the full triangulation, %.1f M samples/s | %s | model %.3f GB -> "
                "%.0f %% of the %.1f TB/s HBM peak (%s)" % (
                    what, count, n_in, st["n_not_live"], st["n_repeated"], st["n_out_of_range"], st["n_zero_weight"],
                    np.log2(max(st["total_weight"], 1)), st["n_none"], st["n_triangles_hit"], med, min(t[1:]), max(t[1:]), med / full_ms,
                    count / (med * 1e-3) / 1e6, " ".join("%s %.3f" % (k, ph[k]) for k in SAMPLE_PHASES), tot / 1e9,
                    100.0 * tot / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12,
                    " ".join("%s %.0f %%" % (k, 100.0 * b[k] / (max(ph[k], 1e-6) * 1e-3) / HBM_PEAK) for k in SAMPLE_PHASES)))
            sample_rows.append({"input": what, "samples": count, "triangles_in": n_in, "reps": len(t) - 1, "call_ms": med, "call_ms_all": t[1:],
                                "phases_ms": ph, "samples_per_s": count / (med * 1e-3), "stats": st, "traffic_model_bytes": b,
                                "fraction_of_hbm_peak": tot / (med * 1e-3) / HBM_PEAK, "ratio_to_full_triangulation": med / full_ms})
    if args.compare:
        for what, src, n_in in inputs[1:]:
            t, phs, st, first = [], [], None, None
            for _ in range(args.reps + 1):
                ms, st = timed(lambda: compare(dtri, T_in, src, n_in))
                t.append(ms)
                phs.append(rec.debug_compare_timings())
                first = st if first is None else first
                assert st == first, "two calls gave different statistics"
            med = float(np.median(t[1:]))
            ph = {k: float(np.median([q[k] for q in phs[1:]])) for k in COMPARE_PHASES}
            summary = meshing.comparison_summary(st)
            say("compare full mesh (%d triangles) with %s (%d triangles), %d samples per side within %g m | call %.2f ms (min %.2f, max %.2f) "
                "= %.2f x the full triangulation | %s" % (T_in, what, n_in, args.compare, args.compare_distance, med, min(t[1:]), max(t[1:]),
                                                         med / full_ms, " ".join("%s %.2f" % (k, ph[k]) for k in COMPARE_PHASES)))
            for line in meshing.format_mesh_comparison(summary, ("full", "decimated")).split("\n"):
                say("  " + line)
            compare_rows.append({"a": "full mesh", "b": what, "triangles_a": T_in, "triangles_b": n_in, "samples": args.compare,
                                 "max_distance": args.compare_distance, "reps": len(t) - 1, "call_ms": med, "call_ms_all": t[1:], "phases_ms": ph,
                                 "stats": st, "summary": summary, "ratio_to_full_triangulation": med / full_ms})
    res = {"metric": "sample_mesh_ms", "slots": n, "live": live, "triangles_in": T_in, "full_triangulation_ms": full_ms,
           "sample_rows": sample_rows, "compare_rows": compare_rows}
    with open(args.json or os.path.join(ROOT, "profiles", "sample_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "sample_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nn.close()


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


RAY_PHASES = ("mark", "index", "cast", "stats")


def raycast_inputs(say):
    """What --raycast and --raycast --scene measure on: the grown map, its mesh and the decimated one on the device, the camera
    rays of the bench pose on the device, and an event timer."""
    import ctypes as C
    from types import SimpleNamespace
    from surfelmeshing_amd import meshing
    L = _lib.load()
    W, H = (int(v) for v in args.raycast.lower().split("x"))
    DEC = float(args.decimate.split(",")[0]) if args.decimate else 0.05
    wl = bench.Workload(api, 640, 480, args.target, args.target + args.target // 10, 0x5EED0001, 0.0)
    t0 = time.time()
    g_end, _ = wl.grow(False)
    rec = wl.pipe.reconstruction
    n, live = rec.surfels_size(), rec.surfel_count()
    say("# grown in %.1f s: %d slots, %d live" % (time.time() - t0, n, live))
    pose = wl.plan(g_end + 10, 4)[3]
    fx, fy, cx, cy = (wl.fx * W / 640.0, wl.fy * H / 480.0, wl.cx * W / 640.0, wl.cy * H / 480.0)
    o, d = meshing.camera_rays(fx, fy, cx, cy, W, H, pose)
    P = o.shape[0]
    drays, dhit, dt = api.CUDABuffer(1, 6 * P, np.float32), api.CUDABuffer(1, P, np.uint32), api.CUDABuffer(1, P, np.float32)
    drays.Upload(np.ascontiguousarray(np.concatenate([o, d], axis=1)).reshape(1, -1))
    nn = api.SurfelNeighborIndex()
    p = _lib.MeshParams.defaults()
    cap = 3 * n
    dtri, dout = api.CUDABuffer(1, 3 * cap, np.uint32), api.CUDABuffer(1, 3 * cap, np.uint32)
    bufs = {"depth": api.CUDABuffer(H, W, np.float32), "index": api.CUDABuffer(H, W, np.uint32)}
    say("# %d x %d camera rays of the bench pose" % (W, H))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    T, st = C.c_uint32(0), _lib.MeshStats()
    _lib.check(L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(0.05), C.byref(p), C.c_void_p(dtri.ToCUDA().address),
                                       C.c_uint32(cap), C.c_int32(1), C.byref(T), C.byref(st)))
    T_in = T.value
    T, dst = C.c_uint32(0), _lib.DecimateStats()
    _lib.check(L.smx_recon_decimate_mesh(rec._h, None, C.c_float(DEC), C.c_void_p(dtri.ToCUDA().address), C.c_uint32(T_in),
                                         C.c_void_p(dout.ToCUDA().address), C.c_uint32(T_in), None, C.c_int32(1), C.byref(T), C.byref(dst)))

    return SimpleNamespace(W=W, H=H, wl=wl, rec=rec, n=n, live=live, pose=pose, fx=fx, fy=fy, cx=cx, cy=cy, P=P, drays=drays, dhit=dhit, dt=dt,
                           nn=nn, dtri=dtri, dout=dout, bufs=bufs, timed=timed, T_in=T_in, T_dec=T.value, dec_cell=DEC)


def raycast_main():
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    q = raycast_inputs(say)
    W, H, rec, n, live, pose, fx, fy, cx, cy, P = q.W, q.H, q.rec, q.n, q.live, q.pose, q.fx, q.fy, q.cx, q.cy, q.P
    drays, dhit, dt, nn, dtri, dout, bufs, timed, T_in = q.drays, q.dhit, q.dt, q.nn, q.dtri, q.dout, q.bufs, q.timed, q.T_in
    T = C.c_uint32(q.T_dec)

    def cast(src, n_in):
        prm, st = api.raycast_params(), _lib.RaycastStats()
        _lib.check(L.smx_recon_raycast_mesh(rec._h, None, C.byref(prm), C.c_void_p(src.ToCUDA().address), C.c_uint32(n_in),
                                            C.c_void_p(drays.ToCUDA().address), C.c_uint32(P), C.c_void_p(dhit.ToCUDA().address),
                                            C.c_void_p(dt.ToCUDA().address), None, C.c_int32(1), C.byref(st)))
        return api.raycast_stats_dict(st)
    out_rows = []
    for what, src, n_in in (("full mesh", dtri, T_in), ("decimated at %g m" % q.dec_cell, dout, T.value)):
        t, phs, st, first = [], [], None, None
        for _ in range(args.reps + 1):
            ms, st2 = timed(lambda: cast(src, n_in))
            t.append(ms)
            phs.append(rec.debug_raycast_timings())
            head = dhit.Download()[0].tobytes() + dt.Download()[0].tobytes()
            first, st = (head, st2) if first is None else (first, st)
            assert head == first and st2 == st, "two calls gave different bytes"
        med = float(np.median(t[1:]))                       # (the first call allocates the workspace)
        ph = {k: float(np.median([q[k] for q in phs[1:]])) for k in RAY_PHASES}
        prm = api.make_mesh_render_params(W, H, fx, fy, cx, cy, pose)
        where = (src.ToCUDA().address, n_in)
        r_ms = []
        for _ in range(args.reps + 1):
            r_ms.append(timed(lambda: rec.RenderMesh(None, prm, where, **bufs))[0])
        raster = float(np.median(r_ms[1:]))
        same = float((bufs["index"].Download().reshape(-1) == dhit.Download()[0]).mean())
        rays_ok = max(1, P - st["n_bad_rays"])
        say("%s: %d triangles (%d not live, %d repeated, %d out of range), cell %.4f m, %d entries in %d cells, %d wide | call %.2f ms "
            "(min %.2f, max %.2f), %.2f M rays/s | %s | index rebuild (mark + index) %.0f %% of the call | %d of %d rays hit (%d front) | per "
            "ray: %.1f layers, %.1f look-ups, %.1f pair tests | smx_recon_render_mesh of the same pose %.2f ms; %.2f %% of the pixels "
            "have the same index" % (
                what, n_in, st["n_not_live"], st["n_repeated"], st["n_out_of_range"], st["cell_size_used"], st["n_entries"], st["n_cells"],
                st["n_wide"], med, min(t[1:]), max(t[1:]), P / (med * 1e-3) / 1e6, " ".join("%s %.2f" % (k, ph[k]) for k in RAY_PHASES),
                100.0 * (ph["mark"] + ph["index"]) / max(sum(ph.values()), 1e-9), st["n_hit"], P, st["n_front_hits"],
                st["n_layers"] / rays_ok, st["n_lookups"] / rays_ok, st["n_pair_tests"] / rays_ok, raster, 100.0 * same))
        out_rows.append({"input": what, "triangles_in": n_in, "rays": P, "width": W, "height": H, "reps": len(t) - 1, "call_ms": med,
                         "call_ms_all": t[1:], "phases_ms": ph, "rays_per_s": P / (med * 1e-3), "stats": st,
                         "index_rebuild_share": (ph["mark"] + ph["index"]) / max(sum(ph.values()), 1e-9),
                         "layers_per_ray": st["n_layers"] / rays_ok, "lookups_per_ray": st["n_lookups"] / rays_ok,
                         "pair_tests_per_ray": st["n_pair_tests"] / rays_ok, "render_mesh_ms": raster, "render_mesh_ms_all": r_ms[1:],
                         "same_index_share": same})
    res = {"metric": "mesh_raycast_ms", "slots": n, "live": live, "triangles_in": T_in, "rows": out_rows}
    with open(args.json or os.path.join(ROOT, "profiles", "raycast_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "raycast_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nn.close()


SCENE_PHASES = ("mark", "index", "occupancy", "cast", "stats")
SCENE_WORK = ("n_layers", "n_bit_tests", "n_lookups", "n_lookup_misses", "n_pair_tests")


def rayscene_main():
    """--raycast WxH --scene: smx_rayscene beside smx_recon_raycast_mesh in one process."""
    import ctypes as C
    _lib.require_gpu()
    L = _lib.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    q = raycast_inputs(say)
    rec, P, timed = q.rec, q.P, q.timed
    rays, hit, t = (C.c_void_p(b.ToCUDA().address) for b in (q.drays, q.dhit, q.dt))
    prm = api.raycast_params()

    def answer():
        return q.dhit.Download()[0].tobytes() + q.dt.Download()[0].tobytes()

    def spread(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    out_rows = []
    for what, src, n_in in (("full mesh", q.dtri, q.T_in), ("decimated at %g m" % q.dec_cell, q.dout, q.T_dec)):
        tri = C.c_void_p(src.ToCUDA().address)
        # the existing call, re-measured here
        calls, phs, st = [], [], _lib.RaycastStats()
        for _ in range(args.reps + 1):
            calls.append(timed(lambda: _lib.check(L.smx_recon_raycast_mesh(rec._h, None, C.byref(prm), tri, C.c_uint32(n_in), rays, C.c_uint32(P),
                                                                            hit, t, None, C.c_int32(1), C.byref(st))))[0])
            phs.append(rec.debug_raycast_timings())
        want, base = answer(), api.raycast_stats_dict(st)
        base_cast = spread([ph["cast"] + ph["stats"] for ph in phs[1:]])          # (the first call allocates the workspace)
        base_ph = {k: float(np.median([ph[k] for ph in phs[1:]])) for k in RAY_PHASES}
        tol = base_cast["max"] - base_cast["min"]
        rays_ok = max(1, P - base["n_bad_rays"])
        say("%s: %d triangles, cell %.4f m, %d entries in %d cells, %d wide | smx_recon_raycast_mesh %.2f ms (%s); its cast + stats %.3f ms "
            "(min %.3f, max %.3f: spread %.3f) | per ray %.1f layers, %.1f look-ups, %.1f pair tests" % (
                what, n_in, base["cell_size_used"], base["n_entries"], base["n_cells"], base["n_wide"], float(np.median(calls[1:])),
                " ".join("%s %.2f" % (k, base_ph[k]) for k in RAY_PHASES), base_cast["median"], base_cast["min"], base_cast["max"], tol,
                base["n_layers"] / rays_ok, base["n_lookups"] / rays_ok, base["n_pair_tests"] / rays_ok))
        settings = []
        for occ in [-1, 0] + list(range(1, 2 + _lib.RAYSCENE_MAX_LOG2)):
            try:
                scene = rec.BuildRayScene(None, _DeviceArray(src, 3 * n_in), 0.0, occ)
            except _lib.SmxError:
                say("  occupancy %2d: does not fit 2^31 bits" % occ)
                continue
            build = []
            for _ in range(args.reps):
                rec.BuildRayScene(None, _DeviceArray(src, 3 * n_in), 0.0, occ, scene=scene)
                build.append(scene.debug_timings())
            bst = scene.stats
            cst, casts, whole, cast_only = _lib.RaySceneCastStats(), [], [], []
            for _ in range(args.reps + 1):
                whole.append(timed(lambda: _lib.check(L.smx_rayscene_cast(scene._h, None, C.byref(prm), rays, C.c_uint32(P), hit, t, None, C.c_int32(1),
                                                                           C.byref(cst))))[0])
                ph = scene.debug_timings()
                casts.append(ph["cast"] + ph["stats"])
                cast_only.append(ph["cast"])
            assert answer() == want, "the scene's bytes differ from smx_recon_raycast_mesh's"
            cs = api.rayscene_stats_dict(cst)
            assert cs["n_layers"] == base["n_layers"] and cs["n_pair_tests"] == base["n_pair_tests"] and cs["n_hit"] == base["n_hit"]
            c = spread(casts[1:])
            bph = {k: float(np.median([b[k] for b in build])) for k in SCENE_PHASES[:3]}
            say("  occupancy %2d: k %2d, grid %.1f MiB with %d blocks set, scene %.1f MiB | build %s | cast + stats %.3f ms (min %.3f, max %.3f) = "
                "%.2f x the call's (cast %.3f, stats %.3f); the whole cast call by device events %.3f ms | per ray %s" % (
                    occ, bst["occupancy_log2"], bst["occupancy_bytes"] / 2.0 ** 20, bst["n_blocks_set"], bst["device_bytes"] / 2.0 ** 20,
                    " ".join("%s %.2f" % (k, bph[k]) for k in SCENE_PHASES[:3]), c["median"], c["min"], c["max"],
                    c["median"] / max(base_cast["median"], 1e-9), float(np.median(cast_only[1:])), c["median"] - float(np.median(cast_only[1:])),
                    float(np.median(whole[1:])), ", ".join("%s %.1f" % (k[2:], cs[k] / rays_ok) for k in SCENE_WORK)))
            settings.append({"occupancy": occ, "build_stats": bst, "build_phases_ms": bph, "cast_ms": c, "cast_ms_all": casts[1:], "cast_phase_ms": float(np.median(cast_only[1:])), "cast_call_ms": float(np.median(whole[1:])), "cast_call_ms_all": whole[1:], "cast_stats": cs})
            scene.close()
        out_rows.append({"input": what, "triangles_in": n_in, "rays": P, "reps": args.reps, "raycast_mesh_call_ms": float(np.median(calls[1:])),
                         "raycast_mesh_phases_ms": base_ph, "raycast_mesh_cast_ms": base_cast, "spread_ms": tol, "raycast_mesh_stats": base,
                         "settings": settings})
    # what the contract asks of occupancy 0, on these numbers
    def cast_of(row, pick):
        c = [s_ for s_ in row["settings"] if pick(s_)]
        return min(c, key=lambda s_: s_["build_stats"]["occupancy_log2"])["cast_ms"]["median"] if c else None
    full, dec = out_rows
    none_f, none_d = (cast_of(r, lambda s_: s_["occupancy"] == -1) for r in (full, dec))
    grid_f, grid_d = (cast_of(r, lambda s_: s_["occupancy"] > 0) for r in (full, dec))
    same = none_f <= full["raycast_mesh_cast_ms"]["median"] + full["spread_ms"] and none_d <= dec["raycast_mesh_cast_ms"]["median"] + dec["spread_ms"]
    pays = grid_f is not None and grid_d is not None and grid_f < none_f - full["spread_ms"] and grid_d <= none_d + dec["spread_ms"]
    say("a scene cast without a grid costs no more than the call's cast + stats within the spread: %s (full %.3f vs %.3f + %.3f, decimated %.3f vs "
        "%.3f + %.3f)" % (same, none_f, full["raycast_mesh_cast_ms"]["median"], full["spread_ms"], none_d, dec["raycast_mesh_cast_ms"]["median"],
                          dec["spread_ms"]))
    say("the smallest grid that fits pays (faster than none on the full mesh by more than the spread, not slower beyond it on the decimated): %s "
        "(full %s vs %.3f, decimated %s vs %.3f)" % (pays, "%.3f" % grid_f if grid_f is not None else "-", none_f, "%.3f" % grid_d if grid_d is not None else "-", none_d))
    res = {"metric": "rayscene_cast_ms", "slots": q.n, "live": q.live, "rows": out_rows, "no_grid_within_spread": bool(same), "grid_pays": bool(pays)}
    with open(args.json or os.path.join(ROOT, "profiles", "rayscene_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(args.txt or os.path.join(ROOT, "profiles", "rayscene_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    q.nn.close()


class _DeviceArray:
    """A CUDABuffer's first 32-bit `count` elements in the shape api.BuildRayScene takes a device tensor in."""
    is_cuda = True

    def __init__(self, buf, count):
        self._address, self._count = buf.ToCUDA().address, int(count)

    def data_ptr(self):
        return self._address

    def is_contiguous(self):
        return True

    def element_size(self):
        return 4

    def numel(self):
        return self._count

    @property
    def device(self):
        return torch.device("cuda", torch.cuda.current_device())


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
    register_global_main() if args.register_global else register_robust_main() if (args.register and args.register_robust) else register_main() if args.register else distscene_main() if (args.distance and args.scene) else sample_main() if (args.sample or args.compare) else (rayscene_main() if args.scene else raycast_main()) if args.raycast else distance_main() if args.distance else fill_main() if args.fill is not None else components_main() if args.components else decimate_main() if args.decimate else update_main() if args.update else main()
