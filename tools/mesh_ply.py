#!/usr/bin/env python3
"""A point cloud file to a triangle mesh, on the device:

      python tools/mesh_ply.py IN.ply --export_mesh OUT.obj [--search_radius METRES] [--k K] [--radius_rank RANK]
                               [--view_point X,Y,Z] [--mesh_min_component TRIANGLES] [--mesh_fill_holes EDGES]
                               [--mesh_decimate METRES]

Reads the vertices of IN.ply (export.read_ply: x y z, red green blue if present), imports them as surfels
(smx_recon_import_points: a normal and a radius per point from its k nearest neighbours; --view_point orients the normals
towards that point), triangulates the map, runs the chain clean -> fill -> decimate as run_tum.py does, and writes the mesh with
the exporter run_tum.py uses.  Prints the import's statistics line and one line per step."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ply")
    ap.add_argument("--export_mesh", required=True, metavar="OUT.obj")
    ap.add_argument("--search_radius", type=float, default=0.1, metavar="METRES")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--radius_rank", type=int, default=8)
    ap.add_argument("--view_point", default=None, metavar="X,Y,Z")
    ap.add_argument("--mesh_min_component", type=int, default=None, metavar="TRIANGLES")
    ap.add_argument("--mesh_fill_holes", type=int, default=0, metavar="EDGES")
    ap.add_argument("--mesh_decimate", type=float, default=None, metavar="METRES")
    args = ap.parse_args(argv)
    if args.view_point is not None:
        try:
            args.view_point = tuple(float(v) for v in args.view_point.split(","))
        except ValueError:
            ap.error("--view_point needs three numbers X,Y,Z")
        if len(args.view_point) != 3 or not np.all(np.isfinite(args.view_point)):
            ap.error("--view_point needs three finite numbers X,Y,Z")
    if not args.search_radius > 0:
        ap.error("--search_radius needs a length > 0")
    if not 4 <= args.k <= 64:
        ap.error("--k needs a value within 4 .. 64")
    if not 1 <= args.radius_rank <= 63:
        ap.error("--radius_rank needs a value within 1 .. 63")
    if args.mesh_min_component is not None and not 0 <= args.mesh_min_component <= 0xFFFFFFFF:
        ap.error("--mesh_min_component needs a triangle count >= 0")
    if args.mesh_fill_holes != 0 and not 3 <= args.mesh_fill_holes <= 32:
        ap.error("--mesh_fill_holes needs an edge count within 3 .. 32 (0 = off)")
    if args.mesh_decimate is not None and not args.mesh_decimate > 0:
        ap.error("--mesh_decimate needs a cell size > 0")
    return args


def format_stats_line(st):
    return "imported %d of %d points (bad %d, sparse %d, degenerate %d, rough %d; %d lists full)" % (
        st["n_imported"], st["n_points"], st["n_bad"], st["n_sparse"], st["n_degenerate"], st["n_rough"], st["n_saturated"])


def main(argv=None):
    args = parse_args(argv)
    from surfelmeshing_amd import export, meshing
    v = export.read_ply(args.ply)
    points = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32)
    colors = None
    if all(c in (v.dtype.names or ()) for c in ("red", "green", "blue")):
        colors = meshing.pack_colors(np.stack([v["red"], v["green"], v["blue"]], axis=1))
    orient = dict(orient="view_point", view_point=args.view_point) if args.view_point is not None else {}
    t0 = time.time()
    rec, st = meshing.map_from_points(points, colors, search_radius=args.search_radius, k=args.k, radius_rank=args.radius_rank, **orient)
    try:
        print(format_stats_line(st))
        print("import took %.1f ms" % (1e3 * (time.time() - t0)))
        triangles, ts = meshing.mesh_map(rec)
        print("triangulated: %d triangles (%d truncated lists, %d star overflows)" % (ts["n_triangles"], ts["truncated_lists"], ts["star_overflow"]))
        if args.mesh_min_component is not None:
            triangles, cs = meshing.clean_map_mesh(rec, triangles, min_triangles=args.mesh_min_component)
            print("cleaned: %d triangles" % triangles.shape[0])
        if args.mesh_fill_holes:
            triangles, fs = meshing.fill_map_mesh(rec, triangles, max_hole_edges=args.mesh_fill_holes)
            print("filled: %d triangles" % triangles.shape[0])
        if args.mesh_decimate is not None:
            triangles, ds = meshing.decimate_map_mesh(rec, triangles, args.mesh_decimate)
            print("decimated at %g m: %d triangles" % (args.mesh_decimate, triangles.shape[0]))
        export.SaveMeshAsOBJ(rec, args.export_mesh, triangles=triangles,
                             referenced_only=args.mesh_decimate is not None or args.mesh_min_component is not None)
        print("Wrote %s: %d triangles." % (args.export_mesh, triangles.shape[0]))
    finally:
        rec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
