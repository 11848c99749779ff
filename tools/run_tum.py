"""The reference application's reconstruction loop (APP/main.cc:884-1267, without the mesher and the viewer) on a TUM
RGB-D folder: reader -> upload -> preprocessing -> Integrate per frame -> optional OBJ / PLY export.
      python tools/run_tum.py <dataset_folder> [--trajectory groundtruth.txt] [--export_mesh out.obj]
                              [--export_point_cloud out.ply] [--max_surfel_count N] [--pyramid_level L]
                              [--compact_every N] [--compact_at_fill F] [--track [--track_write_trajectory FILE]]
                              [--track_rgbd [--track_photometric_weight W]]
                              [--mesh] [--mesh_every N [--mesh_check]] [--mesh_decimate METRES]
                              [--mesh_min_component TRIANGLES] [--mesh_min_extent METRES] [--mesh_keep_largest K]
                              [--mesh_fill_holes EDGES [--mesh_fill_min_angle DEG] [--mesh_fill_max_angle DEG]]
                              [--mesh_eval METRES [--mesh_eval_frames N]] [--mesh_eval_register] [--mesh_eval_rays] [--mesh_eval_rays_frames N]
                              [--mesh_eval_register_global [--mesh_eval_global_k K] [--mesh_eval_global_anchors A] [--mesh_eval_global_starts M]]
                              [--mesh_compare_samples N [--mesh_compare_distance METRES]]
                              [--export_mesh_samples FILE.ply --mesh_samples N]
                              [--render_dir DIR [--render_every N] [--render_overview] [--render_source splats|mesh]]
                              [--merge_split F [--merge_mode keep|blend]] ...
With --mesh the map is triangulated on the device at the end (smx_recon_triangulate) and --export_mesh writes the faces;
without it the OBJ holds the vertices only.
With --mesh_every N the mesh follows the map instead: every N integrated frames smx_recon_triangulate_update recomputes it
where the map changed (one line per update: mode, counts, milliseconds); --export_mesh then writes the last update, made
after the last frame.  --mesh_check triangulates once more at the end with the full call and fails if the two differ.
--mesh_decimate METRES (with --mesh or --mesh_every) decimates the final mesh by vertex clustering on a grid of that cell
size (smx_recon_decimate_mesh) before --export_mesh, which then writes only the vertices the coarse mesh uses.
--mesh_min_component TRIANGLES, --mesh_min_extent METRES and --mesh_keep_largest K (each with --mesh or --mesh_every) remove
the small connected pieces of the final mesh (smx_recon_mesh_components): a piece stays if it has at least that many
triangles and a bounding-box diagonal of at least that length, and of those only the K largest.  Cleaning is applied before
--mesh_decimate; --export_mesh then writes only the vertices the remaining mesh uses.
--mesh_fill_holes EDGES (with --mesh or --mesh_every; 0 = off) closes the holes of the final mesh that have at most that many
edges (smx_recon_fill_holes), after cleaning and before --mesh_decimate; --mesh_fill_min_angle / --mesh_fill_max_angle are the
limits of the triangle filter the new triangles have to pass (default 10 / 170 degrees).  The statistics line is printed.
--mesh_eval METRES (with --mesh or --mesh_every) measures point-to-mesh distances up to METRES with smx_recon_mesh_distance and
prints one summary line per measurement: with --synthetic the noise-free surface points of the integrated frames (every 8th
pixel) against the final mesh -- with --track that is what the tracker's drift does to the surface --, with --mesh_decimate the
fine mesh's vertices against the decimated one.  Without --synthetic and without --mesh_decimate the flag is refused.
--mesh_eval_frames N (with --mesh_eval, --synthetic and --mesh or --mesh_every) builds one distance scene (smx_distscene) of the
final mesh and measures the surface points of each of the last N integrated frames against it: one line per frame under the
head "scene points" and a total, whose figures are those of the --mesh_eval line when N covers every integrated frame.
--mesh_eval_register (with --mesh_eval, --synthetic and --mesh or --mesh_every) splits that surface error into a rigid part and a
surface part: the ground-truth points of each evaluated frame (the last --mesh_eval_frames N, or every integrated frame) are
registered to one distance scene of the final mesh from the identity (smx_distscene_register); one line per frame with the
status, the rotation and translation recovered (the drift) and the surface error before and after the alignment, and a total.
--mesh_eval_register_reject_rim and --mesh_eval_register_kernel {none,huber,tukey} --mesh_eval_register_scale METRES (beside
--mesh_eval_register) run the robust call as well (smx_distscene_register_robust; the scene is built with its rim when asked): the
ground-truth points reach beyond the reconstructed surface, and the plain call is pulled by the matches on the mesh's edge.
Per frame a second line, "robustly registered frame ...", with the two counts of the last iteration (matches rejected on the
rim, samples down-weighted or rejected by the kernel), and a second total.
--mesh_eval_register_global [--mesh_eval_global_k K --mesh_eval_global_anchors A --mesh_eval_global_starts M] (with --mesh_eval,
--synthetic and --mesh or --mesh_every) takes the ground-truth points of each evaluated frame in the CAMERA's frame, as if the
camera pose were lost, and searches the final mesh's scene for them without a start pose (smx_distscene_register_global: the
lattice of order K about the points' mean on A area samples of the mesh, M starts): one line per frame -- found or not, the pose
error against the true camera pose, the winner's rank, the cost margin to the runner-up, the milliseconds -- and a total.
--mesh_compare_samples N prints, for every stage of the chain that was asked for (cleaning, hole filling, decimation), the
two-sided surface error between the mesh before and after it on N area-weighted samples per side (smx_recon_compare_meshes).
--export_mesh_samples FILE.ply with --mesh_samples N writes N such samples of the final mesh with the face normals.
--render_source mesh (with --mesh or --mesh_every) makes --render_dir / --render_every / --render_overview draw the current
mesh with smx_recon_render_mesh instead of splats: the kept array of --mesh_every as of its last update, otherwise a
triangulation of the map as it stands, cleaned, filled and decimated first if those flags are given.
With --track the folder needs no trajectory: every frame is tracked against the map (frame-to-model ICP) `half` frames
ahead of its integration, because the outlier cull of frame f needs the poses of f - half .. f + half.  A trajectory file
that is there is used for the first pose and for an error report only.  --track_rgbd (which implies --track) adds the
photometric term to the tracking (smx_recon_track_rgbd), --track_photometric_weight sets its weight.
--merge_split F reconstructs two sessions and makes one map of them: frames [start, F) go into one object and [F, end) into a
second; the second's mesh is registered to the first's from the identity (smx_recon_register_mesh: the poses are given, so the
line printed says how far from the identity the registration ends), and the second map is merged into the first under that
pose (smx_recon_merge_map, --merge_mode keep drops matched surfels, blend averages them in); the statistics line is printed and
the rest of the chain (--mesh, --mesh_eval, the exports) runs on the merged map.  Not with --track or --mesh_every.
With --synthetic N it first writes an N-frame synthetic dataset into the folder (the test stream), so that the whole
path can be exercised without data."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402


def write_render(args, rec, cam, global_T_camera, frame_index, name, triangles=None):
    """One headless render of the map (surfelmeshing_amd.render) as an RGB PNG: splats, or `triangles` if given."""
    from surfelmeshing_amd import render, tum
    fx, fy, cx, cy = cam.parameters()
    if triangles is None:
        img = render.render_view(rec, cam.width(), cam.height(), fx, fy, cx, cy, global_T_camera,
                                 splat_mode=args.render_splat, color=args.render_color, outputs=("color",),
                                 frame_index=frame_index)
    else:
        img = render.render_mesh_view(rec, triangles, cam.width(), cam.height(), fx, fy, cx, cy, global_T_camera,
                                      color=args.render_color, outputs=("color",), frame_index=frame_index)
    os.makedirs(args.render_dir, exist_ok=True)
    tum.write_png(os.path.join(args.render_dir, name), np.ascontiguousarray(img["color"][:, :, :3]))


def overview_pose(rec):
    """A look-at pose from above and behind the bounding box of the live surfels, towards its centre."""
    from surfelmeshing_amd import render
    rows = rec.debug_download_surfels()
    live = rows[7] >= 0
    p = rows[3:6, live].astype(np.float64)
    lo, hi = p.min(axis=1), p.max(axis=1)
    centre, extent = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    eye = centre + np.array([0.0, -0.6, -1.0]) * extent     # (y points down in the camera-style world frames used here)
    return render.look_at(eye, centre, up=(0.0, -1.0, 0.0))


def run_tracked(args, video, pipe, n, have_trajectory):
    """The frame loop with tracked poses.  The first frame is integrated alone at the start pose, without the cull: the
    map the next 2 * half frames are tracked against.  Then frame f + half is tracked against the map as it stands
    (integrated up to f - 1) before frame f is integrated with the cull and the tracked poses of f - half .. f + half.
    Returns the number of integrated frames."""
    from surfelmeshing_amd import tum
    from surfelmeshing_amd.pipeline import others_TR_reference
    from surfelmeshing_amd.tracking import Tracker
    half = args.outlier_filtering_frame_count // 2
    first = args.start_frame
    truth = {f: np.asarray(video.depth_frame(f).global_T_frame(), np.float64).reshape(3, 4) for f in range(first, n)} \
        if have_trajectory else None
    if args.track_rgbd:
        from surfelmeshing_amd._lib import TrackRGBDParams
        kw = {} if args.track_photometric_weight is None else {"photometric_weight": args.track_photometric_weight}
        tracker = Tracker(pipe, TrackRGBDParams.defaults(**kw), rgbd=True)
    else:
        tracker = Tracker(pipe)
    uploaded = set()

    def need(g):
        if g not in uploaded and g < n:
            pipe.upload(g, video.depth_frame(g).GetImage(), video.color_frame(g).GetImage())
            video.depth_frame(g).ClearImageAndDerivedData()
            video.color_frame(g).ClearImageAndDerivedData()
            uploaded.add(g)

    def track(g):
        need(g)
        out = tracker.track(g)
        if not out.ok:
            print("frame %d: %s, keeping the prediction" % (g, out.status_name))

    start = truth[first] if truth else np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    need(first)
    tracker.set_pose(first, start)
    pipe.process(first, [], None, tracker.poses[first])
    integrated = [first]
    for g in range(first + 1, min(n, first + 2 * half)):
        track(g)
    for f in range(first + half, n - half):
        if f + half not in tracker.poses:
            track(f + half)
        others = [f - k for k in range(1, half + 1)] + [f + k for k in range(1, half + 1)]
        for g in others:
            need(g)
        G = tracker.poses[f]
        T = others_TR_reference(G, [tracker.poses[g] for g in others], args.depth_scaling) if others else None
        pipe.process(f, others, T, G)
        integrated.append(f)
        old = f - half - 1
        if old in uploaded:
            pipe.release(old)
    print("tracked %d frames, %d kept their prediction" % (len(tracker.outcomes), len(tracker.lost)))
    if args.track_write_trajectory:
        tum.write_tum_trajectory(args.track_write_trajectory, [
            (video.depth_frame(f).timestamp, tracker.poses[f][:, 3], tum.quaternion_xyzw_from_matrix(tracker.poses[f][:, :3]))
            for f in integrated])
        print("Wrote %s." % args.track_write_trajectory)
    if truth:
        err = np.array([np.linalg.norm(tracker.poses[f][:, 3].astype(np.float64) - truth[f][:, 3]) for f in integrated])
        still = np.array([np.linalg.norm(truth[first][:, 3] - truth[f][:, 3]) for f in integrated])
        ate, ate_still = float(np.sqrt((err ** 2).mean())), float(np.sqrt((still ** 2).mean()))
        print("ATE RMSE %.5f m over %d frames (a trajectory that never moves from the first pose: %.5f m, ratio %.3f)" % (
            ate, len(integrated), ate_still, ate / max(ate_still, 1e-12)))
    tracker.close()
    return len(integrated)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("dataset_folder")
    ap.add_argument("--trajectory", default="groundtruth.txt")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--max_surfel_count", type=int, default=5_000_000)
    ap.add_argument("--depth_scaling", type=float, default=5000.0)
    ap.add_argument("--max_depth", type=float, default=3.0)
    ap.add_argument("--outlier_filtering_frame_count", type=int, default=8)
    ap.add_argument("--pyramid_level", type=int, default=0)
    ap.add_argument("--median_filter_and_densify_iterations", type=int, default=0)
    ap.add_argument("--start_frame", type=int, default=0)
    ap.add_argument("--end_frame", type=int, default=2 ** 31)
    ap.add_argument("--export_mesh")
    ap.add_argument("--export_point_cloud")
    ap.add_argument("--compact_every", type=int, default=0,
                    help="remove the merged slots from the map before every N-th integrated frame (0 = never)")
    ap.add_argument("--compact_at_fill", type=float, default=0.0,
                    help="remove the merged slots before a frame when surfels_size() >= F * max_surfel_count (0 = never)")
    ap.add_argument("--render_dir", help="write headless renders of the map (render_%%06d.png) into this folder")
    ap.add_argument("--render_every", type=int, default=0,
                    help="render the map from the pose of every N-th integrated frame (0 = never)")
    ap.add_argument("--render_splat", choices=("square", "disc"), default="square")
    ap.add_argument("--render_color", choices=("color", "last_update", "creation", "radii", "normals"), default="color")
    ap.add_argument("--render_overview", action="store_true",
                    help="at the end, render one view from outside the map's bounds looking at its centre")
    ap.add_argument("--render_source", choices=("splats", "mesh"), default="splats",
                    help="what the renders draw: the surfels as splats, or the current mesh (needs --mesh or --mesh_every)")
    ap.add_argument("--mesh", action="store_true",
                    help="triangulate the final map on the device; --export_mesh then writes the faces as well")
    ap.add_argument("--mesh_every", type=int, default=0,
                    help="keep the mesh up to date: update it every N integrated frames and after the last one (0 = never)")
    ap.add_argument("--mesh_check", action="store_true",
                    help="with --mesh_every: compare the last update with one full triangulation, exit 1 if they differ")
    ap.add_argument("--mesh_decimate", type=float, default=None, metavar="METRES",
                    help="with --mesh or --mesh_every: decimate the final mesh by vertex clustering with this cell size; "
                         "--export_mesh then writes the decimated mesh and only the vertices it uses")
    ap.add_argument("--mesh_min_component", type=int, default=None, metavar="TRIANGLES",
                    help="with --mesh or --mesh_every: drop the connected pieces of the final mesh with fewer triangles")
    ap.add_argument("--mesh_min_extent", type=float, default=None, metavar="METRES",
                    help="with --mesh or --mesh_every: drop the connected pieces whose bounding-box diagonal is shorter")
    ap.add_argument("--mesh_keep_largest", type=int, default=None, metavar="K",
                    help="with --mesh or --mesh_every: keep only the K largest connected pieces (of those that pass the other two)")
    ap.add_argument("--mesh_fill_holes", type=int, default=0, metavar="EDGES",
                    help="with --mesh or --mesh_every: close the holes of the final mesh with at most this many edges (3 .. 32; 0 = off)")
    ap.add_argument("--mesh_fill_min_angle", type=float, default=None, metavar="DEG",
                    help="with --mesh_fill_holes: smallest interior angle a new triangle may have (default 10)")
    ap.add_argument("--mesh_fill_max_angle", type=float, default=None, metavar="DEG",
                    help="with --mesh_fill_holes: largest interior angle a new triangle may have (default 170)")
    ap.add_argument("--mesh_eval", type=float, default=None, metavar="METRES",
                    help="with --mesh or --mesh_every: measure point-to-mesh distances up to this far (smx_recon_mesh_distance): with "
                         "--synthetic the noise-free surface points of the integrated frames (every 8th pixel) against the final "
                         "mesh, with --mesh_decimate also the fine mesh's vertices against the decimated one")
    ap.add_argument("--mesh_eval_frames", type=int, default=0, metavar="N",
                    help="with --mesh_eval METRES --synthetic N --mesh: build one distance scene (smx_distscene) of the final mesh and "
                         "measure the noise-free surface points of each of the last N integrated frames against it: one line per "
                         "frame and a total")
    ap.add_argument("--mesh_eval_register", action="store_true",
                    help="with --mesh_eval METRES --synthetic N --mesh: register the ground-truth points of each evaluated frame to the "
                         "final mesh from the identity (smx_distscene_register): the pose recovered and the surface error before and after")
    ap.add_argument("--mesh_eval_register_reject_rim", action="store_true",
                    help="with --mesh_eval_register: also run the robust call with the matches on the mesh's rim rejected")
    ap.add_argument("--mesh_eval_register_kernel", choices=("none", "huber", "tukey"), default="none",
                    help="with --mesh_eval_register: also run the robust call with this weight kernel (needs --mesh_eval_register_scale)")
    ap.add_argument("--mesh_eval_register_scale", type=float, default=None, metavar="METRES",
                    help="the kernel's scale c, 1e-6 .. 16 metres")
    ap.add_argument("--mesh_eval_register_global", action="store_true",
                    help="with --mesh_eval METRES --synthetic N --mesh: take the ground-truth points of each evaluated frame in the CAMERA's "
                         "frame, as if its pose were lost, and search the final mesh's scene for them without a start pose "
                         "(smx_distscene_register_global): found or not, the pose error against the true camera pose, the winner's rank, "
                         "the cost margin to the runner-up, the milliseconds")
    ap.add_argument("--mesh_eval_global_k", type=int, default=3, metavar="K", help="the order of the pose lattice, 1 .. 8 (3: 888 rotations)")
    ap.add_argument("--mesh_eval_global_anchors", type=int, default=8, metavar="A", help="anchors: area samples of the final mesh")
    ap.add_argument("--mesh_eval_global_starts", type=int, default=8, metavar="M", help="starts refined, 1 .. 64")
    ap.add_argument("--mesh_eval_rays", action="store_true",
                    help="with --synthetic N --mesh: cast rays (smx_recon_raycast_mesh) from the last integrated frame's camera "
                         "towards its noise-free surface points (every 8th pixel) and print the share of rays with a hit and the "
                         "mean and rms of |hit range - true range|: accuracy and completeness along the sensor's own rays")
    ap.add_argument("--mesh_eval_rays_frames", type=int, default=0, metavar="N",
                    help="with --synthetic N --mesh: build one ray-casting scene (smx_rayscene) of the final mesh and cast the rays of "
                         "--mesh_eval_rays for each of the last N integrated frames against it: one line per frame and a total")
    ap.add_argument("--mesh_compare_samples", type=int, default=0, metavar="N",
                    help="with --mesh_decimate, --mesh_fill_holes or the cleaning flags: print the two-sided surface error between "
                         "the mesh before and after each such stage, on N area-weighted samples per side (smx_recon_compare_meshes)")
    ap.add_argument("--mesh_compare_distance", type=float, default=0.05, metavar="METRES",
                    help="with --mesh_compare_samples: how far a sample may lie from the other mesh and still match (default 0.05)")
    ap.add_argument("--export_mesh_samples", metavar="FILE.ply",
                    help="with --mesh or --mesh_every and --mesh_samples N: write N area-weighted samples of the final mesh, with the "
                         "face normals, as a point cloud of uniform density (smx_recon_sample_mesh)")
    ap.add_argument("--mesh_samples", type=int, default=0, metavar="N", help="the number of samples of --export_mesh_samples")
    ap.add_argument("--track", action="store_true",
                    help="track the camera against the map instead of reading the poses from the trajectory file")
    ap.add_argument("--track_write_trajectory", help="with --track: write the poses of the integrated frames (TUM format)")
    ap.add_argument("--track_rgbd", action="store_true",
                    help="track with the photometric term as well (implies --track)")
    ap.add_argument("--track_photometric_weight", type=float, default=None,
                    help="with --track_rgbd: metres per unit intensity (default: the library's, 0.1)")
    ap.add_argument("--merge_split", type=int, default=0, metavar="F",
                    help="two sessions: frames before F into one map, from F on into a second, which is registered to the first and "
                         "merged into it (smx_recon_merge_map); the rest of the chain runs on the merged map (0 = one session)")
    ap.add_argument("--merge_mode", choices=["keep", "blend"], default="keep",
                    help="with --merge_split: what a matched surfel of the second session does to the first's (default: nothing)")
    args = ap.parse_args(argv)
    if args.merge_split < 0:
        ap.error("--merge_split needs a frame index >= 0")
    if args.merge_split and (args.track or args.track_rgbd or args.mesh_every > 0):
        ap.error("--merge_split does not go with --track or --mesh_every")
    if args.track_photometric_weight is not None and not args.track_rgbd:
        ap.error("--track_photometric_weight needs --track_rgbd")
    args.track = args.track or args.track_rgbd
    if args.mesh_decimate is not None and not (args.mesh or args.mesh_every > 0):
        ap.error("--mesh_decimate needs --mesh or --mesh_every")
    if args.mesh_decimate is not None and not args.mesh_decimate > 0:
        ap.error("--mesh_decimate needs a cell size > 0")
    for flag, value in (("--mesh_min_component", args.mesh_min_component), ("--mesh_min_extent", args.mesh_min_extent),
                        ("--mesh_keep_largest", args.mesh_keep_largest)):
        if value is not None and not (args.mesh or args.mesh_every > 0):
            ap.error("%s needs --mesh or --mesh_every" % flag)
    if args.mesh_min_component is not None and not 0 <= args.mesh_min_component <= 0xFFFFFFFF:
        ap.error("--mesh_min_component needs a triangle count >= 0")
    if args.mesh_min_extent is not None and not 0 <= args.mesh_min_extent < float("inf"):
        ap.error("--mesh_min_extent needs a finite length >= 0")
    if args.mesh_keep_largest is not None and not 1 <= args.mesh_keep_largest <= 0xFFFFFFFF:
        ap.error("--mesh_keep_largest needs a count >= 1")
    args.mesh_clean = None
    if any(v is not None for v in (args.mesh_min_component, args.mesh_min_extent, args.mesh_keep_largest)):
        args.mesh_clean = dict(min_triangles=args.mesh_min_component or 0, min_diagonal=args.mesh_min_extent or 0.0,
                               keep_largest=args.mesh_keep_largest or 0)
    args.mesh_fill = None
    if args.mesh_fill_holes != 0:
        if not (args.mesh or args.mesh_every > 0):
            ap.error("--mesh_fill_holes needs --mesh or --mesh_every")
        if not 3 <= args.mesh_fill_holes <= 32:
            ap.error("--mesh_fill_holes needs an edge count within 3 .. 32 (0 = off)")
        lo = 10.0 if args.mesh_fill_min_angle is None else args.mesh_fill_min_angle
        hi = 170.0 if args.mesh_fill_max_angle is None else args.mesh_fill_max_angle
        if not 0.0 <= lo < hi <= 180.0:
            ap.error("--mesh_fill_min_angle / --mesh_fill_max_angle need 0 <= min < max <= 180")
        args.mesh_fill = dict(max_hole_edges=args.mesh_fill_holes, min_triangle_angle_deg=lo, max_triangle_angle_deg=hi)
    elif args.mesh_fill_min_angle is not None or args.mesh_fill_max_angle is not None:
        ap.error("--mesh_fill_min_angle / --mesh_fill_max_angle need --mesh_fill_holes")
    if args.mesh_eval is not None:
        if not (args.mesh or args.mesh_every > 0):
            ap.error("--mesh_eval needs --mesh or --mesh_every")
        if not (args.synthetic or args.mesh_decimate is not None):
            ap.error("--mesh_eval has nothing to measure against: it needs --synthetic (the ground-truth surface) or --mesh_decimate "
                     "(the fine mesh's vertices)")
        if not 1e-3 <= args.mesh_eval <= 16.0:
            ap.error("--mesh_eval needs a distance within 0.001 .. 16 metres")
    if args.mesh_eval_frames < 0:
        ap.error("--mesh_eval_frames needs a frame count >= 0")
    if args.mesh_eval_frames and not (args.mesh_eval is not None and args.synthetic and (args.mesh or args.mesh_every > 0)):
        ap.error("--mesh_eval_frames needs --mesh_eval METRES, --synthetic N (the ground-truth surface) and --mesh or --mesh_every")
    if args.mesh_eval_register and not (args.mesh_eval is not None and args.synthetic and (args.mesh or args.mesh_every > 0)):
        ap.error("--mesh_eval_register needs --mesh_eval METRES, --synthetic N (the ground-truth surface) and --mesh or --mesh_every")
    if (args.mesh_eval_register_reject_rim or args.mesh_eval_register_kernel != "none" or args.mesh_eval_register_scale is not None) and \
            not args.mesh_eval_register:
        ap.error("--mesh_eval_register_reject_rim, --mesh_eval_register_kernel and --mesh_eval_register_scale need --mesh_eval_register")
    if (args.mesh_eval_register_kernel != "none") != (args.mesh_eval_register_scale is not None):
        ap.error("--mesh_eval_register_kernel huber|tukey and --mesh_eval_register_scale METRES go together")
    if args.mesh_eval_register_scale is not None and not (1e-6 <= args.mesh_eval_register_scale <= 16.0):
        ap.error("--mesh_eval_register_scale needs 1e-6 .. 16 metres")
    if args.mesh_eval_register_global and not (args.mesh_eval is not None and args.synthetic and (args.mesh or args.mesh_every > 0)):
        ap.error("--mesh_eval_register_global needs --mesh_eval METRES, --synthetic N (the ground-truth surface) and --mesh or --mesh_every")
    if not (1 <= args.mesh_eval_global_k <= 8 and 1 <= args.mesh_eval_global_anchors <= 64 and 1 <= args.mesh_eval_global_starts <= 64):
        ap.error("--mesh_eval_global_k needs 1 .. 8, --mesh_eval_global_anchors and --mesh_eval_global_starts 1 .. 64")
    args.mesh_eval_register_robust = None
    if args.mesh_eval_register_reject_rim or args.mesh_eval_register_kernel != "none":
        args.mesh_eval_register_robust = dict(kernel=args.mesh_eval_register_kernel, scale=args.mesh_eval_register_scale or 0.0,
                                              reject_rim=args.mesh_eval_register_reject_rim)
    if args.mesh_eval_rays and not (args.synthetic and (args.mesh or args.mesh_every > 0)):
        ap.error("--mesh_eval_rays needs --synthetic N (the ground-truth surface) and --mesh or --mesh_every")
    if args.mesh_eval_rays_frames < 0:
        ap.error("--mesh_eval_rays_frames needs a frame count >= 0")
    if args.mesh_eval_rays_frames and not (args.synthetic and (args.mesh or args.mesh_every > 0)):
        ap.error("--mesh_eval_rays_frames needs --synthetic N (the ground-truth surface) and --mesh or --mesh_every")
    if args.render_source == "mesh" and not (args.mesh or args.mesh_every > 0):
        ap.error("--render_source mesh needs a mesh to draw: add --mesh or --mesh_every")
    if not 0 <= args.mesh_compare_samples <= 1 << 28:
        ap.error("--mesh_compare_samples needs a count within 0 .. 2^28")
    if args.mesh_compare_samples:
        if not (args.mesh or args.mesh_every > 0):
            ap.error("--mesh_compare_samples needs --mesh or --mesh_every")
        if args.mesh_decimate is None and args.mesh_fill is None and args.mesh_clean is None:
            ap.error("--mesh_compare_samples has no two meshes to compare: it needs --mesh_decimate, --mesh_fill_holes or a cleaning flag")
        if not 1e-3 <= args.mesh_compare_distance <= 16.0:
            ap.error("--mesh_compare_distance needs a distance within 0.001 .. 16 metres")
    if not 0 <= args.mesh_samples <= 1 << 28:
        ap.error("--mesh_samples needs a count within 0 .. 2^28")
    if bool(args.export_mesh_samples) != bool(args.mesh_samples):
        ap.error("--export_mesh_samples FILE.ply and --mesh_samples N go together")
    if args.export_mesh_samples and not (args.mesh or args.mesh_every > 0):
        ap.error("--export_mesh_samples needs --mesh or --mesh_every")
    return args


def print_mesh_comparison(args, rec, stage, before, after):
    """The lines of --mesh_compare_samples for one stage of the mesh chain."""
    from surfelmeshing_amd import meshing
    stats = meshing.compare_meshes(rec, before, after, args.mesh_compare_distance, args.mesh_compare_samples)
    print("surface error of %s within %g m, %d samples per side:" % (stage, args.mesh_compare_distance, args.mesh_compare_samples))
    print(meshing.format_mesh_comparison(meshing.comparison_summary(stats), ("before", "after")))


def merge_distance_stats(parts):
    """The statistics of several MeshDistance / DistanceScene.Query results over one mesh as those of one call on all their
    points: what distance_summary reads (the counts and the histogram add up, the largest squared distance is the maximum)."""
    out = dict(parts[0])
    for k in ("n_points", "n_bad_points", "n_matched"):
        out[k] = sum(int(p[k]) for p in parts)
    out["histogram"] = [sum(int(p["histogram"][b]) for p in parts) for b in range(len(parts[0]["histogram"]))]
    out["max_dist2_bits"] = max(int(p["max_dist2_bits"]) for p in parts)
    return out


def register_figures(result, before, after):
    """What --mesh_eval_register prints of one frame: status, iterations, the angle (mrad) and length (mm) of the pose recovered,
    mean and rms surface error (mm) before and after it (distance_summary dicts; 0 where nothing matched)."""
    T = np.asarray(result["scene_T_points"], np.float64).reshape(3, 4)
    s = 0.5 * np.linalg.norm([T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]])
    angle = float(np.arctan2(s, 0.5 * (np.trace(T[:, :3]) - 1.0)))
    mm = lambda d, k: 1e3 * (d[k] or 0.0)                                                        # noqa: E731
    return dict(status=int(result["status"]), iterations=int(result["iterations_run"]), mrad=1e3 * angle, mm=1e3 * float(np.linalg.norm(T[:, 3])),
                mean=(mm(before, "mean"), mm(after, "mean")), rms=(mm(before, "rms"), mm(after, "rms")))


def format_register_line(f, fig):
    return "registered frame %d: status %d after %d iterations, %.3f mrad and %.3f mm from the identity; surface error %.3f -> %.3f mm mean, %.3f -> %.3f mm rms" % (
        f, fig["status"], fig["iterations"], fig["mrad"], fig["mm"], fig["mean"][0], fig["mean"][1], fig["rms"][0], fig["rms"][1])


def format_robust_register_line(f, fig, counts):
    """The second line of a frame with --mesh_eval_register_reject_rim / _kernel: the robust call's figures and the two counts of
    its last iteration."""
    return "robustly " + format_register_line(f, fig) + "; last iteration: %d on the rim, %d weighted or rejected" % (int(counts[0]), int(counts[1]))


def format_register_total(figs):
    ok = [g for g in figs if g["status"] <= 1]
    mean = lambda v: float(np.mean(v)) if len(v) else 0.0                                         # noqa: E731
    return "registered %d frames: %d solved, mean %.3f mrad and %.3f mm from the identity; surface error %.3f -> %.3f mm mean" % (
        len(figs), len(ok), mean([g["mrad"] for g in ok]), mean([g["mm"] for g in ok]), mean([g["mean"][0] for g in ok]), mean([g["mean"][1] for g in ok]))


def global_register_figures(out, R, t, call_ms, timings):
    """What --mesh_eval_register_global prints of one frame: found, the winner's status and rank, the angle (degrees) and length
    (mm) between the pose found and the true camera pose (R, t), the winner's cost after refinement and the runner-up's, and the
    milliseconds of the call with the library's own phases."""
    T = np.asarray(out["result"]["scene_T_points"], np.float64).reshape(3, 4)
    c = 0.5 * (np.trace(T[:, :3].T @ np.asarray(R, np.float64)) - 1.0)
    costs = sorted(st["cost_after"] for st in out["starts"])
    return dict(found=int(out["found"]), status=int(out["result"]["status"]), rank=int(out["winner_rank"]), starts=int(out["n_starts_run"]),
                deg=float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), mm=1e3 * float(np.linalg.norm(T[:, 3] - np.asarray(t, np.float64))),
                cost=int(costs[0]), runner_up=int(costs[1]) if len(costs) > 1 else int(costs[0]), call_ms=float(call_ms), timings=dict(timings))


def format_global_register_line(f, fig):
    tm = fig["timings"]
    return ("globally registered frame %d: %s, status %d, winner rank %d of %d, %.3f degrees and %.3f mm from the true camera pose; cost %d, "
            "runner-up %d (margin %d); %.1f ms: score %.2f, select %.2f, refine %.2f, rescore %.2f" % (
                f, "found" if fig["found"] else "NOT found", fig["status"], fig["rank"], fig["starts"], fig["deg"], fig["mm"], fig["cost"], fig["runner_up"],
                fig["runner_up"] - fig["cost"], fig["call_ms"], tm["score"], tm["select"], tm["refine"], tm["rescore"]))


def format_merge_register_line(res):
    """The first line of --merge_split: where the registration of the second session's mesh to the first's ended."""
    T = np.asarray(res["scene_T_points"], np.float64).reshape(3, 4)
    angle = float(np.arccos(np.clip(0.5 * (np.trace(T[:, :3]) - 1.0), -1.0, 1.0)))
    return "second session registered to the first: status %d after %d iterations, %d inliers, %.3f mrad and %.3f mm from the identity" % (
        int(res["status"]), int(res["iterations_run"]), int(res["inliers"]), 1e3 * angle, 1e3 * float(np.linalg.norm(T[:, 3])))


def format_merge_line(mode, stats, ms, timings):
    """The statistics line of --merge_split."""
    return ("merged (%s) in %.1f ms (device %.2f ms: build %.2f, move %.2f, query + select %.2f, number %.2f, append %.2f, blend %.2f, "
            "finish %.2f): %s" % (mode, ms, timings["whole"], timings["build"], timings["move"], timings["query_select"], timings["number"],
                                  timings["append"], timings["blend"], timings["finish"], ", ".join("%s %d" % kv for kv in stats.items())))


def merge_sessions(args, first, second, frame_index):
    """Registers the second session's mesh to the first's from the identity, merges the second map into the first under the pose
    found (the identity if the registration did not solve) and prints both lines."""
    from surfelmeshing_amd import meshing
    tri_first, _ = meshing.mesh_map(first)
    tri_second, _ = meshing.mesh_map(second)
    bound = args.mesh_eval if args.mesh_eval is not None else 0.05
    with meshing.build_distance_scene(first, tri_first, bound) as scene:
        res = meshing.register_mesh(second, scene, tri_second, 20000)
    print(format_merge_register_line(res))
    T = np.asarray(res["scene_T_points"], np.float32).reshape(3, 4)
    if int(res["status"]) > 1:
        print("the registration did not solve: merging under the identity")
        T = np.eye(4, dtype=np.float32)[:3]
    t1 = time.time()
    stats = meshing.merge_maps(first, second, T, mode=args.merge_mode, frame_index=max(1, frame_index))
    print(format_merge_line(args.merge_mode, stats, 1e3 * (time.time() - t1), first.debug_merge_timings()), flush=True)
    return stats


def format_point_eval(summary, what, head="scene points"):
    """A line of --mesh_eval_frames: `what` is "frame 6" or "3 frames"; the figures are format_distance_summary's."""
    from surfelmeshing_amd import meshing
    return "%s of %s: %s" % (head, what, meshing.format_distance_summary(summary))


def format_ray_eval(hit, t, d, frame, head="surface error along the rays"):
    """The line of --mesh_eval_rays: rays to the true surface points (direction d = point - camera, so t = 1 at the truth).
    --mesh_eval_rays_frames prints the same figures per frame under the head "scene rays"."""
    has = np.asarray(hit) != np.uint32(0xFFFFFFFF)
    rng = np.linalg.norm(np.asarray(d, np.float64), axis=1)
    err = np.abs(np.asarray(t, np.float64)[has] * rng[has] - rng[has])
    if not has.size or not has.any():
        return "%s of frame %d: 0 of %d rays hit the mesh" % (head, frame, has.size)
    return "%s of frame %d: %d of %d rays hit the mesh (%.1f %%): mean %.2f mm, rms %.2f mm" % (
        head, frame, int(has.sum()), has.size, 100.0 * has.mean(), 1e3 * err.mean(), 1e3 * np.sqrt((err * err).mean()))


def main():
    args = parse_args()

    import torch  # noqa: F401  (libsmx binds to the HIP runtime torch loaded)
    from surfelmeshing_amd import api, export, tum, _lib
    from surfelmeshing_amd.pipeline import FramePipeline, PreprocessParams, others_TR_reference
    _lib.require_gpu()

    if args.synthetic:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
        from common import small_stream
        from scipy.spatial.transform import Rotation
        s = small_stream(320, 240)
        frames = [s.frame(f) for f in range(args.synthetic)]
        stamps = [1000.0 + f / 30.0 for f in range(args.synthetic)]
        traj = []
        for f, t in enumerate(stamps):
            T = np.asarray(s.pose(f), np.float64).reshape(3, 4)
            traj.append((t, T[:, 3], Rotation.from_matrix(T[:, :3]).as_quat()))
        tum.write_tum_dataset(args.dataset_folder, frames, stamps, (s.fx, s.fy, s.cx - 0.5, s.cy - 0.5), traj)
        args.max_depth = 10.0

    have_trajectory = os.path.exists(os.path.join(args.dataset_folder, args.trajectory))
    video = tum.ReadTUMRGBDDatasetAssociatedAndCalibrated(
        args.dataset_folder, args.trajectory if (have_trajectory or not args.track) else None)
    if video is None:
        sys.exit("Could not read dataset.")
    cam = video.depth_camera
    fx, fy, cx, cy = cam.parameters()
    pre = PreprocessParams(depth_scaling=args.depth_scaling, max_depth=args.max_depth,
                           outlier_filtering_frame_count=args.outlier_filtering_frame_count,
                           depth_valid_region_radius=333.0 * cam.width() / 640.0,
                           pyramid_level=args.pyramid_level,
                           median_filter_and_densify_iterations=args.median_filter_and_densify_iterations)
    pipe = FramePipeline(cam.width(), cam.height(), fx, fy, cx, cy, args.max_surfel_count, pre)
    # --merge_split: the second session's pipeline; both hold every frame either needs (the cull of a frame reads its neighbours)
    second = FramePipeline(cam.width(), cam.height(), fx, fy, cx, cy, args.max_surfel_count, pre) if args.merge_split else None
    pipes = [pipe] + ([second] if second is not None else [])
    half = args.outlier_filtering_frame_count // 2
    n = min(video.frame_count(), args.end_frame)
    mesher = None
    if args.mesh_every > 0:
        from surfelmeshing_amd import meshing
        mesher = meshing.MapMesher(pipe.reconstruction)

    def update_mesh(frames_done):
        t = time.time()
        tri, st, us = mesher.update()
        ph = mesher.timings()
        print("mesh update after %d frames: %s; changed %d, dirty %d, reagreed %d, kept %d triangles of %d; %.2f ms "
              "(device phases %.2f ms)" % (frames_done, meshing.UPDATE_MODES[us["mode"]], us["n_changed"], us["n_dirty"],
                                           us["n_reagreed"], us["n_kept_triangles"], tri.shape[0], 1e3 * (time.time() - t),
                                           sum(ph.values())), flush=True)

    def current_mesh():
        """What --render_source mesh draws: the kept array (as of its last update), or a triangulation of the map as it stands."""
        from surfelmeshing_amd import meshing
        if mesher is not None:
            if mesher.triangles is None:
                mesher.update()
            tri = mesher.triangles
        else:
            tri, _ = meshing.mesh_map(pipe.reconstruction)
        if args.mesh_clean is not None:
            tri, _ = meshing.clean_map_mesh(pipe.reconstruction, tri, **args.mesh_clean)
        if args.mesh_fill is not None:
            tri, _ = meshing.fill_map_mesh(pipe.reconstruction, tri, **args.mesh_fill)
        if args.mesh_decimate is not None:
            tri, _ = meshing.decimate_map_mesh(pipe.reconstruction, tri, args.mesh_decimate)
        return tri
    uploaded = set()
    t0 = time.time()
    done = 0
    compactions, removed = 0, 0
    if args.track:
        done = run_tracked(args, video, pipe, n, have_trajectory)
    for f in range(args.start_frame, n if not args.track else args.start_frame):
        # main.cc:905-968: everything up to f + half + 1 is on the GPU before frame f is processed
        for g in range(f, min(n - 1, f + half + 1) + 1):
            if g not in uploaded:
                for p_ in pipes:
                    p_.upload(g, video.depth_frame(g).GetImage(), video.color_frame(g).GetImage())
                video.depth_frame(g).ClearImageAndDerivedData()
                video.color_frame(g).ClearImageAndDerivedData()
                uploaded.add(g)
        if f < args.start_frame + half or f >= n - half:      # main.cc:986-995: not enough neighbours
            continue
        others = [f - k for k in range(1, half + 1)] + [f + k for k in range(1, half + 1)]    # main.cc:1039-1059
        G = video.depth_frame(f).global_T_frame()
        T = others_TR_reference(G, [video.depth_frame(g).global_T_frame() for g in others], args.depth_scaling)
        if done and ((args.compact_every > 0 and done % args.compact_every == 0) or
                     (args.compact_at_fill > 0 and
                      pipe.reconstruction.surfels_size() >= args.compact_at_fill * args.max_surfel_count)):
            before = pipe.reconstruction.surfels_size()
            _, after, _ = pipe.compact(return_map=False)
            compactions, removed = compactions + 1, removed + before - after
        (second if second is not None and f >= args.merge_split else pipe).process(f, others, T, G)
        done += 1
        if mesher is not None and done % args.mesh_every == 0:
            update_mesh(done)
        if args.render_dir and args.render_every > 0 and done % args.render_every == 0:
            write_render(args, pipe.reconstruction, cam, G, f, "render_%06d.png" % f,
                         current_mesh() if args.render_source == "mesh" else None)
        old = f - half - 1                                                                      # main.cc:1226-1240
        if old in uploaded:
            for p_ in pipes:
                p_.release(old)
    api.StreamSynchronize(None)
    dt = time.time() - t0
    rec = pipe.reconstruction
    if second is not None:
        print("two sessions: %d surfels from the frames before %d, %d from the rest" % (
            rec.surfels_size(), args.merge_split, second.reconstruction.surfels_size()))
        merge_sessions(args, rec, second.reconstruction, n)
    print("%d frames integrated in %.2f s (%.1f frames/s incl. PNG decoding); %d surfels (%d merged)" % (
        done, dt, done / max(dt, 1e-9), rec.surfels_size(), rec.surfels_size() - rec.surfel_count()))
    if compactions:
        print("%d compactions removed %d merged slots" % (compactions, removed))
    if args.render_dir and args.render_overview and args.render_source == "splats":
        write_render(args, rec, cam, overview_pose(rec), n, "render_overview.png")
    triangles = None
    if mesher is not None:
        update_mesh(done)                         # (nothing changed since the last one: the kept array)
        triangles = mesher.triangles
        if args.mesh_check:
            want, want_stats = meshing.mesh_map(rec)
            same = want.tobytes() == triangles.tobytes() and want_stats == mesher.stats
            print("mesh check: the last update %s the full triangulation (%d triangles)" % (
                "equals" if same else "DIFFERS FROM", want.shape[0]))
            if not same:
                sys.exit(1)
        mesher.close()
    elif args.mesh:
        from surfelmeshing_amd import meshing
        t1 = time.time()
        triangles, mesh_stats = meshing.mesh_map(rec)
        print("%d triangles in %.1f ms; %s" % (triangles.shape[0], 1e3 * (time.time() - t1),
                                              ", ".join("%s %d" % (k, mesh_stats[k]) for k in meshing.STAT_NAMES)))
    if args.mesh_clean is not None:
        from surfelmeshing_amd import meshing
        t1 = time.time()
        n_before, before = triangles.shape[0], triangles
        triangles, cst = meshing.clean_map_mesh(rec, triangles, **args.mesh_clean)
        print("cleaned in %.1f ms: components %d in / %d kept (the largest has %d triangles), triangles %d in / %d out" % (
            1e3 * (time.time() - t1), cst["n_components"], cst["n_kept_components"], cst["n_largest_triangles"], n_before,
            triangles.shape[0]))
        if args.mesh_compare_samples:
            print_mesh_comparison(args, rec, "the cleaning", before, triangles)
    if args.mesh_fill is not None:
        from surfelmeshing_amd import meshing
        t1 = time.time()
        before = triangles
        triangles, fst = meshing.fill_map_mesh(rec, triangles, **args.mesh_fill)
        print("holes of up to %d edges filled in %.1f ms: %s" % (args.mesh_fill["max_hole_edges"], 1e3 * (time.time() - t1),
                                                                 ", ".join("%s %d" % (k, fst[k]) for k in meshing.FILL_STAT_NAMES)))
        if args.mesh_compare_samples:
            print_mesh_comparison(args, rec, "the hole filling", before, triangles)
    if args.mesh_decimate is not None:
        from surfelmeshing_amd import meshing
        t1 = time.time()
        fine = triangles
        triangles, dst = meshing.decimate_map_mesh(rec, triangles, args.mesh_decimate)
        print("decimated at %g m in %.1f ms: %s" % (args.mesh_decimate, 1e3 * (time.time() - t1),
                                                    ", ".join("%s %d" % (k, dst[k]) for k in meshing.DECIMATE_STAT_NAMES)))
        if args.mesh_compare_samples:
            print_mesh_comparison(args, rec, "the decimation", fine, triangles)
    if args.mesh_eval is not None:
        from surfelmeshing_amd import meshing
        if args.mesh_decimate is not None:
            summary = meshing.decimation_error(rec, fine, triangles, args.mesh_eval)[0]
            print("decimation error within %g m, fine vertices to the coarse mesh: %s" % (args.mesh_eval, meshing.format_distance_summary(summary)))
        if args.synthetic:
            half_ = args.outlier_filtering_frame_count // 2
            truth = np.concatenate([s.surface_points(f, 8) for f in range(args.start_frame + half_, n - half_)] or [np.zeros((0, 3), np.float32)])
            _, distance, dstats = meshing.mesh_distance(rec, triangles, truth, args.mesh_eval)
            print("surface error within %g m, ground truth of %d frames to the mesh (%s poses): %s" % (
                args.mesh_eval, max(0, n - 2 * half_ - args.start_frame), "tracked" if args.track else "true",
                meshing.format_distance_summary(meshing.distance_summary(distance, dstats))))
    if args.mesh_eval_frames:
        from surfelmeshing_amd import meshing
        half_ = args.outlier_filtering_frame_count // 2
        last = n - half_ - 1
        frames = [f for f in range(last - args.mesh_eval_frames + 1, last + 1) if f >= args.start_frame + half_]
        t1 = time.time()
        parts = []
        with meshing.build_distance_scene(rec, triangles, args.mesh_eval) as scene:
            built = time.time()
            for f in frames:
                _, distance, dstats = meshing.mesh_distance(rec, triangles, s.surface_points(f, 8), args.mesh_eval, scene=scene)
                print(format_point_eval(meshing.distance_summary(distance, dstats), "frame %d" % f))
                parts.append((distance, dstats))
        if parts:
            total = meshing.distance_summary(np.concatenate([d for d, _ in parts]), merge_distance_stats([st for _, st in parts]))
            print(format_point_eval(total, "%d frames" % len(frames)))
        print("scene points: one scene of %d triangles (%d bytes on the device) built in %.1f ms, %d frames queried in %.1f ms" % (
            triangles.shape[0], scene.device_bytes, 1e3 * (built - t1), len(frames), 1e3 * (time.time() - built)))
    if args.mesh_eval_register:
        from surfelmeshing_amd import meshing
        half_ = args.outlier_filtering_frame_count // 2
        last = n - half_ - 1
        first = last - args.mesh_eval_frames + 1 if args.mesh_eval_frames else args.start_frame + half_
        figs, robust_figs = [], []
        robust = meshing.register_robust_params(**args.mesh_eval_register_robust) if args.mesh_eval_register_robust else None
        with meshing.build_distance_scene(rec, triangles, args.mesh_eval, rim=bool(robust is not None and robust.reject_rim)) as scene:
            def figures(pts, res):
                T = res["scene_T_points"].astype(np.float64)
                moved = np.ascontiguousarray(pts.astype(np.float64) @ T[:, :3].T + T[:, 3], np.float32)
                summaries = [meshing.distance_summary(*meshing.mesh_distance(None, None, p, args.mesh_eval, scene=scene)[1:]) for p in (pts, moved)]
                return register_figures(res, *summaries)
            for f in range(max(first, args.start_frame + half_), last + 1):
                pts = np.ascontiguousarray(s.surface_points(f, 8), np.float32)
                figs.append(figures(pts, meshing.register_points(scene, pts)))
                print(format_register_line(f, figs[-1]))
                if robust is not None:
                    res = meshing.register_points(scene, pts, robust=robust)
                    counts = scene.RegisterRobustCounts()          # (before the queries below: the records belong to the scene's last call)
                    robust_figs.append(figures(pts, res))
                    print(format_robust_register_line(f, robust_figs[-1], counts[-1] if len(counts) else (0, 0)))
        print(format_register_total(figs))
        if robust is not None:
            print("robustly " + format_register_total(robust_figs))
    if args.mesh_eval_register_global:
        from surfelmeshing_amd import meshing
        half_ = args.outlier_filtering_frame_count // 2
        last = n - half_ - 1
        first = last - args.mesh_eval_frames + 1 if args.mesh_eval_frames else args.start_frame + half_
        figs = []
        with meshing.build_distance_scene(rec, triangles, args.mesh_eval) as scene:
            for f in range(max(first, args.start_frame + half_), last + 1):
                R, t = s.pose64(f)
                world = s.surface_points(f, 8).astype(np.float64)
                pts = np.ascontiguousarray((world - t) @ R, np.float32)          # (the camera's frame: R^T (p - t) row by row)
                stride = max(1, -(-pts.shape[0] // 4096))                        # (a few thousand samples score a pose)
                t1 = time.time()
                out = meshing.register_global(scene, pts, k=args.mesh_eval_global_k, n_starts=args.mesh_eval_global_starts, stride=stride,
                                              mesh=(rec, triangles), n_anchors=args.mesh_eval_global_anchors, seed=f)
                figs.append(global_register_figures(out, R, t, 1e3 * (time.time() - t1), scene.debug_global_timings()))
                print(format_global_register_line(f, figs[-1]))
        print("globally registered %d frames: %d found" % (len(figs), sum(g["found"] for g in figs)))
    if args.mesh_eval_rays:
        from surfelmeshing_amd import meshing
        half_ = args.outlier_filtering_frame_count // 2
        last = n - half_ - 1                                             # (the last frame the loop above integrated, if any)
        truth = s.surface_points(last, 8) if last >= args.start_frame + half_ else np.zeros((0, 3), np.float32)
        centre = s.pose64(max(last, 0))[1].astype(np.float32)
        d = truth - centre[None, :]
        hit, t, rstats = meshing.cast_rays(rec, triangles, np.broadcast_to(centre, d.shape), d, 0.0, 2.0)
        print(format_ray_eval(hit, t, d, last))
    if args.mesh_eval_rays_frames:
        from surfelmeshing_amd import meshing
        half_ = args.outlier_filtering_frame_count // 2
        last = n - half_ - 1
        frames = [f for f in range(last - args.mesh_eval_rays_frames + 1, last + 1) if f >= args.start_frame + half_]
        t1 = time.time()
        n_hit = n_rays = 0
        with meshing.build_ray_scene(rec, triangles) as scene:
            built = time.time()
            for f in frames:
                centre = s.pose64(f)[1].astype(np.float32)
                d = s.surface_points(f, 8) - centre[None, :]
                hit, t, _ = meshing.cast_rays(rec, triangles, np.broadcast_to(centre, d.shape), d, 0.0, 2.0, scene=scene)
                print(format_ray_eval(hit, t, d, f, "scene rays"))
                n_hit, n_rays = n_hit + int(np.sum(hit != np.uint32(0xFFFFFFFF))), n_rays + hit.size
        print("scene rays of %d frames: %d of %d rays hit the mesh; one scene of %d triangles built in %.1f ms, cast in %.1f ms" % (
            len(frames), n_hit, n_rays, triangles.shape[0], 1e3 * (built - t1), 1e3 * (time.time() - built)))
    if args.render_dir and args.render_overview and args.render_source == "mesh":      # (the final mesh, decimated if asked)
        write_render(args, rec, cam, overview_pose(rec), n, "render_overview.png", triangles)
    if args.export_mesh:
        export.SaveMeshAsOBJ(rec, args.export_mesh, triangles=triangles, referenced_only=args.mesh_decimate is not None or args.mesh_clean is not None)
        print("Wrote %s." % args.export_mesh)
    if args.export_mesh_samples:
        from surfelmeshing_amd import meshing
        points, tri_of, normals, sst = meshing.sample_mesh(rec, triangles, args.mesh_samples, return_normals=True)
        keep = tri_of != np.uint32(0xFFFFFFFF)
        export.write_ply(args.export_mesh_samples, points[keep], normals=normals[keep])
        print("Wrote %s: %d samples of %d triangles (%d hit)." % (args.export_mesh_samples, int(keep.sum()), triangles.shape[0], sst["n_triangles_hit"]))
    if args.export_point_cloud:
        export.SavePointCloudAsPLY(rec, args.export_point_cloud, export_colors=True)
        print("Wrote %s." % args.export_point_cloud)


if __name__ == "__main__":
    main()
