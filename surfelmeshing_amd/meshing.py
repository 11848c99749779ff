"""Meshing the surfel map on the device (smx_recon_triangulate): a localized Delaunay triangulation.

    from surfelmeshing_amd import meshing
    triangles, stats = meshing.mesh_map(rec)                       # [T,3] uint32 slot indices
    export.SaveMeshAsOBJ(rec, "map.obj", triangles=triangles)

Following the map while it grows (smx_recon_triangulate_update) -- the same triangles, recomputed only where
the map changed:

    mesher = meshing.MapMesher(rec)
    for every few frames: triangles, stats, update_stats = mesher.update()

A coarser level of detail of either (smx_recon_decimate_mesh) -- vertex clustering on a grid of cell_size:

    coarse, decimate_stats = meshing.decimate_map_mesh(rec, triangles, 0.05)

Without its small pieces (smx_recon_mesh_components) -- connected components through shared vertices:

    clean, component_stats = meshing.clean_map_mesh(rec, triangles, min_triangles=20, min_diagonal=0.05)

With its small holes closed (smx_recon_fill_holes) -- fans over boundary loops of at most max_hole_edges edges:

    filled, fill_stats = meshing.fill_map_mesh(rec, clean, max_hole_edges=8)

How far points lie from any of these arrays (smx_recon_mesh_distance) -- the exact closest triangle within
max_distance, and what a decimation moved:

    nearest, distance, stats = meshing.mesh_distance(rec, triangles, points, max_distance=0.05)
    print(meshing.distance_summary(distance, stats))
    print(meshing.decimation_error(rec, triangles, coarse, max_distance=0.1)[0])

What a ray hits first on any of these arrays (smx_recon_raycast_mesh) -- any set of rays, a pinhole camera's, or
the segments from the vertices to a camera (visibility):

    hit, t, stats = meshing.cast_rays(rec, triangles, origins, directions)
    o, d = meshing.camera_rays(fx, fy, cx, cy, width, height, global_T_camera)
    slots, visible = meshing.vertex_visibility(rec, triangles, camera_centre)

Another session's map into this one (smx_recon_merge_map) -- under the pose a registration found; a mesh of the
source follows through src_to_dst:

    stats, src_to_dst = meshing.merge_maps(rec, other, dst_T_src, mode="blend", return_map=True)
    moved_mesh = meshing.remap_triangles(other_triangles, src_to_dst)

A point cloud -- positions, perhaps colours and sensor origins -- as surfels (smx_recon_import_points), into a map
of its own or through a merge into an existing one:

    rec, stats = meshing.map_from_points(points, colors, search_radius=0.05, orient="view_point", view_point=(0, 0, 1.5))
    import_stats, merge_stats = meshing.merge_points(rec, scan_points, rec_T_scan, origins=scan_origins, mode="blend")

The order of the chain is clean -> fill -> decimate: cleaning first, so that no hole of a piece that goes is filled, and
decimation last, because it does not keep the mesh manifold and puts the whole array back into (p, a, b) order.
"""
from ._lib import MeshParams as _MeshParamsPOD

UPDATE_STAT_NAMES = ("mode", "n_changed", "n_dirty", "n_reagreed", "n_kept_triangles")
UPDATE_MODES = ("incremental", "full: no state", "full: parameters differ", "full: fewer slots than kept",
                "full: dirty fraction above the limit")
DECIMATE_STAT_NAMES = ("n_in", "n_not_live", "n_used_vertices", "n_cells", "n_collapsed", "n_duplicates", "n_triangles")
COMPONENTS_STAT_NAMES = ("n_in", "n_not_live", "n_used_vertices", "n_components", "n_kept_components", "n_largest_triangles",
                         "n_triangles")
CLEAN_KEYS = ("min_triangles", "min_diagonal", "keep_largest")
FILL_STAT_NAMES = ("n_in", "n_not_live", "n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_pinched_vertices", "n_listed_loops",
                   "n_filled_loops", "n_rejected_diagonal", "n_rejected_filter", "n_new_triangles", "n_triangles")
FILL_KEYS = ("max_hole_edges", "min_triangle_angle_deg", "max_triangle_angle_deg")
STAT_NAMES = ("n_live", "n_star_triangles", "n_triangles", "star_overflow", "truncated_lists")


class MeshParams:
    """The thresholds by name (the reference's names where it has the same notion); to_pod() gives smx_mesh_params."""

    def __init__(self, max_angle_between_normals_deg=90.0, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0,
                 search_radius_factor=1.0, max_neighbors=64):
        if not 1 <= int(max_neighbors) <= 64:
            raise ValueError("max_neighbors must be within 1 .. 64")
        if not 1.0 <= float(search_radius_factor) <= 2.0:
            raise ValueError("search_radius_factor must be within 1 .. 2")
        if not 0.0 <= min_triangle_angle_deg <= max_triangle_angle_deg <= 180.0:
            raise ValueError("triangle angle limits must satisfy 0 <= min <= max <= 180")
        if not 0.0 < max_angle_between_normals_deg <= 180.0:
            raise ValueError("max_angle_between_normals_deg must be within (0, 180]")
        self.max_angle_between_normals_deg = float(max_angle_between_normals_deg)
        self.min_triangle_angle_deg = float(min_triangle_angle_deg)
        self.max_triangle_angle_deg = float(max_triangle_angle_deg)
        self.search_radius_factor = float(search_radius_factor)
        self.max_neighbors = int(max_neighbors)

    def to_pod(self):
        return _MeshParamsPOD.defaults(
            max_angle_between_normals_deg=self.max_angle_between_normals_deg,
            min_triangle_angle_deg=self.min_triangle_angle_deg, max_triangle_angle_deg=self.max_triangle_angle_deg,
            search_radius_factor=self.search_radius_factor, max_neighbors=self.max_neighbors)


def mesh_map(rec, params=None, stream=None, index=None, cell_size=None):
    """Triangulates the map of `rec` (a CUDASurfelReconstruction) as it stands.  params: a MeshParams here, an
    smx_mesh_params POD, or None for the defaults.  Returns (triangles [T,3] uint32, stats dict)."""
    pod = params.to_pod() if isinstance(params, MeshParams) else params
    return rec.Triangulate(stream, pod, index=index, cell_size=cell_size)


def decimate_map_mesh(rec, triangles, cell_size, stream=None):
    """Decimates `triangles` ([T,3] slot indices of `rec`'s map) by vertex clustering on a grid of cell_size metres.  The
    result has the format of the input (and may be decimated again with a larger cell); it is not kept manifold.
    Returns (triangles [T_out,3] uint32, stats dict)."""
    return rec.DecimateMesh(stream, triangles, cell_size)


def clean_options(clean):
    """`clean` of MapMesher.update as keyword arguments of clean_map_mesh: None, or a dict with keys out of CLEAN_KEYS whose
    values the library would take (checked here, before anything runs)."""
    if clean is None:
        return None
    from .api import components_params
    unknown = sorted(set(clean) - set(CLEAN_KEYS))
    if unknown:
        raise ValueError("clean: unknown key(s) %s (known: %s)" % (", ".join(map(str, unknown)), ", ".join(CLEAN_KEYS)))
    components_params(**clean)
    return dict(clean)


def clean_map_mesh(rec, triangles, min_triangles=0, min_diagonal=0.0, keep_largest=0, stream=None, return_labels=False,
                   return_components=False):
    """Removes the small connected pieces of `triangles` ([T,3] slot indices of `rec`'s map): a piece stays if it has at
    least min_triangles triangles and a bounding-box diagonal of at least min_diagonal metres, and with keep_largest = K > 0
    only the K largest of those.  The result is a subsequence of the input.  Returns (triangles [T_out,3] uint32, stats
    dict[, labels][, component table])."""
    from .api import components_params
    components_params(min_triangles, min_diagonal, keep_largest)
    return rec.MeshComponents(stream, triangles, min_triangles, min_diagonal, keep_largest, return_labels, return_components)


def fill_options(fill):
    """`fill` of MapMesher.update as keyword arguments of fill_map_mesh: None, or a dict with keys out of FILL_KEYS whose
    values the library would take (checked here, before anything runs)."""
    if fill is None:
        return None
    from .api import fill_params
    unknown = sorted(set(fill) - set(FILL_KEYS))
    if unknown:
        raise ValueError("fill: unknown key(s) %s (known: %s)" % (", ".join(map(str, unknown)), ", ".join(FILL_KEYS)))
    fill_params(**fill)
    return dict(fill)


def fill_map_mesh(rec, triangles, max_hole_edges=8, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0, stream=None,
                  return_holes=False):
    """Closes the small holes of `triangles` ([T,3] slot indices of `rec`'s map): every closed loop of 3 .. max_hole_edges
    boundary edges that touches no other hole gets a fan of new triangles, unless a diagonal of the fan exists already or a
    fan triangle fails the triangulation's triangle filter at the two angle limits.  The result is the live input triangles
    in input order, then the new ones.  Returns (triangles [T_out,3] uint32, stats dict[, table of the listed loops])."""
    from .api import fill_params
    fill_params(max_hole_edges, min_triangle_angle_deg, max_triangle_angle_deg)
    return rec.FillHoles(stream, triangles, max_hole_edges, min_triangle_angle_deg, max_triangle_angle_deg, return_holes)


class MapMesher:
    """Keeps the mesh of `rec`'s map up to date.  Owns the neighbour index; update() returns what mesh_map would return
    on the map as it stands, plus the update statistics, and keeps the triangles in .triangles / .stats.  With a
    cell_size, update() also decimates the result (.decimated / .decimate_stats) and returns that array as a fourth value.
    With clean, the small pieces are removed first (.cleaned / .clean_stats): cleaning is applied before cell_size.
    With fill, the small holes are closed (.filled / .fill_stats).  The order is clean -> fill -> decimate."""

    def __init__(self, rec, params=None, cell_size=None, full_above_fraction=None):
        from .api import SurfelNeighborIndex
        self._rec = rec
        self._pod = params.to_pod() if isinstance(params, MeshParams) else params
        self._cell_size = cell_size
        self._fraction = full_above_fraction
        self._index = SurfelNeighborIndex(rec._device_id)
        self.triangles, self.stats, self.update_stats = None, None, None
        self.decimated, self.decimate_stats = None, None
        self.cleaned, self.clean_stats = None, None
        self.filled, self.fill_stats = None, None

    @property
    def index(self):
        """The neighbour index, built over the map as of the last update()."""
        return self._index

    def update(self, stream=None, cell_size=None, clean=None, fill=None):
        """cell_size (of the decimation grid, metres; not the index's): None = no decimation.  clean: None, or a dict of
        clean_map_mesh's thresholds (CLEAN_KEYS); the cleaned array (.cleaned / .clean_stats) is what gets decimated, and
        without a cell_size it is returned as the fourth value.  fill: None, or a dict of fill_map_mesh's parameters
        (FILL_KEYS); the order is clean -> fill -> decimate, each step takes the array of the one before, and the fourth
        value is the array of the last step that ran (.filled / .fill_stats keep the filled one)."""
        options = clean_options(clean)
        filling = fill_options(fill)
        self.triangles, self.stats, self.update_stats = self._rec.TriangulateUpdate(
            stream, self._pod, index=self._index, cell_size=self._cell_size, full_above_fraction=self._fraction)
        self.decimated, self.decimate_stats = None, None
        self.cleaned, self.clean_stats = None, None
        self.filled, self.fill_stats = None, None
        source = self.triangles
        if options is not None:
            self.cleaned, self.clean_stats = self._rec.MeshComponents(stream, self.triangles, **options)
            source = self.cleaned
        if filling is not None:
            self.filled, self.fill_stats = self._rec.FillHoles(stream, source, **filling)
            source = self.filled
        if cell_size is None:
            if options is None and filling is None:
                return self.triangles, self.stats, self.update_stats
            return self.triangles, self.stats, self.update_stats, source
        self.decimated, self.decimate_stats = self._rec.DecimateMesh(stream, source, cell_size)
        return self.triangles, self.stats, self.update_stats, self.decimated

    def timings(self):
        return self._rec.debug_mesh_update_timings()

    def reset(self):
        """Drops the kept state (and its device memory); the next update() runs the full path."""
        self._rec.ResetTriangulation()
        self.triangles, self.stats, self.update_stats = None, None, None
        self.decimated, self.decimate_stats = None, None
        self.cleaned, self.clean_stats = None, None
        self.filled, self.fill_stats = None, None

    def close(self):
        if self._index is not None:
            self._index.close()
            self._index = None


def merge_maps(dst, src, dst_T_src, stream=None, index=None, return_map=False, **params):
    """Merges the map of `src` into the map of `dst` (two CUDASurfelReconstruction objects on one device) under the pose
    dst_T_src ([3,4], dst <- src): CUDASurfelReconstruction.MergeMap.  params: the keywords of api.merge_params (cell_size,
    radius_factor_squared, max_normal_angle_deg, k, mode "keep" / "blend", confidence_cap, frame_index).  Returns the statistics
    dict and, with return_map, src_to_dst.  A neighbour index, a MapMesher's kept state and every slot array over dst stay
    valid for dst's old slots (they keep their indices); the index itself is stale.  ValueError on what the library would refuse."""
    return dst.MergeMap(stream, src, dst_T_src, index=index, return_map=return_map, **params)


def remap_triangles(triangles, src_to_dst):
    """A triangle array over the source map through a merge's src_to_dst (or a compaction's old_to_new): every index is replaced,
    a triangle that loses a corner (0xFFFFFFFF) is dropped.  Returns [T_out,3] uint32."""
    import numpy as np
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    m = np.asarray(src_to_dst, np.uint32)
    if t.size and int(t.max()) >= m.size:
        raise ValueError("a triangle index lies beyond the map")
    out = m[t]
    return np.ascontiguousarray(out[(out != 0xFFFFFFFF).all(1)])


def import_points(rec, points, colors=None, origins=None, stream=None, index=None, return_map=False, **params):
    """Appends a point cloud -- a LiDAR scan, a photogrammetry cloud, the vertices of a PLY -- to the map of `rec` as surfels:
    CUDASurfelReconstruction.ImportPoints.  params: the keywords of api.import_params (cell_size, search_radius, k,
    min_neighbors, max_surface_variation, radius_rank, radius_scale_squared, confidence, default_color, frame_index, orient
    "none" / "view_point" / "origins", view_point).  Returns the statistics dict and, with return_map, point_to_slot."""
    return rec.ImportPoints(stream, points, colors=colors, origins=origins, index=index, return_map=return_map, **params)


def pack_colors(rgb):
    """[n,3] uint8 colours as the 32-bit words row 24 holds (red in the low byte)."""
    import numpy as np
    c = np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.uint32)
    return np.ascontiguousarray(c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16))


def map_from_points(points, colors=None, origins=None, camera=None, room=0, stream=None, index=None, return_map=False, **params):
    """A fresh CUDASurfelReconstruction sized to the cloud (its point count + room slots) that holds the imported cloud.  camera: a
    PinholeCamera4f for frames to come (a small default otherwise: the map services do not use it).  Returns (rec, statistics
    dict[, point_to_slot]); the caller closes rec."""
    import numpy as np
    from . import api
    n = int(points.numel() // 3) if hasattr(points, "numel") else int(np.asarray(points).size // 3)
    rec = api.CUDASurfelReconstruction(max(n + int(room), 1), camera or api.PinholeCamera4f(64, 48, 50.0, 50.0, 32.0, 24.0))
    try:
        out = import_points(rec, points, colors, origins, stream=stream, index=index, return_map=return_map, **params)
    except Exception:
        rec.close()
        raise
    return (rec,) + (out if return_map else (out,))


def merge_points(rec, points, dst_T_src, colors=None, origins=None, stream=None, import_params=None, **merge_params):
    """A cloud given in its own frame into the map of `rec` under the pose dst_T_src ([3,4], rec <- cloud, e.g. the scene_T_points of
    a registration): the cloud is imported into a temporary object (import_params: a dict of api.import_params keywords) and
    that map is merged (merge_maps with merge_params), so that points the map already covers are dropped or blended.
    Returns (import statistics, merge statistics)."""
    tmp, ist = map_from_points(points, colors, origins, camera=rec.depth_camera, stream=stream, **(import_params or {}))
    try:
        return ist, merge_maps(rec, tmp, dst_T_src, stream=stream, **merge_params)
    finally:
        tmp.close()


def build_distance_scene(rec, triangles, max_distance, cell_size=0.0, stream=None, rim=False):
    """A DistanceScene of `triangles` over the map as it stands (CUDASurfelReconstruction.BuildDistanceScene), for queries within
    max_distance: build it once, then pass it as scene= to mesh_distance or decimation_error, or as scene_b= to compare_meshes,
    as often as needed.  It is a snapshot: later changes of the map do not reach it.  rim=True keeps mesh_rim's bytes with the
    scene, which register_points(robust=register_robust_params(reject_rim=True)) needs.  ValueError on parameters the library
    would refuse."""
    from .api import distscene_params
    distscene_params(max_distance, cell_size)
    if rim:
        return rec.BuildDistanceScene(stream, triangles, max_distance, cell_size, rim=True)
    return rec.BuildDistanceScene(stream, triangles, max_distance, cell_size)


def register_params(**kw):
    """The parameters of register_points as a RegisterParams: the library's defaults (strides 4, 2, 1; iterations 4, 5, 10; every
    level gated at the scene's bound; 30 degrees; the tracker's thresholds), then levels=[(stride, iterations[, max_distance]),
    ...] and any field of smx_register_params by name.  AttributeError on a name that is no field."""
    from ._lib import RegisterParams
    return RegisterParams.defaults(**kw)


def register_robust_params(**kw):
    """The robust part of a registration (smx_register_robust_params): kernel "none" / "huber" / "tukey", scale (the kernel's c in
    metres, one value or one per level; 0 = no weights on that level), reject_rim (matches whose closest point lies on the rim of
    the scene's mesh are no inliers; the scene must have been built with rim=True).  Where two surfaces overlap only in part,
    reject_rim removes the pull of the samples beyond the mesh's edge, and Tukey at a few times the noise removes points that
    belong to nothing in the mesh.  ValueError on what the library would refuse."""
    from .api import register_robust_params as make
    return make(**kw)


def register_mesh(rec, scene, triangles, n_samples, seed=0, T_init=None, params=None, robust=None, stream=None):
    """Mesh to mesh in one call: n_samples points with their normals drawn on `triangles` over rec's map (as sample_mesh draws
    them), registered to the mesh `scene` holds (as register_points does): the dict of DistanceScene.Register.  The samples
    never leave the device.  ValueError on what the library would refuse."""
    return rec.RegisterMesh(stream, scene, triangles, n_samples, seed, T_init, params if params is not None else register_params(), robust)


def register_points(scene, points, normals=None, T_init=None, params=None, stream=None, robust=None):
    """Aligns `points` ([P,3], their own frame) to the mesh a DistanceScene holds (build_distance_scene) by point-to-plane ICP
    from the pose T_init (scene <- points, [3,4]; None = the identity): the dict of DistanceScene.Register, whose scene_T_points
    is the pose found and whose status is one of the tracker's.  normals ([P,3], optional) adds the normal gate.  params: a
    register_params(...) (None = the defaults).  The scene's bound limits how far a point may lie from the mesh and still
    count, so build the scene for the misalignment expected.  robust: a register_robust_params(...) (None = the plain call).
    ValueError on what the library would refuse."""
    if robust is not None:
        return scene.Register(stream, points, normals, T_init, params if params is not None else register_params(), robust=robust)
    return scene.Register(stream, points, normals, T_init, params if params is not None else register_params())


def pose_lattice(k, centre, anchors):
    """The candidate poses of register_global, [N_k * A, 3, 4] float32 (api.pose_lattice): every rotation of the integer-quaternion
    lattice of order k about `centre` (points' frame), placed on every one of `anchors` ([A,3], scene's frame).  N_k = 40, 272,
    888, 2080 for k = 1 .. 4; the largest angle from a rotation to the nearest of them, sampled: 60, 41, 28, 23 degrees."""
    from .api import pose_lattice as make
    return make(k, centre, anchors)


def register_global(scene, points, normals=None, k=3, anchors=None, centre=None, n_starts=8, params=None, robust=None, stride=1,
                    max_distance=0.0, reject_rim=False, min_matched_fraction=0.5, mesh=None, n_anchors=8, seed=0, stream=None,
                    return_scores=False):
    """Aligns `points` ([P,3], their own frame; a numpy array or a device tensor, as register_points takes them) to the mesh a
    DistanceScene holds WITHOUT a start pose: the poses of pose_lattice(k, centre, anchors) are scored in one pass over the scene,
    the n_starts cheapest are refined by register_points' ICP (params, robust as there) and the cheapest result wins: the dict of
    DistanceScene.RegisterGlobal, whose result["scene_T_points"] is the pose found and whose found says whether to believe it.
    centre: None = the float64 mean of the finite points.  anchors ([A,3], scene's frame): where that centre may lie -- required,
    unless mesh=(rec, triangles) is given: then n_anchors points of sample_mesh(rec, triangles, n_anchors, seed) are used.
    stride, max_distance (0 = the scene's bound) and reject_rim are the score's; at most 2^16 samples are scored per pose, so a
    large point set needs a stride.  ValueError on what the library would refuse."""
    import numpy as np
    from .api import _device_address, score_params
    if centre is None:
        host = points.detach().cpu().numpy() if _device_address(points) is not None else np.asarray(points)
        host = np.asarray(host, np.float64).reshape(-1, 3)
        ok = np.all(np.isfinite(host), axis=1)
        if not np.any(ok):
            raise ValueError("no finite point to take the centre from")
        centre = host[ok].mean(axis=0)
    if anchors is None:
        if mesh is None:
            raise ValueError("anchors is required unless mesh=(rec, triangles) is given")
        rec, triangles = mesh
        drawn = sample_mesh(rec, triangles, n_anchors, seed, stream=stream)[0]
        anchors = np.asarray(drawn.cpu().numpy() if _device_address(drawn) is not None else drawn, np.float64).reshape(-1, 3)
        anchors = anchors[np.all(np.isfinite(anchors), axis=1)]
    poses = pose_lattice(k, centre, anchors)
    return scene.RegisterGlobal(stream, points, normals, poses, params if params is not None else register_params(), robust,
                                score_params(stride, max_distance, reject_rim), n_starts, min_matched_fraction, return_scores)


def mesh_distance(rec, triangles, points, max_distance, cell_size=0.0, signed=False, return_closest=False, stream=None, scene=None):
    """For every point its closest triangle of `triangles` within max_distance, on the device: (nearest, distance[, closest],
    stats) as CUDASurfelReconstruction.MeshDistance returns them.  With scene (build_distance_scene) the points are measured
    against that scene instead: rec, triangles and cell_size are not used.  ValueError on parameters the library would refuse."""
    from .api import distance_params, distscene_check_query
    p = distance_params(max_distance, cell_size, signed)
    if scene is not None:
        distscene_check_query(scene, p.max_distance)
        return scene.Query(stream, points, max_distance, signed, return_closest)
    return rec.MeshDistance(stream, triangles, points, max_distance, cell_size, signed, return_closest)


def distance_summary(distance, stats):
    """What one MeshDistance call says in a few numbers: the matched fraction (of all points), mean, rms and maximum of
    |distance| over the matched points (float64 sums over the returned array), and the upper edges of the histogram bins that
    hold the 50 / 90 / 99 % points of the matched ones, in metres (None without a match).  `distance` may be a device tensor."""
    import numpy as np
    d = np.asarray(distance.cpu() if hasattr(distance, "cpu") else distance, np.float64).reshape(-1)
    m = np.abs(d[np.isfinite(d)])
    n_points, n_matched = int(stats["n_points"]), int(stats["n_matched"])
    if m.size != n_matched or d.size != n_points:
        raise ValueError("distance and stats are not of one call: %d finite of %d entries, %d matched of %d points"
                         % (m.size, d.size, n_matched, n_points))
    out = dict(n_points=n_points, n_matched=n_matched, matched_fraction=n_matched / n_points if n_points else 0.0,
               mean=float(m.mean()) if m.size else None, rms=float(np.sqrt((m * m).mean())) if m.size else None,
               max=float(m.max()) if m.size else None)
    hist = np.asarray(stats["histogram"], np.int64)
    max_distance = stats.get("max_distance")
    cum = np.cumsum(hist)
    for q in (50, 90, 99):
        # the first bin at which the running count reaches q % of the matched points
        b = int(np.searchsorted(cum, -(-q * n_matched // 100))) if n_matched else None
        out["bin%d" % q] = b
        out["p%d_below" % q] = None if b is None or max_distance is None else (b + 1) * float(max_distance) / hist.size
    return out


def format_distance_summary(summary):
    """distance_summary as one line."""
    if not summary["n_matched"]:
        return "0 of %d points matched" % summary["n_points"]
    mm = lambda v: "n/a" if v is None else "%.2f mm" % (1000.0 * v)     # noqa: E731
    return ("%d of %d points matched (%.1f %%): mean %s, rms %s, max %s; 50 / 90 / 99 %% below %s / %s / %s" % (
        summary["n_matched"], summary["n_points"], 100.0 * summary["matched_fraction"], mm(summary["mean"]), mm(summary["rms"]),
        mm(summary["max"]), mm(summary["p50_below"]), mm(summary["p90_below"]), mm(summary["p99_below"])))


def map_positions(rec, slots=None, stream=None):
    """The smooth positions (rows 3-5) of the map's slots, or of `slots` only, as [m, 3] float32 on the host (NaN rows for merged
    slots): the three rows through ExportVertices, not the whole map."""
    import numpy as np
    from . import export
    pos = np.ascontiguousarray(export.export_vertices(rec, stream)[0], np.float32)
    return pos if slots is None else pos[np.asarray(slots, np.int64)]


def decimation_error(rec, fine, coarse, max_distance, cell_size=0.0, stream=None, scene=None):
    """How far a decimation moved the surface: the points are the positions of the vertices `fine` uses (ascending by slot),
    measured against `coarse`.  scene: a DistanceScene of `coarse` (build_distance_scene) to measure against; coarse and
    cell_size are then not used.  Returns (distance_summary, nearest, distance, stats)."""
    import numpy as np
    used = np.unique(np.ascontiguousarray(fine, np.uint32))
    nearest, distance, stats = mesh_distance(rec, coarse, map_positions(rec, used, stream), max_distance, cell_size, stream=stream, scene=scene)
    return distance_summary(distance, stats), nearest, distance, stats


RIM_STAT_NAMES = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_edges", "n_rim_edges", "n_nonmanifold_edges", "n_rim_vertices",
                  "n_rim_triangles")
RIM_REGIONS = ("A", "B", "AB", "C", "AC", "BC")      # bit k of a triangle's byte: region k of the distance call's closest point


def mesh_rim(rec, triangles, stream=None):
    """Which corners and edges of every triangle lie on the boundary of the surface `triangles` shows: (rim [T] uint8, stats) as
    CUDASurfelReconstruction.MeshRim returns them.  An edge is a rim edge iff one triangle alone has it; a closest point of
    mesh_distance in region k of triangle t lies on the rim iff (rim[t] >> k) & 1."""
    return rec.MeshRim(stream, triangles)


def sample_mesh(rec, triangles, n_samples, seed=0, return_bary=False, return_normals=False, stream=None):
    """n_samples points on `triangles`, drawn on the device in proportion to area and stratified over the total area: (points,
    tri[, bary][, normals], stats) as CUDASurfelReconstruction.SampleMesh returns them.  With return_normals this is the
    uniform-density point cloud of the mesh.  ValueError on parameters the library would refuse."""
    from .api import sample_params
    sample_params(n_samples, seed)
    return rec.SampleMesh(stream, triangles, n_samples, seed, return_bary, return_normals)


def compare_meshes(rec, a, b, max_distance, n_samples, seed=0, cell_size=0.0, directions=3, stream=None, scene_b=None):
    """Both one-sided surface distances between the triangle arrays a and b, on the device: the dict
    CUDASurfelReconstruction.CompareMeshes returns (comparison_summary reads it).  scene_b: a DistanceScene of b
    (build_distance_scene) for the A -> B side, which then builds no index of b: b and cell_size are not used on that side
    (CUDASurfelReconstruction.CompareToDistanceScene); the B -> A side, if asked for, runs as without a scene.  ValueError on
    parameters the library would refuse."""
    from .api import compare_params, compare_stats_dict, distscene_check_query
    p = compare_params(max_distance, n_samples, seed, cell_size, directions)
    if scene_b is None:
        return rec.CompareMeshes(stream, a, b, max_distance, n_samples, seed, cell_size, directions)
    if directions & 1:
        distscene_check_query(scene_b, p.max_distance)
    if directions & 2:
        out = rec.CompareMeshes(stream, a, b, max_distance, n_samples, seed, cell_size, 2)
    else:
        from ._lib import CompareStats
        out = compare_stats_dict(CompareStats(), p.max_distance)
    if directions & 1:
        out["a_to_b"] = rec.CompareToDistanceScene(stream, a, scene_b, max_distance, n_samples, seed)
    return out


def _side_summary(side):
    """One side of compare_meshes in a few numbers, all from its integer words: the distances in units of 2^-20 m."""
    import math
    import struct
    dist, n_samples = side["distance"], int(side["sample"]["n_samples"])
    n_matched = int(dist["n_matched"])
    unit = 2.0 ** -20
    out = dict(n_samples=n_samples, n_none=int(side["sample"]["n_none"]), n_matched=n_matched,
               matched_fraction=n_matched / n_samples if n_samples else 0.0, mean=None, rms=None, max=None)
    if n_matched:
        square_sum = (int(side["sum_sq_hi"]) << 32) + int(side["sum_sq_lo"])          # (a Python integer: it may pass 2^64)
        out["mean"] = int(side["sum_d"]) / n_matched * unit
        out["rms"] = math.sqrt(square_sum / n_matched) * unit
        out["max"] = math.sqrt(struct.unpack("<f", struct.pack("<I", int(dist["max_dist2_bits"])))[0])
    hist, max_distance = [int(v) for v in dist["histogram"]], dist.get("max_distance")
    for q in (50, 90, 99):
        b = None
        if n_matched:
            need, run = -(-q * n_matched // 100), 0
            for b, count in enumerate(hist):
                run += count
                if run >= need:
                    break
        out["bin%d" % q] = b
        out["p%d_below" % q] = None if b is None or max_distance is None else (b + 1) * float(max_distance) / len(hist)
    return out


def comparison_summary(stats):
    """What one compare_meshes call says: per side ("a_to_b", "b_to_a"; None for a side not asked for) the matched fraction of
    the samples, mean, rms and maximum of the matched distances from the integer words, and the upper edges of the histogram
    bins that hold the 50 / 90 / 99 % points as distance_summary gives them; "hausdorff" = the larger one-sided maximum (None
    without a match), and "hausdorff_is_lower_bound" = True whenever a side has samples without a match (their distance is
    beyond max_distance, or they are "none")."""
    out = {}
    for name in ("a_to_b", "b_to_a"):
        side = stats[name]
        out[name] = _side_summary(side) if int(side["sample"]["n_samples"]) or int(side["sample"]["n_in"]) else None
    sides = [s for s in (out["a_to_b"], out["b_to_a"]) if s is not None]
    maxima = [s["max"] for s in sides if s["max"] is not None]
    out["hausdorff"] = max(maxima) if maxima else None
    out["hausdorff_is_lower_bound"] = any(s["n_matched"] < s["n_samples"] for s in sides)
    return out


def format_mesh_comparison(summary, names=("A", "B")):
    """comparison_summary as a few lines."""
    mm = lambda v: "n/a" if v is None else "%.3f mm" % (1000.0 * v)     # noqa: E731
    lines = []
    for key, (x, y) in (("a_to_b", (names[0], names[1])), ("b_to_a", (names[1], names[0]))):
        s = summary[key]
        if s is None:
            continue
        if not s["n_matched"]:
            lines.append("%s -> %s: 0 of %d samples matched" % (x, y, s["n_samples"]))
            continue
        lines.append("%s -> %s: %d of %d samples matched (%.1f %%): mean %s, rms %s, max %s; 50 / 90 / 99 %% below %s / %s / %s" % (
            x, y, s["n_matched"], s["n_samples"], 100.0 * s["matched_fraction"], mm(s["mean"]), mm(s["rms"]), mm(s["max"]),
            mm(s["p50_below"]), mm(s["p90_below"]), mm(s["p99_below"])))
    lines.append("Hausdorff distance %s %s" % (">=" if summary["hausdorff_is_lower_bound"] else "=", mm(summary["hausdorff"])))
    return "\n".join(lines)


def build_ray_scene(rec, triangles, cell_size=0.0, occupancy=0, stream=None):
    """A RayScene of `triangles` over the map as it stands (CUDASurfelReconstruction.BuildRayScene): build it once, then pass it
    as scene= to cast_rays, vertex_visibility or render.raycast_mesh_view as often as needed.  It is a snapshot: later changes
    of the map do not reach it.  ValueError on parameters the library would refuse."""
    from .api import rayscene_params
    rayscene_params(cell_size, occupancy)
    return rec.BuildRayScene(stream, triangles, cell_size, occupancy)


def cast_rays(rec, triangles, origins, directions, t_min=0.0, t_max=2.0 ** 20, cull=0, cell_size=0.0, return_uv=False, stream=None,
              scene=None):
    """For every ray (origins [P,3], directions [P,3], not normalised: t is in units of |direction|) the first triangle of
    `triangles` it hits with t_min <= t <= t_max, on the device: (hit, t[, uv], stats) as CUDASurfelReconstruction.RaycastMesh
    returns them.  With scene (build_ray_scene) the rays are cast against that scene instead: rec, triangles and cell_size
    are not used, and the statistics are those of RayScene.Cast.  ValueError on parameters the library would refuse."""
    import numpy as np
    from .api import raycast_params
    raycast_params(t_min, t_max, cell_size, cull)
    o, d = np.asarray(origins, np.float32), np.asarray(directions, np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("origins and directions must both be [P, 3]")
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    if scene is not None:
        return scene.Cast(stream, rays, t_min, t_max, cull, return_uv)
    return rec.RaycastMesh(stream, triangles, rays, t_min, t_max, cell_size, cull, return_uv)


def camera_rays(fx, fy, cx, cy, width, height, global_T_camera):
    """The rays of a pinhole camera in the pixel-corner convention of smx_recon_render, row by row: (origins, directions), both
    [height * width, 3] float32.  The direction of pixel (x, y) is R ((x + 1/2 - cx) / fx, (y + 1/2 - cy) / fy, 1) with
    global_T_camera = (R | centre), so t is the camera depth of the hit."""
    import numpy as np
    T = np.asarray(global_T_camera, np.float64).reshape(3, 4)
    width, height = int(width), int(height)
    if width < 1 or height < 1 or not (fx > 0 and fy > 0):
        raise ValueError("width, height, fx and fy must be positive")
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    local = np.stack([(x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, np.ones_like(x)], axis=-1).reshape(-1, 3)
    d = (local @ T[:, :3].T).astype(np.float32)
    o = np.broadcast_to(T[:, 3].astype(np.float32), d.shape).copy()
    return o, d


def vertex_visibility(rec, triangles, camera_centre, t_min=2.0 ** -10, cell_size=0.0, stream=None, scene=None):
    """Which of the vertices `triangles` uses are seen from camera_centre: the segment from each used vertex (ascending by
    slot) to the camera is cast with t in [t_min, 1], and a vertex is visible iff its segment hits nothing.  t_min keeps the
    triangles around the vertex itself out.  scene: a RayScene of `triangles` (build_ray_scene) to cast against, for one camera
    after another.  Returns (slots [m] uint32, visible [m] bool, stats)."""
    import numpy as np
    used = np.unique(np.ascontiguousarray(triangles, np.uint32))
    c = np.asarray(camera_centre, np.float32).reshape(3)
    v = map_positions(rec, used, stream)
    hit, t, stats = cast_rays(rec, triangles, v, c[None, :] - v, t_min, 1.0, 0, cell_size, stream=stream, scene=scene)
    return used, hit == np.uint32(0xFFFFFFFF), stats
