"""Host-side mirror of the reference's interface for the surfel-integration path.

Same names, argument order and meaning as the reference's C++ API, on top of the
C-ABI of include/smx.h (no torch types anywhere):

  CUDABuffer                     VIS/cuda/cuda_buffer.h:45-129
  BilateralFilteringAndDepthCutoffCUDA, OutlierDepthMapFusionCUDA, ErodeDepthMapCUDA,
  CopyWithoutBorderCUDA, ComputeNormalsAndDropBadPixelsCUDA,
  ComputePointRadiiAndRemoveIsolatedPixelsCUDA
                                 APP/cuda_depth_processing.cuh:43-122
  CUDASurfelReconstruction       APP/cuda_surfel_reconstruction.h:44-176
  CUDASurfelBuffersCPU, CUDASurfelsCPU
                                 APP/cuda_surfels_cpu.h:40-124
  SurfelNeighborIndex            batched FindNearestSurfelsWithinRadius, APP/octree.h:470-477

Errors: the reference aborts through LOG(FATAL); here a non-zero C-ABI status
raises SmxError (there is no CPU fallback).
"""
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import (BufferDesc, IntegrateParams, RenderParams, SmxError, SurfelBuffersCPU, ReconStats,  # noqa: F401
                   COMPONENTS_PHASES, ComponentsParams, ComponentsStats,
                   FILL_MAX_HOLE_EDGES, FILL_PHASES, FillParams, FillStats,
                   DIST_BINS, DIST_PHASES, DistanceParams, DistanceStats,
                   COMPARE_PHASES, SAMPLE_MAX, SAMPLE_PHASES, CompareParams, CompareStats, SampleStats, RimStats,
                   RAY_MAX_T, RAY_PHASES, RaycastParams, RaycastStats,
                   RAYSCENE_MAX_LOG2, RAYSCENE_PHASES, RaySceneCastStats, RaySceneParams, RaySceneStats,
                   DISTSCENE_PHASES, CompareSide, DistSceneParams, DistSceneStats,
                   REGISTER_MAX_POINTS, REGISTER_MAX_STRIDE, REGISTER_PHASES, RegisterIteration, RegisterParams, RegisterResult, RegisterRobustParams, REGISTER_KERNELS,
                   GLOBAL_MAX_POSES, GLOBAL_MAX_SAMPLES, GLOBAL_MAX_STARTS, GLOBAL_PHASES, GlobalParams, GlobalResult, POSE_SCORE_DTYPE, ScoreParams,
                   DECIMATE_PHASES, DecimateStats, MeshParams, MeshRenderParams, MeshRenderStats, MeshStats, MeshUpdateStats, TrackIteration, TrackParams, TrackResult,
                   TrackRGBDIteration, TrackRGBDParams, TrackRGBDResult)

kInvalidSurfelIndex = 0xFFFFFFFF  # APP/surfel.h (Surfel::kInvalidIndex)
# smx_mesh_component as a numpy record: what MeshComponents(return_components=True) returns
COMPONENT_DTYPE = np.dtype([("label", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("kept", "<u4"),
                            ("lo", "<f4", (3,)), ("hi", "<f4", (3,))])


def components_params(min_triangles=0, min_diagonal=0.0, keep_largest=0):
    """The thresholds of MeshComponents as smx_components_params; ValueError on what the library would refuse (and on what
    a uint32 cannot hold), before anything is called."""
    for name, v in (("min_triangles", min_triangles), ("keep_largest", keep_largest)):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s must be an integer within 0 .. 2^32 - 1" % name)
    d = float(min_diagonal)
    if not (d >= 0.0 and d != float("inf")):
        raise ValueError("min_diagonal must be finite and >= 0")
    return ComponentsParams(int(min_triangles), d, int(keep_largest))


# smx_mesh_hole as a numpy record: what FillHoles(return_holes=True) returns; its status values
HOLE_DTYPE = np.dtype([("label", "<u4"), ("n_edges", "<u4"), ("status", "<u4")])
SMX_HOLE_FILLED, SMX_HOLE_DIAGONAL, SMX_HOLE_FILTER = 1, 2, 3


def fill_params(max_hole_edges=8, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0):
    """The parameters of FillHoles as smx_fill_params; ValueError on what the library would refuse, before anything is
    called."""
    if isinstance(max_hole_edges, bool) or int(max_hole_edges) != max_hole_edges or not 3 <= int(max_hole_edges) <= FILL_MAX_HOLE_EDGES:
        raise ValueError("max_hole_edges must be an integer within 3 .. %d" % FILL_MAX_HOLE_EDGES)
    lo, hi = float(np.float32(min_triangle_angle_deg)), float(np.float32(max_triangle_angle_deg))
    if not (lo - lo == 0.0 and hi - hi == 0.0 and 0.0 <= lo < hi <= 180.0):
        raise ValueError("the triangle angles must be finite with 0 <= min < max <= 180")
    return FillParams(int(max_hole_edges), lo, hi)


def distance_params(max_distance, cell_size=0.0, signed=False):
    """The parameters of MeshDistance as smx_distance_params; ValueError on what the library would refuse, before anything
    is called."""
    m, c = float(np.float32(max_distance)), float(np.float32(cell_size))
    if not (m - m == 0.0 and float(np.float32(1e-3)) <= m <= 16.0):
        raise ValueError("max_distance must be finite within 1e-3 .. 16")
    if not (c - c == 0.0 and c >= 0.0):
        raise ValueError("cell_size must be 0 (the library chooses) or finite and > 0")
    if signed not in (False, True, 0, 1):
        raise ValueError("signed must be a bool")
    return DistanceParams(m, c, int(bool(signed)))


def distance_stats_dict(st):
    """smx_distance_stats as a dict: integers, histogram a list of DIST_BINS integers, cell_size_used a float."""
    d = {n: int(getattr(st, n)) for n, _ in DistanceStats._fields_ if n not in ("histogram", "cell_size_used")}
    d["histogram"] = [int(v) for v in st.histogram]
    d["cell_size_used"] = float(st.cell_size_used)
    return d


def sample_params(n_samples, seed=0):
    """(n_samples, seed) of SampleMesh as integers; ValueError on what the library would refuse (and on what a uint32 cannot
    hold), before anything is called."""
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 0 <= int(n_samples) <= SAMPLE_MAX:
        raise ValueError("n_samples must be an integer within 0 .. 2^28")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("seed must be an integer within 0 .. 2^32 - 1")
    return int(n_samples), int(seed)


def sample_stats_dict(st):
    """smx_sample_stats as a dict of integers."""
    return {n: int(getattr(st, n)) for n, _ in SampleStats._fields_}


def compare_params(max_distance, n_samples, seed=0, cell_size=0.0, directions=3):
    """The parameters of CompareMeshes as smx_compare_params; ValueError on what the library would refuse, before anything is
    called."""
    d = distance_params(max_distance, cell_size)
    n, sd = sample_params(n_samples, seed)
    if isinstance(directions, bool) or directions not in (1, 2, 3):
        raise ValueError("directions must be 1 (A to B), 2 (B to A) or 3 (both)")
    return CompareParams(d.max_distance, d.cell_size, n, sd, int(directions))


def compare_stats_dict(st, max_distance=None):
    """smx_compare_stats as {"a_to_b": side, "b_to_a": side}; a side: {"sample": dict, "distance": dict, "sum_d", "sum_sq_lo",
    "sum_sq_hi": integers}.  max_distance goes into each distance dict (what the histogram's bins are fractions of)."""
    out = {}
    for name in ("a_to_b", "b_to_a"):
        side = getattr(st, name)
        dist = distance_stats_dict(side.distance)
        if max_distance is not None:
            dist["max_distance"] = float(max_distance)
        out[name] = dict(sample=sample_stats_dict(side.sample), distance=dist, sum_d=int(side.sum_d), sum_sq_lo=int(side.sum_sq_lo),
                         sum_sq_hi=int(side.sum_sq_hi))
    return out


def raycast_params(t_min=0.0, t_max=RAY_MAX_T, cell_size=0.0, cull=0):
    """The parameters of RaycastMesh as smx_raycast_params; ValueError on what the library would refuse, before anything is
    called."""
    t0, t1, c = float(np.float32(t_min)), float(np.float32(t_max)), float(np.float32(cell_size))
    if not (t0 - t0 == 0.0 and t1 - t1 == 0.0 and 0.0 <= t0 <= t1 <= RAY_MAX_T):
        raise ValueError("t_min and t_max must be finite with 0 <= t_min <= t_max <= 2^20")
    if not (c - c == 0.0 and c >= 0.0):
        raise ValueError("cell_size must be 0 (the library chooses) or finite and > 0")
    if cull not in (0, 1, 2) or isinstance(cull, bool):
        raise ValueError("cull must be 0 (both sides), 1 (front faces only) or 2 (back faces only)")
    return RaycastParams(t0, t1, c, int(cull))


def raycast_stats_dict(st):
    """smx_raycast_stats as a dict: integers, cell_size_used a float."""
    d = {n: int(getattr(st, n)) for n, _ in RaycastStats._fields_ if n not in ("reserved", "cell_size_used")}
    d["cell_size_used"] = float(st.cell_size_used)
    return d


def rayscene_params(cell_size=0.0, occupancy=0):
    """The parameters of BuildRayScene as smx_rayscene_params; ValueError on what the library would refuse, before anything
    is called."""
    c = float(np.float32(cell_size))
    if not (c - c == 0.0 and c >= 0.0):
        raise ValueError("cell_size must be 0 (the library chooses) or finite and > 0")
    if isinstance(occupancy, bool) or not isinstance(occupancy, (int, np.integer)) or not -1 <= int(occupancy) <= 1 + RAYSCENE_MAX_LOG2:
        raise ValueError("occupancy must be -1 (no bit grid), 0 (the library chooses) or 1 + k with 0 <= k <= %d" % RAYSCENE_MAX_LOG2)
    return RaySceneParams(c, int(occupancy))


def rayscene_stats_dict(st):
    """smx_rayscene_stats or smx_rayscene_cast_stats as a dict: integers, cell_size_used a float."""
    d = {n: int(getattr(st, n)) for n, _ in st._fields_ if n not in ("reserved", "cell_size_used")}
    if hasattr(st, "cell_size_used"):
        d["cell_size_used"] = float(st.cell_size_used)
    return d


class RayScene:
    """Not in the reference: a snapshot of a triangle array over the map with its search structure (smx_rayscene), built once
    by CUDASurfelReconstruction.BuildRayScene and cast against many times.  After the build a cast reads neither the map nor
    the triangle array: it answers what RaycastMesh answered on the map as it stood at the build, through later Integrate,
    Compact and deformation calls and after the reconstruction object is gone.  .stats is the dict of smx_rayscene_stats of
    the build.  close() frees the device memory; the object is a context manager."""

    def __init__(self, device_id=-1):
        self._h = C.c_void_p()
        self.stats = None
        _lib.check(_lib.load().smx_rayscene_create(C.c_int32(device_id), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().smx_rayscene_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Cast(self, stream, rays, t_min=0.0, t_max=RAY_MAX_T, cull=0, return_uv=False):
        """For every ray of `rays` ([P,6] float32: origin, then direction, not normalised) what RaycastMesh returns for the
        triangles and the map of the build (smx_rayscene_cast): byte for byte the same hit, t and uv.  Synchronous.  rays is
        a numpy array or a contiguous float32 device tensor; the results then are device tensors too.  Returns (hit, t, then
        with return_uv uv, then the dict of smx_rayscene_cast_stats)."""
        p = raycast_params(t_min, t_max, 0.0, cull)
        if not getattr(self, "_h", None):
            raise ValueError("the scene is closed")
        L = _lib.load()
        st = RaySceneCastStats()
        dev = _device_address(rays) is not None
        if dev:
            import torch
            if not (rays.is_contiguous() and rays.dtype == torch.float32 and rays.numel() % 6 == 0):
                raise ValueError("a device tensor of rays must be contiguous [P,6] float32")
            n_rays = rays.numel() // 6
            hit = torch.empty(n_rays, dtype=torch.uint32, device=rays.device)
            t = torch.empty(n_rays, dtype=torch.float32, device=rays.device)
            uv = torch.empty((n_rays, 2), dtype=torch.float32, device=rays.device) if return_uv else None
            rin = rays.data_ptr() if n_rays else None
            outs = [a.data_ptr() if a is not None and n_rays else None for a in (hit, t, uv)]
            torch.cuda.current_stream(rays.device).synchronize()      # (the tensor's producers; the call runs on `stream`)
        else:
            ry = np.ascontiguousarray(rays, np.float32)
            if ry.size % 6:
                raise ValueError("rays must hold six values per row")
            n_rays = ry.size // 6
            hit, t = np.zeros(n_rays, np.uint32), np.zeros(n_rays, np.float32)
            uv = np.zeros((n_rays, 2), np.float32) if return_uv else None
            rin = ry.ctypes.data if n_rays else None
            outs = [a.ctypes.data if a is not None and n_rays else None for a in (hit, t, uv)]
        _lib.check(L.smx_rayscene_cast(self._h, _sv(stream), C.byref(p), C.c_void_p(rin), C.c_uint32(n_rays), C.c_void_p(outs[0]),
                                       C.c_void_p(outs[1]), C.c_void_p(outs[2]), C.c_int32(1 if dev else 0), C.byref(st)))
        stats = rayscene_stats_dict(st)
        return (hit, t, uv, stats) if return_uv else (hit, t, stats)

    def debug_timings(self):
        """Milliseconds of the last build (mark, index, occupancy) and of the last cast (cast, stats)."""
        out = (C.c_float * RAYSCENE_PHASES)()
        _lib.check(_lib.load().smx_rayscene_debug_timings(self._h, out, C.c_int32(RAYSCENE_PHASES)))
        return dict(zip(("mark", "index", "occupancy", "cast", "stats"), [float(v) for v in out]))


def distscene_params(max_distance, cell_size=0.0):
    """The parameters of BuildDistanceScene as smx_distscene_params; ValueError on what the library would refuse, before
    anything is called."""
    d = distance_params(max_distance, cell_size)
    return DistSceneParams(d.max_distance, d.cell_size)


def distscene_stats_dict(st):
    """smx_distscene_stats as a dict: integers, cell_size_used and max_distance floats."""
    d = {n: int(getattr(st, n)) for n, _ in DistSceneStats._fields_ if n not in ("cell_size_used", "max_distance")}
    d["cell_size_used"], d["max_distance"] = float(st.cell_size_used), float(st.max_distance)
    return d


def distscene_check_query(scene, max_distance):
    """ValueError if `scene` is closed, holds no build, or was built for less than max_distance: what the library would refuse
    of a query, before anything is called."""
    if not getattr(scene, "_h", None):
        raise ValueError("the scene is closed")
    if not getattr(scene, "stats", None):
        raise ValueError("the scene holds no build")
    if np.float32(max_distance) > np.float32(scene.stats["max_distance"]):
        raise ValueError("max_distance %g is above the %g the scene was built for" % (max_distance, scene.stats["max_distance"]))


def register_check_params(p, bound):
    """ValueError on what smx_distscene_register would refuse of a RegisterParams for a scene built for `bound`, before
    anything is called."""
    used = 0
    for k in range(3):
        it, s, q = int(p.level_iterations[k]), int(p.level_stride[k]), np.float32(p.level_max_distance[k])
        if not 0 <= it <= 32:
            raise ValueError("level_iterations must lie in 0 .. 32")
        if it == 0:
            continue
        used += 1
        if not 1 <= s <= REGISTER_MAX_STRIDE:
            raise ValueError("level_stride must lie in 1 .. %d" % REGISTER_MAX_STRIDE)
        if not (q == 0 or (np.isfinite(q) and np.float32(1e-3) <= q <= np.float32(bound))):
            raise ValueError("level_max_distance %g must be 0 (the scene's bound) or lie in 0.001 .. %g, the bound" % (q, bound))
    if used == 0:
        raise ValueError("no level with iterations")
    if not (0 < p.max_normal_angle_deg <= 180):
        raise ValueError("max_normal_angle_deg must lie in (0, 180]")
    if not (p.convergence_rotation >= 0 and p.convergence_translation >= 0 and p.min_inliers >= 0 and 0 <= p.min_inlier_fraction <= 1 and
            p.min_pivot_ratio >= 0):
        raise ValueError("convergence bounds, min_inliers, min_inlier_fraction (at most 1) and min_pivot_ratio must not be negative")


def register_result_dict(res):
    """smx_register_result as a dict: scene_T_points [3,4] and information [6,6] float32 arrays, the rest numbers."""
    d = {n: getattr(res, n) for n, _ in RegisterResult._fields_ if n not in ("scene_T_points", "information")}
    d["scene_T_points"] = np.array(res.scene_T_points, np.float32).reshape(3, 4)
    d["information"] = np.array(res.information, np.float32).reshape(6, 6)
    return d


def compare_side_dict(side, max_distance=None):
    """smx_compare_side as a dict, as one side of compare_stats_dict."""
    dist = distance_stats_dict(side.distance)
    if max_distance is not None:
        dist["max_distance"] = float(max_distance)
    return dict(sample=sample_stats_dict(side.sample), distance=dist, sum_d=int(side.sum_d), sum_sq_lo=int(side.sum_sq_lo),
                sum_sq_hi=int(side.sum_sq_hi))


def register_robust_params(kernel="none", scale=0.0, reject_rim=False):
    """The robust part of a registration as smx_register_robust_params; ValueError on what the library would refuse, before
    anything is launched.  kernel: "none", "huber" or "tukey" (or 0, 1, 2); scale: the kernel's c in metres, one value for all
    levels or three (0 = no weights on that level, else 1e-6 .. 16); reject_rim: reject matches on the rim of the scene's mesh."""
    if isinstance(kernel, str):
        if kernel not in REGISTER_KERNELS:
            raise ValueError("kernel must be one of %s" % ", ".join(REGISTER_KERNELS))
        kernel = REGISTER_KERNELS[kernel]
    if isinstance(kernel, bool) or not isinstance(kernel, (int, np.integer)) or not 0 <= int(kernel) <= 2:
        raise ValueError("kernel must be 0 (none), 1 (Huber) or 2 (Tukey)")
    if not isinstance(reject_rim, (bool, np.bool_)) and reject_rim not in (0, 1):
        raise ValueError("reject_rim must be False or True")
    scales = [float(v) for v in (np.asarray(scale, np.float64).reshape(-1).tolist())]
    if len(scales) == 1:
        scales = scales * 3
    if len(scales) != 3:
        raise ValueError("scale must be one value or three, one per level")
    for c in scales:
        c32 = float(np.float32(c))
        if not (c32 == 0.0 or (np.isfinite(c32) and np.float32(1e-6) <= np.float32(c) <= np.float32(16.0))):
            raise ValueError("a scale must be 0 or finite in 1e-6 .. 16 metres")
    return RegisterRobustParams(int(kernel), (C.c_float * 3)(*scales), 1 if reject_rim else 0)


def pose_lattice(k, centre, anchors):
    """The candidate poses of a registration without a start (smx_register_pose_lattice), [N_k * A, 3, 4] float32, scene <- points:
    every rotation of the integer-quaternion lattice of order k (40, 272, 888, 2080, ... for k = 1, 2, 3, 4; k <= 8) about
    `centre` (a point in the points' frame), its image placed on every anchor ([A,3], points in the scene's frame where the
    centre may lie).  Pose index = rotation index * A + anchor index.  Host only.  ValueError on what the library would refuse."""
    c = np.ascontiguousarray(centre, np.float64).reshape(-1)
    a = np.ascontiguousarray(anchors, np.float64).reshape(-1)
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= 8:
        raise ValueError("k must lie in 1 .. 8")
    if c.size != 3 or a.size == 0 or a.size % 3 or not (np.all(np.isfinite(c)) and np.all(np.isfinite(a))):
        raise ValueError("centre must hold three finite values and anchors at least one finite [A,3] row")
    n = C.c_uint32(0)
    _lib.load().smx_register_pose_lattice(C.c_int32(int(k)), c.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), C.c_uint32(a.size // 3),
                                          None, C.c_uint32(0), C.byref(n))
    if n.value == 0:
        raise ValueError("more than 2^20 poses: fewer anchors or a smaller k")
    poses = np.zeros((n.value, 3, 4), np.float32)
    _lib.check(_lib.load().smx_register_pose_lattice(C.c_int32(int(k)), c.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                                     C.c_uint32(a.size // 3), poses.ctypes.data_as(C.c_void_p), C.c_uint32(n.value), C.byref(n)))
    return poses


def score_params(stride=1, max_distance=0.0, reject_rim=False):
    """smx_score_params; ValueError on what the library would refuse whatever the scene."""
    if isinstance(stride, bool) or int(stride) != stride or not 1 <= int(stride) <= REGISTER_MAX_STRIDE:
        raise ValueError("stride must lie in 1 .. %d" % REGISTER_MAX_STRIDE)
    q = np.float32(max_distance)
    if not (q == 0 or (np.isfinite(q) and np.float32(1e-3) <= q <= np.float32(16.0))):
        raise ValueError("max_distance must be 0 (the scene's bound) or lie in 0.001 .. 16")
    if not isinstance(reject_rim, (bool, np.bool_)) and reject_rim not in (0, 1):
        raise ValueError("reject_rim must be False or True")
    return ScoreParams(int(stride), float(q), 1 if reject_rim else 0)


def global_result_dict(res):
    """smx_global_result as a dict: result (register_result_dict of the winner), found, winner_rank, n_starts_run, starts (a list
    of dicts, one per start run)."""
    starts = [{n: int(getattr(s, n)) for n, _ in s._fields_} for s in res.starts[:res.n_starts_run]]
    return dict(result=register_result_dict(res.result), found=int(res.found), winner_rank=int(res.winner_rank),
                n_starts_run=int(res.n_starts_run), starts=starts)


def _points_for_call(points, normals=None):
    """(device?, n_points, address of points, address of normals, what to keep alive) of a numpy array or a contiguous float32
    device tensor of points, and of normals of the same kind and shape."""
    dev = _device_address(points) is not None
    if normals is not None and (_device_address(normals) is not None) != dev:
        raise ValueError("points and normals must both be device tensors or both be host arrays")
    if dev:
        import torch
        for a in (points, normals):
            if a is not None and not (a.is_contiguous() and a.dtype == torch.float32 and a.numel() % 3 == 0):
                raise ValueError("a device tensor of points or normals must be contiguous [P,3] float32")
        n_points = points.numel() // 3
        if normals is not None and normals.numel() != points.numel():
            raise ValueError("normals must have the shape of points")
        torch.cuda.current_stream(points.device).synchronize()      # (the tensors' producers; the call runs on its own stream)
        return True, n_points, points.data_ptr() if n_points else None, normals.data_ptr() if normals is not None and n_points else None, [points, normals]
    pts = np.ascontiguousarray(points, np.float32)
    if pts.size % 3:
        raise ValueError("points must hold three values per row")
    n_points = pts.size // 3
    nr = None
    if normals is not None:
        nr = np.ascontiguousarray(normals, np.float32)
        if nr.size != pts.size:
            raise ValueError("normals must have the shape of points")
    return False, n_points, pts.ctypes.data if n_points else None, nr.ctypes.data if nr is not None and n_points else None, [pts, nr]


class DistanceScene:
    """Not in the reference: a snapshot of a triangle array over the map with the search structure of MeshDistance
    (smx_distscene), built once by CUDASurfelReconstruction.BuildDistanceScene for one bound on max_distance and queried many
    times.  After the build a query reads neither the map nor the triangle array: it answers what MeshDistance answered on the
    map as it stood at the build, through later Integrate, Compact and deformation calls and after the reconstruction object
    is gone.  .stats is the dict of smx_distscene_stats of the build.  close() frees the device memory; the object is a context
    manager."""

    def __init__(self, device_id=-1):
        self._h = C.c_void_p()
        self.stats = None
        self.has_rim = False           # the last build kept the rim bytes of its triangles (BuildDistanceScene(rim=True))
        self.rim_stats = None
        _lib.check(_lib.load().smx_distscene_create(C.c_int32(device_id), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().smx_distscene_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        """Device memory the scene held after its build (smx_distscene_stats.device_bytes); 0 for a scene without a build."""
        return self.stats["device_bytes"] if self.stats else 0

    def Query(self, stream, points, max_distance=None, signed=False, return_closest=False):
        """For every point of `points` ([P,3] float32) what MeshDistance returns for the triangles and the map of the build
        (smx_distscene_query): byte for byte the same nearest, distance, closest and statistics.  max_distance: at most the
        bound of the build (None: the bound).  Synchronous.  points is a numpy array or a contiguous float32 device tensor; the
        results then are device tensors too.  Returns (nearest, distance, then with return_closest closest, then the dict of
        smx_distance_stats)."""
        if max_distance is None:
            if not getattr(self, "stats", None):
                raise ValueError("the scene holds no build")
            max_distance = self.stats["max_distance"]
        p = distance_params(max_distance, 0.0, signed)
        distscene_check_query(self, p.max_distance)
        st = DistanceStats()
        dev = _device_address(points) is not None
        if dev:
            import torch
            if not (points.is_contiguous() and points.dtype == torch.float32 and points.numel() % 3 == 0):
                raise ValueError("a device tensor of points must be contiguous [P,3] float32")
            n_points = points.numel() // 3
            nearest = torch.empty(n_points, dtype=torch.uint32, device=points.device)
            distance = torch.empty(n_points, dtype=torch.float32, device=points.device)
            closest = torch.empty((n_points, 3), dtype=torch.float32, device=points.device) if return_closest else None
            pin = points.data_ptr() if n_points else None
            outs = [a.data_ptr() if a is not None and n_points else None for a in (nearest, distance, closest)]
            torch.cuda.current_stream(points.device).synchronize()      # (the tensor's producers; the call runs on `stream`)
        else:
            pts = np.ascontiguousarray(points, np.float32)
            if pts.size % 3:
                raise ValueError("points must hold three values per row")
            n_points = pts.size // 3
            nearest, distance = np.zeros(n_points, np.uint32), np.zeros(n_points, np.float32)
            closest = np.zeros((n_points, 3), np.float32) if return_closest else None
            pin = pts.ctypes.data if n_points else None
            outs = [a.ctypes.data if a is not None and n_points else None for a in (nearest, distance, closest)]
        _lib.check(_lib.load().smx_distscene_query(self._h, _sv(stream), C.byref(p), C.c_void_p(pin), C.c_uint32(n_points), C.c_void_p(outs[0]),
                                                   C.c_void_p(outs[1]), C.c_void_p(outs[2]), C.c_int32(1 if dev else 0), C.byref(st)))
        stats = distance_stats_dict(st)
        stats["max_distance"] = float(p.max_distance)      # (what the histogram's bins are fractions of)
        return (nearest, distance, closest, stats) if return_closest else (nearest, distance, stats)

    def Register(self, stream, points, normals=None, T_init=None, params=None, result_buffer=None, robust=None):
        """Point-to-plane ICP of `points` ([P,3] float32, in their own frame) against the scene's triangles
        (smx_distscene_register): every iteration moves the samples by the pose, asks the scene's own query for their closest
        triangles and solves for a left twist; all iterations are enqueued back to back on `stream`.  normals ([P,3], optional)
        switches the normal gate on.  T_init: the start pose scene <- points ([3,4] or 12 values; None = the identity).
        params: a RegisterParams (RegisterParams.defaults()).  points (and normals) are numpy arrays or contiguous float32
        device tensors.  Without result_buffer the call is synchronous and returns a dict: scene_T_points [3,4] float32,
        status, iterations_run, inliers, points_used, rms_residual, last_update_rotation, last_update_translation, information
        [6,6].  With result_buffer (a CUDABuffer of at least ctypes.sizeof(RegisterResult) bytes in one row, or a device
        address) the smx_register_result stays on the device, and with device points nothing waits for the host.
        robust: a RegisterRobustParams (register_robust_params(...)) -- Huber or Tukey weights on the rows and / or rejection of
        the matches whose closest point lies on the rim of the scene's mesh, which needs a scene built with rim=True
        (smx_distscene_register_robust); None is the plain call."""
        if not getattr(self, "_h", None):
            raise ValueError("the scene is closed")
        if not getattr(self, "stats", None):
            raise ValueError("the scene holds no build")
        p = params if params is not None else RegisterParams.defaults()
        register_check_params(p, self.stats["max_distance"])
        if robust is not None:
            if not isinstance(robust, RegisterRobustParams):
                raise ValueError("robust must be a RegisterRobustParams (register_robust_params(...))")
            if robust.reject_rim and not self.has_rim:
                raise ValueError("reject_rim needs a scene built with rim=True")
        T = np.ascontiguousarray(np.asarray(np.eye(3, 4) if T_init is None else T_init, np.float32).reshape(-1))
        if T.size != 12 or not np.all(np.isfinite(T)):
            raise ValueError("T_init must hold 12 finite values")
        dev, n_points, pin, nin, keep = _points_for_call(points, normals)
        if n_points > REGISTER_MAX_POINTS:
            raise ValueError("at most 2^28 points")
        on_device = result_buffer is not None
        res = RegisterResult()
        if on_device:
            out = C.c_void_p(result_buffer.ToCUDA().address if isinstance(result_buffer, CUDABuffer) else int(result_buffer))
        tail = (C.c_void_p(pin), C.c_void_p(nin), C.c_uint32(n_points), C.c_int32(1 if dev else 0), T.ctypes.data_as(C.c_void_p),
                out if on_device else C.byref(res), C.c_int32(1 if on_device else 0))
        if robust is None:
            _lib.check(_lib.load().smx_distscene_register(self._h, _sv(stream), C.byref(p), *tail))
        else:
            _lib.check(_lib.load().smx_distscene_register_robust(self._h, _sv(stream), C.byref(p), C.byref(robust), *tail))
        del keep
        return None if on_device else register_result_dict(res)

    def RegisterRobustCounts(self, stream=None):
        """Per iteration of the scene's last Register call the two counts of the robust row, [iterations, 2] uint32
        (smx_distscene_debug_register_robust_counts): the matches rejected on the rim (sum [31]) and the samples Huber
        down-weighted or Tukey rejected (sum [32]).  Zeros after a plain call; like RegisterIterations, empty once a later
        Query or build on the scene has waited for the registration."""
        counts = (C.c_uint32 * 2 * 96)()
        n = C.c_int32(0)
        _lib.check(_lib.load().smx_distscene_debug_register_robust_counts(self._h, _sv(stream), counts, C.c_int32(96), C.byref(n)))
        return np.array([[row[0], row[1]] for row in counts[:n.value]], np.uint32).reshape(-1, 2)

    def RegisterIterations(self, stream=None):
        """One dict per iteration of the scene's last Register call (smx_distscene_debug_register_iterations): level, stride,
        status, Tf (the 12 floats the iteration linearised at), sums (31 float64: JtJ upper triangle, Jtr, sum r^2, inliers,
        samples that are not BAD, samples matched), x (6)."""
        recs = (RegisterIteration * 96)()
        n = C.c_int32(0)
        _lib.check(_lib.load().smx_distscene_debug_register_iterations(self._h, _sv(stream), recs, C.c_int32(96), C.byref(n)))
        return [{"level": r.level, "stride": r.stride, "status": r.status, "Tf": np.array(r.Tf, np.float32), "sums": np.array(r.sums, np.float64),
                 "x": np.array(r.x, np.float64)} for r in recs[:n.value]]

    def debug_register_timings(self):
        """Milliseconds of the last Register call: the whole call, then move, query, reduce and solve of its last iteration."""
        out = (C.c_float * REGISTER_PHASES)()
        _lib.check(_lib.load().smx_distscene_debug_register_timings(self._h, out, C.c_int32(REGISTER_PHASES)))
        return dict(zip(("call", "move", "query", "reduce", "solve"), [float(v) for v in out]))

    def _score_inputs(self, score, points, normals, poses):
        """What ScorePoses and RegisterGlobal check and marshal alike."""
        if not getattr(self, "_h", None):
            raise ValueError("the scene is closed")
        if not getattr(self, "stats", None):
            raise ValueError("the scene holds no build")
        sp = score if score is not None else score_params()
        if not isinstance(sp, ScoreParams):
            raise ValueError("score must be a ScoreParams (score_params(...))")
        if np.float32(sp.max_distance) > np.float32(self.stats["max_distance"]):
            raise ValueError("max_distance %g is above the %g the scene was built for" % (sp.max_distance, self.stats["max_distance"]))
        if sp.reject_rim and not self.has_rim:
            raise ValueError("reject_rim needs a scene built with rim=True")
        T = np.ascontiguousarray(poses, np.float32).reshape(-1)
        if T.size == 0 or T.size % 12 or T.size // 12 > GLOBAL_MAX_POSES or not np.all(np.isfinite(T)):
            raise ValueError("poses must hold 1 .. 2^20 finite [3,4] poses")
        dev, n_points, pin, nin, keep = _points_for_call(points, normals)
        if n_points > REGISTER_MAX_POINTS or -(-n_points // sp.stride) > GLOBAL_MAX_SAMPLES:
            raise ValueError("at most 2^28 points and 2^16 samples of them: a larger stride")
        return sp, T, dev, n_points, pin, nin, keep

    def ScorePoses(self, stream, points, poses, score=None):
        """The integer score of every pose of `poses` ([P,3,4] float32, scene <- points) for `points` ([n,3] float32, a numpy
        array or a contiguous device tensor) against the scene's triangles, all poses in one pass over the scene
        (smx_distscene_score_poses): a numpy record array [P] with cost (the sum over the samples of the matched distance in
        units of 2^-20 m, the gate's word for a sample that is not matched, BAD or rejected on the rim), n_ok, n_matched, n_rim.
        score: a ScoreParams (score_params(stride, max_distance, reject_rim)).  Synchronous."""
        sp, T, dev, n_points, pin, _, keep = self._score_inputs(score, points, None, poses)
        out = np.zeros(T.size // 12, np.dtype(POSE_SCORE_DTYPE))
        _lib.check(_lib.load().smx_distscene_score_poses(self._h, _sv(stream), C.byref(sp), C.c_void_p(pin), C.c_uint32(n_points),
                                                         C.c_int32(1 if dev else 0), T.ctypes.data_as(C.c_void_p), C.c_uint32(T.size // 12),
                                                         out.ctypes.data_as(C.c_void_p)))
        del keep
        return out

    def RegisterGlobal(self, stream, points, normals, poses, params=None, robust=None, score=None, n_starts=8, min_matched_fraction=0.5,
                       return_scores=False):
        """Registration without a start pose (smx_distscene_register_global): every pose of `poses` ([P,3,4], pose_lattice(...))
        is scored as ScorePoses does, the n_starts cheapest -- ties to the smaller index -- are each refined by Register (params,
        robust as there; byte for byte that call's result from that start), the results are scored again and the cheapest wins.
        Returns global_result_dict: result (the winner's Register dict), found (its status is OK or CONVERGED and at least
        min_matched_fraction of its samples that are not BAD are matched), winner_rank, n_starts_run, starts (pose_index, status,
        iterations_run, n_matched_after, cost_before, cost_after per start); with return_scores also the [P] record array of all
        scores.  Synchronous."""
        sp, T, dev, n_points, pin, nin, keep = self._score_inputs(score, points, normals, poses)
        p = params if params is not None else RegisterParams.defaults()
        register_check_params(p, self.stats["max_distance"])
        if robust is not None:
            if not isinstance(robust, RegisterRobustParams):
                raise ValueError("robust must be a RegisterRobustParams (register_robust_params(...))")
            if robust.reject_rim and not self.has_rim:
                raise ValueError("reject_rim needs a scene built with rim=True")
        if isinstance(n_starts, bool) or int(n_starts) != n_starts or not 1 <= int(n_starts) <= GLOBAL_MAX_STARTS:
            raise ValueError("n_starts must lie in 1 .. %d" % GLOBAL_MAX_STARTS)
        if not 0.0 <= float(min_matched_fraction) <= 1.0:
            raise ValueError("min_matched_fraction must lie in 0 .. 1")
        gp = GlobalParams(sp, int(n_starts), float(min_matched_fraction))
        res = GlobalResult()
        scores = np.zeros(T.size // 12, np.dtype(POSE_SCORE_DTYPE)) if return_scores else None
        _lib.check(_lib.load().smx_distscene_register_global(
            self._h, _sv(stream), C.byref(gp), C.byref(p), C.byref(robust) if robust is not None else None, C.c_void_p(pin), C.c_void_p(nin),
            C.c_uint32(n_points), C.c_int32(1 if dev else 0), T.ctypes.data_as(C.c_void_p), C.c_uint32(T.size // 12), C.byref(res),
            scores.ctypes.data_as(C.c_void_p) if return_scores else None))
        del keep
        out = global_result_dict(res)
        return (out, scores) if return_scores else out

    def debug_set_score_chunk(self, chunk_points):
        """Tests: the samples a chunk of ScorePoses may hold (smx_distscene_debug_set_score_chunk; the library's 2^22 bounds the
        workspace), so that a small case crosses chunk edges."""
        _lib.check(_lib.load().smx_distscene_debug_set_score_chunk(self._h, C.c_uint32(int(chunk_points))))

    def debug_global_timings(self):
        """Milliseconds of the last ScorePoses / RegisterGlobal: the score phase, then move, query and score kernel of its last
        chunk, then select, refine and rescore of the last RegisterGlobal (0 after a bare ScorePoses)."""
        out = (C.c_float * GLOBAL_PHASES)()
        _lib.check(_lib.load().smx_distscene_debug_global_timings(self._h, out, C.c_int32(GLOBAL_PHASES)))
        return dict(zip(("score", "move", "query", "score_kernel", "select", "refine", "rescore"), [float(v) for v in out]))

    def debug_timings(self):
        """Milliseconds of the last build (mark, index, first) and of the last query (query, stats)."""
        out = (C.c_float * DISTSCENE_PHASES)()
        _lib.check(_lib.load().smx_distscene_debug_timings(self._h, out, C.c_int32(DISTSCENE_PHASES)))
        return dict(zip(("mark", "index", "first", "query", "stats"), [float(v) for v in out]))


def merge_params(cell_size=0.05, radius_factor_squared=1.0, max_normal_angle_deg=30.0, k=8, mode="keep", confidence_cap=None,
                 frame_index=1):
    """smx_merge_params from keyword arguments: mode "keep" / "blend" (or 0 / 1); confidence_cap None = FLT_MAX.  ValueError on
    what the library would refuse."""
    if isinstance(mode, str):
        if mode not in _lib.MERGE_MODES:
            raise ValueError("mode must be one of %s" % ", ".join(_lib.MERGE_MODES))
        mode = _lib.MERGE_MODES[mode]
    cap = float(np.finfo(np.float32).max) if confidence_cap is None else float(confidence_cap)
    if not (float(cell_size) > 0 and float(radius_factor_squared) > 0):
        raise ValueError("cell_size and radius_factor_squared must be > 0")
    if not 0.0 <= float(max_normal_angle_deg) <= 180.0:
        raise ValueError("max_normal_angle_deg must be within 0 .. 180")
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be within 1 .. 64")
    if int(mode) not in (0, 1):
        raise ValueError("mode must be 0 (keep) or 1 (blend)")
    if not 1 <= int(frame_index) <= 0xFFFFFFFF:
        raise ValueError("frame_index must be >= 1")
    if cap != cap:
        raise ValueError("confidence_cap must not be NaN")
    return _lib.MergeParams(cell_size, radius_factor_squared, max_normal_angle_deg, int(k), int(mode), cap, int(frame_index))


def merge_stats_dict(st):
    return {n: int(getattr(st, n)) for n, _ in _lib.MergeStats._fields_}


def import_params(cell_size=0.05, search_radius=0.1, k=16, min_neighbors=6, max_surface_variation=None, radius_rank=8,
                  radius_scale_squared=2.0, confidence=1.0, default_color=0, frame_index=1, orient="none", view_point=(0.0, 0.0, 0.0)):
    """smx_import_params from keyword arguments: orient "none" / "view_point" / "origins" (or 0 / 1 / 2);
    max_surface_variation None = 1/3, which rejects nothing.  ValueError on what the library would refuse."""
    if isinstance(orient, str):
        if orient not in _lib.IMPORT_ORIENTS:
            raise ValueError("orient must be one of %s" % ", ".join(_lib.IMPORT_ORIENTS))
        orient = _lib.IMPORT_ORIENTS[orient]
    third = float(np.float32(1.0 / 3.0))
    msv = third if max_surface_variation is None else float(np.float32(max_surface_variation))
    if not (float(cell_size) > 0 and float(search_radius) > 0 and float(radius_scale_squared) > 0):
        raise ValueError("cell_size, search_radius and radius_scale_squared must be > 0")
    if not 4 <= int(k) <= 64:
        raise ValueError("k must be within 4 .. 64")
    if not 3 <= int(min_neighbors) <= int(k):
        raise ValueError("min_neighbors must be within 3 .. k")
    if not 0.0 <= msv <= third:
        raise ValueError("max_surface_variation must be within 0 .. 1/3")
    if not 1 <= int(radius_rank) <= 63:
        raise ValueError("radius_rank must be within 1 .. 63")
    if not 1 <= int(frame_index) <= 0xFFFFFFFF:
        raise ValueError("frame_index must be >= 1")
    if int(orient) not in (0, 1, 2):
        raise ValueError("orient must be 0 (none), 1 (view_point) or 2 (origins)")
    vp = [float(v) for v in np.asarray(view_point, np.float64).reshape(3)]
    if not (np.isfinite(float(confidence)) and np.all(np.isfinite(vp))):
        raise ValueError("confidence and view_point must be finite")
    return _lib.ImportParams(cell_size, search_radius, int(k), int(min_neighbors), msv, int(radius_rank), radius_scale_squared,
                             confidence, int(default_color) & 0xFFFFFFFF, int(frame_index), int(orient), (C.c_float * 3)(*vp))


def import_stats_dict(st):
    return {n: int(getattr(st, n)) for n, _ in _lib.ImportStats._fields_}


def _cloud_arg(a, width, dtype, what):
    """A per-point input of ImportPoints: (points it holds, address or None, on_device, the object that keeps it alive)."""
    if _device_address(a) is not None:
        if not (a.is_contiguous() and a.element_size() == 4 and a.numel() % width == 0):
            raise ValueError("a device tensor of %s must be contiguous 32-bit values, %d per point" % (what, width))
        import torch
        torch.cuda.current_stream(a.device).synchronize()      # (the tensor's producers; the call runs on its own stream)
        return a.numel() // width, (a.data_ptr() if a.numel() else None), True, a
    h = np.ascontiguousarray(a, dtype)
    if h.size % width:
        raise ValueError("%s must hold %d values per point" % (what, width))
    return h.size // width, (h.ctypes.data if h.size else None), False, h


def _device_address(a):
    """The device address of a device tensor (anything with is_cuda / data_ptr), None for everything else."""
    if getattr(a, "is_cuda", False) and hasattr(a, "data_ptr"):
        return int(a.data_ptr())
    return None


def _triangles_arg(triangles):
    """A triangle array for the library: (n_in, address or None, on_device, the object that keeps the address alive).
    ValueError on what is not [T,3] 32-bit integers."""
    if _device_address(triangles) is not None:
        if not (triangles.is_contiguous() and triangles.element_size() == 4 and triangles.numel() % 3 == 0):
            raise ValueError("a device tensor of triangles must be contiguous [T,3] 32-bit integers")
        import torch
        n_in = triangles.numel() // 3
        torch.cuda.current_stream(triangles.device).synchronize()      # (the tensor's producers; the call runs on its own stream)
        return n_in, (triangles.data_ptr() if n_in else None), True, triangles
    tri = np.ascontiguousarray(triangles, np.uint32)
    if tri.size % 3:
        raise ValueError("triangles must hold three values per row")
    n_in = tri.size // 3
    return n_in, (tri.ctypes.data if n_in else None), False, tri


kSurfelAttributeCount = 25        # APP/cuda_surfel_reconstruction_kernels.cuh:76

# smx.h: colour modes of the viewer buffers and the render, splat shapes of the render
SMX_VIS_LAST_UPDATE, SMX_VIS_CREATION, SMX_VIS_RADII, SMX_VIS_NORMALS = 1, 2, 4, 8
SMX_SPLAT_SQUARE, SMX_SPLAT_DISC = 0, 1
# smx.h: where the mesh render takes its normals from; the box size above which a triangle goes to the tiled kernel
SMX_MESH_NORMAL_VERTEX, SMX_MESH_NORMAL_FACE = 0, 1
SMX_MESH_RENDER_LARGE_PIXELS = 256
# smx.h: outcome of smx_recon_track (>= SMX_TRACK_TOO_FEW_INLIERS: nothing usable was solved)
SMX_TRACK_OK, SMX_TRACK_CONVERGED, SMX_TRACK_TOO_FEW_INLIERS, SMX_TRACK_DEGENERATE, SMX_TRACK_NOT_FINITE = range(5)
TRACK_STATUS_NAMES = ("OK", "CONVERGED", "TOO_FEW_INLIERS", "DEGENERATE", "NOT_FINITE")


class TrackOutcome:
    """What CUDASurfelReconstruction.Track returns: global_T_frame (3 x 4 float32), status (SMX_TRACK_*), ok,
    iterations_run, inliers, pixels_with_depth, rms_residual (metres), last_update_rotation / _translation,
    information (6 x 6, JtJ of the last iteration: rotation first)."""

    def __init__(self, res):
        self.global_T_frame = np.array(res.global_T_frame, np.float32).reshape(3, 4)
        self.status = int(res.status)
        self.ok = self.status < SMX_TRACK_TOO_FEW_INLIERS
        self.status_name = TRACK_STATUS_NAMES[self.status] if 0 <= self.status < 5 else "?"
        self.iterations_run = int(res.iterations_run)
        self.inliers, self.pixels_with_depth = int(res.inliers), int(res.pixels_with_depth)
        self.rms_residual = float(res.rms_residual)
        self.last_update_rotation = float(res.last_update_rotation)
        self.last_update_translation = float(res.last_update_translation)
        self.information = np.array(res.information, np.float32).reshape(6, 6)

    def __repr__(self):
        return "TrackOutcome(%s, %d iterations, %d / %d inliers, rms %.4g m)" % (
            self.status_name, self.iterations_run, self.inliers, self.pixels_with_depth, self.rms_residual)


class TrackRGBDOutcome(TrackOutcome):
    """What CUDASurfelReconstruction.TrackRGBD returns: a TrackOutcome (inliers and rms_residual are the geometric ones,
    information the combined JtJ) plus photometric_inliers and rms_intensity_residual (0..1 intensity scale)."""

    def __init__(self, res):
        TrackOutcome.__init__(self, res.icp)
        self.photometric_inliers = int(res.photometric_inliers)
        self.rms_intensity_residual = float(res.rms_intensity_residual)

    def __repr__(self):
        return "TrackRGBDOutcome(%s, %d iterations, %d / %d inliers, rms %.4g m; %d photometric, rms %.4g)" % (
            self.status_name, self.iterations_run, self.inliers, self.pixels_with_depth, self.rms_residual,
            self.photometric_inliers, self.rms_intensity_residual)


def vis_flags(visualize_last_update_timestamp=False, visualize_creation_timestamp=False, visualize_radii=False,
              visualize_normals=False):
    return ((SMX_VIS_LAST_UPDATE if visualize_last_update_timestamp else 0) |
            (SMX_VIS_CREATION if visualize_creation_timestamp else 0) |
            (SMX_VIS_RADII if visualize_radii else 0) | (SMX_VIS_NORMALS if visualize_normals else 0))


def make_render_params(width, height, fx, fy, cx, cy, global_T_camera, near_z=0.05, far_z=1000.0,
                       splat_mode=SMX_SPLAT_SQUARE, splat_half_extent_in_pixels=3.0, disc_radius_factor=1.0,
                       max_splat_extent_in_pixels=16.0, color_flags=0, frame_index=0,
                       surfel_integration_active_window_size=2147483647):
    """An smx_render_params.  Defaults: the reference viewer's --splat_half_extent_in_pixels (APP/main.cc:506), a disc as
    large as the surfel, splats of at most 16 pixels, the surfels' own colours."""
    T = np.asarray(global_T_camera, np.float32).reshape(12)
    return RenderParams(int(width), int(height), fx, fy, cx, cy, (C.c_float * 12)(*[float(v) for v in T]), near_z,
                        far_z, int(splat_mode), splat_half_extent_in_pixels, disc_radius_factor,
                        max_splat_extent_in_pixels, int(color_flags), int(frame_index) & 0xFFFFFFFF,
                        int(surfel_integration_active_window_size))


def make_mesh_render_params(width, height, fx, fy, cx, cy, global_T_camera, near_z=0.05, far_z=1000.0, color_flags=0,
                            frame_index=0, surfel_integration_active_window_size=2147483647, cull_back_faces=False,
                            normal_mode=SMX_MESH_NORMAL_VERTEX):
    """An smx_mesh_render_params.  Defaults: the depth range of make_render_params, the surfels' own colours, both faces
    drawn, normals interpolated from the corners."""
    T = np.asarray(global_T_camera, np.float32).reshape(12)
    return MeshRenderParams(int(width), int(height), fx, fy, cx, cy, (C.c_float * 12)(*[float(v) for v in T]), near_z, far_z,
                            int(color_flags), int(frame_index) & 0xFFFFFFFF, int(surfel_integration_active_window_size),
                            int(cull_back_faces), int(normal_mode))


def _slots_of(buf, slot_bytes):
    """(device pointer, capacity in slots) of a viewer buffer: None, a CUDABuffer whose rows lie back to back, an
    object with data_ptr() / numel() / element_size() (a torch tensor on the GPU), or a (pointer, capacity) pair."""
    if buf is None:
        return C.c_void_p(0), 0
    if isinstance(buf, CUDABuffer):
        d = buf.ToCUDA()
        if d.height > 1 and d.pitch != d.width * buf.elem_bytes:
            raise ValueError("a viewer buffer needs its rows back to back (height 1)")
        return C.c_void_p(d.address), (d.width * d.height * buf.elem_bytes) // slot_bytes
    if hasattr(buf, "data_ptr"):
        return C.c_void_p(buf.data_ptr()), (buf.numel() * buf.element_size()) // slot_bytes
    ptr, cap = buf
    return C.c_void_p(int(ptr)), int(cap)


def _stream(s):
    return C.c_void_p(s) if s else C.c_void_p(0)


class Stream:
    """A HIP stream (cudaStream_t in the reference's signatures)."""

    def __init__(self, priority_class=None, cu_mask=None):
        """priority_class: None = plain stream; -1 / 0 / +1 = lowest / default / highest device priority
        (cudaStreamCreateWithPriority).  cu_mask: list of 32-bit words, bit k = compute unit k may be used
        (smx_stream_create_with_cu_mask; default priority)."""
        self.handle = C.c_void_p()
        if cu_mask:
            arr = (C.c_uint32 * len(cu_mask))(*cu_mask)
            _lib.check(_lib.load().smx_stream_create_with_cu_mask(C.byref(self.handle), arr, C.c_uint32(len(cu_mask))))
        elif priority_class is None:
            _lib.check(_lib.load().smx_stream_create(C.byref(self.handle)))
        else:
            _lib.check(_lib.load().smx_stream_create_with_priority(C.byref(self.handle), C.c_int32(priority_class)))

    def synchronize(self):
        _lib.check(_lib.load().smx_stream_synchronize(self.handle))

    def __int__(self):
        return self.handle.value or 0

    def close(self):
        if self.handle:
            _lib.load().smx_stream_destroy(self.handle)
            self.handle = C.c_void_p()


class _PagelockedBlock:
    """Owner of one smx_host_alloc block; numpy arrays made from it keep it alive (it is their base object)."""

    def __init__(self, nbytes, write_combined):
        self._p = C.c_void_p()
        _lib.check(_lib.load().smx_host_alloc(C.byref(self._p), C.c_size_t(max(nbytes, 1)),
                                              C.c_int32(1 if write_combined else 0)))
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (self._p.value, False), "version": 3}

    def __del__(self):
        try:
            if self._p:
                _lib.load().smx_host_free(self._p)
                self._p = C.c_void_p()
        except Exception:
            pass


class PagelockedArray:
    """Page-locked host memory as a numpy array (cudaHostAlloc in the reference's upload staging,
    APP/main.cc:825-829, 917): uploads from `.array` are asynchronous to the host.  The memory lives as long as this
    object or any view of `.array` does; keep one of them until the copies that read it have finished."""

    def __init__(self, shape, dtype, write_combined=False):
        self.dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * self.dtype.itemsize
        self.array = np.asarray(_PagelockedBlock(n, write_combined)).view(self.dtype).reshape(shape)

    def close(self):
        """Drop this object's reference (the block is freed once no view is left)."""
        self.array = None


def _sv(stream):
    if stream is None:
        return C.c_void_p(0)
    if isinstance(stream, Stream):
        return stream.handle
    return C.c_void_p(int(stream))


def StreamSynchronize(stream=None):
    _lib.check(_lib.load().smx_stream_synchronize(_sv(stream)))


def DebugLiveAllocations():
    """(blocks, bytes) of device and page-locked memory the library's objects hold right now (smx_debug_live_allocations)."""
    blocks, nbytes = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.load().smx_debug_live_allocations(C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


def DebugFailAllocation(nth):
    """Test hook: the nth next allocation of the library's objects fails (0 = the next one), nth < 0 disarms."""
    _lib.check(_lib.load().smx_debug_fail_allocation(C.c_int32(nth)))


class CUDABuffer:
    """CUDABuffer<T>(height, width): pitched 2-D device memory.  `dtype` is the numpy scalar type
    and `channels` the number of scalars per element (float2 -> (np.float32, 2), Vec3u8 -> (np.uint8, 3))."""

    def __init__(self, height, width, dtype, channels=1):
        self.dtype = np.dtype(dtype)
        self.channels = int(channels)
        self.elem_bytes = self.dtype.itemsize * self.channels
        self._h = C.c_void_p()
        _lib.check(_lib.load().smx_buffer_create(int(height), int(width), self.elem_bytes, C.byref(self._h)))
        self._desc = BufferDesc()
        _lib.check(_lib.load().smx_buffer_get_desc(self._h, C.byref(self._desc)))

    # -- reference accessors
    def width(self):
        return self._desc.width

    def height(self):
        return self._desc.height

    def Size(self):
        return self._desc.pitch * self._desc.height

    def ToCUDA(self):
        return self._desc

    def _host_shape(self):
        return (self.height(), self.width()) + ((self.channels,) if self.channels > 1 else ())

    def UploadAsync(self, stream, data):
        a = np.ascontiguousarray(data, dtype=self.dtype)
        assert a.shape == self._host_shape(), (a.shape, self._host_shape())
        _lib.check(_lib.load().smx_buffer_upload(self._h, _sv(stream), a.ctypes.data_as(C.c_void_p), C.c_size_t(0)))
        self._keep = a  # keep the host array alive until the caller synchronises

    def UploadByKernelAsync(self, stream, data):
        """The same copy done by a kernel that reads the page-locked source over the bus (smx_buffer_upload_by_kernel); `data`
        must be (a view of) a PagelockedArray of the buffer's shape and dtype -- raises SmxError otherwise."""
        assert data.dtype == self.dtype and data.shape == self._host_shape() and data.flags.c_contiguous
        _lib.check(_lib.load().smx_buffer_upload_by_kernel(self._h, _sv(stream), data.ctypes.data_as(C.c_void_p), C.c_size_t(0), C.c_void_p(0)))
        self._keep = data

    def UploadPitchedAsync(self, stream, pitch, data):
        _lib.check(_lib.load().smx_buffer_upload(self._h, _sv(stream), data.ctypes.data_as(C.c_void_p), C.c_size_t(pitch)))
        self._keep = data

    def UploadPartAsync(self, start, length, stream, data):
        a = np.ascontiguousarray(data)
        _lib.check(_lib.load().smx_buffer_upload_part(self._h, _sv(stream), C.c_size_t(start), C.c_size_t(length),
                                                      a.ctypes.data_as(C.c_void_p)))
        self._keep = a

    def DownloadAsync(self, stream, out=None):
        if out is None:
            out = np.empty(self._host_shape(), self.dtype)
        assert out.flags.c_contiguous and out.dtype == self.dtype and out.shape == self._host_shape()
        _lib.check(_lib.load().smx_buffer_download(self._h, _sv(stream), out.ctypes.data_as(C.c_void_p), C.c_size_t(0)))
        return out

    def DownloadPartAsync(self, start, length, stream, out):
        _lib.check(_lib.load().smx_buffer_download_part(self._h, _sv(stream), C.c_size_t(start), C.c_size_t(length),
                                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def Download(self, stream=None):
        """DebugDownload: blocking convenience."""
        out = self.DownloadAsync(stream)
        StreamSynchronize(stream)
        return out

    def Upload(self, data, stream=None):
        """DebugUpload: blocking convenience."""
        self.UploadAsync(stream, data)
        StreamSynchronize(stream)

    def Clear(self, value, stream=None):
        pat = np.asarray(value, dtype=self.dtype).reshape(-1)
        if pat.size == 1 and self.channels > 1:
            pat = np.repeat(pat, self.channels)
        assert pat.size == self.channels
        pat = np.ascontiguousarray(pat)
        _lib.check(_lib.load().smx_buffer_clear(self._h, _sv(stream), pat.ctypes.data_as(C.c_void_p)))

    def SetTo(self, other, stream=None):
        _lib.check(_lib.load().smx_buffer_set_to(self._h, other._h, _sv(stream)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().smx_buffer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _d(buf):
    return C.byref(buf.ToCUDA() if isinstance(buf, CUDABuffer) else buf)


# ---- depth preprocessing free functions (APP/cuda_depth_processing.cuh) -----------------------
def BilateralFilteringAndDepthCutoffCUDA(stream, sigma_xy, sigma_value_factor, value_to_ignore, radius_factor,
                                         max_depth, depth_valid_region_radius, input_depth, output_depth):
    _lib.check(_lib.load().smx_bilateral_filtering_and_depth_cutoff(
        _sv(stream), C.c_float(sigma_xy), C.c_float(sigma_value_factor), C.c_uint16(int(value_to_ignore)),
        C.c_float(radius_factor), C.c_uint16(int(max_depth)), C.c_float(depth_valid_region_radius),
        _d(input_depth), _d(output_depth)))


def OutlierDepthMapFusionCUDA(stream, tolerance, input_depth, depth_fx, depth_fy, depth_cx, depth_cy, other_depths,
                              others_TR_reference, output_depth, required_count=-1):
    """Both overloads of OutlierDepthMapFusionCUDA<count,u16>: count-1 == len(other_depths);
    required_count=-1 is the all-must-agree overload (APP/main.cc:1061-1112)."""
    n = len(other_depths)
    descs = (BufferDesc * n)(*[b.ToCUDA() if isinstance(b, CUDABuffer) else b for b in other_depths])
    T = np.ascontiguousarray(np.asarray(others_TR_reference, np.float32).reshape(n, 12))
    _lib.check(_lib.load().smx_outlier_depth_map_fusion(
        _sv(stream), C.c_int32(n), C.c_int32(required_count), C.c_float(tolerance), _d(input_depth),
        C.c_float(depth_fx), C.c_float(depth_fy), C.c_float(depth_cx), C.c_float(depth_cy),
        descs, T.ctypes.data_as(C.c_void_p), _d(output_depth)))


def BilateralFilteringAndOutlierFusionCUDA(stream, sigma_xy, sigma_value_factor, radius_factor, max_depth,
                                           depth_valid_region_radius, input_depth, tolerance, depth_fx, depth_fy, depth_cx,
                                           depth_cy, other_depths, others_TR_reference, scratch_depth, output_depth,
                                           required_count=-1):
    """BilateralFilteringAndDepthCutoffCUDA (value_to_ignore 0) + OutlierDepthMapFusionCUDA as the reference's caller chains
    them (APP/main.cc:1015-1115): one launch where the library can fuse them (smx_bilateral_outlier_fusion), same output."""
    n = len(other_depths)
    descs = (BufferDesc * n)(*[b.ToCUDA() if isinstance(b, CUDABuffer) else b for b in other_depths])
    T = np.ascontiguousarray(np.asarray(others_TR_reference, np.float32).reshape(n, 12))
    _lib.check(_lib.load().smx_bilateral_outlier_fusion(
        _sv(stream), C.c_float(sigma_xy), C.c_float(sigma_value_factor), C.c_float(radius_factor), C.c_uint16(int(max_depth)),
        C.c_float(depth_valid_region_radius), _d(input_depth), C.c_int32(n), C.c_int32(required_count), C.c_float(tolerance),
        C.c_float(depth_fx), C.c_float(depth_fy), C.c_float(depth_cx), C.c_float(depth_cy),
        descs, T.ctypes.data_as(C.c_void_p), _d(scratch_depth), _d(output_depth)))


def ErodeDepthMapCUDA(stream, radius, input_depth, output_depth):
    _lib.check(_lib.load().smx_erode_depth_map(_sv(stream), C.c_int32(radius), _d(input_depth), _d(output_depth)))


def MedianFilterAndDensifyDepthMapCUDA(stream, input_depth, output_depth):
    """MedianFilterAndDensifyDepthMap (APP/main.cc:206-252, a CPU function in the reference) on the GPU."""
    _lib.check(_lib.load().smx_median_filter_and_densify_depth_map(_sv(stream), _d(input_depth), _d(output_depth)))


def DownscaleUsingMedianWhileExcludingCUDA(stream, value_to_ignore, input_depth, output_depth):
    """Image<u16>::DownscaleUsingMedianWhileExcluding (VIS/image.h:1003-1053, the depth half of --pyramid_level)."""
    _lib.check(_lib.load().smx_downscale_using_median_while_excluding(_sv(stream), C.c_uint16(value_to_ignore),
                                                                      _d(input_depth), _d(output_depth)))


def ColorImagePyramidCUDA(stream, pyramid_level, input_color, output_color):
    """ImagePyramid(color_frame, pyramid_level) (VIS/image_cache.h:203-275 over Image<Vec3u8>::DownscaleToHalfSize,
    VIS/image.h:929-948): the colour half of --pyramid_level (APP/main.cc:973-981)."""
    _lib.check(_lib.load().smx_color_image_pyramid(_sv(stream), C.c_int32(pyramid_level), _d(input_color),
                                                   _d(output_color)))


def CopyWithoutBorderCUDA(stream, input_depth, output_depth):
    _lib.check(_lib.load().smx_copy_without_border(_sv(stream), _d(input_depth), _d(output_depth)))


def ComputeNormalsAndDropBadPixelsCUDA(stream, observation_angle_threshold_deg, depth_scaling, depth_fx, depth_fy,
                                       depth_cx, depth_cy, in_depth, out_depth, out_normals):
    _lib.check(_lib.load().smx_compute_normals_and_drop_bad_pixels(
        _sv(stream), C.c_float(observation_angle_threshold_deg), C.c_float(depth_scaling),
        C.c_float(depth_fx), C.c_float(depth_fy), C.c_float(depth_cx), C.c_float(depth_cy),
        _d(in_depth), _d(out_depth), _d(out_normals)))


def ComputePointRadiiAndRemoveIsolatedPixelsCUDA(stream, point_radius_extension_factor, point_radius_clamp_factor,
                                                 depth_scaling, depth_fx, depth_fy, depth_cx, depth_cy,
                                                 depth_buffer, radius_buffer, out_depth):
    _lib.check(_lib.load().smx_compute_point_radii_and_remove_isolated_pixels(
        _sv(stream), C.c_float(point_radius_extension_factor), C.c_float(point_radius_clamp_factor),
        C.c_float(depth_scaling), C.c_float(depth_fx), C.c_float(depth_fy), C.c_float(depth_cx), C.c_float(depth_cy),
        _d(depth_buffer), _d(radius_buffer), _d(out_depth)))


def ErodeNormalsRadiiCUDA(stream, erosion_radius, observation_angle_threshold_deg, point_radius_extension_factor,
                          point_radius_clamp_factor, depth_scaling, depth_fx, depth_fy, depth_cx, depth_cy, in_depth,
                          out_depth, out_normals, radius_buffer):
    """Erosion (radius 0: border copy) + normals + radii as one launch (smx_erode_normals_radii): the final depth, the
    normals and the radii of the three separate calls (APP/main.cc:1128-1191)."""
    _lib.check(_lib.load().smx_erode_normals_radii(
        _sv(stream), C.c_int32(erosion_radius), C.c_float(observation_angle_threshold_deg),
        C.c_float(point_radius_extension_factor), C.c_float(point_radius_clamp_factor), C.c_float(depth_scaling),
        C.c_float(depth_fx), C.c_float(depth_fy), C.c_float(depth_cx), C.c_float(depth_cy), _d(in_depth), _d(out_depth),
        _d(out_normals), _d(radius_buffer)))


def SynthRenderRoom(stream, depth_out, color_out, fx, fy, cx, cy, global_T_frame, seed, frame_index,
                    depth_scaling=5000.0, noise_sigma=0.001, dropout=0.01):
    """Benchmark input generator (smx_synth_render_room): one synthetic room frame into device buffers."""
    T = np.ascontiguousarray(np.asarray(global_T_frame, np.float32).reshape(12))
    _lib.check(_lib.load().smx_synth_render_room(
        _sv(stream), _d(depth_out), _d(color_out), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
        T.ctypes.data_as(C.c_void_p), C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(frame_index),
        C.c_float(depth_scaling), C.c_float(noise_sigma), C.c_float(dropout)))


# ---- GPU -> CPU hand-off types (APP/cuda_surfels_cpu.h) ---------------------------------------
class CUDASurfelBuffersCPU:
    def __init__(self, max_surfel_count):
        n = int(max_surfel_count)
        self.frame_index = 0
        self.surfel_count = 0
        self.surfel_x_buffer = np.empty(n, np.float32)
        self.surfel_y_buffer = np.empty(n, np.float32)
        self.surfel_z_buffer = np.empty(n, np.float32)
        self.surfel_radius_squared_buffer = np.empty(n, np.float32)
        self.surfel_normal_x_buffer = np.empty(n, np.float32)
        self.surfel_normal_y_buffer = np.empty(n, np.float32)
        self.surfel_normal_z_buffer = np.empty(n, np.float32)
        self.surfel_last_update_stamp_buffer = np.empty(n, np.uint32)

    def _pod(self):
        p = SurfelBuffersCPU()
        for name, _ in SurfelBuffersCPU._fields_[2:]:
            setattr(p, name, getattr(self, name).ctypes.data)
        return p


class CUDASurfelDeltaCPU:
    """Changed surfels: slot indices (ascending) and the eight attributes TransferAllToCPU moves, for those slots."""
    ROWS = (("x", np.float32, "surfel_x_buffer"), ("y", np.float32, "surfel_y_buffer"), ("z", np.float32, "surfel_z_buffer"),
            ("radius_squared", np.float32, "surfel_radius_squared_buffer"),
            ("normal_x", np.float32, "surfel_normal_x_buffer"), ("normal_y", np.float32, "surfel_normal_y_buffer"),
            ("normal_z", np.float32, "surfel_normal_z_buffer"),
            ("last_update_stamp", np.uint32, "surfel_last_update_stamp_buffer"))

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.count = 0
        self.frame_index = 0
        self.surfel_count = 0
        self.surfel_index = np.empty(self.capacity, np.uint32)
        for name, dt, _ in self.ROWS:
            setattr(self, name, np.empty(self.capacity, dt))

    def _pod(self):
        from ._lib import SurfelDeltaCPU
        p = SurfelDeltaCPU()
        p.capacity = self.capacity
        p.surfel_index = self.surfel_index.ctypes.data
        for name, _, _ in self.ROWS:
            setattr(p, name, getattr(self, name).ctypes.data)
        return p

    def ApplyTo(self, buffers):
        """Patch a CUDASurfelBuffersCPU (a previous full transfer + all deltas since) to the current state."""
        idx = self.surfel_index[:self.count]
        for name, _, full in self.ROWS:
            getattr(buffers, full)[idx] = getattr(self, name)[:self.count]
        buffers.frame_index = self.frame_index
        buffers.surfel_count = self.surfel_count


class CUDASurfelsCPU:
    """Mutex-guarded write/read double buffer, APP/cuda_surfels_cpu.h:83-124."""

    def __init__(self, max_surfel_count):
        self._write = CUDASurfelBuffersCPU(max_surfel_count)
        self._read = CUDASurfelBuffersCPU(max_surfel_count)
        self._lock = threading.Lock()
        self._debug_wrote_data = False

    def LockWriteBuffers(self):
        self._lock.acquire()

    def UnlockWriteBuffers(self):
        self._debug_wrote_data = True
        self._lock.release()

    def WaitForLockAndSwapBuffers(self):
        with self._lock:
            if not self._debug_wrote_data:
                # LOG(FATAL) in the reference (:109-111)
                raise SmxError("Trying to swap the CUDASurfelsCPU buffers, but no data was written. "
                               "Possible multi-threading bug!")
            self._write, self._read = self._read, self._write
            self._debug_wrote_data = False

    def write_buffers(self):
        return self._write

    def read_buffers(self):
        return self._read


# ---- CUDASurfelReconstruction (APP/cuda_surfel_reconstruction.h) ------------------------------
class PinholeCamera4f:
    """The accessors of VIS/camera.h's PinholeCamera4f that the hot path uses."""

    def __init__(self, width, height, fx, fy, cx, cy):
        self._w, self._h = int(width), int(height)
        self._p = (float(fx), float(fy), float(cx), float(cy))

    def width(self):
        return self._w

    def height(self):
        return self._h

    def parameters(self):
        return self._p

    def Scaled(self, factor):
        """Camera::Scaled (VIS/camera.h:1564-1574): size = factor * size + 0.5 truncated, the four pinhole parameters
        times factor in float (PinholeProjection::ScaleParameters, camera.h:954-964; origin at the image corner)."""
        f = np.float32(factor)
        return PinholeCamera4f(int(factor * self._w + np.float32(0.5)), int(factor * self._h + np.float32(0.5)),
                               *[float(np.float32(v) * f) for v in self._p])


class CUDASurfelReconstruction:
    def __init__(self, max_surfel_count, depth_camera, vertex_buffer_resource=None,
                 neighbor_index_buffer_resource=None, normal_vertex_buffer_resource=None, render_window=None,
                 device_id=-1):
        """device_id (not in the reference's constructor): the GPU the object lives on, -1 = the current device."""
        _lib.require_gpu()
        self.max_surfel_count = int(max_surfel_count)
        self.depth_camera = depth_camera
        fx, fy, cx, cy = depth_camera.parameters()
        self._h = C.c_void_p()
        _lib.check(_lib.load().smx_recon_create(C.c_uint32(self.max_surfel_count), depth_camera.width(),
                                                depth_camera.height(), C.c_float(fx), C.c_float(fy), C.c_float(cx),
                                                C.c_float(cy), C.c_int32(device_id), C.byref(self._h)))
        self._last_stream = None
        self._device_id = int(device_id)

    def Integrate(self, stream, frame_index, depth_scaling, depth_buffer, normals_buffer, radius_buffer, color_buffer,
                  global_T_local, sensor_noise_factor, max_surfel_confidence, regularizer_weight,
                  regularization_frame_window_size, do_blending, measurement_blending_radius,
                  regularization_iterations_per_integration_iteration, radius_factor_for_regularization_neighbors,
                  normal_compatibility_threshold_deg, surfel_integration_active_window_size):
        p = IntegrateParams(sensor_noise_factor, max_surfel_confidence, regularizer_weight,
                            regularization_frame_window_size, 1 if do_blending else 0, measurement_blending_radius,
                            regularization_iterations_per_integration_iteration,
                            radius_factor_for_regularization_neighbors, normal_compatibility_threshold_deg,
                            surfel_integration_active_window_size)
        self.IntegrateP(stream, frame_index, depth_scaling, depth_buffer, normals_buffer, radius_buffer, color_buffer,
                        global_T_local, p)

    def IntegrateP(self, stream, frame_index, depth_scaling, depth_buffer, normals_buffer, radius_buffer,
                   color_buffer, global_T_local, params):
        T = np.ascontiguousarray(np.asarray(global_T_local, np.float32).reshape(12))
        self._last_stream = stream
        _lib.check(_lib.load().smx_recon_integrate(
            self._h, _sv(stream), C.c_uint32(frame_index), C.c_float(depth_scaling), _d(depth_buffer),
            _d(normals_buffer), _d(radius_buffer), _d(color_buffer), T.ctypes.data_as(C.c_void_p), C.byref(params)))

    def Regularize(self, stream, frame_index, regularizer_weight, radius_factor_for_regularization_neighbors,
                   regularization_frame_window_size):
        _lib.check(_lib.load().smx_recon_regularize(self._h, _sv(stream), C.c_uint32(frame_index),
                                                    C.c_float(regularizer_weight),
                                                    C.c_float(radius_factor_for_regularization_neighbors),
                                                    C.c_int32(regularization_frame_window_size)))

    def TransferAllToCPU(self, stream, frame_index, buffers):
        """Requires the caller to hold buffers.LockWriteBuffers() (APP/main.cc:1261-1264)."""
        wb = buffers.write_buffers()
        pod = wb._pod()
        _lib.check(_lib.load().smx_recon_transfer_all_to_cpu(self._h, _sv(stream), C.c_uint32(frame_index),
                                                             C.byref(pod)))
        wb.frame_index = pod.frame_index
        wb.surfel_count = pod.surfel_count

    def SetDeltaTracking(self, stream, enabled):
        """Not in the reference: mark the slots whose transferred attributes change, for
        TransferChangedToCPU.  Enabling marks every existing slot."""
        _lib.check(_lib.load().smx_recon_set_delta_tracking(self._h, _sv(stream), C.c_int32(1 if enabled else 0)))

    def TransferChangedToCPU(self, stream, frame_index, capacity=None, delta=None):
        """The changed-surfel delta since the previous call (synchronous): a CUDASurfelDeltaCPU (pass `delta` to
        reuse one instead of allocating capacity-sized arrays per call)."""
        cap = int(capacity if capacity is not None else self.max_surfel_count)
        d = delta if delta is not None else CUDASurfelDeltaCPU(cap)
        pod = d._pod()
        rc = _lib.load().smx_recon_transfer_changed_to_cpu(self._h, _sv(stream), C.c_uint32(frame_index), C.byref(pod))
        d.count, d.frame_index, d.surfel_count = pod.count, pod.frame_index, pod.surfel_count
        if rc != 0:
            d.count_needed = pod.count
            d.count = 0
            self.last_failed_delta = d
            _lib.check(rc)
        return d

    def Compact(self, stream, return_map=True):
        """Not in the reference: removes the merged slots from the map, keeping the rest in ascending order
        (synchronous; smx_recon_compact).  Returns (old_to_new, new_size, links_dropped): old_to_new (uint32 per old
        slot: its new index, or 0xFFFFFFFF for a removed slot) is None unless return_map.  links_dropped == 0 means the
        continuation is an exact relabelling of the uncompacted run.  A neighbour index built before is stale."""
        old_to_new = None
        if return_map:
            old_to_new = np.empty(self._counts_on(stream)[1], np.uint32)
        new_size, dropped = C.c_uint32(0), C.c_uint32(0)
        ptr = old_to_new.ctypes.data_as(C.c_void_p) if old_to_new is not None and old_to_new.size else None
        cap = old_to_new.size if old_to_new is not None else 0
        _lib.check(_lib.load().smx_recon_compact(self._h, _sv(stream), ptr, C.c_uint32(cap), C.c_int32(0),
                                                 C.byref(new_size), C.byref(dropped)))
        return old_to_new, int(new_size.value), int(dropped.value)

    def MergeMap(self, stream, src, dst_T_src, index=None, return_map=False, **params):
        """Not in the reference: merges the map of `src` (another CUDASurfelReconstruction on the same device, read only) into
        this one under the pose dst_T_src ([3,4], this <- src, e.g. the scene_T_points of a registration): a source surfel
        with a compatible surfel of this map among its k nearest is dropped (mode "keep") or blended into it ("blend"),
        every other one is appended (smx_recon_merge_map; synchronous).  params: the keywords of merge_params, or
        params=<MergeParams>.  index: a SurfelNeighborIndex to build and use (stale afterwards); one is created and closed
        here if None.  Returns the statistics dict, or (dict, src_to_dst [uint32 per slot of src: its slot here, 0xFFFFFFFF
        for dead and BAD slots]) with return_map.  Too little room for the appended slots raises SmxError and leaves the map
        as it was; .last_merge_stats then says how much was needed."""
        pod = params.pop("params", None)
        if pod is None:
            pod = merge_params(**params)
        elif params:
            raise ValueError("either params= or keywords")
        if not isinstance(src, CUDASurfelReconstruction) or src is self:
            raise ValueError("src must be another CUDASurfelReconstruction")
        T = np.ascontiguousarray(np.asarray(dst_T_src, np.float32).reshape(12))
        own = index is None
        nn = SurfelNeighborIndex(self._device_id) if own else index
        try:
            s2d = np.empty(src._counts_on(stream)[1], np.uint32) if return_map else None
            st = _lib.MergeStats()
            rc = _lib.load().smx_recon_merge_map(
                self._h, _sv(stream), nn._h, src._h, T.ctypes.data_as(C.c_void_p), C.byref(pod),
                s2d.ctypes.data_as(C.c_void_p) if s2d is not None and s2d.size else None, C.c_uint32(s2d.size if s2d is not None else 0),
                C.c_int32(0), C.byref(st))
            self.last_merge_stats = merge_stats_dict(st)
            _lib.check(rc)
            return (self.last_merge_stats, s2d) if return_map else self.last_merge_stats
        finally:
            if own:
                nn.close()

    def debug_merge_timings(self):
        """Milliseconds of the last MergeMap into this object by the library's events: {whole, build, move, query_select, number,
        append, blend, finish}."""
        out = (C.c_float * (_lib.MERGE_PHASES + 1))()
        _lib.check(_lib.load().smx_recon_debug_merge_timings(self._h, out, C.c_int32(_lib.MERGE_PHASES + 1)))
        return dict(zip(_lib.MERGE_PHASE_NAMES, (float(v) for v in out)))

    def debug_set_merge_chunk(self, chunk_queries):
        """Tests: MergeMap queries in chunks of this many source slots (0 = the default); results do not depend on it."""
        _lib.check(_lib.load().smx_recon_debug_set_merge_chunk(self._h, C.c_uint32(int(chunk_queries))))

    def ImportPoints(self, stream, points, colors=None, origins=None, index=None, return_map=False, **params):
        """Not in the reference: appends a point cloud to this map as surfels (smx_recon_import_points; synchronous).  points
        [n,3] float32, colors [n] 32-bit words for row 24 (None: default_color), origins [n,3] float32 (the sensor position each
        point was seen from; needed by orient="origins") -- numpy arrays, or device tensors, all on the same side.  Every point
        gets the smallest eigenvector of its k nearest neighbours' covariance as its normal and a neighbour distance as its
        radius; points without enough neighbours, with a degenerate fit or a rough neighbourhood are left out.  params: the
        keywords of import_params, or params=<ImportParams>.  index: a SurfelNeighborIndex to build and use (it indexes the
        cloud afterwards); one is created and closed here if None.  Returns the statistics dict, or (dict, point_to_slot
        [uint32 per point: its slot, 0xFFFFFFFF if it was not imported]) with return_map.  Too little room raises SmxError and
        leaves the map as it was; .last_import_stats then says how much was needed."""
        pod = params.pop("params", None)
        if pod is None:
            pod = import_params(**params)
        elif params:
            raise ValueError("either params= or keywords")
        n, p_addr, on_device, keep_p = _cloud_arg(points, 3, np.float32, "points")
        keep = [keep_p]
        c_addr = o_addr = None
        for a, width, dtype, what in ((colors, 1, np.uint32, "colors"), (origins, 3, np.float32, "origins")):
            if a is None:
                continue
            m, addr, dev, k = _cloud_arg(a, width, dtype, what)
            if m != n or (dev != on_device and n):
                raise ValueError("%s must hold one entry per point, on the same side as points" % what)
            keep.append(k)
            if what == "colors":
                c_addr = addr
            else:
                o_addr = addr
        if pod.orient == _lib.IMPORT_ORIENTS["origins"] and origins is None:
            raise ValueError('orient="origins" needs origins')
        own = index is None
        nn = SurfelNeighborIndex(self._device_id) if own else index
        try:
            p2s = np.empty(n, np.uint32) if return_map else None
            st = _lib.ImportStats()
            rc = _lib.load().smx_recon_import_points(
                self._h, _sv(stream), nn._h, C.c_void_p(p_addr), C.c_void_p(c_addr), C.c_void_p(o_addr), C.c_uint32(n),
                C.c_int32(1 if on_device else 0), C.byref(pod), p2s.ctypes.data_as(C.c_void_p) if p2s is not None and n else None,
                C.c_uint32(n if p2s is not None else 0), C.c_int32(0), C.byref(st))
            self.last_import_stats = import_stats_dict(st)
            _lib.check(rc)
            return (self.last_import_stats, p2s) if return_map else self.last_import_stats
        finally:
            if own:
                nn.close()

    def debug_import_timings(self):
        """Milliseconds of the last ImportPoints into this object by the library's events: {whole, stage, build, query, fit, number,
        write, finish}."""
        out = (C.c_float * (_lib.IMPORT_PHASES + 1))()
        _lib.check(_lib.load().smx_recon_debug_import_timings(self._h, out, C.c_int32(_lib.IMPORT_PHASES + 1)))
        return dict(zip(_lib.IMPORT_PHASE_NAMES, (float(v) for v in out)))

    def DeformByCreationFrame(self, stream, frame_T, reactivate=None, frame_index=0):
        """The loop-closure hook the reference describes but does not ship (README.md:152-176): surfels created at
        frame c move by the rigid correction frame_T[c] ([n_frames, 3, 4] / [n_frames, 12]); reactivate[c] != 0
        re-stamps them with frame_index."""
        T = np.ascontiguousarray(np.asarray(frame_T, np.float32).reshape(-1, 12))
        ra = np.ascontiguousarray(reactivate, np.uint8) if reactivate is not None else None
        if ra is not None and ra.size != T.shape[0]:
            raise ValueError("reactivate needs one byte per frame")
        _lib.check(_lib.load().smx_recon_deform_by_creation_frame(
            self._h, _sv(stream), T.ctypes.data_as(C.c_void_p), C.c_uint32(T.shape[0]),
            ra.ctypes.data_as(C.c_void_p) if ra is not None else C.c_void_p(0), C.c_uint32(frame_index), C.c_int32(0)))

    def CheckTrianglesForRemeshing(self, stream, triangles, long_edge_total_factor_squared):
        """The per-triangle tests of SurfelMeshing::CheckRemeshing (APP/surfel_meshing.cc:590-650) for triangles
        [T,3] of slot indices against the device-resident map.  Returns flags [T] (bits: see smx.h)."""
        tri = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        flags = np.zeros(tri.shape[0], np.uint8)
        _lib.check(_lib.load().smx_recon_check_triangles(
            self._h, _sv(stream), tri.ctypes.data_as(C.c_void_p), C.c_uint32(tri.shape[0]),
            C.c_float(long_edge_total_factor_squared), flags.ctypes.data_as(C.c_void_p), C.c_int32(0)))
        return flags

    def Triangulate(self, stream, params=None, index=None, cell_size=None):
        """Not in the reference: triangulates the map as it stands on the device (smx_recon_triangulate: a localized
        Delaunay triangulation -- every surfel triangulates its neighbours in its tangent plane, a triangle is kept if
        its three corners agree).  params: a MeshParams (MeshParams.defaults()); index: a SurfelNeighborIndex to
        (re)build and use, one is created and closed here if None; cell_size of that index (default: 5 cm, results do
        not depend on it).  Synchronous.  Returns (triangles [T,3] uint32 of slot indices -- p smallest, counter-
        clockwise seen from the normals' side, ascending -- and a dict of smx_mesh_stats)."""
        p = params if params is not None else MeshParams.defaults()
        own = index is None
        nn = SurfelNeighborIndex(self._device_id) if own else index
        cs = C.c_float(0.05 if cell_size is None else cell_size)
        try:
            L = _lib.load()
            T, st = C.c_uint32(0), MeshStats()
            rc = L.smx_recon_triangulate(self._h, _sv(stream), nn._h, cs, C.byref(p), None, C.c_uint32(0), C.c_int32(0),
                                         C.byref(T), C.byref(st))
            if rc != 0 and not (rc == -1 and T.value > 0):   # (SMX_ERR_INVALID_ARGUMENT with the count: the capacity rule)
                _lib.check(rc)
            tri = np.zeros((T.value, 3), np.uint32)
            if T.value:
                _lib.check(L.smx_recon_triangulate(self._h, _sv(stream), nn._h, cs, C.byref(p), tri.ctypes.data_as(C.c_void_p),
                                                   C.c_uint32(T.value), C.c_int32(0), C.byref(T), C.byref(st)))
            return tri, {n: int(getattr(st, n)) for n, _ in MeshStats._fields_}
        finally:
            if own:
                nn.close()

    def TriangulateUpdate(self, stream, params=None, index=None, cell_size=None, full_above_fraction=None):
        """Not in the reference: Triangulate's result, kept up to date (smx_recon_triangulate_update: the object keeps the
        last triangulation, finds the slots that changed since, and recomputes only their stars and the triangles around
        them).  Arguments as Triangulate; full_above_fraction: the share of dirty slots above which the full path runs
        (None: the library's default; it chooses the path, never the result).  Synchronous.  Returns (triangles, stats
        dict, update stats dict: mode, n_changed, n_dirty, n_reagreed, n_kept_triangles) -- the update stats are those
        of the call that did the work, the first of the ask-then-fill pair."""
        p = params if params is not None else MeshParams.defaults()
        own = index is None
        nn = SurfelNeighborIndex(self._device_id) if own else index
        cs = C.c_float(0.05 if cell_size is None else cell_size)
        frac = C.c_float(-1.0 if full_above_fraction is None else full_above_fraction)
        try:
            L = _lib.load()
            T, st, us = C.c_uint32(0), MeshStats(), MeshUpdateStats()
            rc = L.smx_recon_triangulate_update(self._h, _sv(stream), nn._h, cs, C.byref(p), frac, None, C.c_uint32(0),
                                                C.c_int32(0), C.byref(T), C.byref(st), C.byref(us))
            if rc != 0 and not (rc == -1 and T.value > 0):   # (SMX_ERR_INVALID_ARGUMENT with the count: the capacity rule)
                _lib.check(rc)
            tri = np.zeros((T.value, 3), np.uint32)
            if T.value:
                # (the state has advanced: this call finds nothing changed and copies the kept array out)
                _lib.check(L.smx_recon_triangulate_update(self._h, _sv(stream), nn._h, cs, C.byref(p), frac,
                                                          tri.ctypes.data_as(C.c_void_p), C.c_uint32(T.value), C.c_int32(0),
                                                          C.byref(T), C.byref(st), None))
            return (tri, {n: int(getattr(st, n)) for n, _ in MeshStats._fields_},
                    {n: int(getattr(us, n)) for n, _ in MeshUpdateStats._fields_})
        finally:
            if own:
                nn.close()

    def ResetTriangulation(self):
        """Drops the state TriangulateUpdate keeps and frees its memory; the next update runs the full path."""
        _lib.check(_lib.load().smx_recon_triangulate_reset(self._h))

    def debug_mesh_update_timings(self):
        """Milliseconds of the last TriangulateUpdate call, by phase."""
        out = (C.c_float * 6)()
        _lib.check(_lib.load().smx_recon_debug_mesh_update_timings(self._h, out))
        return dict(zip(("diff", "index_builds", "reverse_test", "subset_lists", "stars", "agree_merge"), [float(v) for v in out]))

    def debug_mesh_timings(self):
        """Milliseconds of the last Triangulate call: index build, list query, star kernel, agreement + scan + write."""
        out = (C.c_float * 4)()
        _lib.check(_lib.load().smx_recon_debug_mesh_timings(self._h, out))
        return dict(zip(("index_build", "list_query", "star", "agree_write"), [float(v) for v in out]))

    def DecimateMesh(self, stream, triangles, cell_size, return_vertex_map=False):
        """Not in the reference: a coarser level of detail of `triangles` ([T,3] slot indices, e.g. Triangulate's) by vertex
        clustering (smx_recon_decimate_mesh): the vertices of a cubic cell of edge cell_size collapse onto the one nearest
        to the cell's centre, triangles that lose a corner or repeat an earlier one go.  The result is again a triangle array
        over slot indices in Triangulate's format, so export, colours and a further, coarser call work on it unchanged; it
        is not kept manifold.  Synchronous.  Returns (triangles [T_out,3] uint32, dict of smx_decimate_stats), and with
        return_vertex_map also vertex_map [surfels_size()] uint32 (the representative of every used slot, 0xFFFFFFFF for
        the others)."""
        tri = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        L = _lib.load()
        T, st = C.c_uint32(0), DecimateStats()
        tin = tri.ctypes.data_as(C.c_void_p) if tri.shape[0] else None
        rc = L.smx_recon_decimate_mesh(self._h, _sv(stream), C.c_float(cell_size), tin, C.c_uint32(tri.shape[0]), None,
                                       C.c_uint32(0), None, C.c_int32(0), C.byref(T), C.byref(st))
        if rc != 0 and not (rc == -1 and T.value > 0):   # (SMX_ERR_INVALID_ARGUMENT with the count: the capacity rule)
            _lib.check(rc)
        out = np.zeros((T.value, 3), np.uint32)
        vmap = np.zeros(self._counts_on(stream)[1], np.uint32) if return_vertex_map else None
        if T.value or return_vertex_map:
            _lib.check(L.smx_recon_decimate_mesh(
                self._h, _sv(stream), C.c_float(cell_size), tin, C.c_uint32(tri.shape[0]),
                out.ctypes.data_as(C.c_void_p) if T.value else None, C.c_uint32(T.value),
                vmap.ctypes.data_as(C.c_void_p) if vmap is not None and vmap.size else None, C.c_int32(0), C.byref(T), C.byref(st)))
        stats = {n: int(getattr(st, n)) for n, _ in DecimateStats._fields_}
        return (out, stats, vmap) if return_vertex_map else (out, stats)

    def debug_decimate_timings(self):
        """Milliseconds of the last DecimateMesh call, by phase."""
        out = (C.c_float * DECIMATE_PHASES)()
        _lib.check(_lib.load().smx_recon_debug_decimate_timings(self._h, out, C.c_int32(DECIMATE_PHASES)))
        return dict(zip(("cluster", "remap_dedupe", "survivors", "order"), [float(v) for v in out]))

    def MeshComponents(self, stream, triangles, min_triangles=0, min_diagonal=0.0, keep_largest=0, return_labels=False,
                       return_components=False):
        """Not in the reference: the connected pieces of `triangles` ([T,3] slot indices in any order, e.g. Triangulate's or
        DecimateMesh's) labelled, measured and filtered on the device (smx_recon_mesh_components).  Pieces are connected
        through shared vertices; a piece is kept if it has at least min_triangles triangles and a bounding-box diagonal of
        at least min_diagonal, and with keep_largest = K > 0 only the K largest of those.  The result is the subsequence of
        the input whose piece is kept: same order, same format.  Synchronous.  Returns (triangles [T_out,3] uint32, dict of
        smx_components_stats), then with return_labels vertex_labels [surfels_size()] uint32 (the smallest slot of every
        used slot's piece, 0xFFFFFFFF for the others), then with return_components the table of all pieces, ascending by
        label, as a structured array of COMPONENT_DTYPE."""
        p = components_params(min_triangles, min_diagonal, keep_largest)
        tri = np.ascontiguousarray(triangles, np.uint32)
        if tri.size % 3:
            raise ValueError("triangles must hold three indices per triangle")
        tri = tri.reshape(-1, 3)
        L = _lib.load()
        T, nc, st = C.c_uint32(0), C.c_uint32(0), ComponentsStats()
        tin = tri.ctypes.data_as(C.c_void_p) if tri.shape[0] else None

        def call(out, labels, table):
            return L.smx_recon_mesh_components(
                self._h, _sv(stream), C.byref(p), tin, C.c_uint32(tri.shape[0]),
                out.ctypes.data_as(C.c_void_p) if out is not None and out.size else None,
                C.c_uint32(0 if out is None else out.shape[0]),
                labels.ctypes.data_as(C.c_void_p) if labels is not None and labels.size else None,
                table.ctypes.data_as(C.c_void_p) if table is not None and table.size else None,
                C.c_uint32(0 if table is None else table.shape[0]), C.c_int32(0), C.byref(T), C.byref(nc), C.byref(st))
        rc = call(None, None, None)
        if rc != 0 and not (rc == -1 and T.value > 0):   # (SMX_ERR_INVALID_ARGUMENT with the counts: the capacity rule)
            _lib.check(rc)
        out = np.zeros((T.value, 3), np.uint32)
        labels = np.zeros(self._counts_on(stream)[1], np.uint32) if return_labels else None
        table = np.zeros(nc.value, COMPONENT_DTYPE) if return_components else None
        if T.value or (labels is not None and labels.size) or (table is not None and table.size):
            _lib.check(call(out, labels, table))
        ret = (out, {n: int(getattr(st, n)) for n, _ in ComponentsStats._fields_})
        if return_labels:
            ret += (labels,)
        if return_components:
            ret += (table,)
        return ret

    def debug_components_timings(self):
        """Milliseconds of the last MeshComponents call, by phase."""
        out = (C.c_float * COMPONENTS_PHASES)()
        _lib.check(_lib.load().smx_recon_debug_components_timings(self._h, out, C.c_int32(COMPONENTS_PHASES)))
        return dict(zip(("mark_link", "flatten_number", "measure", "write"), [float(v) for v in out]))

    def FillHoles(self, stream, triangles, max_hole_edges=8, min_triangle_angle_deg=10.0, max_triangle_angle_deg=170.0,
                  return_holes=False):
        """Not in the reference: the small holes of `triangles` ([T,3] slot indices in any order, e.g. Triangulate's or
        MeshComponents') closed on the device (smx_recon_fill_holes).  A hole is a closed loop of 3 .. max_hole_edges
        boundary edges through vertices no other hole touches; it is closed by a fan from the vertex with the shortest
        diagonals, whole or not at all: not if a diagonal of the fan is an edge of the mesh already, and not if a fan
        triangle fails Triangulate's triangle filter with the two angle limits given.  The result is the live triangles of
        the input, in input order, followed by the new ones (each starting at its smallest index, ascending); no vertex is
        made.  Synchronous.  Returns (triangles [T_out,3] uint32, dict of smx_fill_stats plus n_kept = where the new run
        starts), then with return_holes the table of the listed loops, filled or not, ascending by label, as a structured
        array of HOLE_DTYPE."""
        p = fill_params(max_hole_edges, min_triangle_angle_deg, max_triangle_angle_deg)
        tri = np.ascontiguousarray(triangles, np.uint32)
        if tri.size % 3:
            raise ValueError("triangles must hold three indices per triangle")
        tri = tri.reshape(-1, 3)
        L = _lib.load()
        T, kept, nh, st = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), FillStats()
        tin = tri.ctypes.data_as(C.c_void_p) if tri.shape[0] else None

        def call(out, table):
            return L.smx_recon_fill_holes(
                self._h, _sv(stream), C.byref(p), tin, C.c_uint32(tri.shape[0]),
                out.ctypes.data_as(C.c_void_p) if out is not None and out.size else None,
                C.c_uint32(0 if out is None else out.shape[0]),
                table.ctypes.data_as(C.c_void_p) if table is not None and table.size else None,
                C.c_uint32(0 if table is None else table.shape[0]), C.c_int32(0), C.byref(T), C.byref(kept), C.byref(nh), C.byref(st))
        rc = call(None, None)
        if rc != 0 and not (rc == -1 and T.value > 0):   # (SMX_ERR_INVALID_ARGUMENT with the counts: the capacity rule)
            _lib.check(rc)
        out = np.zeros((T.value, 3), np.uint32)
        table = np.zeros(nh.value, HOLE_DTYPE) if return_holes else None
        if T.value or (table is not None and table.size):
            _lib.check(call(out, table))
        stats = {n: int(getattr(st, n)) for n, _ in FillStats._fields_}
        stats["n_kept"] = int(kept.value)
        return (out, stats, table) if return_holes else (out, stats)

    def debug_fill_timings(self):
        """Milliseconds of the last FillHoles call, by phase."""
        out = (C.c_float * FILL_PHASES)()
        _lib.check(_lib.load().smx_recon_debug_fill_timings(self._h, out, C.c_int32(FILL_PHASES)))
        return dict(zip(("edges", "loops", "fill", "write"), [float(v) for v in out]))

    def MeshDistance(self, stream, triangles, points, max_distance, cell_size=0.0, signed=False, return_closest=False):
        """Not in the reference: for every point of `points` ([P,3] float32) the closest point on `triangles` ([T,3] slot
        indices in any order, e.g. Triangulate's, DecimateMesh's, MeshComponents' or FillHoles') over the map's smooth
        positions (smx_recon_mesh_distance).  Only triangles within max_distance count; the answer is exactly the minimum over
        all of them (ties go to the earlier triangle) whatever cell_size the search grid uses (0: the library chooses).
        Synchronous.  Both arrays are numpy arrays, or both are contiguous device tensors (uint32 / int32 and float32); the
        results then are device tensors too (nearest a torch.uint32 tensor).  Returns (nearest [P] uint32 with 0xFFFFFFFF for "none", distance [P] float32
        with +inf for "none" -- negative behind the triangle if signed --, then with return_closest closest [P,3] float32,
        then the dict of smx_distance_stats)."""
        p = distance_params(max_distance, cell_size, signed)
        L = _lib.load()
        st = DistanceStats()
        dev = _device_address(triangles) is not None or _device_address(points) is not None
        if dev:
            import torch
            if _device_address(triangles) is None or _device_address(points) is None:
                raise ValueError("triangles and points must both be device tensors, or both host arrays")
            if not (triangles.is_contiguous() and points.is_contiguous() and triangles.element_size() == 4 and
                    points.dtype == torch.float32 and triangles.numel() % 3 == 0 and points.numel() % 3 == 0):
                raise ValueError("device tensors must be contiguous: [T,3] 32-bit integers and [P,3] float32")
            n_in, n_points = triangles.numel() // 3, points.numel() // 3
            nearest = torch.empty(n_points, dtype=torch.uint32, device=points.device)
            distance = torch.empty(n_points, dtype=torch.float32, device=points.device)
            closest = torch.empty((n_points, 3), dtype=torch.float32, device=points.device) if return_closest else None
            tin, pin = triangles.data_ptr() if n_in else None, points.data_ptr() if n_points else None
            outs = [a.data_ptr() if a is not None and n_points else None for a in (nearest, distance, closest)]
            torch.cuda.current_stream(points.device).synchronize()      # (the tensors' producers; the call runs on `stream`)
        else:
            tri = np.ascontiguousarray(triangles, np.uint32)
            pts = np.ascontiguousarray(points, np.float32)
            if tri.size % 3 or pts.size % 3:
                raise ValueError("triangles and points must hold three values per row")
            n_in, n_points = tri.size // 3, pts.size // 3
            nearest, distance = np.zeros(n_points, np.uint32), np.zeros(n_points, np.float32)
            closest = np.zeros((n_points, 3), np.float32) if return_closest else None
            tin, pin = tri.ctypes.data if n_in else None, pts.ctypes.data if n_points else None
            outs = [a.ctypes.data if a is not None and n_points else None for a in (nearest, distance, closest)]
        _lib.check(L.smx_recon_mesh_distance(self._h, _sv(stream), C.byref(p), C.c_void_p(tin), C.c_uint32(n_in), C.c_void_p(pin),
                                             C.c_uint32(n_points), C.c_void_p(outs[0]), C.c_void_p(outs[1]), C.c_void_p(outs[2]),
                                             C.c_int32(1 if dev else 0), C.byref(st)))
        stats = distance_stats_dict(st)
        stats["max_distance"] = float(p.max_distance)      # (what the histogram's bins are fractions of)
        return (nearest, distance, closest, stats) if return_closest else (nearest, distance, stats)

    def debug_distance_timings(self):
        """Milliseconds of the last MeshDistance call, by phase."""
        out = (C.c_float * DIST_PHASES)()
        _lib.check(_lib.load().smx_recon_debug_distance_timings(self._h, out, C.c_int32(DIST_PHASES)))
        return dict(zip(("mark", "index", "query", "stats"), [float(v) for v in out]))

    def MeshRim(self, stream, triangles):
        """Not in the reference: per triangle of `triangles` ([T,3] slot indices in any order) one byte that says which of its
        corners and edges lie on the boundary of the surface the array shows (smx_recon_mesh_rim).  An edge is a rim edge iff
        exactly one triangle of the array has it, a slot a rim vertex iff it ends one; bit k of the byte stands for region k of
        MeshDistance's closest point (A, B, AB, C, AC, BC), so (rim[t] >> region) & 1 says whether that point lies on the rim.
        Integers only.  Synchronous.  `triangles` is a numpy array or a contiguous device tensor (uint32 / int32); the bytes
        then are a device tensor too.  Returns (rim [T] uint8, the dict of smx_rim_stats)."""
        st = RimStats()
        dev = _device_address(triangles) is not None
        if dev:
            import torch
            if not (triangles.is_contiguous() and triangles.element_size() == 4 and triangles.numel() % 3 == 0):
                raise ValueError("a device tensor must be contiguous: [T,3] 32-bit integers")
            n_in = triangles.numel() // 3
            rim = torch.empty(n_in, dtype=torch.uint8, device=triangles.device)
            tin, out = (triangles.data_ptr(), rim.data_ptr()) if n_in else (None, None)
            torch.cuda.current_stream(triangles.device).synchronize()      # (the tensor's producers; the call runs on `stream`)
        else:
            t = np.ascontiguousarray(triangles, np.uint32)
            if t.size % 3:
                raise ValueError("triangles must hold three values per row")
            n_in = t.size // 3
            rim = np.zeros(n_in, np.uint8)
            tin, out = (t.ctypes.data, rim.ctypes.data) if n_in else (None, None)
        _lib.check(_lib.load().smx_recon_mesh_rim(self._h, _sv(stream), C.c_void_p(tin), C.c_uint32(n_in), C.c_int32(1 if dev else 0),
                                                  C.c_void_p(out), C.byref(st)))
        return rim, {n: int(getattr(st, n)) for n, _ in RimStats._fields_}

    def SampleMesh(self, stream, triangles, n_samples, seed=0, return_bary=False, return_normals=False):
        """Not in the reference: n_samples points on `triangles` ([T,3] slot indices in any order) over the map's smooth
        positions, drawn in proportion to area, one per stratum of the total area, in the order of the triangles
        (smx_recon_sample_mesh).  A pure function of the map, the array, n_samples and seed.  Synchronous.  `triangles` is a
        numpy array or a contiguous device tensor (uint32 / int32); the results then are device tensors too.  Returns (points
        [n,3] float32, tri [n] uint32 with 0xFFFFFFFF for "none", then with return_bary bary [n,2] float32, then with
        return_normals normals [n,3] float32, then the dict of smx_sample_stats)."""
        n, sd = sample_params(n_samples, seed)
        st = SampleStats()
        dev = _device_address(triangles) is not None
        if dev:
            import torch
            if not (triangles.is_contiguous() and triangles.element_size() == 4 and triangles.numel() % 3 == 0):
                raise ValueError("a device tensor must be contiguous: [T,3] 32-bit integers")
            n_in = triangles.numel() // 3
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=triangles.device)      # noqa: E731
            points, tri = new((n, 3), torch.float32), new(n, torch.uint32)
            bary = new((n, 2), torch.float32) if return_bary else None
            normals = new((n, 3), torch.float32) if return_normals else None
            tin = triangles.data_ptr() if n_in else None
            outs = [a.data_ptr() if a is not None and n else None for a in (points, tri, bary, normals)]
            torch.cuda.current_stream(triangles.device).synchronize()      # (the tensor's producers; the call runs on `stream`)
        else:
            t = np.ascontiguousarray(triangles, np.uint32)
            if t.size % 3:
                raise ValueError("triangles must hold three values per row")
            n_in = t.size // 3
            points, tri = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
            bary = np.zeros((n, 2), np.float32) if return_bary else None
            normals = np.zeros((n, 3), np.float32) if return_normals else None
            tin = t.ctypes.data if n_in else None
            outs = [a.ctypes.data if a is not None and n else None for a in (points, tri, bary, normals)]
        _lib.check(_lib.load().smx_recon_sample_mesh(self._h, _sv(stream), C.c_void_p(tin), C.c_uint32(n_in), C.c_uint32(n), C.c_uint32(sd),
                                                     C.c_void_p(outs[0]), C.c_void_p(outs[1]), C.c_void_p(outs[2]), C.c_void_p(outs[3]),
                                                     C.c_int32(1 if dev else 0), C.byref(st)))
        return tuple([points, tri] + ([bary] if return_bary else []) + ([normals] if return_normals else []) + [sample_stats_dict(st)])

    def debug_sample_timings(self):
        """Milliseconds of the last SampleMesh call, by phase."""
        out = (C.c_float * SAMPLE_PHASES)()
        _lib.check(_lib.load().smx_recon_debug_sample_timings(self._h, out, C.c_int32(SAMPLE_PHASES)))
        return dict(zip(("weights", "scan", "draw"), [float(v) for v in out]))

    def CompareMeshes(self, stream, a, b, max_distance, n_samples, seed=0, cell_size=0.0, directions=3):
        """Not in the reference: both one-sided surface distances between the triangle arrays a and b ([T,3] slot indices) over
        the map (smx_recon_compare_meshes): per side n_samples points drawn on one array as SampleMesh draws them, measured
        against the other as MeshDistance measures them, within max_distance.  The samples stay on the device.  Synchronous.
        Both arrays are numpy arrays, or both are contiguous device tensors.  Returns the dict of compare_stats_dict."""
        p = compare_params(max_distance, n_samples, seed, cell_size, directions)
        st = CompareStats()
        dev = _device_address(a) is not None or _device_address(b) is not None
        if dev:
            import torch
            if _device_address(a) is None or _device_address(b) is None:
                raise ValueError("a and b must both be device tensors, or both host arrays")
            if not all(t.is_contiguous() and t.element_size() == 4 and t.numel() % 3 == 0 for t in (a, b)):
                raise ValueError("device tensors must be contiguous: [T,3] 32-bit integers")
            n_a, n_b = a.numel() // 3, b.numel() // 3
            pa, pb = a.data_ptr() if n_a else None, b.data_ptr() if n_b else None
            torch.cuda.current_stream(a.device).synchronize()
        else:
            ta, tb = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
            if ta.size % 3 or tb.size % 3:
                raise ValueError("a and b must hold three values per row")
            n_a, n_b = ta.size // 3, tb.size // 3
            pa, pb = ta.ctypes.data if n_a else None, tb.ctypes.data if n_b else None
        _lib.check(_lib.load().smx_recon_compare_meshes(self._h, _sv(stream), C.byref(p), C.c_void_p(pa), C.c_uint32(n_a), C.c_void_p(pb),
                                                        C.c_uint32(n_b), C.c_int32(1 if dev else 0), C.byref(st)))
        return compare_stats_dict(st, p.max_distance)

    def debug_compare_timings(self):
        """Milliseconds of the last CompareMeshes call, by phase and side."""
        out = (C.c_float * COMPARE_PHASES)()
        _lib.check(_lib.load().smx_recon_debug_compare_timings(self._h, out, C.c_int32(COMPARE_PHASES)))
        names = ("a_to_b.sample", "a_to_b.distance", "a_to_b.sums", "b_to_a.sample", "b_to_a.distance", "b_to_a.sums")
        return dict(zip(names, [float(v) for v in out]))

    def RaycastMesh(self, stream, triangles, rays, t_min=0.0, t_max=RAY_MAX_T, cell_size=0.0, cull=0, return_uv=False):
        """Not in the reference: for every ray of `rays` ([P,6] float32: origin, then direction, not normalised) the first
        triangle of `triangles` ([T,3] slot indices in any order, e.g. Triangulate's, DecimateMesh's, MeshComponents' or
        FillHoles') over the map's smooth positions it hits with t_min <= t <= t_max (smx_recon_raycast_mesh).  The answer is
        exactly the minimum over all triangles (ties go to the earlier triangle) whatever cell_size the search grid uses (0:
        the library chooses); cull 1 keeps front faces only, 2 back faces only.  Synchronous.  Both arrays are numpy arrays,
        or both are contiguous device tensors (uint32 / int32 and float32); the results then are device tensors too (hit a
        torch.uint32 tensor).  Returns (hit [P] uint32 with 0xFFFFFFFF for "none", t [P] float32 with +inf for "none", then
        with return_uv uv [P,2] float32, then the dict of smx_raycast_stats)."""
        p = raycast_params(t_min, t_max, cell_size, cull)
        L = _lib.load()
        st = RaycastStats()
        dev = _device_address(triangles) is not None or _device_address(rays) is not None
        if dev:
            import torch
            if _device_address(triangles) is None or _device_address(rays) is None:
                raise ValueError("triangles and rays must both be device tensors, or both host arrays")
            if not (triangles.is_contiguous() and rays.is_contiguous() and triangles.element_size() == 4 and
                    rays.dtype == torch.float32 and triangles.numel() % 3 == 0 and rays.numel() % 6 == 0):
                raise ValueError("device tensors must be contiguous: [T,3] 32-bit integers and [P,6] float32")
            n_in, n_rays = triangles.numel() // 3, rays.numel() // 6
            hit = torch.empty(n_rays, dtype=torch.uint32, device=rays.device)
            t = torch.empty(n_rays, dtype=torch.float32, device=rays.device)
            uv = torch.empty((n_rays, 2), dtype=torch.float32, device=rays.device) if return_uv else None
            tin, rin = triangles.data_ptr() if n_in else None, rays.data_ptr() if n_rays else None
            outs = [a.data_ptr() if a is not None and n_rays else None for a in (hit, t, uv)]
            torch.cuda.current_stream(rays.device).synchronize()      # (the tensors' producers; the call runs on `stream`)
        else:
            tri = np.ascontiguousarray(triangles, np.uint32)
            ry = np.ascontiguousarray(rays, np.float32)
            if tri.size % 3 or ry.size % 6:
                raise ValueError("triangles must hold three values per row and rays six")
            n_in, n_rays = tri.size // 3, ry.size // 6
            hit, t = np.zeros(n_rays, np.uint32), np.zeros(n_rays, np.float32)
            uv = np.zeros((n_rays, 2), np.float32) if return_uv else None
            tin, rin = tri.ctypes.data if n_in else None, ry.ctypes.data if n_rays else None
            outs = [a.ctypes.data if a is not None and n_rays else None for a in (hit, t, uv)]
        _lib.check(L.smx_recon_raycast_mesh(self._h, _sv(stream), C.byref(p), C.c_void_p(tin), C.c_uint32(n_in), C.c_void_p(rin),
                                            C.c_uint32(n_rays), C.c_void_p(outs[0]), C.c_void_p(outs[1]), C.c_void_p(outs[2]),
                                            C.c_int32(1 if dev else 0), C.byref(st)))
        stats = raycast_stats_dict(st)
        return (hit, t, uv, stats) if return_uv else (hit, t, stats)

    def BuildRayScene(self, stream, triangles, cell_size=0.0, occupancy=0, scene=None):
        """Not in the reference: a RayScene of `triangles` ([T,3] slot indices, a numpy array or a contiguous 32-bit device
        tensor) over the map as it stands (smx_recon_build_rayscene).  cell_size as in RaycastMesh; occupancy -1: no occupancy
        bit grid, 0: the library chooses, 1 + k: a bit per block of 2^k cells per axis.  Synchronous.  scene: an existing
        RayScene to rebuild in place.  A refused build leaves the scene empty (and closes a scene made here)."""
        p = rayscene_params(cell_size, occupancy)
        dev = _device_address(triangles) is not None
        if dev:
            if not (triangles.is_contiguous() and triangles.element_size() == 4 and triangles.numel() % 3 == 0):
                raise ValueError("a device tensor of triangles must be contiguous [T,3] 32-bit integers")
            n_in = triangles.numel() // 3
            tin = triangles.data_ptr() if n_in else None
            import torch
            torch.cuda.current_stream(triangles.device).synchronize()      # (the tensor's producers; the call runs on `stream`)
        else:
            tri = np.ascontiguousarray(triangles, np.uint32)
            if tri.size % 3:
                raise ValueError("triangles must hold three values per row")
            n_in = tri.size // 3
            tin = tri.ctypes.data if n_in else None
        own = scene is None
        sc = RayScene() if own else scene
        st = RaySceneStats()
        try:
            _lib.check(_lib.load().smx_recon_build_rayscene(self._h, _sv(stream), sc._h, C.byref(p), C.c_void_p(tin), C.c_uint32(n_in),
                                                            C.c_int32(1 if dev else 0), C.byref(st)))
        except Exception:
            sc.stats = None
            if own:
                sc.close()
            raise
        sc.stats = rayscene_stats_dict(st)
        return sc

    def BuildDistanceScene(self, stream, triangles, max_distance, cell_size=0.0, scene=None, rim=False):
        """Not in the reference: a DistanceScene of `triangles` ([T,3] slot indices, a numpy array or a contiguous 32-bit device
        tensor) over the map as it stands (smx_recon_build_distscene).  max_distance is the bound on what a query may ask for;
        cell_size as in MeshDistance.  Synchronous.  scene: an existing DistanceScene to rebuild in place.  A refused build
        leaves the scene empty (and closes a scene made here).  rim=True also keeps MeshRim's bytes of the array with the scene
        (smx_recon_build_distscene_rim): .has_rim, .rim_stats; Register(robust=...) can then reject matches on the rim."""
        p = distscene_params(max_distance, cell_size)
        n_in, tin, dev, _keep = _triangles_arg(triangles)
        own = scene is None
        sc = DistanceScene() if own else scene
        st, rst = DistSceneStats(), RimStats()
        sc.has_rim, sc.rim_stats = False, None
        try:
            if rim:
                _lib.check(_lib.load().smx_recon_build_distscene_rim(self._h, _sv(stream), sc._h, C.byref(p), C.c_void_p(tin), C.c_uint32(n_in),
                                                                     C.c_int32(1 if dev else 0), C.byref(st), C.byref(rst)))
            else:
                _lib.check(_lib.load().smx_recon_build_distscene(self._h, _sv(stream), sc._h, C.byref(p), C.c_void_p(tin), C.c_uint32(n_in),
                                                                 C.c_int32(1 if dev else 0), C.byref(st)))
        except Exception:
            sc.stats = None
            if own:
                sc.close()
            raise
        sc.stats = distscene_stats_dict(st)
        if rim:
            sc.has_rim, sc.rim_stats = True, {n: int(getattr(rst, n)) for n, _ in RimStats._fields_}
        return sc

    def RegisterMesh(self, stream, scene, triangles, n_samples, seed=0, T_init=None, params=None, robust=None):
        """Not in the reference: mesh to mesh in one call (smx_recon_register_mesh): n_samples points with their normals drawn
        on `triangles` over this object's map as SampleMesh draws them, registered to `scene` as DistanceScene.Register does
        with robust (None: no weights, no rim rejection).  The samples never leave the device.  Synchronous.  Returns
        Register's dict."""
        if not getattr(scene, "_h", None):
            raise ValueError("the scene is closed")
        if not getattr(scene, "stats", None):
            raise ValueError("the scene holds no build")
        n, sd = sample_params(n_samples, seed)
        p = params if params is not None else RegisterParams.defaults()
        register_check_params(p, scene.stats["max_distance"])
        rp = robust if robust is not None else register_robust_params()
        if not isinstance(rp, RegisterRobustParams):
            raise ValueError("robust must be a RegisterRobustParams (register_robust_params(...))")
        if rp.reject_rim and not scene.has_rim:
            raise ValueError("reject_rim needs a scene built with rim=True")
        T = np.ascontiguousarray(np.asarray(np.eye(3, 4) if T_init is None else T_init, np.float32).reshape(-1))
        if T.size != 12 or not np.all(np.isfinite(T)):
            raise ValueError("T_init must hold 12 finite values")
        n_in, tin, dev, _keep = _triangles_arg(triangles)
        res = RegisterResult()
        _lib.check(_lib.load().smx_recon_register_mesh(self._h, _sv(stream), scene._h, C.c_void_p(tin), C.c_uint32(n_in), C.c_int32(1 if dev else 0),
                                                       C.c_uint32(n), C.c_uint32(sd), C.byref(p), C.byref(rp), T.ctypes.data_as(C.c_void_p),
                                                       C.byref(res), C.c_int32(0)))
        return register_result_dict(res)

    def CompareToDistanceScene(self, stream, triangles, scene, max_distance, n_samples, seed=0):
        """Not in the reference: n_samples points drawn on `triangles` over the map as it stands as SampleMesh draws them,
        measured against `scene` as DistanceScene.Query measures them, unsigned, within max_distance (at most the scene's bound)
        (smx_recon_compare_to_distscene).  While the map is unchanged since the scene's build this is the a_to_b side of
        CompareMeshes(triangles, the scene's triangles, directions=1, cell_size=the scene's cell_size_used).  The samples stay
        on the device.  Synchronous.  Returns one side of compare_stats_dict."""
        d = distance_params(max_distance)
        n, sd = sample_params(n_samples, seed)
        distscene_check_query(scene, d.max_distance)
        n_in, tin, dev, _keep = _triangles_arg(triangles)
        side = CompareSide()
        _lib.check(_lib.load().smx_recon_compare_to_distscene(self._h, _sv(stream), scene._h, C.c_float(d.max_distance), C.c_uint32(n), C.c_uint32(sd),
                                                              C.c_void_p(tin), C.c_uint32(n_in), C.c_int32(1 if dev else 0), C.byref(side)))
        return compare_side_dict(side, d.max_distance)

    def debug_raycast_timings(self):
        """Milliseconds of the last RaycastMesh call, by phase."""
        out = (C.c_float * RAY_PHASES)()
        _lib.check(_lib.load().smx_recon_debug_raycast_timings(self._h, out, C.c_int32(RAY_PHASES)))
        return dict(zip(("mark", "index", "cast", "stats"), [float(v) for v in out]))

    def UpdateVisualizationBuffers(self, stream, frame_index, latest_triangulated_frame_index, latest_mesh_surfel_count,
                                   surfel_integration_active_window_size, visualize_last_update_timestamp=False,
                                   visualize_creation_timestamp=False, visualize_radii=False, visualize_normals=False,
                                   vertex_buffer=None, neighbor_index_buffer=None, normal_vertex_buffer=None):
        """The reference fills its viewer's GL buffers (.cc:361-403); here the caller passes the device buffers it wants
        filled (smx_recon_update_visualization_buffers): vertex_buffer 16 B per slot (Point3fC3u8), neighbor_index_buffer
        32 B, normal_vertex_buffer 24 B; see _slots_of for what a buffer may be.  With none given it does nothing."""
        if vertex_buffer is None and neighbor_index_buffer is None and normal_vertex_buffer is None:
            return
        vp, vc = _slots_of(vertex_buffer, 16)
        ip, ic = _slots_of(neighbor_index_buffer, 32)
        npt, nc = _slots_of(normal_vertex_buffer, 24)
        flags = vis_flags(visualize_last_update_timestamp, visualize_creation_timestamp, visualize_radii,
                          visualize_normals)
        _lib.check(_lib.load().smx_recon_update_visualization_buffers(
            self._h, _sv(stream), C.c_uint32(int(frame_index) & 0xFFFFFFFF),
            C.c_uint32(int(latest_triangulated_frame_index) & 0xFFFFFFFF),
            C.c_uint32(int(latest_mesh_surfel_count) & 0xFFFFFFFF), C.c_int32(surfel_integration_active_window_size),
            C.c_int32(flags), vp, C.c_uint32(vc), ip, C.c_uint32(ic), npt, C.c_uint32(nc)))

    def Render(self, stream, params, depth=None, index=None, normal=None, color=None):
        """Not in the reference: splat rendering of the map (smx_recon_render) into height x width device images --
        depth float, index uint32, normal float4, color uchar4 (CUDABuffer or BufferDesc; None = not wanted).
        params: an smx_render_params (make_render_params).  Enqueued on `stream`, no host synchronisation."""
        def opt(b):
            return _d(b) if b is not None else None
        _lib.check(_lib.load().smx_recon_render(self._h, _sv(stream), C.byref(params) if params is not None else None,
                                                opt(depth), opt(index), opt(normal), opt(color)))

    def RenderMesh(self, stream, params, triangles, depth=None, index=None, normal=None, color=None, return_stats=False):
        """Not in the reference: rasterises a triangle array over the map (smx_recon_render_mesh) into height x width device
        images -- depth float, index uint32 (the triangle's position in the array), normal float4, color uchar4 (CUDABuffer
        or BufferDesc; None = not wanted).  triangles: [T,3] slot indices as a numpy array (staged), or a (device address,
        count) pair.  params: an smx_mesh_render_params (make_mesh_render_params).  Enqueued on `stream`; with a device
        array and without return_stats nothing waits on the host.  return_stats: synchronises and returns the dict of
        smx_mesh_render_stats."""
        def opt(b):
            return _d(b) if b is not None else None
        if isinstance(triangles, tuple):
            ptr, count, on_device = C.c_void_p(int(triangles[0])) if triangles[1] else None, int(triangles[1]), 1
        else:
            tri = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
            ptr, count, on_device = tri.ctypes.data_as(C.c_void_p) if tri.shape[0] else None, tri.shape[0], 0
        st = MeshRenderStats() if return_stats else None
        _lib.check(_lib.load().smx_recon_render_mesh(self._h, _sv(stream), C.byref(params) if params is not None else None, ptr,
                                                     C.c_uint32(count), C.c_int32(on_device), opt(depth), opt(index), opt(normal),
                                                     opt(color), C.byref(st) if return_stats else None))
        return {n: int(getattr(st, n)) for n, _ in MeshRenderStats._fields_} if return_stats else None

    def debug_mesh_render_timings(self):
        """Milliseconds of the last RenderMesh call: k_mrast_small (with the clears), k_mrast_large, k_mrast_resolve."""
        out = (C.c_float * 3)()
        _lib.check(_lib.load().smx_recon_debug_mesh_render_timings(self._h, out))
        return dict(zip(("small", "large", "resolve"), [float(v) for v in out]))

    def _track(self, fn, stream, depth_scaling, images, global_T_pred, params, result, model_images):
        """smx_recon_track / smx_recon_track_rgbd (fn): the frame's `images`, then pose, params and result, then the
        optional model images.  result: a ctypes struct to fill (synchronous) or a CUDABuffer / device pointer."""
        T = np.ascontiguousarray(np.asarray(global_T_pred, np.float32).reshape(12))
        on_device = not isinstance(result, C.Structure)
        if on_device:
            result = C.c_void_p(result.ToCUDA().address if isinstance(result, CUDABuffer) else int(result))
        _lib.check(fn(self._h, _sv(stream), C.c_float(depth_scaling), *[_d(b) for b in images], T.ctypes.data_as(C.c_void_p),
                      C.byref(params), result if on_device else C.byref(result), C.c_int32(on_device),
                      *[_d(b) if b is not None else None for b in model_images]))
        return result

    def Track(self, stream, depth_scaling, depth_buffer, normals_buffer, global_T_pred, params=None, model_depth=None,
              model_normal=None):
        """Not in the reference: frame-to-model ICP of a preprocessed frame (depth u16, normals float2, as Integrate
        takes them) against the map rendered at the predicted pose (smx_recon_track).  params: a TrackParams
        (TrackParams.defaults()).  model_depth / model_normal (float / float4 CUDABuffer, optional) receive the model
        images.  Synchronous; returns a TrackOutcome.  Changes no map state."""
        return TrackOutcome(self._track(_lib.load().smx_recon_track, stream, depth_scaling, (depth_buffer, normals_buffer),
                                        global_T_pred, params if params is not None else TrackParams.defaults(),
                                        TrackResult(), (model_depth, model_normal)))

    def TrackAsync(self, stream, depth_scaling, depth_buffer, normals_buffer, global_T_pred, params, result_buffer,
                   model_depth=None, model_normal=None):
        """The same call with the smx_track_result left in device memory (result_buffer: a CUDABuffer of at least
        ctypes.sizeof(TrackResult) bytes in one row, or a device pointer): nothing waits for the host."""
        self._track(_lib.load().smx_recon_track, stream, depth_scaling, (depth_buffer, normals_buffer), global_T_pred, params,
                    result_buffer, (model_depth, model_normal))

    def TrackRGBD(self, stream, depth_scaling, depth_buffer, normals_buffer, color_buffer, global_T_pred, params=None,
                  model_depth=None, model_normal=None, model_photo=None):
        """Track with a photometric term (smx_recon_track_rgbd): color_buffer is the frame's uchar3 colour image as
        Integrate takes it, params a TrackRGBDParams (TrackRGBDParams.defaults()), model_photo (float4 CUDABuffer,
        optional) receives P = (L, gx, gy, valid).  Synchronous; returns a TrackRGBDOutcome.  Changes no map state."""
        return TrackRGBDOutcome(self._track(_lib.load().smx_recon_track_rgbd, stream, depth_scaling,
                                            (depth_buffer, normals_buffer, color_buffer), global_T_pred,
                                            params if params is not None else TrackRGBDParams.defaults(), TrackRGBDResult(),
                                            (model_depth, model_normal, model_photo)))

    def TrackRGBDAsync(self, stream, depth_scaling, depth_buffer, normals_buffer, color_buffer, global_T_pred, params,
                       result_buffer, model_depth=None, model_normal=None, model_photo=None):
        """The same call with the smx_track_rgbd_result left in device memory (result_buffer: a CUDABuffer of at least
        ctypes.sizeof(TrackRGBDResult) bytes in one row, or a device pointer): nothing waits for the host."""
        self._track(_lib.load().smx_recon_track_rgbd, stream, depth_scaling, (depth_buffer, normals_buffer, color_buffer),
                    global_T_pred, params, result_buffer, (model_depth, model_normal, model_photo))

    def _track_iterations(self, fn, record_type, stream):
        recs = (record_type * 96)()
        n = C.c_int32(0)
        _lib.check(fn(self._h, _sv(stream), recs, C.c_int32(96), C.byref(n)))
        return [{"level": r.level, "stride": r.stride, "status": r.status, "sums": np.array(r.sums, np.float64),
                 "x": np.array(r.x, np.float64)} for r in recs[:n.value]]

    def debug_track_iterations(self, stream=None):
        """One dict per iteration of the last Track call (smx_recon_debug_track_iterations): level, stride, status,
        sums (31 float64: JtJ upper triangle, Jtr, sum r^2, inliers, pixels with depth, associated), x (6)."""
        return self._track_iterations(_lib.load().smx_recon_debug_track_iterations, TrackIteration, stream)

    def debug_track_rgbd_iterations(self, stream=None):
        """One dict per iteration of the last TrackRGBD call (smx_recon_debug_track_rgbd_iterations): as
        debug_track_iterations with 33 sums ([31] sum e^2, [32] photometric inliers)."""
        return self._track_iterations(_lib.load().smx_recon_debug_track_rgbd_iterations, TrackRGBDIteration, stream)

    def ExportVertices(self, stream, position_buffer, color_buffer):
        _lib.check(_lib.load().smx_recon_export_vertices(self._h, _sv(stream), _d(position_buffer), _d(color_buffer)))

    def GetTimings(self):
        """(data_association, surfel_merging, measurement_blending, integration, neighbor_update,
        new_surfel_creation, regularization) in ms."""
        out = (C.c_float * 7)()
        _lib.check(_lib.load().smx_recon_get_timings(self._h, out))
        return tuple(out)

    def debug_stamp_ring(self):
        """(records [8][16] uint64, wall clock kHz): smx_recon_debug_stamp_ring."""
        out = np.zeros((8, 16), np.uint64)
        khz = C.c_int32(0)
        _lib.check(_lib.load().smx_recon_debug_stamp_ring(self._h, out.ctypes.data_as(C.c_void_p), C.c_int32(out.size), C.byref(khz)))
        return out, int(khz.value)

    def GetTimingsNoWait(self):
        """(the seven stage times in ms, call number) of the newest Integrate call that is known to be through, without
        waiting for the last one (smx_recon_get_timings_nowait); call number 0 = none yet."""
        out = (C.c_float * 7)()
        call = C.c_uint64(0)
        _lib.check(_lib.load().smx_recon_get_timings_nowait(self._h, out, C.byref(call)))
        return tuple(out), int(call.value)

    def _counts(self):
        return self._counts_on(self._last_stream)

    def _counts_on(self, stream):
        a, b = C.c_uint32(), C.c_uint32()
        _lib.check(_lib.load().smx_recon_counts(self._h, _sv(stream), C.byref(a), C.byref(b)))
        return a.value, b.value

    def surfel_count(self):
        return self._counts()[0]

    def surfels_size(self):
        return self._counts()[1]

    # -- extras (not in the reference interface)
    def stats(self):
        s = ReconStats()
        _lib.check(_lib.load().smx_recon_get_stats(self._h, _sv(self._last_stream), C.byref(s)))
        return {n: int(getattr(s, n)) for n, _ in ReconStats._fields_}

    def set_timing_enabled(self, enabled):
        """False/0 = off, True/1 = the reference's stage events, 3 = stage events + per-kernel events."""
        _lib.check(_lib.load().smx_recon_set_timing_enabled(self._h, C.c_int32(int(enabled))))

    @staticmethod
    def kernel_time_names():
        L = _lib.load()
        return [L.smx_recon_kernel_slot_name(i).decode() for i in range(L.smx_recon_kernel_slot_count())]

    def kernel_times_ms(self):
        n = _lib.load().smx_recon_kernel_slot_count()
        out = (C.c_float * n)()
        _lib.check(_lib.load().smx_recon_get_kernel_timings(self._h, out, C.c_int32(n)))
        return list(out)

    def profile_begin(self, kernel_name, max_frames):
        _lib.check(_lib.load().smx_recon_profile_begin(self._h, C.c_int32(self.kernel_time_names().index(kernel_name)),
                                                       C.c_int32(max_frames)))

    def profile_end(self):
        ms, n = C.c_float(), C.c_int32()
        _lib.check(_lib.load().smx_recon_profile_end(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_stats_enabled(self, enabled):
        _lib.check(_lib.load().smx_recon_set_stats_enabled(self._h, C.c_int32(1 if enabled else 0)))

    def set_scan_mode(self, mode):
        _lib.check(_lib.load().smx_recon_set_scan_mode(self._h, C.c_int32(mode)))

    def set_handover_mode(self, mode):
        """smx_recon_set_handover_mode: 1 = device word + gate kernel (default), 0 = event"""
        _lib.check(_lib.load().smx_recon_set_handover_mode(self._h, C.c_int32(int(mode))))

    def handover_mode(self):
        m = C.c_int32(-1)
        _lib.check(_lib.load().smx_recon_get_handover_mode(self._h, C.byref(m)))
        return int(m.value)

    def set_internal_cu_mask(self, mask_words):
        """experiment (smx_recon_set_internal_cu_mask): the internal stream on the compute units of the mask (empty = all)"""
        arr = (C.c_uint32 * max(1, len(mask_words)))(*mask_words)
        _lib.check(_lib.load().smx_recon_set_internal_cu_mask(self._h, arr, C.c_uint32(len(mask_words))))

    def debug_set_skip(self, mask):
        """TIMING ONLY (smx_recon_debug_set_skip): bit 0 = no regulariser, bit 1 = front of the frame only."""
        _lib.check(_lib.load().smx_recon_debug_set_skip(self._h, C.c_int32(mask)))

    def set_overlap(self, enabled):
        """Frame pipelining on/off (regulariser of frame f beside the first kernels of frame f+1)."""
        _lib.check(_lib.load().smx_recon_set_overlap(self._h, C.c_int32(1 if enabled else 0)))

    def debug_download_surfels(self, count=None):
        n = self.surfels_size() if count is None else int(count)
        rows = np.zeros((kSurfelAttributeCount, n), np.float32)
        _lib.check(_lib.load().smx_recon_debug_download_surfels(self._h, _sv(self._last_stream),
                                                                rows.ctypes.data_as(C.c_void_p), C.c_uint32(n)))
        return rows

    def debug_upload_surfels(self, rows, merge_count=0):
        rows = np.ascontiguousarray(rows, np.float32)
        assert rows.ndim == 2 and rows.shape[0] == kSurfelAttributeCount
        _lib.check(_lib.load().smx_recon_debug_upload_surfels(self._h, _sv(self._last_stream),
                                                              rows.ctypes.data_as(C.c_void_p),
                                                              C.c_uint32(rows.shape[1]), C.c_uint32(merge_count)))

    _SCRATCH = {"supporting": (0, np.uint32), "support_counts": (1, np.uint32), "depth_sums_q": (2, np.int64),
                "conflicting": (3, np.uint32), "first_depth": (4, np.float32), "new_flags": (5, np.uint8),
                "new_indices": (6, np.uint32)}

    def debug_count_skipped_segments(self):
        out = C.c_uint32(0)
        _lib.check(_lib.load().smx_recon_debug_count_skipped_segments(self._h, _sv(self._last_stream), C.byref(out)))
        return int(out.value)

    def debug_download_scratch(self, name):
        which, dt = self._SCRATCH[name]
        out = np.empty((self.depth_camera.height(), self.depth_camera.width()), dt)
        _lib.check(_lib.load().smx_recon_debug_download_scratch(self._h, _sv(self._last_stream), C.c_int32(which),
                                                                out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().smx_recon_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- radius-neighbor search -------------------------------------------------------------------
class SurfelNeighborIndex:
    """Batched replacement of CompressedOctree::FindNearestSurfelsWithinRadius (APP/octree.h:470-477):
    uniform-grid index rebuilt from the surfel position rows, queried for many positions at once."""

    def __init__(self, device_id=-1):
        _lib.require_gpu()
        self._h = C.c_void_p()
        _lib.check(_lib.load().smx_nn_create(C.c_int32(device_id), C.byref(self._h)))

    def Build(self, x, y, z, cell_size, stream=None):
        x, y, z = (np.ascontiguousarray(a, np.float32) for a in (x, y, z))
        self._keep = (x, y, z)
        _lib.check(_lib.load().smx_nn_build(self._h, _sv(stream), x.ctypes.data_as(C.c_void_p),
                                            y.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                                            C.c_uint32(x.size), C.c_float(cell_size), C.c_int32(0)))

    def FindNearestSurfelsWithinRadius(self, positions, radius_squared, max_result_count, state=None, skip_mask=0,
                                       stream=None):
        """positions [nq,3]; radius_squared scalar or [nq].  Returns (counts [nq], dist2 [nq,K], indices [nq,K])."""
        q = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        nq = q.shape[0]
        qx, qy, qz = (np.ascontiguousarray(q[:, i]) for i in range(3))
        r2 = np.ascontiguousarray(np.broadcast_to(np.asarray(radius_squared, np.float32), (nq,)))
        k = int(max_result_count)
        idx = np.zeros((nq, k), np.uint32)
        d2 = np.zeros((nq, k), np.float32)
        cnt = np.zeros(nq, np.int32)
        st = np.ascontiguousarray(state, np.uint8) if state is not None else None
        _lib.check(_lib.load().smx_nn_query_batch(
            self._h, _sv(stream), C.c_uint32(nq), qx.ctypes.data_as(C.c_void_p), qy.ctypes.data_as(C.c_void_p),
            qz.ctypes.data_as(C.c_void_p), r2.ctypes.data_as(C.c_void_p), C.c_int32(k),
            st.ctypes.data_as(C.c_void_p) if st is not None else C.c_void_p(0), C.c_uint8(skip_mask), C.c_int32(0),
            idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
            C.c_int32(0)))
        return cnt, d2, idx

    def BuildFromReconstruction(self, reconstruction, cell_size, stream=None):
        """Index over the smooth positions of all slots of the device-resident map, merged slots left out; no host
        round trip.  A snapshot: rebuild after Integrate / Regularize."""
        self._keep = None
        _lib.check(_lib.load().smx_recon_build_neighbor_index(reconstruction._h, _sv(stream), self._h,
                                                              C.c_float(cell_size)))

    def FindNeighborCandidates(self, reconstruction, surfel_indices, radius_factor_squared, max_result_count,
                               state=None, skip_mask=0, stream=None):
        """Candidate lists of SurfelMeshing::TriangulateSurfel (APP/surfel_meshing.cc:417-425) for a batch of slots:
        ball = radius_factor_squared * radius_squared of the slot around its smooth position, read on the device.
        Returns (counts [n], dist2 [n,K], indices [n,K])."""
        sl = np.ascontiguousarray(surfel_indices, np.uint32).reshape(-1)
        n, k = sl.size, int(max_result_count)
        idx = np.zeros((n, k), np.uint32)
        d2 = np.zeros((n, k), np.float32)
        cnt = np.zeros(n, np.int32)
        st = np.ascontiguousarray(state, np.uint8) if state is not None else None
        _lib.check(_lib.load().smx_recon_neighbor_candidates(
            reconstruction._h, _sv(stream), self._h, sl.ctypes.data_as(C.c_void_p), C.c_uint32(n),
            C.c_float(radius_factor_squared), C.c_int32(k),
            st.ctypes.data_as(C.c_void_p) if st is not None else C.c_void_p(0), C.c_uint8(skip_mask), C.c_int32(0),
            idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
            C.c_int32(0)))
        return cnt, d2, idx

    def FindNearestOfIndexedPoints(self, n_points, max_result_count, radius_squared=None, factor=1.0, state=None,
                                   skip_mask=0, stream=None):
        """Every indexed point queries its own neighbourhood (smx_nn_query_self): r^2 = factor * radius_squared[i], or
        r^2 = factor for all if radius_squared is None.  n_points (optional check) = the number of points given to Build.  Returns
        (counts [n], dist2 [n,K], indices [n,K]); device staging is allocated here (the C entry point takes device
        pointers only)."""
        n, k = int(self.stats()["n_points"]), int(max_result_count)   # (the C entry point writes one row per point of the BUILD)
        if n_points is not None and int(n_points) != n:
            raise ValueError("n_points = %d, but the index was built over %d points" % (int(n_points), n))
        didx, dd2, dcnt = CUDABuffer(1, n * k, np.uint32), CUDABuffer(1, n * k, np.float32), CUDABuffer(1, n, np.int32)
        dr2 = dst = None
        if radius_squared is not None:
            dr2 = CUDABuffer(1, n, np.float32)
            dr2.UploadAsync(stream, np.ascontiguousarray(radius_squared, np.float32).reshape(1, n))
        if state is not None:
            dst = CUDABuffer(1, n, np.uint8)
            dst.UploadAsync(stream, np.ascontiguousarray(state, np.uint8).reshape(1, n))
        _lib.check(_lib.load().smx_nn_query_self(
            self._h, _sv(stream), C.c_void_p(dr2.ToCUDA().address if dr2 else 0), C.c_float(factor), C.c_int32(k),
            C.c_void_p(dst.ToCUDA().address if dst else 0), C.c_uint8(skip_mask), C.c_void_p(didx.ToCUDA().address),
            C.c_void_p(dd2.ToCUDA().address), C.c_void_p(dcnt.ToCUDA().address)))
        cnt = dcnt.Download(stream)[0].copy()
        d2 = dd2.Download(stream)[0].reshape(n, k).copy()
        idx = didx.Download(stream)[0].reshape(n, k).copy()
        for b in (didx, dd2, dcnt, dr2, dst):
            if b is not None:
                b.close()
        return cnt, d2, idx

    def set_query_mode(self, mode):
        """A/B switch (results identical): 2 = one lane per query, the tile kernel for what it marks (k_query_lanes; the
        default), 0 = one wavefront per query over LDS-staged brick tiles (k_query_tiles alone), 1 = one wavefront per query
        through L1 / L2 (k_query_stream; the self-query entry point has no such kernel and runs mode 0 there)."""
        _lib.check(_lib.load().smx_nn_set_query_mode(self._h, C.c_int32(mode)))

    def set_stats_enabled(self, enabled, stream=None):
        _lib.check(_lib.load().smx_nn_set_stats_enabled(self._h, _sv(stream), C.c_int32(1 if enabled else 0)))

    def stats(self, stream=None):
        """Index geometry and, while enabled, the tile / candidate / test / result counters of the queries (smx_nn_stats)."""
        st = _lib.NNStats()
        _lib.check(_lib.load().smx_nn_get_stats(self._h, _sv(stream), C.byref(st)))
        d = {n: getattr(st, n) for n, _ in _lib.NNStats._fields_ if n != "dim"}
        d["dim"] = [int(v) for v in st.dim]
        return d

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().smx_nn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
