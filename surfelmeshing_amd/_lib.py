"""Loads surfelmeshing_amd/libsmx.so (the C-ABI of include/smx.h) through ctypes.

There is no CPU fallback: if the HIP library is missing or does not load, every
entry point of this package raises.  If torch is already imported (bench.py
imports it first for torch.distributed), the library binds to the HIP runtime
torch has loaded, so both share one runtime per process.
"""
import ctypes as C
import os

# One hardware queue per busy stream (smx_buffer.hip: runtime_advice): decided when the HIP runtime initialises, i.e. at the
# process's first HIP call -- possibly torch's -- so this module, the APPLICATION side of the binding, raises the default as
# early as its import.  libsmx.so itself does not touch the environment (smx_runtime_advice reports instead).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
_HERE = os.path.dirname(os.path.abspath(__file__))
# (SMX_LIB_PATH: A/B measurements of two builds in one session; the product loads the in-tree library)
SO_PATH = os.environ.get("SMX_LIB_PATH") or os.path.join(_HERE, "libsmx.so")


class SmxError(RuntimeError):
    pass


class BufferDesc(C.Structure):
    """smx_buffer_desc == CUDABuffer_<T> (VIS/cuda/cuda_buffer.cuh:44-119)."""
    _fields_ = [("address", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("pitch", C.c_size_t)]


class IntegrateParams(C.Structure):
    """smx_integrate_params: trailing arguments of CUDASurfelReconstruction::Integrate."""
    _fields_ = [("sensor_noise_factor", C.c_float),
                ("max_surfel_confidence", C.c_float),
                ("regularizer_weight", C.c_float),
                ("regularization_frame_window_size", C.c_int32),
                ("do_blending", C.c_int32),
                ("measurement_blending_radius", C.c_int32),
                ("regularization_iterations_per_integration_iteration", C.c_int32),
                ("radius_factor_for_regularization_neighbors", C.c_float),
                ("normal_compatibility_threshold_deg", C.c_float),
                ("surfel_integration_active_window_size", C.c_int32)]

    @classmethod
    def defaults(cls, **kw):
        p = cls(0.05, 5.0, 10.0, 30, 1, 12, 1, 2.0, 40.0, 2147483647)  # APP/main.cc:323-368
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class RenderParams(C.Structure):
    """smx_render_params: camera, splat shape and colour mode of smx_recon_render."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("global_T_camera", C.c_float * 12),
                ("near_z", C.c_float), ("far_z", C.c_float),
                ("splat_mode", C.c_int32),
                ("splat_half_extent_in_pixels", C.c_float),
                ("disc_radius_factor", C.c_float),
                ("max_splat_extent_in_pixels", C.c_float),
                ("color_flags", C.c_int32),
                ("frame_index", C.c_uint32),
                ("surfel_integration_active_window_size", C.c_int32)]


class TrackParams(C.Structure):
    """smx_track_params: schedule, gates, status thresholds and model-render settings of smx_recon_track."""
    _fields_ = [("level_stride", C.c_int32 * 3), ("level_iterations", C.c_int32 * 3),
                ("max_distance", C.c_float), ("max_normal_angle_deg", C.c_float),
                ("convergence_rotation", C.c_float), ("convergence_translation", C.c_float),
                ("min_inliers", C.c_int32), ("min_inlier_fraction", C.c_float), ("min_pivot_ratio", C.c_float),
                ("near_z", C.c_float), ("far_z", C.c_float), ("disc_radius_factor", C.c_float),
                ("max_splat_extent_in_pixels", C.c_float)]

    @classmethod
    def defaults(cls, levels=None, **kw):
        """smx_track_params_default(), then `levels` (up to three (stride, iterations) pairs, coarse to fine) and
        any field by name."""
        p = cls()
        check(load().smx_track_params_default(C.byref(p)))
        if levels is not None:
            levels = list(levels)
            if not 1 <= len(levels) <= 3:
                raise ValueError("one to three (stride, iterations) levels")
            for k in range(3):
                p.level_stride[k], p.level_iterations[k] = levels[k] if k < len(levels) else (1, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class TrackResult(C.Structure):
    """smx_track_result"""
    _fields_ = [("global_T_frame", C.c_float * 12), ("status", C.c_int32), ("iterations_run", C.c_int32),
                ("inliers", C.c_uint32), ("pixels_with_depth", C.c_uint32), ("rms_residual", C.c_float),
                ("last_update_rotation", C.c_float), ("last_update_translation", C.c_float),
                ("information", C.c_float * 36)]


TRACK_SUMS = 31   # SMX_TRACK_SUMS


class TrackIteration(C.Structure):
    """smx_track_iteration"""
    _fields_ = [("level", C.c_int32), ("stride", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32),
                ("sums", C.c_double * TRACK_SUMS), ("x", C.c_double * 6)]


class TrackRGBDParams(C.Structure):
    """smx_track_rgbd_params: smx_track_params plus the weight and the gates of the photometric term."""
    _fields_ = [("icp", TrackParams), ("photometric_weight", C.c_float), ("max_intensity_difference", C.c_float),
                ("min_gradient", C.c_float), ("gradient_max_relative_depth_step", C.c_float)]

    @classmethod
    def defaults(cls, levels=None, **kw):
        """smx_track_rgbd_params_default(), then `levels` and any field by name -- the photometric ones, or one of the
        embedded smx_track_params."""
        p = cls()
        check(load().smx_track_rgbd_params_default(C.byref(p)))
        own = [f for f, _ in cls._fields_ if f != "icp"]
        p.icp = TrackParams.defaults(levels, **{k: v for k, v in kw.items() if k not in own})
        for k, v in kw.items():
            if k in own:
                setattr(p, k, v)
        return p


class TrackRGBDResult(C.Structure):
    """smx_track_rgbd_result"""
    _fields_ = [("icp", TrackResult), ("photometric_inliers", C.c_uint32), ("rms_intensity_residual", C.c_float)]


TRACK_RGBD_SUMS = 33   # SMX_TRACK_RGBD_SUMS


class TrackRGBDIteration(C.Structure):
    """smx_track_rgbd_iteration"""
    _fields_ = [("level", C.c_int32), ("stride", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32),
                ("sums", C.c_double * TRACK_RGBD_SUMS), ("x", C.c_double * 6)]


class MeshParams(C.Structure):
    """smx_mesh_params: thresholds of smx_recon_triangulate (names as in the reference's main.cc)."""
    _fields_ = [("max_angle_between_normals_deg", C.c_float), ("min_triangle_angle_deg", C.c_float),
                ("max_triangle_angle_deg", C.c_float), ("search_radius_factor", C.c_float),
                ("max_neighbors", C.c_int32), ("max_star_degree", C.c_int32)]

    @classmethod
    def defaults(cls, **kw):
        """smx_mesh_params_default(), then any field by name."""
        p = cls()
        check(load().smx_mesh_params_default(C.byref(p)))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class MeshStats(C.Structure):
    """smx_mesh_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_live", "n_star_triangles", "n_triangles", "star_overflow", "truncated_lists")]


class MeshUpdateStats(C.Structure):
    """smx_mesh_update_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("mode", "n_changed", "n_dirty", "n_reagreed", "n_kept_triangles")]


class DecimateStats(C.Structure):
    """smx_decimate_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_used_vertices", "n_cells", "n_collapsed", "n_duplicates",
                                          "n_triangles")]


DECIMATE_PHASES = 4   # SMX_DECIMATE_PHASES


class ComponentsParams(C.Structure):
    """smx_components_params: the thresholds of smx_recon_mesh_components."""
    _fields_ = [("min_triangles", C.c_uint32), ("min_diagonal", C.c_float), ("keep_largest", C.c_uint32)]


class MeshComponent(C.Structure):
    """smx_mesh_component: one row of the component table."""
    _fields_ = [("label", C.c_uint32), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32), ("kept", C.c_uint32),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


class ComponentsStats(C.Structure):
    """smx_components_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_used_vertices", "n_components", "n_kept_components",
                                          "n_largest_triangles", "n_triangles")]


COMPONENTS_PHASES = 4   # SMX_COMPONENTS_PHASES


class FillParams(C.Structure):
    """smx_fill_params: the longest loop smx_recon_fill_holes lists, and the limits of the triangle filter."""
    _fields_ = [("max_hole_edges", C.c_uint32), ("min_triangle_angle_deg", C.c_float), ("max_triangle_angle_deg", C.c_float)]


class MeshHole(C.Structure):
    """smx_mesh_hole: one row of the table of listed loops."""
    _fields_ = [("label", C.c_uint32), ("n_edges", C.c_uint32), ("status", C.c_uint32)]


class FillStats(C.Structure):
    """smx_fill_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_edges", "n_boundary_edges", "n_nonmanifold_edges",
                                          "n_pinched_vertices", "n_listed_loops", "n_filled_loops", "n_rejected_diagonal",
                                          "n_rejected_filter", "n_new_triangles", "n_triangles")]


FILL_PHASES = 4             # SMX_FILL_PHASES
FILL_MAX_HOLE_EDGES = 32    # SMX_FILL_MAX_HOLE_EDGES


class DistanceParams(C.Structure):
    """smx_distance_params: the search radius, the grid's cell (0: the library chooses) and the sign switch."""
    _fields_ = [("max_distance", C.c_float), ("cell_size", C.c_float), ("signed_distance", C.c_int32)]


DIST_PHASES = 4             # SMX_DIST_PHASES
DIST_BINS = 32              # SMX_DIST_BINS
DIST_MAX_COORD = 64.0       # SMX_DIST_MAX_COORD
DIST_WIDE_CELLS = 64        # SMX_DIST_WIDE_CELLS
DIST_MARGIN = 1.125         # the grid's cell is at least this many max_distance (smx.h step 5)


class DistanceStats(C.Structure):
    """smx_distance_stats"""
    _fields_ = ([(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_points", "n_bad_points",
                                           "n_matched", "max_dist2_bits")] + [("histogram", C.c_uint32 * DIST_BINS)] +
                [(n, C.c_uint32) for n in ("n_wide", "n_entries", "n_cells")] + [("cell_size_used", C.c_float)])


class RimStats(C.Structure):
    """smx_rim_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_edges", "n_rim_edges", "n_nonmanifold_edges",
                                          "n_rim_vertices", "n_rim_triangles")]


class SampleStats(C.Structure):
    """smx_sample_stats"""
    _fields_ = ([(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_zero_weight", "n_samples", "n_none",
                                           "n_triangles_hit")] + [("total_weight", C.c_uint64), ("stride", C.c_uint64)])


SAMPLE_PHASES = 3           # SMX_SAMPLE_PHASES
SAMPLE_MAX = 1 << 28        # the most triangles and the most samples of one call


class CompareParams(C.Structure):
    """smx_compare_params: the search radius and the grid's cell of the distance half, the samples per side and their seed, and
    which sides to measure (1: A->B, 2: B->A, 3: both)."""
    _fields_ = [("max_distance", C.c_float), ("cell_size", C.c_float), ("n_samples", C.c_uint32), ("seed", C.c_uint32),
                ("directions", C.c_int32)]


class CompareSide(C.Structure):
    """smx_compare_side"""
    _fields_ = [("sample", SampleStats), ("distance", DistanceStats), ("sum_d", C.c_uint64), ("sum_sq_lo", C.c_uint64),
                ("sum_sq_hi", C.c_uint64)]


class CompareStats(C.Structure):
    """smx_compare_stats"""
    _fields_ = [("a_to_b", CompareSide), ("b_to_a", CompareSide)]


COMPARE_PHASES = 6          # SMX_COMPARE_PHASES


class RaycastParams(C.Structure):
    """smx_raycast_params: the range of the ray parameter, the grid's cell (0: the library chooses) and the culling mode."""
    _fields_ = [("t_min", C.c_float), ("t_max", C.c_float), ("cell_size", C.c_float), ("cull", C.c_int32)]


RAY_PHASES = 4              # SMX_RAY_PHASES
RAY_MAX_DIR = 1024.0        # SMX_RAY_MAX_DIR
RAY_MIN_DIR = 2.0 ** -10    # SMX_RAY_MIN_DIR
RAY_MAX_T = 2.0 ** 20       # SMX_RAY_MAX_T
RAY_BOX_SLACK = 2.0 ** -12  # SMX_RAY_BOX_SLACK
RAY_MIN_CELL = 2.0 ** -9    # SMX_RAY_MIN_CELL


class RaycastStats(C.Structure):
    """smx_raycast_stats"""
    _fields_ = ([(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_rays", "n_bad_rays", "n_hit",
                                           "n_front_hits", "max_t_bits", "n_wide", "n_entries", "n_cells")] +
                [("cell_size_used", C.c_float), ("reserved", C.c_uint32)] +
                [(n, C.c_uint64) for n in ("n_layers", "n_lookups", "n_pair_tests")])


class RaySceneParams(C.Structure):
    """smx_rayscene_params: the grid's cell (0: the library chooses) and the occupancy bit grid (-1 none, 0 the library chooses,
    1 + k: a bit per block of 2^k cells per axis)."""
    _fields_ = [("cell_size", C.c_float), ("occupancy", C.c_int32)]


RAYSCENE_PHASES = 5         # SMX_RAYSCENE_PHASES
RAYSCENE_MAX_LOG2 = 6       # the largest k of an occupancy block


class RaySceneStats(C.Structure):
    """smx_rayscene_stats"""
    _fields_ = ([(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_wide", "n_entries", "n_cells")] +
                [("cell_size_used", C.c_float), ("occupancy_log2", C.c_int32), ("n_blocks_set", C.c_uint32),
                 ("occupancy_bytes", C.c_uint64), ("device_bytes", C.c_uint64)])


class RaySceneCastStats(C.Structure):
    """smx_rayscene_cast_stats"""
    _fields_ = ([(n, C.c_uint32) for n in ("n_rays", "n_bad_rays", "n_hit", "n_front_hits", "max_t_bits", "reserved")] +
                [(n, C.c_uint64) for n in ("n_layers", "n_bit_tests", "n_lookups", "n_lookup_misses", "n_pair_tests")])


class DistSceneParams(C.Structure):
    """smx_distscene_params: the bound on a query's max_distance and the grid's cell (0: the library chooses)."""
    _fields_ = [("max_distance", C.c_float), ("cell_size", C.c_float)]


DISTSCENE_PHASES = 5        # SMX_DISTSCENE_PHASES


class DistSceneStats(C.Structure):
    """smx_distscene_stats"""
    _fields_ = ([(n, C.c_uint32) for n in ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_wide", "n_entries", "n_cells")] +
                [("cell_size_used", C.c_float), ("max_distance", C.c_float), ("device_bytes", C.c_uint64)])


class RegisterParams(C.Structure):
    """smx_register_params: schedule, gates and status thresholds of smx_distscene_register."""
    _fields_ = [("level_stride", C.c_int32 * 3), ("level_iterations", C.c_int32 * 3), ("level_max_distance", C.c_float * 3),
                ("max_normal_angle_deg", C.c_float), ("convergence_rotation", C.c_float), ("convergence_translation", C.c_float),
                ("min_inliers", C.c_int32), ("min_inlier_fraction", C.c_float), ("min_pivot_ratio", C.c_float)]

    @classmethod
    def defaults(cls, levels=None, **kw):
        """smx_register_params_default(), then `levels` (up to three (stride, iterations) or (stride, iterations,
        max_distance) tuples, coarse to fine) and any field by name."""
        p = cls()
        check(load().smx_register_params_default(C.byref(p)))
        if levels is not None:
            levels = [tuple(lv) for lv in levels]
            if not 1 <= len(levels) <= 3 or any(len(lv) not in (2, 3) for lv in levels):
                raise ValueError("one to three (stride, iterations[, max_distance]) levels")
            for k in range(3):
                lv = levels[k] if k < len(levels) else (1, 0, 0.0)
                p.level_stride[k], p.level_iterations[k], p.level_max_distance[k] = lv[0], lv[1], lv[2] if len(lv) == 3 else 0.0
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise AttributeError(k)
            kind = dict(cls._fields_)[k]
            setattr(p, k, kind(*v) if issubclass(kind, C.Array) else v)
        return p


class RegisterRobustParams(C.Structure):
    """smx_register_robust_params: the weight kernel (0 none, 1 Huber, 2 Tukey), its scale per level in metres (0 = no weights on
    that level) and whether a match whose closest point lies on the rim of the scene's mesh is rejected."""
    _fields_ = [("kernel", C.c_int32), ("level_scale", C.c_float * 3), ("reject_rim", C.c_int32)]


REGISTER_KERNELS = {"none": 0, "huber": 1, "tukey": 2}


class RegisterResult(C.Structure):
    """smx_register_result"""
    _fields_ = [("scene_T_points", C.c_float * 12), ("status", C.c_int32), ("iterations_run", C.c_int32),
                ("inliers", C.c_uint32), ("points_used", C.c_uint32), ("rms_residual", C.c_float),
                ("last_update_rotation", C.c_float), ("last_update_translation", C.c_float), ("information", C.c_float * 36)]


REGISTER_SUMS = 31      # SMX_REGISTER_SUMS
REGISTER_PHASES = 5     # SMX_REGISTER_PHASES
REGISTER_MAX_STRIDE = 65536
REGISTER_MAX_POINTS = 1 << 28


class RegisterIteration(C.Structure):
    """smx_register_iteration"""
    _fields_ = [("level", C.c_int32), ("stride", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32),
                ("Tf", C.c_float * 12), ("sums", C.c_double * REGISTER_SUMS), ("x", C.c_double * 6)]


class ScoreParams(C.Structure):
    """smx_score_params: which samples a pose is scored on (stride), the gate q (0 = the scene's bound) and whether a match on
    the rim of the scene's mesh pays q."""
    _fields_ = [("stride", C.c_int32), ("max_distance", C.c_float), ("reject_rim", C.c_int32)]


class PoseScore(C.Structure):
    """smx_pose_score"""
    _fields_ = [("cost", C.c_uint64), ("n_ok", C.c_uint32), ("n_matched", C.c_uint32), ("n_rim", C.c_uint32), ("reserved", C.c_uint32)]


POSE_SCORE_DTYPE = [("cost", "<u8"), ("n_ok", "<u4"), ("n_matched", "<u4"), ("n_rim", "<u4"), ("reserved", "<u4")]   # numpy's view of it


class GlobalParams(C.Structure):
    """smx_global_params: the score's parameters, the number of starts refined and the matched fraction `found` asks for."""
    _fields_ = [("score", ScoreParams), ("n_starts", C.c_int32), ("min_matched_fraction", C.c_float)]


GLOBAL_MAX_STARTS = 64      # SMX_GLOBAL_MAX_STARTS
GLOBAL_PHASES = 7           # SMX_GLOBAL_PHASES
GLOBAL_MAX_POSES = 1 << 20
GLOBAL_MAX_SAMPLES = 1 << 16


class GlobalStart(C.Structure):
    """smx_global_start"""
    _fields_ = [("pose_index", C.c_uint32), ("status", C.c_int32), ("iterations_run", C.c_int32), ("n_matched_after", C.c_uint32),
                ("cost_before", C.c_uint64), ("cost_after", C.c_uint64)]


class GlobalResult(C.Structure):
    """smx_global_result"""
    _fields_ = [("result", RegisterResult), ("found", C.c_int32), ("winner_rank", C.c_int32), ("n_starts_run", C.c_int32),
                ("reserved", C.c_int32), ("starts", GlobalStart * GLOBAL_MAX_STARTS)]


class MergeParams(C.Structure):
    """smx_merge_params: the index cell, the ball and the normal gate of the match, k, the mode and the stamp of smx_recon_merge_map."""
    _fields_ = [("cell_size", C.c_float), ("radius_factor_squared", C.c_float), ("max_normal_angle_deg", C.c_float), ("k", C.c_int32),
                ("mode", C.c_int32), ("confidence_cap", C.c_float), ("frame_index", C.c_uint32)]

    @classmethod
    def defaults(cls, **kw):
        """smx_merge_params_default(), then any field by name."""
        p = cls()
        check(load().smx_merge_params_default(C.byref(p)))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


MERGE_MODES = {"keep": 0, "blend": 1}      # SMX_MERGE_KEEP_DST, SMX_MERGE_BLEND
MERGE_PHASES = 7                           # SMX_MERGE_PHASES
MERGE_PHASE_NAMES = ("whole", "build", "move", "query_select", "number", "append", "blend", "finish")


class MergeStats(C.Structure):
    """smx_merge_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_src_slots", "n_src_live", "n_bad", "n_matched", "n_appended", "n_blended_dst", "n_saturated",
                                          "links_dropped", "old_size", "new_size")]


class ImportParams(C.Structure):
    """smx_import_params: the index cell, the search ball, k, the gates, the radius rule, the constant rows and the orientation of
    smx_recon_import_points."""
    _fields_ = [("cell_size", C.c_float), ("search_radius", C.c_float), ("k", C.c_int32), ("min_neighbors", C.c_int32),
                ("max_surface_variation", C.c_float), ("radius_rank", C.c_int32), ("radius_scale_squared", C.c_float),
                ("confidence", C.c_float), ("default_color", C.c_uint32), ("frame_index", C.c_uint32), ("orient", C.c_int32),
                ("view_point", C.c_float * 3)]

    @classmethod
    def defaults(cls, **kw):
        """smx_import_params_default(), then any field by name."""
        p = cls()
        check(load().smx_import_params_default(C.byref(p)))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise AttributeError(k)
            setattr(p, k, (C.c_float * 3)(*v) if k == "view_point" else v)
        return p


IMPORT_ORIENTS = {"none": 0, "view_point": 1, "origins": 2}      # SMX_IMPORT_ORIENT_*
IMPORT_PHASES = 7                                                # SMX_IMPORT_PHASES
IMPORT_PHASE_NAMES = ("whole", "stage", "build", "query", "fit", "number", "write", "finish")


class ImportStats(C.Structure):
    """smx_import_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_points", "n_bad", "n_sparse", "n_degenerate", "n_rough", "n_imported", "n_saturated",
                                          "old_size", "new_size")]


class MeshRenderParams(C.Structure):
    """smx_mesh_render_params: camera, colour mode, culling and normal mode of smx_recon_render_mesh."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("global_T_camera", C.c_float * 12),
                ("near_z", C.c_float), ("far_z", C.c_float),
                ("color_flags", C.c_int32), ("frame_index", C.c_uint32),
                ("surfel_integration_active_window_size", C.c_int32),
                ("cull_back_faces", C.c_int32), ("normal_mode", C.c_int32)]

    @classmethod
    def defaults(cls, **kw):
        """smx_mesh_render_params_default(), then any field by name."""
        p = cls()
        check(load().smx_mesh_render_params_default(C.byref(p)))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class MeshRenderStats(C.Structure):
    """smx_mesh_render_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("n_in", "n_out_of_range", "n_not_live", "n_clipped", "n_degenerate", "n_culled",
                                          "n_drawn", "n_large", "n_covered_pixels")]


class SurfelBuffersCPU(C.Structure):
    """smx_surfel_buffers_cpu == CUDASurfelBuffersCPU (APP/cuda_surfels_cpu.h:40-74)."""
    _fields_ = [("frame_index", C.c_uint32), ("surfel_count", C.c_size_t),
                ("surfel_x_buffer", C.c_void_p), ("surfel_y_buffer", C.c_void_p), ("surfel_z_buffer", C.c_void_p),
                ("surfel_radius_squared_buffer", C.c_void_p),
                ("surfel_normal_x_buffer", C.c_void_p), ("surfel_normal_y_buffer", C.c_void_p),
                ("surfel_normal_z_buffer", C.c_void_p), ("surfel_last_update_stamp_buffer", C.c_void_p)]


class SurfelDeltaCPU(C.Structure):
    """smx_surfel_delta_cpu: the changed-surfel delta of smx_recon_transfer_changed_to_cpu."""
    _fields_ = [("capacity", C.c_uint32), ("count", C.c_uint32), ("frame_index", C.c_uint32), ("surfel_count", C.c_uint32),
                ("surfel_index", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p),
                ("radius_squared", C.c_void_p), ("normal_x", C.c_void_p), ("normal_y", C.c_void_p),
                ("normal_z", C.c_void_p), ("last_update_stamp", C.c_void_p)]


class ReconStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in
                ("surfels_size", "merge_count", "n_visible", "n_new", "n_merged", "n_recent", "n_edges",
                 "n_integrated", "n_replaced", "n_conflict_hits", "capacity_clamped", "n_window_edges", "n_contributors",
                 "n_segments_skipped", "regularizer_saturated", "n_pairs", "n_overflow_pairs", "max_tile_pairs")]


class NNStats(C.Structure):
    """smx_nn_stats"""
    _fields_ = [("n_points", C.c_uint32), ("n_indexed", C.c_uint32), ("n_bricks", C.c_uint32), ("cell_size", C.c_float),
                ("dim", C.c_int32 * 3), ("key_bits", C.c_int32), ("tiles", C.c_uint64), ("staged_candidates", C.c_uint64),
                ("distance_tests", C.c_uint64), ("results", C.c_uint64)]


# every symbol include/smx.h declares (tests/test_abi.py checks the .so exports them all)
EXPORTS = [
    "smx_last_error", "smx_runtime_advice", "smx_host_is_page_locked", "smx_device_count", "smx_set_device", "smx_device_name",
    "smx_stream_create", "smx_stream_create_with_priority", "smx_stream_create_with_cu_mask", "smx_recon_set_internal_cu_mask", "smx_recon_set_handover_mode", "smx_recon_get_handover_mode", "smx_host_alloc", "smx_host_free", "smx_stream_destroy", "smx_stream_synchronize", "smx_debug_marker", "smx_debug_handover_probe",
    "smx_debug_live_allocations", "smx_debug_fail_allocation",
    "smx_event_create", "smx_event_create_timed", "smx_event_elapsed_ms", "smx_event_destroy", "smx_event_record", "smx_stream_wait_event",
    "smx_buffer_create", "smx_buffer_destroy", "smx_buffer_get_desc", "smx_buffer_upload", "smx_buffer_upload_by_kernel", "smx_buffer_download",
    "smx_buffer_upload_part", "smx_buffer_download_part", "smx_buffer_clear", "smx_buffer_set_to",
    "smx_bilateral_filtering_and_depth_cutoff", "smx_outlier_depth_map_fusion", "smx_bilateral_outlier_fusion", "smx_erode_depth_map",
    "smx_copy_without_border", "smx_median_filter_and_densify_depth_map", "smx_downscale_using_median_while_excluding", "smx_color_image_pyramid", "smx_compute_normals_and_drop_bad_pixels",
    "smx_compute_point_radii_and_remove_isolated_pixels", "smx_erode_normals_radii", "smx_erode_normals_radii_signal",
    "smx_recon_create", "smx_recon_destroy", "smx_recon_integrate", "smx_recon_regularize",
    "smx_recon_transfer_all_to_cpu", "smx_recon_set_delta_tracking", "smx_recon_transfer_changed_to_cpu", "smx_recon_export_vertices", "smx_recon_get_timings", "smx_recon_get_timings_nowait", "smx_recon_debug_stamp_ring", "smx_recon_debug_internal_stream",
    "smx_recon_build_neighbor_index", "smx_recon_neighbor_candidates", "smx_recon_check_triangles",
    "smx_mesh_params_default", "smx_recon_triangulate", "smx_recon_debug_mesh_timings",
    "smx_recon_triangulate_update", "smx_recon_triangulate_reset", "smx_recon_debug_mesh_update_timings", "smx_recon_deform_by_creation_frame",
    "smx_recon_decimate_mesh", "smx_recon_debug_decimate_timings",
    "smx_components_params_default", "smx_recon_mesh_components", "smx_recon_debug_components_timings",
    "smx_fill_params_default", "smx_recon_fill_holes", "smx_recon_debug_fill_timings",
    "smx_distance_params_default", "smx_recon_mesh_distance", "smx_recon_debug_distance_timings",
    "smx_recon_mesh_rim", "smx_recon_build_distscene_rim", "smx_register_robust_params_default", "smx_distscene_register_robust",
    "smx_distscene_debug_register_robust_counts", "smx_recon_register_mesh",
    "smx_recon_sample_mesh", "smx_recon_debug_sample_timings", "smx_recon_compare_meshes", "smx_recon_debug_compare_timings",
    "smx_raycast_params_default", "smx_recon_raycast_mesh", "smx_recon_debug_raycast_timings",
    "smx_rayscene_create", "smx_rayscene_destroy", "smx_rayscene_params_default", "smx_recon_build_rayscene", "smx_rayscene_cast",
    "smx_rayscene_debug_timings",
    "smx_distscene_create", "smx_distscene_destroy", "smx_distscene_params_default", "smx_recon_build_distscene", "smx_distscene_query",
    "smx_recon_compare_to_distscene", "smx_distscene_debug_timings",
    "smx_register_params_default", "smx_distscene_register", "smx_distscene_debug_register_iterations", "smx_distscene_debug_register_timings",
    "smx_register_pose_lattice", "smx_global_params_default", "smx_distscene_score_poses", "smx_distscene_register_global",
    "smx_distscene_debug_set_score_chunk", "smx_distscene_debug_global_timings",
    "smx_mesh_render_params_default", "smx_recon_render_mesh", "smx_recon_debug_mesh_render_timings",
    "smx_recon_set_timing_enabled", "smx_recon_counts", "smx_recon_get_stats", "smx_recon_set_stats_enabled",
    "smx_recon_kernel_slot_count", "smx_recon_kernel_slot_name", "smx_recon_get_kernel_timings",
    "smx_recon_profile_begin", "smx_recon_profile_end",
    "smx_merge_params_default", "smx_recon_merge_map", "smx_recon_debug_merge_timings", "smx_recon_debug_set_merge_chunk",
    "smx_import_params_default", "smx_recon_import_points", "smx_recon_debug_import_timings",
    "smx_recon_compact", "smx_recon_update_visualization_buffers", "smx_recon_render", "smx_track_params_default", "smx_recon_track", "smx_recon_debug_track_iterations", "smx_track_rgbd_params_default", "smx_recon_track_rgbd", "smx_recon_debug_track_rgbd_iterations", "smx_recon_debug_download_surfels", "smx_recon_debug_upload_surfels", "smx_recon_debug_download_scratch", "smx_recon_debug_count_skipped_segments",
    "smx_recon_set_scan_mode", "smx_recon_debug_set_skip", "smx_recon_set_overlap", "smx_recon_integrate_hooks", "smx_recon_integrate_inputs_ready",
    "smx_nn_create", "smx_nn_destroy", "smx_nn_build", "smx_nn_query_batch", "smx_nn_query_self", "smx_nn_set_query_mode", "smx_nn_set_stats_enabled", "smx_nn_get_stats",
    "smx_synth_render_room",
]

_lib = None


def load():
    """Returns the ctypes handle of libsmx.so; raises SmxError if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise SmxError("%s is missing: run `python -m surfelmeshing_amd.build` (hipcc, gfx950). "
                       "There is no CPU fallback." % SO_PATH)
    try:
        L = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise SmxError("cannot load %s: %s" % (SO_PATH, e))
    L.smx_last_error.restype = C.c_char_p
    L.smx_recon_kernel_slot_name.restype = C.c_char_p
    for name in EXPORTS:
        if name not in ("smx_last_error", "smx_recon_kernel_slot_name"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = load().smx_last_error()
        raise SmxError("libsmx error %d: %s" % (rc, msg.decode() if msg else "?"))


def device_count():
    n = C.c_int(0)
    check(load().smx_device_count(C.byref(n)))
    return n.value


def require_gpu():
    if device_count() == 0:
        raise SmxError("no HIP device visible: the surfel-integration path needs an MI355X (no CPU fallback)")
