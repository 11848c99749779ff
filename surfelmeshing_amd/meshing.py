"""Meshing the surfel map on the device (smx_recon_triangulate): a localized Delaunay triangulation.

    from surfelmeshing_amd import meshing
    triangles, stats = meshing.mesh_map(rec)                       # [T,3] uint32 slot indices
    export.SaveMeshAsOBJ(rec, "map.obj", triangles=triangles)
"""
from ._lib import MeshParams as _MeshParamsPOD

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
