"""Headless views of the device-resident surfel map, as splats (smx_recon_render) or through a triangle array
(smx_recon_render_mesh): images from any camera, as numpy arrays.

    img = render_view(rec, 640, 480, 525.0, 525.0, 320.0, 240.0, pose, splat_mode="disc")
    img["depth"], img["index"], img["normal"], img["color"]
    img = render_mesh_view(rec, triangles, 640, 480, 525.0, 525.0, 320.0, 240.0, pose)
    img = raycast_mesh_view(rec, triangles, 640, 480, 525.0, 525.0, 320.0, 240.0, pose)      # depth and index by ray casting

Cameras follow the project's conventions: intrinsics in the pixel-corner convention, poses global_T_camera as
row-major 3x4 with the camera's x right, y down, z forward.
"""
import numpy as np

from . import api

_SPLAT = {"square": api.SMX_SPLAT_SQUARE, "disc": api.SMX_SPLAT_DISC}
_COLOR = {"color": 0, "last_update": api.SMX_VIS_LAST_UPDATE, "creation": api.SMX_VIS_CREATION,
          "radii": api.SMX_VIS_RADII, "normals": api.SMX_VIS_NORMALS}
_NORMALS = {"vertex": api.SMX_MESH_NORMAL_VERTEX, "face": api.SMX_MESH_NORMAL_FACE}
_OUTPUTS = {"depth": (np.float32, 1), "index": (np.uint32, 1), "normal": (np.float32, 4), "color": (np.uint8, 4)}


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """global_T_camera (3x4 float32) of a camera at `eye` looking at `target`; `up` is the world direction that appears
    upwards in the image (the synthetic room's y axis points down, hence the default)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-9:
        raise ValueError("up is parallel to the viewing direction")
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], axis=1), eye[:, None]], axis=1).astype(np.float32)


def render_view(rec, width, height, fx, fy, cx, cy, global_T_camera, splat_mode="square", color="color",
                outputs=("depth", "index", "normal", "color"), stream=None, **opts):
    """Renders `rec` (an api.CUDASurfelReconstruction) and returns {name: array} for the requested outputs: depth
    float32 [H, W] (0 = empty), index uint32 [H, W] (0xFFFFFFFF = empty), normal float32 [H, W, 4] (camera frame),
    color uint8 [H, W, 4] (alpha 255 where covered).  splat_mode "square" / "disc" (or SMX_SPLAT_*), color one of
    color / last_update / creation / radii / normals (or SMX_VIS_* bits); further options are the fields of
    smx_render_params (near_z, far_z, splat_half_extent_in_pixels, disc_radius_factor, max_splat_extent_in_pixels,
    frame_index, surfel_integration_active_window_size).  Synchronises `stream`."""
    mode = _SPLAT[splat_mode] if isinstance(splat_mode, str) else int(splat_mode)
    flags = _COLOR[color] if isinstance(color, str) else int(color)
    params = api.make_render_params(width, height, fx, fy, cx, cy, global_T_camera, splat_mode=mode,
                                    color_flags=flags, **opts)
    bufs = {name: api.CUDABuffer(int(height), int(width), *_OUTPUTS[name]) for name in outputs}
    try:
        rec.Render(stream, params, **bufs)
        out = {name: b.DownloadAsync(stream) for name, b in bufs.items()}
        api.StreamSynchronize(stream)
    finally:
        for b in bufs.values():
            b.close()
    return out


def render_mesh_view(rec, triangles, width, height, fx, fy, cx, cy, global_T_camera, color="color", normal_mode="vertex",
                     cull_back_faces=False, outputs=("depth", "index", "normal", "color"), stream=None, **opts):
    """Draws `triangles` ([T,3] slot indices of `rec`: the output of Triangulate, TriangulateUpdate or DecimateMesh) and
    returns {name: array} in the shapes of render_view; index holds the triangle's position in the array.  normal_mode
    "vertex" (interpolated from the corners' normals) / "face" (or SMX_MESH_NORMAL_*), color as in render_view; further
    options are the fields of smx_mesh_render_params (near_z, far_z, frame_index,
    surfel_integration_active_window_size).  Synchronises `stream`."""
    mode = _NORMALS[normal_mode] if isinstance(normal_mode, str) else int(normal_mode)
    flags = _COLOR[color] if isinstance(color, str) else int(color)
    params = api.make_mesh_render_params(width, height, fx, fy, cx, cy, global_T_camera, color_flags=flags,
                                         cull_back_faces=cull_back_faces, normal_mode=mode, **opts)
    bufs = {name: api.CUDABuffer(int(height), int(width), *_OUTPUTS[name]) for name in outputs}
    try:
        rec.RenderMesh(stream, params, triangles, **bufs)
        out = {name: b.DownloadAsync(stream) for name, b in bufs.items()}
        api.StreamSynchronize(stream)
    finally:
        for b in bufs.values():
            b.close()
    return out


def raycast_mesh_view(rec, triangles, width, height, fx, fy, cx, cy, global_T_camera, cull_back_faces=False, near_z=0.0,
                      far_z=2.0 ** 20, cell_size=0.0, stream=None, scene=None):
    """The depth and index images of `triangles` by ray casting (smx_recon_raycast_mesh) instead of rasterising: {"depth":
    float32 [H, W] (0 = empty), "index": uint32 [H, W] (0xFFFFFFFF = empty)}, the sizes and dtypes render_mesh_view gives.
    One ray per pixel centre (meshing.camera_rays), so depth is the ray parameter t = the camera depth of the hit.  There is no
    near plane to clip against: it also works for a camera whose plane cuts triangles.  Different arithmetic from the
    rasteriser, so the two images agree on most pixels, not on all.  scene: a RayScene of `triangles` (meshing.build_ray_scene)
    to cast against, for one pose after another."""
    from . import meshing
    o, d = meshing.camera_rays(fx, fy, cx, cy, width, height, global_T_camera)
    hit, t, _ = meshing.cast_rays(rec, triangles, o, d, near_z, far_z, 1 if cull_back_faces else 0, cell_size, stream=stream, scene=scene)
    depth = np.where(hit != np.uint32(0xFFFFFFFF), t, np.float32(0.0)).astype(np.float32)
    return {"depth": depth.reshape(int(height), int(width)), "index": hit.reshape(int(height), int(width))}
