"""The viewer buffers and the headless render at the boundary (no GPU): the C-ABI symbols, the smx_render_params
layout against its ctypes mirror, the shim's calls compiling against libsmx.so, and the numpy restatement of
tests/viz_ref.py checked against closed-form answers and against the synthetic stream's noise-free ray cast of an
oracle-built map (which fixes the geometric thresholds the GPU test reuses)."""
import ctypes
import os
import subprocess

import numpy as np

import viz_ref as vr
from common import ROOT, small_pre, small_stream

NEW_SYMBOLS = ("smx_recon_update_visualization_buffers", "smx_recon_render")

# Rendering the oracle's map at a capture pose against the ray-cast depth of that frame (measured by
# test_reference_render_matches_the_raycast_depth on the CPU; the GPU test applies the same bounds to its render).
# Measured: 64.7 % of the hit pixels covered by discs after 8 frames of small_stream (the map is still sparse),
# relative depth error median 2.7e-4, 95th percentile 8.3e-4.
RAYCAST_MIN_COVERAGE = 0.55       # covered fraction of the pixels the ray cast hits (disc splats)
RAYCAST_MEDIAN_REL_ERR = 1e-3     # median |depth - raycast| / raycast over covered pixels
RAYCAST_P95_REL_ERR = 3e-3        # 95th percentile


def test_symbols_are_declared_and_exported():
    from surfelmeshing_amd import _lib
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.EXPORTS and name in exported, name
    for name in ("SMX_VIS_LAST_UPDATE", "SMX_VIS_CREATION", "SMX_VIS_RADII", "SMX_VIS_NORMALS", "SMX_SPLAT_SQUARE",
                 "SMX_SPLAT_DISC", "smx_render_params"):
        assert name in header, name


def test_render_params_layout_matches_the_ctypes_mirror(tmp_path):
    from surfelmeshing_amd._lib import RenderParams
    fields = [f for f, _ in RenderParams._fields_]
    src = tmp_path / "render_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smx.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(smx_render_params));\n' +
                   "".join('  printf(" %%zu", offsetof(smx_render_params, %s));\n' % f for f in fields) +
                   '  printf(" %d %d %d %d %d %d\\n", SMX_VIS_LAST_UPDATE, SMX_VIS_CREATION, SMX_VIS_RADII, SMX_VIS_NORMALS,'
                   ' SMX_SPLAT_SQUARE, SMX_SPLAT_DISC);\n  return 0;\n}\n')
    exe = tmp_path / "render_probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(RenderParams)
    assert vals[1:1 + len(fields)] == [getattr(RenderParams, f).offset for f in fields]
    from surfelmeshing_amd import api
    assert vals[1 + len(fields):] == [api.SMX_VIS_LAST_UPDATE, api.SMX_VIS_CREATION, api.SMX_VIS_RADII,
                                      api.SMX_VIS_NORMALS, api.SMX_SPLAT_SQUARE, api.SMX_SPLAT_DISC]


SHIM_SNIPPET = r'''
#include "smx_shim.hpp"
using namespace vis;
void viewer_frame(cudaStream_t stream, CUDASurfelReconstruction& reconstruction, void* vertices, void* neighbors,
                  void* normal_vertices, u32 capacity, u32 frame_index) {
  reconstruction.SetVisualizationBuffers(vertices, capacity, neighbors, capacity, normal_vertices, capacity);
  // APP/main.cc:1323-1330, token for token
  reconstruction.UpdateVisualizationBuffers(
      stream,
      frame_index,
      /*latest_triangulated_frame_index*/ 0,
      /*latest_mesh_surfel_count*/ 0,
      /*surfel_integration_active_window_size*/ 30,
      /*visualize_last_update_timestamp*/ false,
      /*visualize_creation_timestamp*/ false,
      /*visualize_radii*/ true,
      /*visualize_normals*/ false);
  smx_render_params p = {};
  p.width = 64; p.height = 48; p.fx = p.fy = 50.f; p.cx = 32.f; p.cy = 24.f;
  p.global_T_camera[0] = p.global_T_camera[5] = p.global_T_camera[10] = 1.f;
  p.near_z = 0.1f; p.far_z = 100.f; p.splat_mode = SMX_SPLAT_DISC;
  p.splat_half_extent_in_pixels = 3.f; p.disc_radius_factor = 1.f; p.max_splat_extent_in_pixels = 16.f;
  p.color_flags = SMX_VIS_NORMALS; p.frame_index = frame_index; p.surfel_integration_active_window_size = 30;
  CUDABuffer<float> depth(48, 64);
  CUDABuffer<u32> index(48, 64);
  CUDABuffer<RenderNormal> normal(48, 64);
  CUDABuffer<RenderColor> color(48, 64);
  reconstruction.Render(stream, p, &depth, &index, &normal, &color);
  reconstruction.Render(stream, p, &depth, nullptr, nullptr, nullptr);
}
int main() { return 0; }
'''


def test_shim_viewer_and_render_calls_compile(tmp_path):
    from surfelmeshing_amd import _lib
    src = tmp_path / "viewer.cc"
    src.write_text(SHIM_SNIPPET)
    lib_dir = os.path.dirname(_lib.SO_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(tmp_path / "viewer"), "-L", lib_dir, "-l:libsmx.so", "-Wl,-rpath," + lib_dir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the numpy restatement ------------------------------------------------------------------------------------------
def _rows(p, nrm, r2, color=None):
    """Reference-order rows for slots at positions p [k, 3] (smooth = raw), normals nrm, radius^2 r2."""
    k = len(p)
    rows = np.zeros((25, k), np.float32)
    rows[0:3] = rows[3:6] = np.asarray(p, np.float32).T
    rows[8:11] = np.asarray(nrm, np.float32).T
    rows[7] = r2
    rows[19:23] = np.full((4, k), vr.INVALID, np.uint32).view(np.float32)
    if color is not None:
        rows[24] = np.asarray(color, np.uint32).view(np.float32)
    return rows


IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def test_reference_disc_facing_the_camera_is_the_analytic_circle():
    W = H = 64
    f, c, z, rho = 100.0, 32.0, 2.0, 0.2          # radius in pixels: f rho / z = 10
    rows = _rows([[0.0, 0.0, z]], [[0.0, 0.0, -1.0]], rho * rho)
    ref = vr.render(rows, 1, W, H, f, f, c, c, IDENT, mode=vr.SPLAT_DISC, max_extent=16.0)
    ys, xs = np.mgrid[0:H, 0:W]
    r_px = np.hypot(xs + 0.5 - c, ys + 0.5 - c)
    want = r_px <= f * rho / z
    assert np.array_equal(ref["index"] != vr.INVALID, want)
    assert np.allclose(ref["depth"][want], z, rtol=1e-12)
    assert want.sum() > 300


def test_reference_square_covers_2h_plus_1_squared_pixels():
    for h in (0.0, 1.0, 3.0):
        # u = v = 20.5 exactly: the centre of pixel (20, 20)
        rows = _rows([[0.0, 0.0, 1.0]], [[0.0, 0.0, -1.0]], 1e-4)
        ref = vr.render(rows, 1, 41, 41, 100.0, 100.0, 20.5, 20.5, IDENT, mode=vr.SPLAT_SQUARE, half_extent=h)
        cov = ref["index"] != vr.INVALID
        assert cov.sum() == (2 * h + 1) ** 2, (h, cov.sum())
        assert cov[20, 20] and np.all(ref["depth"][cov] == 1.0)


def test_reference_ties_go_to_the_lower_slot():
    rows = _rows([[0.0, 0.0, 1.0]] * 3, [[0.0, 0.0, -1.0]] * 3, [1e-4, -1.0, 1e-4])   # slot 1 merged
    ref = vr.render(rows, 3, 21, 21, 100.0, 100.0, 10.5, 10.5, IDENT, half_extent=2.0)
    cov = ref["index"] != vr.INVALID
    assert cov.sum() == 25 and np.all(ref["index"][cov] == 0) and np.all(ref["gap"][cov] == 0)
    assert vr.unstable(ref)[cov].all()   # (an exact tie: any float evaluation must break it by slot, flagged anyway)


def test_reference_vertex_colours_follow_the_flag_precedence():
    rows = _rows([[0, 0, 1]] * 4, [[0, 0, -1]] * 4, [1e-6, 2.5e-5, 1e-3, -1.0], color=[0x11223344] * 4)
    rows[17] = np.array([5, 5, 5, 5], np.uint32).view(np.float32)     # creation
    rows[18] = np.array([10, 9, 4, 10], np.uint32).view(np.float32)   # last update
    plain = vr.vis_color(rows, np.arange(4), 0, 10, 30)
    assert np.all(plain == 0x11223344)
    last = vr.vis_color(rows, np.arange(4), vr.VIS_LAST_UPDATE | vr.VIS_RADII, 10, 30)
    assert last[0] == vr._rgb(255, 80, 80) and last[1] == vr._rgb(255, 255, 255)
    g = 255 - int(np.float32(255.99) * np.float32(5.0 / 29.0))
    assert last[2] == vr._rgb(g, g, g)
    # creation wins over last update (the stamp is the creation stamp)
    cr = vr.vis_color(rows, np.arange(4), vr.VIS_LAST_UPDATE | vr.VIS_CREATION, 10, 30)
    g = 255 - int(np.float32(255.99) * np.float32(4.0 / 2999.0))
    assert np.all(cr == vr._rgb(g, g, g))
    rad = vr.vis_color(rows, np.arange(4), vr.VIS_RADII | vr.VIS_NORMALS, 10, 30)
    assert rad[3] == vr._rgb(0, 255, 80)                                # merged: sqrt(<0) = NaN -> blend 0
    assert rad[2] == vr._rgb(255, 0, 80)                                # 3.2 cm > 1 cm
    nb = vr.neighbor_buffer(rows, 4)
    assert np.array_equal(nb[:, 1::2], np.repeat(np.arange(4, dtype=np.uint32)[:, None], 4, 1))
    nv = vr.normal_vertex_buffer(rows, 4).view(np.float32)
    assert np.isnan(nv[3, 3:]).all() and np.allclose(nv[0, 3:], [0, 0, 1 - 1e-3])


def test_reference_render_matches_the_raycast_depth(orc):
    """An oracle-built map rendered at a capture pose against SyntheticStream's noise-free ray cast: this is where the
    RAYCAST_* bounds come from (the measured values sit well inside them)."""
    from oracle_pipeline import OraclePipeline
    s = small_stream(obstacle_until=8)
    po = OraclePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, small_pre(s.width))
    for f in range(0, 16):
        po.upload(f, *s.frame(f))
    for f in range(4, 12):
        po.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    rows = po.recon.surfels()
    n = po.recon.surfels_size
    f = 11
    ref = vr.render(rows, n, s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.pose(f), mode=vr.SPLAT_DISC)
    cov, err, _ = raycast_agreement(s, f, ref["depth"])
    assert cov >= RAYCAST_MIN_COVERAGE, cov
    assert np.median(err) <= RAYCAST_MEDIAN_REL_ERR and np.percentile(err, 95) <= RAYCAST_P95_REL_ERR, (
        np.median(err), np.percentile(err, 95))


def raycast_agreement(s, f, depth):
    """(covered fraction of the ray-cast hits, relative depth errors at covered hits, covered mask)."""
    z, _ = s._raycast(f)
    hit = np.isfinite(z)
    covered = depth > 0
    both = hit & covered
    err = np.abs(depth[both] - z[both]) / z[both]
    return both.sum() / max(hit.sum(), 1), err, covered
