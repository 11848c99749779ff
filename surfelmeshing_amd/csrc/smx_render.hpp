// smx_render.hpp -- what smx_recon_render (smx_recon_map.hip), smx_recon_render_mesh (smx_mesh_raster.hip) and the tracking
// calls (smx_track.hip, which render their model images with the first) share (internal): the workspace -- one per object,
// a z-buffer serves one render at a time -- the rules for a view and for an image, and the two calls that bracket a render's
// enqueued work.  A view's camera_T_global is mr_invert_pose (smx_mesh_raster.hpp, where that arithmetic's host test reaches it).
#pragma once

#include <cmath>

#include "smx_common.hpp"
#include "smx_mesh_raster.hpp"

namespace smx {

struct RenderWork {
  DevBuf<unsigned long long> zbuf;   // [height][width] keys (depth bits, slot or triangle); grows on demand
  StreamMark mark;                   // behind the last render's resolve: the next render clears the z-buffer after it
  // smx_recon_render_mesh
  DevBuf<uint32_t> list;             // [n_triangles] the triangles k_mrast_large walks
  DevBuf<uint32_t> counters;         // [kMrWords] the verdict counts, the covered pixels, the list's length
  DevBuf<uint32_t> in;               // staging when the caller's array is host memory
  PhaseStamps<3> stamps;             // around the last call's three kernels
};

// The part of smx_render_params and smx_mesh_render_params that describes the view.
template <typename Params>
int check_view(const Params& p) {
  SMX_CHECK_ARG(p.width > 0 && p.height > 0 && p.width <= 16384 && p.height <= 16384);
  SMX_CHECK_ARG(std::isfinite(p.fx) && std::isfinite(p.fy) && p.fx > 0 && p.fy > 0 && std::isfinite(p.cx) && std::isfinite(p.cy));
  for (int k = 0; k < 12; ++k) SMX_CHECK_ARG(std::isfinite(p.global_T_camera[k]));
  SMX_CHECK_ARG(std::isfinite(p.near_z) && p.near_z > 0 && p.far_z > p.near_z);
  SMX_CHECK_ARG((p.color_flags & ~15) == 0);
  return SMX_OK;
}

// A width x height image of elem-byte elements the kernels can address: rows that hold the width, pitch and address
// multiples of the element.
inline bool image_desc_ok(const smx_buffer_desc* d, int width, int height, size_t elem) {
  return d && d->address && d->width == width && d->height == height && d->pitch >= (size_t)width * elem && d->pitch % elem == 0 &&
         (uintptr_t)d->address % elem == 0;
}
// ... for an output the caller may leave out
inline bool image_desc_ok_or_null(const smx_buffer_desc* d, int width, int height, size_t elem) {
  return !d || image_desc_ok(d, width, height, elem);
}
template <typename T>
Img<T> img_or_null(const smx_buffer_desc* d) { return d ? as_img<T>(d) : Img<T>{nullptr, 0, 0, 0}; }

// Before a render enqueues anything: orders st behind the pipelined regulariser, makes room for px pixels, and orders st
// behind the previous render's resolve, on whatever stream.  A block of the workspace that has to grow -- the z-buffer
// here, or, with `caller_grows`, buffers the caller reserves right after this returns -- may still be in use by that
// render: then, and only then, the device is synchronised first, and the mark cleared.
int render_begin(smx_recon r, hipStream_t st, size_t px, bool caller_grows = false);
// After its last kernel: the mark the next render waits for.
int render_end(smx_recon r, hipStream_t st);

}  // namespace smx
