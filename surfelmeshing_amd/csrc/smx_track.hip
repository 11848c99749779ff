// smx_track.hip -- frame-to-model point-to-plane ICP against the rendered surfel map, without (smx_recon_track) and with a
// photometric term (smx_recon_track_rgbd); the algorithms are stated once, in include/smx.h, and their arithmetic lives in
// smx_track.hpp.  Two kernels per iteration, all iterations of a call enqueued back to back:
//
//   k_track_reduce<STRIDE>       a lane per sampled frame pixel (grid-stride): track_pixel<false> -- projective association,
//                                the two gates, the 31 sums of the normal equations.  Per-pixel terms in float, sums in
//                                double; wavefront reduction by cross-lane shifts, workgroup reduction through LDS, ONE slab
//                                of plain stores per workgroup -- no float atomics, so the sums do not depend on scheduling.
//   k_track_reduce_rgbd<STRIDE>  the same loop and epilogue around track_pixel<true>: one 16-byte gather into P and one
//                                3-byte frame-colour read per associated pixel that passes the distance gate; 33 sums.
//                                A call with colour at weight 0 launches k_track_reduce.
//   k_track_solve                one wavefront: adds the slabs in index order, lane 0 factorises (LDL^T), decides the status,
//                                updates T_rel (closed-form SE(3) exponential) and writes the iteration's record.
//   k_track_photo_prepare        once per call with a weight, a lane per model pixel: P = (L, gx, gy, valid).
//
// Nothing is cleared between iterations: every slab is rewritten by its workgroup, the grid is fixed per level.  A kernel
// that finds a bad status (or its level converged) returns at once; nothing waits on the device.
//
// The entry points are at the end of the file: track_call validates, allocates the workspace (TrackWork, smx_track.hpp),
// renders the model images with smx_recon_render and enqueues the schedule.
#include <algorithm>
#include <cmath>
#include <vector>

#include "smx_recon_state.hpp"

namespace smx {
namespace {

__global__ void k_track_begin(TrackDev* st) {
  for (int k = 0; k < 12; ++k) {
    const double v = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
    st->T_rel[k] = v; st->T_prev[k] = v; st->Tf[k] = (float)v;
  }
  st->status = SMX_TRACK_OK;
  st->iterations_run = 0;
  st->converged_level = -1;
}

__device__ __forceinline__ bool track_skips(const TrackDev* st, int level) {
  return st->status >= SMX_TRACK_TOO_FEW_INLIERS || st->converged_level == level;
}

// The body of both reduce kernels (color, ph and P are not looked at without kPhoto).
template <int STRIDE, bool kPhoto>
__device__ __forceinline__ void track_reduce(TrackK k, TrackPhotoK ph, Img<uint16_t> depth,
                                             Img<float2> normals, Img<uchar3> color, const float* __restrict__ D,
                                             const float4* __restrict__ M, const float4* __restrict__ P,
                                             const TrackDev* __restrict__ st, int level, double* __restrict__ slabs) {
  constexpr int kStride = kPhoto ? kTrackRgbdSlabStride : kTrackSlabStride;
  constexpr int kSums = kPhoto ? SMX_TRACK_RGBD_SUMS : SMX_TRACK_SUMS;
  if (track_skips(st, level)) return;
  float T[12];
  for (int i = 0; i < 12; ++i) T[i] = st->Tf[i];
  double acc[28], acc_ee = 0.0;
  for (int i = 0; i < 28; ++i) acc[i] = 0.0;
  uint32_t n_in = 0, n_px = 0, n_as = 0, n_ph = 0;
  const int n = k.sw * k.sh;
  for (int i = blockIdx.x * kTrackBlock + threadIdx.x; i < n; i += gridDim.x * kTrackBlock) {
    const int sy = i / k.sw, sx = i - sy * k.sw;
    const int x = STRIDE / 2 + sx * STRIDE, y = STRIDE / 2 + sy * STRIDE;
    const unsigned char* rgb = kPhoto ? reinterpret_cast<const unsigned char*>(&color(y, x)) : nullptr;
    track_pixel<kPhoto>(k, ph, T, x, y, depth(y, x), &normals(y, x), rgb, D, M, P, acc, acc_ee, n_in, n_px, n_as, n_ph);
  }
  // wavefront: shifts towards lane 0; workgroup: one row of LDS per wavefront, added in wavefront order
  __shared__ double part[kTrackBlock / 64][kStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 28; ++e) {
    double v = acc[e];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][e] = v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    if (kPhoto) { acc_ee += __shfl_down(acc_ee, off, 64); n_ph += __shfl_down(n_ph, off, 64); }
    n_in += __shfl_down(n_in, off, 64); n_px += __shfl_down(n_px, off, 64);
    n_as += __shfl_down(n_as, off, 64);
  }
  if (lane == 0) {
    part[wave][kSumInliers] = (double)n_in; part[wave][kSumPixels] = (double)n_px;
    part[wave][kSumAssociated] = (double)n_as;
    if (kPhoto) { part[wave][kSumEE] = acc_ee; part[wave][kSumPhotoInliers] = (double)n_ph; }
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double v = part[0][threadIdx.x];
    for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][threadIdx.x];
    slabs[(size_t)blockIdx.x * kStride + threadIdx.x] = v;
  }
}

template <int STRIDE>
__global__ void __launch_bounds__(kTrackBlock)
k_track_reduce(TrackK k, Img<uint16_t> depth, Img<float2> normals, const float* __restrict__ D,
               const float4* __restrict__ M, const TrackDev* __restrict__ st, int level, double* __restrict__ slabs) {
  track_reduce<STRIDE, false>(k, TrackPhotoK(), depth, normals, Img<uchar3>(), D, M, nullptr, st, level, slabs);
}

template <int STRIDE>
__global__ void __launch_bounds__(kTrackBlock)
k_track_reduce_rgbd(TrackK k, TrackPhotoK ph, Img<uint16_t> depth, Img<float2> normals, Img<uchar3> color,
                    const float* __restrict__ D, const float4* __restrict__ M, const float4* __restrict__ P,
                    const TrackDev* __restrict__ st, int level, double* __restrict__ slabs) {
  track_reduce<STRIDE, true>(k, ph, depth, normals, color, D, M, P, st, level, slabs);
}

// (sums [31] and [32] read as 0 without the photometric term, whose slabs are kTrackSlabStride apart)
__global__ void __launch_bounds__(64)
k_track_solve(TrackSolveK k, const double* __restrict__ slabs, TrackDev* st, smx_track_result* out,
              smx_track_rgbd_result* out_rgbd) {
  __shared__ double S[SMX_TRACK_RGBD_SUMS];
  const bool skip = track_skips(st, k.level);
  if (!skip && threadIdx.x < SMX_TRACK_RGBD_SUMS) {
    const int stride = k.photo ? kTrackRgbdSlabStride : kTrackSlabStride;
    double v = 0.0;
    if (threadIdx.x < SMX_TRACK_SUMS || k.photo)
      for (int b = 0; b < k.n_slabs; ++b) v += slabs[(size_t)b * stride + threadIdx.x];   // (index order)
    S[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!skip) track_solve_step(S, k, st);
  if (k.final_launch) {
    track_finish(k, st);
    if (out) *out = st->result.icp;
    if (out_rgbd) *out_rgbd = st->result;
  }
}

__global__ void __launch_bounds__(kTrackBlock)
k_track_photo_prepare(int W, int H, float max_relative_step, const float* __restrict__ D, const uint32_t* __restrict__ Cm,
                      float4* __restrict__ P) {
  const long long i = (long long)blockIdx.x * kTrackBlock + threadIdx.x;
  if (i >= (long long)W * H) return;
  P[i] = track_photo_pixel(W, H, max_relative_step, D, Cm, i);
}

template <int STRIDE>
void launch_reduce(hipStream_t st, int grid, const TrackK& k, const TrackPhotoK* ph, const smx_buffer_desc* depth,
                   const smx_buffer_desc* normals, const smx_buffer_desc* color, const TrackWork& b, int level) {
  if (ph)
    hipLaunchKernelGGL(k_track_reduce_rgbd<STRIDE>, dim3(grid), dim3(kTrackBlock), 0, st, k, *ph, as_img<uint16_t>(depth),
                       as_img<float2>(normals), as_img<uchar3>(color), b.depth.get(), b.normal.get(), b.photo.get(),
                       b.state.get(), level, b.slabs.get());
  else
    hipLaunchKernelGGL(k_track_reduce<STRIDE>, dim3(grid), dim3(kTrackBlock), 0, st, k, as_img<uint16_t>(depth),
                       as_img<float2>(normals), b.depth.get(), b.normal.get(), b.state.get(), level, b.slabs.get());
}

// The constants of one level of the schedule: the reduce kernel's, the solve kernel's, the grid.
struct TrackLevel { TrackK k; TrackSolveK sk; int grid; };

TrackLevel track_level(int l, int W, int H, float fx, float fy, float cx, float cy, float depth_scaling,
                       const float global_T_pred[12], const smx_track_params& p, bool photo) {
  TrackLevel t;
  const int s = p.level_stride[l];
  TrackK& k = t.k;
  k.W = W; k.H = H;
  k.sw = track_samples(W, s); k.sh = track_samples(H, s);
  k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy; k.depth_scaling = depth_scaling;
  k.max_distance_sq = p.max_distance * p.max_distance;
  k.cos_max_angle = (float)cos((double)p.max_normal_angle_deg * (M_PI / 180.0));
  t.grid = track_grid((long long)k.sw * k.sh);
  TrackSolveK& sk = t.sk;
  sk.level = l; sk.stride = s; sk.n_slabs = t.grid; sk.final_launch = 0;
  sk.min_inliers = p.min_inliers; sk.photo = photo ? 1 : 0;
  sk.min_inlier_fraction = p.min_inlier_fraction; sk.min_pivot_ratio = p.min_pivot_ratio;
  sk.convergence_rotation = p.convergence_rotation; sk.convergence_translation = p.convergence_translation;
  for (int i = 0; i < 12; ++i) sk.pred[i] = global_T_pred[i];
  return t;
}

// Enqueues begin + every (reduce, solve) pair of the schedule on st; the last solve launch writes b.state->result and, where
// not null, *result_dev (its .icp) / *result_rgbd_dev (all of it).  q is null for smx_recon_track; with one, p is q->icp,
// color the frame's image, and a weight other than 0 puts one k_track_photo_prepare launch in front and the photometric
// term into the sums (at weight 0 b.color / b.photo are not touched).  Arguments are validated by the caller.
int track_enqueue(hipStream_t st, const TrackWork& b, int W, int H, float fx, float fy, float cx, float cy,
                  float depth_scaling, const smx_buffer_desc* depth, const smx_buffer_desc* normals,
                  const float global_T_pred[12], const smx_track_params& p, smx_track_result* result_dev,
                  const smx_buffer_desc* color, const smx_track_rgbd_params* q, smx_track_rgbd_result* result_rgbd_dev) {
  hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(1), 0, st, b.state.get());
  const bool photo = q && q->photometric_weight != 0.0f;
  TrackPhotoK ph;
  if (photo) {
    hipLaunchKernelGGL(k_track_photo_prepare, dim3((unsigned)div_up((long long)W * H, kTrackBlock)), dim3(kTrackBlock), 0, st,
                       W, H, q->gradient_max_relative_depth_step, b.depth.get(), b.color.get(), b.photo.get());
    ph.weight = q->photometric_weight; ph.max_intensity_difference = q->max_intensity_difference;
    ph.min_gradient_sq = q->min_gradient * q->min_gradient;
  }
  int last_level = -1;
  for (int l = 0; l < kTrackLevels; ++l) if (p.level_iterations[l] > 0) last_level = l;
  for (int l = 0; l < kTrackLevels; ++l) {
    const int iters = p.level_iterations[l];
    if (iters <= 0) continue;
    TrackLevel t = track_level(l, W, H, fx, fy, cx, cy, depth_scaling, global_T_pred, p, photo);
    for (int it = 0; it < iters; ++it) {
      switch (t.sk.stride) {
        case 1: launch_reduce<1>(st, t.grid, t.k, photo ? &ph : nullptr, depth, normals, color, b, l); break;
        case 2: launch_reduce<2>(st, t.grid, t.k, photo ? &ph : nullptr, depth, normals, color, b, l); break;
        case 4: launch_reduce<4>(st, t.grid, t.k, photo ? &ph : nullptr, depth, normals, color, b, l); break;
        default: launch_reduce<8>(st, t.grid, t.k, photo ? &ph : nullptr, depth, normals, color, b, l); break;
      }
      const bool last = l == last_level && it == iters - 1;
      t.sk.final_launch = last ? 1 : 0;
      hipLaunchKernelGGL(k_track_solve, dim3(1), dim3(64), 0, st, t.sk, b.slabs.get(), b.state.get(), last ? result_dev : nullptr,
                         last ? result_rgbd_dev : nullptr);
    }
  }
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

// smx_recon_track (q, color, result_rgbd and model_photo_out null) and smx_recon_track_rgbd (p = &q->icp, result =
// &result_rgbd->icp).
int track_call(smx_recon r, smx_stream s, float depth_scaling, const smx_buffer_desc* depth,
               const smx_buffer_desc* normals, const float global_T_pred[12], const smx_track_params* params,
               smx_track_result* result, int32_t result_on_device, const smx_buffer_desc* model_depth_out,
               const smx_buffer_desc* model_normal_out, const smx_buffer_desc* color,
               const smx_track_rgbd_params* q, smx_track_rgbd_result* result_rgbd,
               const smx_buffer_desc* model_photo_out) {
  SMX_CHECK_ARG(r != nullptr && depth != nullptr && normals != nullptr && global_T_pred != nullptr && params != nullptr &&
                result != nullptr);
  const smx_track_params& p = *params;
  SMX_CHECK_ARG(std::isfinite(depth_scaling) && depth_scaling > 0);
  SMX_CHECK_ARG(image_desc_ok(depth, r->W, r->H, 2) && image_desc_ok(normals, r->W, r->H, 8));
  SMX_CHECK_ARG(image_desc_ok_or_null(model_depth_out, r->W, r->H, 4) && image_desc_ok_or_null(model_normal_out, r->W, r->H, 16));
  for (int k = 0; k < 12; ++k) SMX_CHECK_ARG(std::isfinite(global_T_pred[k]));
  int levels_used = 0;
  for (int l = 0; l < kTrackLevels; ++l) {
    SMX_CHECK_ARG(p.level_iterations[l] >= 0 && p.level_iterations[l] <= kTrackMaxIterationsPerLevel);
    if (p.level_iterations[l] == 0) continue;
    ++levels_used;
    SMX_CHECK_ARG(p.level_stride[l] == 1 || p.level_stride[l] == 2 || p.level_stride[l] == 4 || p.level_stride[l] == 8);
  }
  SMX_CHECK_ARG(levels_used > 0);
  SMX_CHECK_ARG(std::isfinite(p.max_distance) && p.max_distance > 0);
  SMX_CHECK_ARG(p.max_normal_angle_deg > 0 && p.max_normal_angle_deg <= 180.0f);
  SMX_CHECK_ARG(p.convergence_rotation >= 0 && p.convergence_translation >= 0 && p.min_inliers >= 0);
  SMX_CHECK_ARG(p.min_inlier_fraction >= 0 && p.min_inlier_fraction <= 1 && p.min_pivot_ratio >= 0);
  SMX_CHECK_ARG(std::isfinite(p.near_z) && p.near_z > 0 && p.far_z > p.near_z);
  SMX_CHECK_ARG(std::isfinite(p.disc_radius_factor) && p.disc_radius_factor > 0);
  SMX_CHECK_ARG(p.max_splat_extent_in_pixels > 0 && p.max_splat_extent_in_pixels <= 1024);
  if (q) {
    // (3-byte elements: any pitch that holds a row, as smx_recon_integrate takes the image)
    SMX_CHECK_ARG(color != nullptr && color->address && color->width == r->W && color->height == r->H &&
                  color->pitch >= (size_t)r->W * 3);
    SMX_CHECK_ARG(image_desc_ok_or_null(model_photo_out, r->W, r->H, 16));
    SMX_CHECK_ARG(std::isfinite(q->photometric_weight) && q->photometric_weight >= 0);
    SMX_CHECK_ARG(std::isfinite(q->max_intensity_difference) && q->max_intensity_difference > 0);
    SMX_CHECK_ARG(std::isfinite(q->min_gradient) && q->min_gradient >= 0);
    SMX_CHECK_ARG(std::isfinite(q->gradient_max_relative_depth_step) && q->gradient_max_relative_depth_step > 0);
  }
  const bool photo = q && q->photometric_weight != 0.0f;
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  const size_t px = (size_t)r->W * r->H;
  TrackWork& w = r->track;
  // (all or none: a call that fails here leaves nothing behind for the next one to trip over)
  if (!w.state.get()) SMX_CALL(alloc_all(w.depth, px, w.normal, px, w.slabs, (size_t)kTrackMaxSlabs * kTrackRgbdSlabStride, w.state, 1));
  if (q && !w.photo.get()) SMX_CALL(alloc_all(w.color, px, w.photo, px));
  SMX_CALL(w.mark.wait(st));   // (the previous call's kernels, on any stream)
  // the model images: smx_recon_render itself (it orders st behind the pipelined regulariser and the previous render)
  smx_render_params rp;
  memset(&rp, 0, sizeof(rp));
  rp.width = r->W; rp.height = r->H; rp.fx = r->fx; rp.fy = r->fy; rp.cx = r->cx; rp.cy = r->cy;
  for (int k = 0; k < 12; ++k) rp.global_T_camera[k] = global_T_pred[k];
  rp.near_z = p.near_z; rp.far_z = p.far_z; rp.splat_mode = SMX_SPLAT_DISC;
  rp.disc_radius_factor = p.disc_radius_factor; rp.max_splat_extent_in_pixels = p.max_splat_extent_in_pixels;
  rp.surfel_integration_active_window_size = 2147483647;
  smx_buffer_desc dd, nd, cd;
  dd.address = w.depth.get(); dd.height = r->H; dd.width = r->W; dd.pitch = (size_t)r->W * sizeof(float);
  nd.address = w.normal.get(); nd.height = r->H; nd.width = r->W; nd.pitch = (size_t)r->W * sizeof(float4);
  cd.address = w.color.get(); cd.height = r->H; cd.width = r->W; cd.pitch = (size_t)r->W * sizeof(uint32_t);
  SMX_CALL(smx_recon_render(r, s, &rp, &dd, nullptr, &nd, photo ? &cd : nullptr));   // (color_flags 0: the colour row)
  if (model_depth_out)
    SMX_HIP(hipMemcpy2DAsync(model_depth_out->address, model_depth_out->pitch, dd.address, dd.pitch, dd.pitch, (size_t)r->H,
                             hipMemcpyDeviceToDevice, st));
  if (model_normal_out)
    SMX_HIP(hipMemcpy2DAsync(model_normal_out->address, model_normal_out->pitch, nd.address, nd.pitch, nd.pitch, (size_t)r->H,
                             hipMemcpyDeviceToDevice, st));
  SMX_CALL(track_enqueue(st, w, r->W, r->H, r->fx, r->fy, r->cx, r->cy, depth_scaling, depth, normals, global_T_pred, p,
                         result_on_device && !q ? result : nullptr, color, q, result_on_device ? result_rgbd : nullptr));
  if (photo && model_photo_out) {
    const size_t row = (size_t)r->W * sizeof(float4);
    SMX_HIP(hipMemcpy2DAsync(model_photo_out->address, model_photo_out->pitch, w.photo.get(), row, row, (size_t)r->H,
                             hipMemcpyDeviceToDevice, st));
  }
  SMX_CALL(w.mark.record(st));
  w.last_rgbd = q != nullptr;
  if (!result_on_device) {
    const smx_track_rgbd_result* res = &w.state.get()->result;
    if (q) SMX_HIP(hipMemcpyAsync(result_rgbd, res, sizeof(*res), hipMemcpyDeviceToHost, st));
    else SMX_HIP(hipMemcpyAsync(result, &res->icp, sizeof(res->icp), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
  }
  return SMX_OK;
}

// The records of the last tracking call, the first *count of them (at most kTrackRing) copied into recs.
int track_records(smx_recon r, smx_stream s, smx_track_rgbd_iteration* recs, int32_t* count) {
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  *count = 0;
  const TrackWork& w = r->track;
  if (!w.state.get() || !w.mark.busy()) return SMX_OK;
  SMX_CALL(w.mark.wait(st));
  int32_t n = 0;
  SMX_HIP(hipMemcpyAsync(&n, &w.state.get()->iterations_run, sizeof(n), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  n = std::max(0, std::min(n, (int32_t)kTrackRing));
  if (n > 0) {
    SMX_HIP(hipMemcpyAsync(recs, w.state.get()->ring, sizeof(smx_track_rgbd_iteration) * (size_t)n, hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
  }
  *count = n;
  return SMX_OK;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_track_params_default(smx_track_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  const int32_t stride[3] = {4, 2, 1}, iters[3] = {4, 5, 10};
  for (int l = 0; l < 3; ++l) { out->level_stride[l] = stride[l]; out->level_iterations[l] = iters[l]; }
  out->max_distance = 0.10f; out->max_normal_angle_deg = 30.0f;
  out->convergence_rotation = 1e-5f; out->convergence_translation = 1e-5f;
  out->min_inliers = 50; out->min_inlier_fraction = 0.1f; out->min_pivot_ratio = 1e-6f;
  out->near_z = 0.05f; out->far_z = 20.0f; out->disc_radius_factor = 1.0f; out->max_splat_extent_in_pixels = 16.0f;
  return SMX_OK;
}

int smx_track_rgbd_params_default(smx_track_rgbd_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  SMX_CALL(smx_track_params_default(&out->icp));
  out->photometric_weight = 0.1f; out->max_intensity_difference = 0.2f;
  out->min_gradient = 0.02f; out->gradient_max_relative_depth_step = 0.02f;
  return SMX_OK;
}

int smx_recon_track(smx_recon r, smx_stream s, float depth_scaling, const smx_buffer_desc* depth,
                    const smx_buffer_desc* normals, const float global_T_pred[12], const smx_track_params* params,
                    smx_track_result* result, int32_t result_on_device, const smx_buffer_desc* model_depth_out,
                    const smx_buffer_desc* model_normal_out) {
  return track_call(r, s, depth_scaling, depth, normals, global_T_pred, params, result, result_on_device, model_depth_out,
                    model_normal_out, nullptr, nullptr, nullptr, nullptr);
}

int smx_recon_track_rgbd(smx_recon r, smx_stream s, float depth_scaling, const smx_buffer_desc* depth,
                         const smx_buffer_desc* normals, const smx_buffer_desc* color, const float global_T_pred[12],
                         const smx_track_rgbd_params* params, smx_track_rgbd_result* result, int32_t result_on_device,
                         const smx_buffer_desc* model_depth_out, const smx_buffer_desc* model_normal_out,
                         const smx_buffer_desc* model_photo_out) {
  SMX_CHECK_ARG(params != nullptr);
  return track_call(r, s, depth_scaling, depth, normals, global_T_pred, &params->icp, result ? &result->icp : nullptr,
                    result_on_device, model_depth_out, model_normal_out, color, params, result, model_photo_out);
}

int smx_recon_debug_track_rgbd_iterations(smx_recon r, smx_stream s, smx_track_rgbd_iteration* records, int32_t capacity,
                                          int32_t* count) {
  SMX_CHECK_ARG(r != nullptr && count != nullptr && capacity >= 0 && (capacity == 0 || records != nullptr));
  *count = 0;
  if (!r->track.last_rgbd) return SMX_OK;
  std::vector<smx_track_rgbd_iteration> recs(kTrackRing);
  SMX_CALL(track_records(r, s, recs.data(), count));
  std::copy_n(recs.begin(), std::min(*count, capacity), records);
  return SMX_OK;
}

// (the same records without their last two sums, which a call without colour leaves 0)
int smx_recon_debug_track_iterations(smx_recon r, smx_stream s, smx_track_iteration* records, int32_t capacity,
                                     int32_t* count) {
  SMX_CHECK_ARG(r != nullptr && count != nullptr && capacity >= 0 && (capacity == 0 || records != nullptr));
  std::vector<smx_track_rgbd_iteration> recs(kTrackRing);
  SMX_CALL(track_records(r, s, recs.data(), count));
  for (int32_t i = 0; i < std::min(*count, capacity); ++i) {
    const smx_track_rgbd_iteration& f = recs[i];
    smx_track_iteration& t = records[i];
    t.level = f.level; t.stride = f.stride; t.status = f.status; t.reserved = f.reserved;
    std::copy_n(f.sums, SMX_TRACK_SUMS, t.sums);
    std::copy_n(f.x, 6, t.x);
  }
  return SMX_OK;
}

}  // extern "C"
