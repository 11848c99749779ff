// smx_track.hip -- frame-to-model point-to-plane ICP against the rendered surfel map (smx_recon_track; the algorithm
// is stated once, in include/smx.h).  Two kernels per iteration, all iterations of a call enqueued back to back:
//
//   k_track_reduce<STRIDE>  a lane per sampled frame pixel (grid-stride): projective association, the two gates, the
//                           31 sums of the normal equations.  Per-pixel terms in float, sums in double; wavefront
//                           reduction by cross-lane shifts, workgroup reduction through LDS, ONE slab of plain stores per
//                           workgroup -- no float atomics, so the sums do not depend on scheduling.
//   k_track_solve           one wavefront: adds the slabs in index order, lane 0 factorises (LDL^T), decides the status,
//                           updates T_rel (closed-form SE(3) exponential) and writes the iteration's record.
//
// Nothing is cleared between iterations: every slab is rewritten by its workgroup, the grid is fixed per level.  A kernel
// that finds a bad status (or its level converged) returns at once; nothing waits on the device.
// smx_recon_track_rgbd (the photometric term on top; further down): k_track_photo_prepare once per call, then
// k_track_reduce_rgbd<STRIDE> and k_track_solve_rgbd in the place of the two above.
#include "smx_track.hpp"

#include <math.h>

#include <algorithm>

namespace smx {
namespace {

constexpr int kTrackBlock = 256;
constexpr int kTrackPixelsPerLane = 8;    // sampled pixels a lane visits before the grid is widened
enum { kSumRR = 27, kSumInliers = 28, kSumPixels = 29, kSumAssociated = 30 };

struct TrackK {
  int W, H, sw, sh;          // image size; sampled columns / rows at this stride
  float fx, fy, cx, cy;
  float depth_scaling;
  float max_distance_sq, cos_max_angle;
};

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

template <int STRIDE>
__global__ void __launch_bounds__(kTrackBlock)
k_track_reduce(TrackK k, Img<uint16_t> depth, Img<float2> normals, const float* __restrict__ D,
               const float4* __restrict__ M, const TrackDev* __restrict__ st, int level, double* __restrict__ slabs) {
  if (track_skips(st, level)) return;
  float T[12];
  for (int i = 0; i < 12; ++i) T[i] = st->Tf[i];
  double acc[28];
  for (int i = 0; i < 28; ++i) acc[i] = 0.0;
  uint32_t n_in = 0, n_px = 0, n_as = 0;
  const int n = k.sw * k.sh;
  for (int i = blockIdx.x * kTrackBlock + threadIdx.x; i < n; i += gridDim.x * kTrackBlock) {
    const int sy = i / k.sw, sx = i - sy * k.sw;
    const int x = STRIDE / 2 + sx * STRIDE, y = STRIDE / 2 + sy * STRIDE;
    const uint16_t du = depth(y, x);
    if (du == 0) continue;
    ++n_px;
    const float2 nxy = normals(y, x);
    const float z = (float)du / k.depth_scaling;
    const float vx = z * (((float)x + 0.5f - k.cx) / k.fx), vy = z * (((float)y + 0.5f - k.cy) / k.fy);
    const float nz = -sqrtf(fmaxf(0.0f, 1.0f - nxy.x * nxy.x - nxy.y * nxy.y));
    const float px = T[0] * vx + T[1] * vy + T[2] * z + T[3];
    const float py = T[4] * vx + T[5] * vy + T[6] * z + T[7];
    const float pz = T[8] * vx + T[9] * vy + T[10] * z + T[11];
    if (!(pz > 0.0f)) continue;
    const float uf = floorf(k.fx * px / pz + k.cx), wf = floorf(k.fy * py / pz + k.cy);
    if (!(uf >= 0.0f && uf < (float)k.W && wf >= 0.0f && wf < (float)k.H)) continue;
    const int u = (int)uf, w = (int)wf;
    const size_t mi = (size_t)w * k.W + u;
    const float Dq = D[mi];
    if (!(Dq > 0.0f)) continue;
    ++n_as;
    const float4 Mq = M[mi];
    const float qx = Dq * ((uf + 0.5f - k.cx) / k.fx), qy = Dq * ((wf + 0.5f - k.cy) / k.fy);
    const float dx = px - qx, dy = py - qy, dz = pz - Dq;
    if (!(dx * dx + dy * dy + dz * dz <= k.max_distance_sq)) continue;
    const float mx = T[0] * nxy.x + T[1] * nxy.y + T[2] * nz;
    const float my = T[4] * nxy.x + T[5] * nxy.y + T[6] * nz;
    const float mz = T[8] * nxy.x + T[9] * nxy.y + T[10] * nz;
    if (!(mx * Mq.x + my * Mq.y + mz * Mq.z >= k.cos_max_angle)) continue;
    ++n_in;
    const float r = Mq.x * dx + Mq.y * dy + Mq.z * dz;
    float J[6];
    J[0] = py * Mq.z - pz * Mq.y;
    J[1] = pz * Mq.x - px * Mq.z;
    J[2] = px * Mq.y - py * Mq.x;
    J[3] = Mq.x; J[4] = Mq.y; J[5] = Mq.z;
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) acc[e++] += (double)(J[a] * J[b]);
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += (double)(J[a] * r);
    acc[kSumRR] += (double)(r * r);
  }
  // wavefront: shifts towards lane 0; workgroup: one row of LDS per wavefront, added in wavefront order
  __shared__ double part[kTrackBlock / 64][kTrackSlabStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 28; ++e) {
    double v = acc[e];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][e] = v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    n_in += __shfl_down(n_in, off, 64); n_px += __shfl_down(n_px, off, 64); n_as += __shfl_down(n_as, off, 64);
  }
  if (lane == 0) {
    part[wave][kSumInliers] = (double)n_in; part[wave][kSumPixels] = (double)n_px; part[wave][kSumAssociated] = (double)n_as;
  }
  __syncthreads();
  if (threadIdx.x < SMX_TRACK_SUMS) {
    double v = part[0][threadIdx.x];
    for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][threadIdx.x];
    slabs[(size_t)blockIdx.x * kTrackSlabStride + threadIdx.x] = v;
  }
}

struct TrackSolveK {
  int level, stride, n_slabs, final_launch;
  int min_inliers;
  double min_inlier_fraction, min_pivot_ratio, convergence_rotation, convergence_translation;
  double pred[12];
};

// exp of the twist x = (w, u) as a row-major 3x4: R = I + A K + B K^2, t = (I + B K + C K^2) u with K = [w]x
__device__ void se3_exp(const double* x, double* E) {
  const double wx = x[0], wy = x[1], wz = x[2];
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double A, B, Cc;
  if (th < 1e-6) {
    A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; Cc = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double sh = sin(0.5 * th);
    A = sin(th) / th; B = 2.0 * sh * sh / th2; Cc = (th - sin(th)) / (th2 * th);
  }
  const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double K2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
  for (int i = 0; i < 3; ++i) {
    double t = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double id = i == j ? 1.0 : 0.0;
      E[4 * i + j] = id + A * K[3 * i + j] + B * K2[3 * i + j];
      t += (id + B * K[3 * i + j] + Cc * K2[3 * i + j]) * x[3 + j];
    }
    E[4 * i + 3] = t;
  }
}

// C = A B for row-major 3x4 rigid transforms
__device__ void se3_mul(const double* A, const double* B, double* Cm) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) {
      double v = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
      if (j == 3) v += A[4 * i + 3];
      Cm[4 * i + j] = v;
    }
  }
}

// One iteration's decision and update (lane 0).  Returns the status after it; x is zero where nothing was solved.
__device__ int track_solve_one(const double* S, const TrackSolveK& k, TrackDev* st, double* x) {
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  for (int i = 0; i < SMX_TRACK_SUMS; ++i)
    if (!isfinite(S[i])) return SMX_TRACK_NOT_FINITE;
  if (S[kSumPixels] > 0.0 && S[kSumAssociated] == 0.0) return SMX_TRACK_DEGENERATE;
  if (S[kSumInliers] < (double)k.min_inliers) return SMX_TRACK_TOO_FEW_INLIERS;
  double A[6][6], L[6][6], d[6], b[6];
  {
    int e = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) { A[i][j] = S[e]; A[j][i] = S[e]; ++e; }
  }
  double max_diag = 0.0;
  for (int i = 0; i < 6; ++i) { b[i] = -S[21 + i]; max_diag = fmax(max_diag, A[i][i]); }
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j];
    for (int m = 0; m < j; ++m) dj -= L[j][m] * L[j][m] * d[m];
    if (!(dj >= k.min_pivot_ratio * max_diag) || !(dj > 0.0)) return SMX_TRACK_DEGENERATE;
    d[j] = dj;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int m = 0; m < j; ++m) v -= L[i][m] * L[j][m] * d[m];
      L[i][j] = v / dj;
    }
  }
  double y[6], sol[6];
  for (int i = 0; i < 6; ++i) { double v = b[i]; for (int m = 0; m < i; ++m) v -= L[i][m] * y[m]; y[i] = v; }
  for (int i = 5; i >= 0; --i) { double v = y[i] / d[i]; for (int m = i + 1; m < 6; ++m) v -= L[m][i] * sol[m]; sol[i] = v; }
  for (int i = 0; i < 6; ++i)
    if (!isfinite(sol[i])) return SMX_TRACK_NOT_FINITE;
  // (the twist corrects the pose the reduce kernel linearised at: T_rel as the 12 floats it read)
  double E[12], Tl[12], Tn[12];
  se3_exp(sol, E);
  for (int i = 0; i < 12; ++i) Tl[i] = (double)st->Tf[i];
  se3_mul(E, Tl, Tn);
  for (int i = 0; i < 12; ++i)
    if (!isfinite(Tn[i])) return SMX_TRACK_NOT_FINITE;
  for (int i = 0; i < 6; ++i) x[i] = sol[i];
  for (int i = 0; i < 12; ++i) { st->T_prev[i] = st->T_rel[i]; st->T_rel[i] = Tn[i]; st->Tf[i] = (float)Tn[i]; }
  const double rot = sqrt(sol[0] * sol[0] + sol[1] * sol[1] + sol[2] * sol[2]);
  const double tra = sqrt(sol[3] * sol[3] + sol[4] * sol[4] + sol[5] * sol[5]);
  return (rot < k.convergence_rotation && tra < k.convergence_translation) ? SMX_TRACK_CONVERGED : SMX_TRACK_OK;
}

// The end of the call (lane 0 of the last solve launch): the fraction test on the last iteration run, the pose, the result.
__device__ void track_finish(const TrackSolveK& k, TrackDev* st, smx_track_result* out) {
  smx_track_result res;
  const int n = st->iterations_run;
  int status = st->status;
  const smx_track_iteration* rec = n > 0 ? &st->ring[n - 1] : nullptr;
  if (rec && status < SMX_TRACK_TOO_FEW_INLIERS &&
      rec->sums[kSumInliers] < k.min_inlier_fraction * rec->sums[kSumPixels]) {
    status = SMX_TRACK_TOO_FEW_INLIERS;
    for (int i = 0; i < 12; ++i) { st->T_rel[i] = st->T_prev[i]; st->Tf[i] = (float)st->T_prev[i]; }
    st->status = status;
  }
  // (nothing solved, T_rel still the identity: the prediction itself, bit for bit -- signs of zeros included)
  bool identity = true;
  for (int i = 0; i < 12; ++i) identity = identity && st->T_rel[i] == ((i == 0 || i == 5 || i == 10) ? 1.0 : 0.0);
  double G[12];
  if (identity) { for (int i = 0; i < 12; ++i) G[i] = k.pred[i]; } else se3_mul(k.pred, st->T_rel, G);
  for (int i = 0; i < 12; ++i) res.global_T_frame[i] = (float)G[i];
  res.status = status;
  res.iterations_run = n;
  res.inliers = rec ? (uint32_t)rec->sums[kSumInliers] : 0u;
  res.pixels_with_depth = rec ? (uint32_t)rec->sums[kSumPixels] : 0u;
  res.rms_residual = (rec && rec->sums[kSumInliers] > 0.0) ? (float)sqrt(rec->sums[kSumRR] / rec->sums[kSumInliers]) : 0.0f;
  res.last_update_rotation = rec ? (float)sqrt(rec->x[0] * rec->x[0] + rec->x[1] * rec->x[1] + rec->x[2] * rec->x[2]) : 0.0f;
  res.last_update_translation = rec ? (float)sqrt(rec->x[3] * rec->x[3] + rec->x[4] * rec->x[4] + rec->x[5] * rec->x[5]) : 0.0f;
  {
    int e = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) {
        const float v = rec ? (float)rec->sums[e] : 0.0f;
        res.information[6 * i + j] = v; res.information[6 * j + i] = v; ++e;
      }
  }
  st->result = res;
  if (out) *out = res;
}

__global__ void __launch_bounds__(64)
k_track_solve(TrackSolveK k, const double* __restrict__ slabs, TrackDev* st, smx_track_result* out) {
  __shared__ double S[kTrackSlabStride];
  const bool skip = track_skips(st, k.level);
  if (!skip) {
    if (threadIdx.x < SMX_TRACK_SUMS) {
      double v = 0.0;
      for (int b = 0; b < k.n_slabs; ++b) v += slabs[(size_t)b * kTrackSlabStride + threadIdx.x];   // (index order)
      S[threadIdx.x] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!skip) {
    double x[6];
    const int status = track_solve_one(S, k, st, x);
    const int slot = st->iterations_run;
    if (slot < kTrackRing) {
      smx_track_iteration& rec = st->ring[slot];
      rec.level = k.level; rec.stride = k.stride; rec.status = status; rec.reserved = 0;
      for (int i = 0; i < SMX_TRACK_SUMS; ++i) rec.sums[i] = S[i];
      for (int i = 0; i < 6; ++i) rec.x[i] = x[i];
      st->iterations_run = slot + 1;
    }
    st->status = status;
    if (status == SMX_TRACK_CONVERGED) st->converged_level = k.level;
  }
  if (k.final_launch) track_finish(k, st, out);
}

// ---- tracking with colour (smx_recon_track_rgbd): the photometric term on top of the above ----------------------------
//
//   k_track_photo_prepare    once per call, a lane per model pixel: P = (L, gx, gy, valid) from the colour and depth renders
//   k_track_reduce_rgbd<S>   the body of k_track_reduce plus the term: one 16-byte gather into P and one 3-byte frame-colour
//                            read per associated pixel that passes the distance gate; 33 sums, slabs of their own
//   k_track_solve_rgbd       k_track_solve on the first 31 sums (track_solve_one, track_finish), the finiteness of the two
//                            others, both rings
enum { kSumEE = 31, kSumPhotoInliers = 32 };

struct TrackPhotoK {
  float weight, max_intensity_difference, min_gradient_sq;
};

__device__ __forceinline__ float track_luma(float r, float g, float b) {
  return ((0.299f * r + 0.587f * g) + 0.114f * b) * (1.0f / 255.0f);
}
__device__ __forceinline__ float track_luma_u32(uint32_t c) {
  return track_luma((float)(c & 255u), (float)((c >> 8) & 255u), (float)((c >> 16) & 255u));
}

__global__ void __launch_bounds__(kTrackBlock)
k_track_photo_prepare(int W, int H, float max_relative_step, const float* __restrict__ D, const uint32_t* __restrict__ Cm,
                      float4* __restrict__ P) {
  const long long i = (long long)blockIdx.x * kTrackBlock + threadIdx.x;
  if (i >= (long long)W * H) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const float d = D[i];
  float gx = 0.0f, gy = 0.0f, valid = 0.0f;
  if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && d > 0.0f) {
    const float dl = D[i - 1], dr = D[i + 1], du = D[i - W], dd = D[i + W];
    const float lim = max_relative_step * d;
    if (dl > 0.0f && dr > 0.0f && du > 0.0f && dd > 0.0f && fabsf(dl - d) <= lim && fabsf(dr - d) <= lim &&
        fabsf(du - d) <= lim && fabsf(dd - d) <= lim) {
      gx = 0.5f * (track_luma_u32(Cm[i + 1]) - track_luma_u32(Cm[i - 1]));
      gy = 0.5f * (track_luma_u32(Cm[i + W]) - track_luma_u32(Cm[i - W]));
      valid = 1.0f;
    }
  }
  P[i] = make_float4(track_luma_u32(Cm[i]), gx, gy, valid);
}

// (P == nullptr: weight 0 -- the geometric sums alone, by the same operations in the same order as k_track_reduce)
template <int STRIDE>
__global__ void __launch_bounds__(kTrackBlock)
k_track_reduce_rgbd(TrackK k, TrackPhotoK ph, Img<uint16_t> depth, Img<float2> normals, Img<uchar3> color,
                    const float* __restrict__ D, const float4* __restrict__ M, const float4* __restrict__ P,
                    const TrackDev* __restrict__ st, int level, double* __restrict__ slabs) {
  if (track_skips(st, level)) return;
  float T[12];
  for (int i = 0; i < 12; ++i) T[i] = st->Tf[i];
  double acc[28];
  for (int i = 0; i < 28; ++i) acc[i] = 0.0;
  double acc_ee = 0.0;
  uint32_t n_in = 0, n_px = 0, n_as = 0, n_ph = 0;
  const int n = k.sw * k.sh;
  for (int i = blockIdx.x * kTrackBlock + threadIdx.x; i < n; i += gridDim.x * kTrackBlock) {
    const int sy = i / k.sw, sx = i - sy * k.sw;
    const int x = STRIDE / 2 + sx * STRIDE, y = STRIDE / 2 + sy * STRIDE;
    const uint16_t du = depth(y, x);
    if (du == 0) continue;
    ++n_px;
    const float2 nxy = normals(y, x);
    const float z = (float)du / k.depth_scaling;
    const float vx = z * (((float)x + 0.5f - k.cx) / k.fx), vy = z * (((float)y + 0.5f - k.cy) / k.fy);
    const float nz = -sqrtf(fmaxf(0.0f, 1.0f - nxy.x * nxy.x - nxy.y * nxy.y));
    const float px = T[0] * vx + T[1] * vy + T[2] * z + T[3];
    const float py = T[4] * vx + T[5] * vy + T[6] * z + T[7];
    const float pz = T[8] * vx + T[9] * vy + T[10] * z + T[11];
    if (!(pz > 0.0f)) continue;
    const float uc = k.fx * px / pz + k.cx, wc = k.fy * py / pz + k.cy;
    const float uf = floorf(uc), wf = floorf(wc);
    if (!(uf >= 0.0f && uf < (float)k.W && wf >= 0.0f && wf < (float)k.H)) continue;
    const int u = (int)uf, w = (int)wf;
    const size_t mi = (size_t)w * k.W + u;
    const float Dq = D[mi];
    if (!(Dq > 0.0f)) continue;
    ++n_as;
    const float4 Mq = M[mi];
    const float qx = Dq * ((uf + 0.5f - k.cx) / k.fx), qy = Dq * ((wf + 0.5f - k.cy) / k.fy);
    const float dx = px - qx, dy = py - qy, dz = pz - Dq;
    if (!(dx * dx + dy * dy + dz * dz <= k.max_distance_sq)) continue;
    const float mx = T[0] * nxy.x + T[1] * nxy.y + T[2] * nz;
    const float my = T[4] * nxy.x + T[5] * nxy.y + T[6] * nz;
    const float mz = T[8] * nxy.x + T[9] * nxy.y + T[10] * nz;
    if (mx * Mq.x + my * Mq.y + mz * Mq.z >= k.cos_max_angle) {
      ++n_in;
      const float r = Mq.x * dx + Mq.y * dy + Mq.z * dz;
      float J[6];
      J[0] = py * Mq.z - pz * Mq.y;
      J[1] = pz * Mq.x - px * Mq.z;
      J[2] = px * Mq.y - py * Mq.x;
      J[3] = Mq.x; J[4] = Mq.y; J[5] = Mq.z;
      int e = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) acc[e++] += (double)(J[a] * J[b]);
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[21 + a] += (double)(J[a] * r);
      acc[kSumRR] += (double)(r * r);
    }
    if (P == nullptr) continue;
    const float4 Pq = P[mi];
    const uchar3 cf = color(y, x);
    const float Lm = (Pq.x + Pq.y * (uc - (uf + 0.5f))) + Pq.z * (wc - (wf + 0.5f));
    const float ei = Lm - track_luma((float)cf.x, (float)cf.y, (float)cf.z);
    if (!(Pq.w != 0.0f && Pq.y * Pq.y + Pq.z * Pq.z >= ph.min_gradient_sq && fabsf(ei) <= ph.max_intensity_difference)) continue;
    ++n_ph;
    const float gfx = Pq.y * k.fx, gfy = Pq.z * k.fy;
    const float a0 = gfx / pz, a1 = gfy / pz, a2 = -((gfx * px + gfy * py) / (pz * pz));
    float K[6];
    K[0] = ph.weight * (py * a2 - pz * a1);
    K[1] = ph.weight * (pz * a0 - px * a2);
    K[2] = ph.weight * (px * a1 - py * a0);
    K[3] = ph.weight * a0; K[4] = ph.weight * a1; K[5] = ph.weight * a2;
    const float se = ph.weight * ei;
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) acc[e++] += (double)(K[a] * K[b]);
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += (double)(K[a] * se);
    acc_ee += (double)(ei * ei);
  }
  // the same lane -> wavefront -> workgroup -> slab order as k_track_reduce
  __shared__ double part[kTrackBlock / 64][kTrackRgbdSlabStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 28; ++e) {
    double v = acc[e];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][e] = v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    acc_ee += __shfl_down(acc_ee, off, 64);
    n_in += __shfl_down(n_in, off, 64); n_px += __shfl_down(n_px, off, 64); n_as += __shfl_down(n_as, off, 64);
    n_ph += __shfl_down(n_ph, off, 64);
  }
  if (lane == 0) {
    part[wave][kSumInliers] = (double)n_in; part[wave][kSumPixels] = (double)n_px; part[wave][kSumAssociated] = (double)n_as;
    part[wave][kSumEE] = acc_ee; part[wave][kSumPhotoInliers] = (double)n_ph;
  }
  __syncthreads();
  if (threadIdx.x < SMX_TRACK_RGBD_SUMS) {
    double v = part[0][threadIdx.x];
    for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][threadIdx.x];
    slabs[(size_t)blockIdx.x * kTrackRgbdSlabStride + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(64)
k_track_solve_rgbd(TrackSolveK k, const double* __restrict__ slabs, TrackDev* st, TrackRgbdDev* rst,
                   smx_track_rgbd_result* out) {
  __shared__ double S[kTrackRgbdSlabStride];
  const bool skip = track_skips(st, k.level);
  if (!skip) {
    if (threadIdx.x < SMX_TRACK_RGBD_SUMS) {
      double v = 0.0;
      for (int b = 0; b < k.n_slabs; ++b) v += slabs[(size_t)b * kTrackRgbdSlabStride + threadIdx.x];   // (index order)
      S[threadIdx.x] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!skip) {
    double x[6];
    int status;
    if (!isfinite(S[kSumEE]) || !isfinite(S[kSumPhotoInliers])) {
      status = SMX_TRACK_NOT_FINITE;
      for (int i = 0; i < 6; ++i) x[i] = 0.0;
    } else {
      status = track_solve_one(S, k, st, x);
    }
    const int slot = st->iterations_run;
    if (slot < kTrackRing) {
      smx_track_iteration& rec = st->ring[slot];
      smx_track_rgbd_iteration& rec2 = rst->ring[slot];
      rec.level = k.level; rec.stride = k.stride; rec.status = status; rec.reserved = 0;
      rec2.level = k.level; rec2.stride = k.stride; rec2.status = status; rec2.reserved = 0;
      for (int i = 0; i < SMX_TRACK_SUMS; ++i) rec.sums[i] = S[i];
      for (int i = 0; i < SMX_TRACK_RGBD_SUMS; ++i) rec2.sums[i] = S[i];
      for (int i = 0; i < 6; ++i) { rec.x[i] = x[i]; rec2.x[i] = x[i]; }
      st->iterations_run = slot + 1;
    }
    st->status = status;
    if (status == SMX_TRACK_CONVERGED) st->converged_level = k.level;
  }
  if (k.final_launch) {
    track_finish(k, st, nullptr);
    const int n = st->iterations_run;
    const double ee = n > 0 ? rst->ring[n - 1].sums[kSumEE] : 0.0, np = n > 0 ? rst->ring[n - 1].sums[kSumPhotoInliers] : 0.0;
    smx_track_rgbd_result* res = &rst->result;   // (filled in place: no copy of the struct through scratch)
    res->icp = st->result;
    res->photometric_inliers = (uint32_t)np;
    res->rms_intensity_residual = np > 0.0 ? (float)sqrt(ee / np) : 0.0f;
    if (out) *out = *res;
  }
}

template <int STRIDE>
void launch_reduce_rgbd(hipStream_t st, int grid, const TrackK& k, const TrackPhotoK& ph, const smx_buffer_desc* depth,
                        const smx_buffer_desc* normals, const smx_buffer_desc* color, const TrackRgbdBuffers& b,
                        const float4* photo, int level) {
  hipLaunchKernelGGL(k_track_reduce_rgbd<STRIDE>, dim3(grid), dim3(kTrackBlock), 0, st, k, ph, as_img<uint16_t>(depth),
                     as_img<float2>(normals), as_img<uchar3>(color), b.icp.model_depth, b.icp.model_normal, photo,
                     b.icp.state, level, b.slabs);
}

template <int STRIDE>
void launch_reduce(hipStream_t st, int grid, const TrackK& k, const smx_buffer_desc* depth, const smx_buffer_desc* normals,
                   const TrackBuffers& b, int level) {
  hipLaunchKernelGGL(k_track_reduce<STRIDE>, dim3(grid), dim3(kTrackBlock), 0, st, k, as_img<uint16_t>(depth),
                     as_img<float2>(normals), b.model_depth, b.model_normal, b.state, level, b.slabs);
}

// The constants of one level of the schedule: the reduce kernel's, the solve kernel's, the grid.
struct TrackLevel { TrackK k; TrackSolveK sk; int grid; };

TrackLevel track_level(int l, int W, int H, float fx, float fy, float cx, float cy, float depth_scaling,
                       const float global_T_pred[12], const smx_track_params& p) {
  TrackLevel t;
  const int s = p.level_stride[l];
  TrackK& k = t.k;
  k.W = W; k.H = H;
  k.sw = W > s / 2 ? (W - s / 2 + s - 1) / s : 0;
  k.sh = H > s / 2 ? (H - s / 2 + s - 1) / s : 0;
  k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy; k.depth_scaling = depth_scaling;
  k.max_distance_sq = p.max_distance * p.max_distance;
  k.cos_max_angle = (float)cos((double)p.max_normal_angle_deg * (M_PI / 180.0));
  const long long n = (long long)k.sw * k.sh;
  t.grid = (int)std::min<long long>(std::max<long long>(div_up(n, kTrackBlock * kTrackPixelsPerLane), 1), kTrackMaxSlabs);
  TrackSolveK& sk = t.sk;
  sk.level = l; sk.stride = s; sk.n_slabs = t.grid; sk.final_launch = 0;
  sk.min_inliers = p.min_inliers;
  sk.min_inlier_fraction = p.min_inlier_fraction; sk.min_pivot_ratio = p.min_pivot_ratio;
  sk.convergence_rotation = p.convergence_rotation; sk.convergence_translation = p.convergence_translation;
  for (int i = 0; i < 12; ++i) sk.pred[i] = global_T_pred[i];
  return t;
}

int track_last_level(const smx_track_params& p) {
  int last_level = -1;
  for (int l = 0; l < kTrackLevels; ++l) if (p.level_iterations[l] > 0) last_level = l;
  return last_level;
}

}  // namespace

int track_enqueue(hipStream_t st, const TrackBuffers& b, int W, int H, float fx, float fy, float cx, float cy,
                  float depth_scaling, const smx_buffer_desc* depth, const smx_buffer_desc* normals,
                  const float global_T_pred[12], const smx_track_params& p, smx_track_result* result_dev) {
  hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(1), 0, st, b.state);
  const int last_level = track_last_level(p);
  for (int l = 0; l < kTrackLevels; ++l) {
    const int iters = p.level_iterations[l];
    if (iters <= 0) continue;
    TrackLevel t = track_level(l, W, H, fx, fy, cx, cy, depth_scaling, global_T_pred, p);
    for (int it = 0; it < iters; ++it) {
      switch (t.sk.stride) {
        case 1: launch_reduce<1>(st, t.grid, t.k, depth, normals, b, l); break;
        case 2: launch_reduce<2>(st, t.grid, t.k, depth, normals, b, l); break;
        case 4: launch_reduce<4>(st, t.grid, t.k, depth, normals, b, l); break;
        default: launch_reduce<8>(st, t.grid, t.k, depth, normals, b, l); break;
      }
      t.sk.final_launch = (l == last_level && it == iters - 1) ? 1 : 0;
      hipLaunchKernelGGL(k_track_solve, dim3(1), dim3(64), 0, st, t.sk, b.slabs, b.state, t.sk.final_launch ? result_dev : nullptr);
    }
  }
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int track_rgbd_enqueue(hipStream_t st, const TrackRgbdBuffers& b, int W, int H, float fx, float fy, float cx, float cy,
                       float depth_scaling, const smx_buffer_desc* depth, const smx_buffer_desc* normals,
                       const smx_buffer_desc* color, const float global_T_pred[12], const smx_track_rgbd_params& p,
                       smx_track_rgbd_result* result_dev) {
  hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(1), 0, st, b.icp.state);
  const bool photo = p.photometric_weight != 0.0f;
  if (photo)
    hipLaunchKernelGGL(k_track_photo_prepare, dim3((unsigned)div_up((long long)W * H, kTrackBlock)), dim3(kTrackBlock), 0, st,
                       W, H, p.gradient_max_relative_depth_step, b.icp.model_depth, b.model_color, b.model_photo);
  TrackPhotoK ph;
  ph.weight = p.photometric_weight; ph.max_intensity_difference = p.max_intensity_difference;
  ph.min_gradient_sq = p.min_gradient * p.min_gradient;
  const float4* P = photo ? b.model_photo : nullptr;
  const int last_level = track_last_level(p.icp);
  for (int l = 0; l < kTrackLevels; ++l) {
    const int iters = p.icp.level_iterations[l];
    if (iters <= 0) continue;
    TrackLevel t = track_level(l, W, H, fx, fy, cx, cy, depth_scaling, global_T_pred, p.icp);
    for (int it = 0; it < iters; ++it) {
      switch (t.sk.stride) {
        case 1: launch_reduce_rgbd<1>(st, t.grid, t.k, ph, depth, normals, color, b, P, l); break;
        case 2: launch_reduce_rgbd<2>(st, t.grid, t.k, ph, depth, normals, color, b, P, l); break;
        case 4: launch_reduce_rgbd<4>(st, t.grid, t.k, ph, depth, normals, color, b, P, l); break;
        default: launch_reduce_rgbd<8>(st, t.grid, t.k, ph, depth, normals, color, b, P, l); break;
      }
      t.sk.final_launch = (l == last_level && it == iters - 1) ? 1 : 0;
      hipLaunchKernelGGL(k_track_solve_rgbd, dim3(1), dim3(64), 0, st, t.sk, b.slabs, b.icp.state, b.state,
                         t.sk.final_launch ? result_dev : nullptr);
    }
  }
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

}  // namespace smx

extern "C" int smx_track_params_default(smx_track_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  const int32_t stride[3] = {4, 2, 1}, iters[3] = {4, 5, 10};
  for (int l = 0; l < 3; ++l) { out->level_stride[l] = stride[l]; out->level_iterations[l] = iters[l]; }
  out->max_distance = 0.10f; out->max_normal_angle_deg = 30.0f;
  out->convergence_rotation = 1e-5f; out->convergence_translation = 1e-5f;
  out->min_inliers = 50; out->min_inlier_fraction = 0.1f; out->min_pivot_ratio = 1e-6f;
  out->near_z = 0.05f; out->far_z = 20.0f; out->disc_radius_factor = 1.0f; out->max_splat_extent_in_pixels = 16.0f;
  return SMX_OK;
}

extern "C" int smx_track_rgbd_params_default(smx_track_rgbd_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  SMX_CALL(smx_track_params_default(&out->icp));
  out->photometric_weight = 0.1f; out->max_intensity_difference = 0.2f;
  out->min_gradient = 0.02f; out->gradient_max_relative_depth_step = 0.02f;
  return SMX_OK;
}
