// smx_track.hpp -- camera tracking against the rendered map (smx_recon_track, smx_recon_track_rgbd).
//
// Part 1: the arithmetic as plain inline functions -- one sampled pixel's contribution to the sums (with and without the
// photometric term), the prepare kernel's pixel, the solve, the SE(3) exponential, the end of a call, and the launch rule of
// the reduce kernel (workgroup size, grid, slab strides).  smx_track.hip calls them from its kernels; a test compiles this
// part alone for the host (SMX_TRACK_HOST_ONLY) and runs the same functions in the launch's order.
// Part 2: the workspace the object keeps for the calls (its glue is in smx_track.hip).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(SMX_TRACK_HOST_ONLY)
#include "smx.h"
#define SMX_TRACK_FN static inline
namespace smx {   // (the two vector types of the device images, as the host sees them)
struct alignas(8) float2 { float x, y; };
struct alignas(16) float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
}  // namespace smx
#else
#include "smx_common.hpp"
#define SMX_TRACK_FN __host__ __device__ __forceinline__
#endif

namespace smx {

constexpr int kTrackLevels = 3;
constexpr int kTrackMaxIterationsPerLevel = 32;
constexpr int kTrackRing = kTrackLevels * kTrackMaxIterationsPerLevel;   // one record per iteration of a call
enum { kSumRR = 27, kSumInliers = 28, kSumPixels = 29, kSumAssociated = 30, kSumEE = 31, kSumPhotoInliers = 32 };

// Device-resident state of one call of either kind.  Written by k_track_begin and by lane 0 of k_track_solve only.
struct TrackDev {
  double T_rel[12];       // model camera <- frame camera, row-major 3x4
  double T_prev[12];      // ... before the update of the last iteration run
  float Tf[12];           // T_rel rounded to float: what the reduce kernel of the next iteration reads
  int32_t status;         // SMX_TRACK_*; a bad one is sticky
  int32_t iterations_run; // iterations that produced sums (the one that raised a bad status included)
  int32_t converged_level;// level whose remaining iterations are skipped, -1 = none
  int32_t pad;
  smx_track_rgbd_result result;             // (.icp is the whole result of a call without colour)
  smx_track_rgbd_iteration ring[kTrackRing];// (sums [31] and [32] are 0 where no photometric term ran)
};

struct TrackK {
  int W, H, sw, sh;          // image size; sampled columns / rows at this stride
  float fx, fy, cx, cy;
  float depth_scaling;
  float max_distance_sq, cos_max_angle;
};

struct TrackPhotoK {
  float weight, max_intensity_difference, min_gradient_sq;
};

struct TrackSolveK {
  int level, stride, n_slabs, final_launch;
  int min_inliers;
  int photo;                 // the reduce kernel ran the photometric term: 33 sums, else 31
  double min_inlier_fraction, min_pivot_ratio, convergence_rotation, convergence_translation;
  double pred[12];
};

// Samples along an axis of `size` pixels at stride s: the pixels s/2 + i s.
SMX_TRACK_FN int track_samples(int size, int s) { return size > s / 2 ? (size - s / 2 + s - 1) / s : 0; }

// The reduce launch: kTrackBlock lanes per workgroup; a lane visits kTrackPixelsPerLane samples before the grid is widened,
// up to kTrackMaxSlabs workgroups (one slab each), beyond which a lane visits more.  Workgroups for n samples:
constexpr int kTrackBlock = 256;
constexpr int kTrackPixelsPerLane = 8;
constexpr int kTrackMaxSlabs = 256;
constexpr int kTrackSlabStride = 32;       // doubles per workgroup slab without the photometric term (31 used)
constexpr int kTrackRgbdSlabStride = 40;   // ... with it (33 used)
SMX_TRACK_FN int track_grid(long long n) {
  const long long g = (n + kTrackBlock * kTrackPixelsPerLane - 1) / (kTrackBlock * kTrackPixelsPerLane);
  return (int)(g < 1 ? 1 : g > kTrackMaxSlabs ? kTrackMaxSlabs : g);
}

// One row's share of the normal equations, in the order every sum keeps: the 21 products of the upper triangle row by
// row, the 6 of the right-hand side, then the square of e into its own sum.  Products in float, sums in double.
SMX_TRACK_FN void track_accumulate(double* s, double& sum_sq, const float* J, float r, float e) {
  int i = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) s[i++] += (double)(J[a] * J[b]);
#pragma unroll
  for (int a = 0; a < 6; ++a) s[21 + a] += (double)(J[a] * r);
  sum_sq += (double)(e * e);
}

SMX_TRACK_FN float track_luma(float r, float g, float b) {
  return ((0.299f * r + 0.587f * g) + 0.114f * b) * (1.0f / 255.0f);
}
SMX_TRACK_FN float track_luma_u32(uint32_t c) {
  return track_luma((float)(c & 255u), (float)((c >> 8) & 255u), (float)((c >> 16) & 255u));
}

// The sampled frame pixel (x, y) with raw depth du: unprojection, T (T_rel as 12 floats), projection, association with the
// model images D / M, the distance and angle gates, J and r; with kPhoto the photometric term on top (P, and the frame's
// colour at the pixel, three bytes at rgb; ph, P and rgb are not looked at without).  nxy points at the frame normal's two
// floats; acc [28], acc_ee and the four counts are the lane's.  Every exit is the kernel loop's `continue`.
template <bool kPhoto>
SMX_TRACK_FN void track_pixel(const TrackK& k, const TrackPhotoK& ph, const float* T, int x, int y, uint16_t du,
                              const float2* nxy_at, const unsigned char* rgb, const float* D, const float4* M,
                              const float4* P, double* acc, double& acc_ee, uint32_t& n_in, uint32_t& n_px, uint32_t& n_as,
                              uint32_t& n_ph) {
  if (du == 0) return;
  ++n_px;
  const float2 nxy = *nxy_at;
  const float z = (float)du / k.depth_scaling;
  const float vx = z * (((float)x + 0.5f - k.cx) / k.fx), vy = z * (((float)y + 0.5f - k.cy) / k.fy);
  const float nz = -sqrtf(fmaxf(0.0f, 1.0f - nxy.x * nxy.x - nxy.y * nxy.y));
  const float px = T[0] * vx + T[1] * vy + T[2] * z + T[3];
  const float py = T[4] * vx + T[5] * vy + T[6] * z + T[7];
  const float pz = T[8] * vx + T[9] * vy + T[10] * z + T[11];
  if (!(pz > 0.0f)) return;
  const float uc = k.fx * px / pz + k.cx, wc = k.fy * py / pz + k.cy;
  const float uf = floorf(uc), wf = floorf(wc);
  if (!(uf >= 0.0f && uf < (float)k.W && wf >= 0.0f && wf < (float)k.H)) return;
  const int u = (int)uf, w = (int)wf;
  const size_t mi = (size_t)w * k.W + u;
  const float Dq = D[mi];
  if (!(Dq > 0.0f)) return;
  ++n_as;
  const float4 Mq = M[mi];
  const float qx = Dq * ((uf + 0.5f - k.cx) / k.fx), qy = Dq * ((wf + 0.5f - k.cy) / k.fy);
  const float dx = px - qx, dy = py - qy, dz = pz - Dq;
  if (!(dx * dx + dy * dy + dz * dz <= k.max_distance_sq)) return;
  const float mx = T[0] * nxy.x + T[1] * nxy.y + T[2] * nz;
  const float my = T[4] * nxy.x + T[5] * nxy.y + T[6] * nz;
  const float mz = T[8] * nxy.x + T[9] * nxy.y + T[10] * nz;
  if (!(mx * Mq.x + my * Mq.y + mz * Mq.z >= k.cos_max_angle)) {
    if (!kPhoto) return;   // (the photometric term does not ask for this gate)
  } else {
    ++n_in;
    const float r = Mq.x * dx + Mq.y * dy + Mq.z * dz;
    float J[6];
    J[0] = py * Mq.z - pz * Mq.y;
    J[1] = pz * Mq.x - px * Mq.z;
    J[2] = px * Mq.y - py * Mq.x;
    J[3] = Mq.x; J[4] = Mq.y; J[5] = Mq.z;
    track_accumulate(acc, acc[kSumRR], J, r, r);
  }
  if (!kPhoto) return;
  const float4 Pq = P[mi];
  const float Lm = (Pq.x + Pq.y * (uc - (uf + 0.5f))) + Pq.z * (wc - (wf + 0.5f));
  const float ei = Lm - track_luma((float)rgb[0], (float)rgb[1], (float)rgb[2]);
  if (!(Pq.w != 0.0f && Pq.y * Pq.y + Pq.z * Pq.z >= ph.min_gradient_sq && fabsf(ei) <= ph.max_intensity_difference)) return;
  ++n_ph;
  const float gfx = Pq.y * k.fx, gfy = Pq.z * k.fy;
  const float a0 = gfx / pz, a1 = gfy / pz, a2 = -((gfx * px + gfy * py) / (pz * pz));
  float K[6];
  K[0] = ph.weight * (py * a2 - pz * a1);
  K[1] = ph.weight * (pz * a0 - px * a2);
  K[2] = ph.weight * (px * a1 - py * a0);
  K[3] = ph.weight * a0; K[4] = ph.weight * a1; K[5] = ph.weight * a2;
  track_accumulate(acc, acc_ee, K, ph.weight * ei, ei);
}

// Model pixel i of k_track_photo_prepare: P = (L, gx, gy, valid) from the colour and depth renders.
SMX_TRACK_FN float4 track_photo_pixel(int W, int H, float max_relative_step, const float* D, const uint32_t* Cm, long long i) {
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
  return make_float4(track_luma_u32(Cm[i]), gx, gy, valid);
}

// exp of the twist x = (w, u) as a row-major 3x4: R = I + A K + B K^2, t = (I + B K + C K^2) u with K = [w]x
SMX_TRACK_FN void se3_exp(const double* x, double* E) {
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
SMX_TRACK_FN void se3_mul(const double* A, const double* B, double* Cm) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) {
      double v = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
      if (j == 3) v += A[4 * i + 3];
      Cm[4 * i + j] = v;
    }
  }
}

// One iteration's decision and update (lane 0) from the sums S (31 of them, 33 with k.photo).  Returns the status after
// it; x is zero where nothing was solved.
SMX_TRACK_FN int track_solve_one(const double* S, const TrackSolveK& k, TrackDev* st, double* x) {
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  for (int i = 0; i < (k.photo ? SMX_TRACK_RGBD_SUMS : SMX_TRACK_SUMS); ++i)
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

// What lane 0 of a solve launch does with the iteration's sums: solve, record, status.
SMX_TRACK_FN void track_solve_step(const double* S, const TrackSolveK& k, TrackDev* st) {
  double x[6];
  const int status = track_solve_one(S, k, st, x);
  const int slot = st->iterations_run;
  if (slot < kTrackRing) {
    smx_track_rgbd_iteration& rec = st->ring[slot];
    rec.level = k.level; rec.stride = k.stride; rec.status = status; rec.reserved = 0;
    for (int i = 0; i < SMX_TRACK_RGBD_SUMS; ++i) rec.sums[i] = (i < SMX_TRACK_SUMS || k.photo) ? S[i] : 0.0;
    for (int i = 0; i < 6; ++i) rec.x[i] = x[i];
    st->iterations_run = slot + 1;
  }
  st->status = status;
  if (status == SMX_TRACK_CONVERGED) st->converged_level = k.level;
}

// The end of the call (lane 0 of the last solve launch): the fraction test on the last iteration run, the pose, st->result.
SMX_TRACK_FN void track_finish(const TrackSolveK& k, TrackDev* st) {
  smx_track_result res;
  const int n = st->iterations_run;
  int status = st->status;
  const smx_track_rgbd_iteration* rec = n > 0 ? &st->ring[n - 1] : nullptr;
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
  const double ee = rec ? rec->sums[kSumEE] : 0.0, np = rec ? rec->sums[kSumPhotoInliers] : 0.0;
  st->result.icp = res;
  st->result.photometric_inliers = (uint32_t)np;
  st->result.rms_intensity_residual = np > 0.0 ? (float)sqrt(ee / np) : 0.0f;
}

#if !defined(SMX_TRACK_HOST_ONLY)
// ---- part 2 ----
// The workspace of the two calls, a member of smx_recon_s; allocated by the first call that needs each part.
struct TrackWork {
  // smx_recon_track / _rgbd, all four or none: the model images [H][W] of the last call, the reduce kernel's per-workgroup
  // partial sums (kTrackMaxSlabs * kTrackRgbdSlabStride doubles: either stride fits), the call's device state
  DevBuf<float> depth;
  DevBuf<float4> normal;
  DevBuf<double> slabs;
  DevBuf<TrackDev> state;
  // smx_recon_track_rgbd, both or none: the model colour image [H][W] (uchar4, alpha 0 = empty) and P = (L, gx, gy, valid)
  // of the last call with a weight
  DevBuf<uint32_t> color;
  DevBuf<float4> photo;
  StreamMark mark;          // behind the last call's kernels (the next call, on whatever stream, waits for it)
  bool last_rgbd = false;   // the last call was smx_recon_track_rgbd
};
#endif

}  // namespace smx
