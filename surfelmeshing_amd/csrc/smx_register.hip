// smx_register.hip -- smx_distscene_register (gfx950): point-to-plane ICP of a point set against the triangles of a kept
// distance scene (the contract is in include/smx.h, the move and the row in smx_register.hpp, the association is
// the scene's own query in smx_distance.hip, the sum order, the solve and the end of a call are smx_track.hpp's).  Per
// iteration, all iterations of a call enqueued back to back:
//
//   k_reg_move     a lane per sample: p' = Tf p into the query's point array; NaN in a skipped iteration, so that every key
//                  is the BAD one and the query's kernels walk nothing
//   (the query)    dist_scene_enqueue: k_dist_point_keys -> the sort -> k_dscene_query, unchanged
//   k_reg_reduce   the tracker's slab scheme over the samples: a lane visits i, i + 256 grid, ... four at a time -- the gather
//                  chain nearest -> first_rec -> the winner's record is issued for the four before the first is used -- then
//                  reg_sample in sample order; the cross-lane tree, the wavefronts in index order, one slab per workgroup
//   k_reg_solve    one wavefront: the slabs in index order, lane 0 runs track_solve_step and, in the last launch,
//                  track_finish, and writes the result
//   k_reg_begin    once per call: T = T_init
// smx_distscene_register_robust launches k_reg_reduce_robust in k_reg_reduce's place -- the winner's rim byte as
// one more gather of the batch, reg_sample_robust, the same 31 sums in the same slabs -- and k_reg_counts before the solve, which
// files the two new counts with the iteration's record; k_reg_solve serves both calls.  With no kernel and no rim rejection it
// launches the plain kernels.  smx_recon_register_mesh samples a mesh into the object's workspace and runs the robust call on it.
//
// Nothing is cleared between iterations and nothing waits on the device.  The entry points are at the end of the file.
#include <algorithm>
#include <cmath>
#include <vector>

#include "smx_recon_state.hpp"
#include "smx_register.hpp"
#include "smx_sort.hpp"

namespace smx {
namespace {

constexpr int kRegBatch = 4;       // samples of a lane whose gathers are in flight together

__global__ void k_reg_begin(RegDev* st, RegPose T) {
  for (int k = 0; k < 12; ++k) { st->t.T_rel[k] = (double)T.m[k]; st->t.T_prev[k] = (double)T.m[k]; st->t.Tf[k] = T.m[k]; }
  st->t.status = SMX_TRACK_OK;
  st->t.iterations_run = 0;
  st->t.converged_level = -1;
}

__device__ __forceinline__ bool reg_skips(const RegDev* st, int level) {
  return st->t.status >= SMX_TRACK_TOO_FEW_INLIERS || st->t.converged_level == level;
}

__global__ void __launch_bounds__(kTrackBlock)
k_reg_move(const RegDev* __restrict__ st, int level, const float* __restrict__ points, uint32_t stride, uint32_t m, float* __restrict__ moved) {
  const uint32_t j = blockIdx.x * kTrackBlock + threadIdx.x;
  if (j >= m) return;
  TgVec out{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if (!reg_skips(st, level)) {
    float T[12];
    for (int i = 0; i < 12; ++i) T[i] = st->t.Tf[i];
    const size_t p = (size_t)j * stride;
    out = reg_move(T, TgVec{points[3 * p], points[3 * p + 1], points[3 * p + 2]});
  }
  moved[3 * (size_t)j] = out.x; moved[3 * (size_t)j + 1] = out.y; moved[3 * (size_t)j + 2] = out.z;
}

__global__ void __launch_bounds__(kTrackBlock)
k_reg_reduce(const RegDev* __restrict__ st, int level, const float* __restrict__ moved, const float* __restrict__ normals, uint32_t stride,
             uint32_t m, const uint32_t* __restrict__ nearest, const float* __restrict__ closest, const uint32_t* __restrict__ first_rec,
             const TgRec* __restrict__ recs, const TgRec* __restrict__ wide_recs, float cos_max, double* __restrict__ slabs) {
  if (reg_skips(st, level)) return;
  float T[12];
  for (int i = 0; i < 12; ++i) T[i] = st->t.Tf[i];
  double acc[28];
  for (int i = 0; i < 28; ++i) acc[i] = 0.0;
  uint32_t n_in = 0, n_ok = 0, n_matched = 0;
  const bool with_normal = normals != nullptr;
  const uint32_t step = gridDim.x * kTrackBlock;
  // (m <= 2^28 and step <= 2^16: i + 3 step stays below 2^32)
  for (uint32_t i0 = blockIdx.x * kTrackBlock + threadIdx.x; i0 < m; i0 += kRegBatch * step) {
    uint32_t t[kRegBatch], word[kRegBatch];
    TgVec P[kRegBatch], Q[kRegBatch], nrm[kRegBatch];
    float4 a[kRegBatch], b[kRegBatch], c[kRegBatch];
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      const uint32_t i = i0 + k * step;
      t[k] = i < m ? nearest[i] : kInvalid;
    }
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      const uint32_t i = i0 + k * step;
      word[k] = t[k] != kInvalid ? first_rec[t[k]] : kDsceneNoRec;
      // (a sample past the end is a BAD point: it adds to nothing)
      P[k] = Q[k] = nrm[k] = TgVec{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
      if (i < m) P[k] = TgVec{moved[3 * (size_t)i], moved[3 * (size_t)i + 1], moved[3 * (size_t)i + 2]};
      if (t[k] != kInvalid) {
        Q[k] = TgVec{closest[3 * (size_t)i], closest[3 * (size_t)i + 1], closest[3 * (size_t)i + 2]};
        if (with_normal) {
          const size_t p = (size_t)i * stride;
          nrm[k] = TgVec{normals[3 * p], normals[3 * p + 1], normals[3 * p + 2]};
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      // (a winner came out of a record, so it has a first one; if not: NaN corners, which end as collinear)
      const float nan = __builtin_nanf("");
      a[k] = b[k] = c[k] = make_float4(nan, nan, nan, nan);
      if (word[k] != kDsceneNoRec) {
        const TgRec* r = (word[k] & kDsceneWideBit) ? wide_recs + (word[k] & ~kDsceneWideBit) : recs + word[k];
        a[k] = r->a; b[k] = r->b; c[k] = r->c;
      }
    }
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      const TgVec mk = with_normal ? reg_rotate(T, nrm[k]) : TgVec{0.0f, 0.0f, 0.0f};
      reg_sample(P[k], t[k], Q[k], TgVec{a[k].x, a[k].y, a[k].z}, TgVec{b[k].x, b[k].y, b[k].z}, TgVec{c[k].x, c[k].y, c[k].z}, with_normal, mk,
                 cos_max, acc, n_in, n_ok, n_matched);
    }
  }
  // wavefront: shifts towards lane 0; workgroup: one row of LDS per wavefront, added in wavefront order (k_track_reduce's)
  __shared__ double part[kTrackBlock / 64][kTrackSlabStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 28; ++e) {
    double v = acc[e];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][e] = v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    n_in += __shfl_down(n_in, off, 64); n_ok += __shfl_down(n_ok, off, 64);
    n_matched += __shfl_down(n_matched, off, 64);
  }
  if (lane == 0) {
    part[wave][kSumInliers] = (double)n_in; part[wave][kSumPixels] = (double)n_ok;
    part[wave][kSumAssociated] = (double)n_matched;
  }
  __syncthreads();
  if (threadIdx.x < SMX_REGISTER_SUMS) {
    double v = part[0][threadIdx.x];
    for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][threadIdx.x];
    slabs[(size_t)blockIdx.x * kTrackSlabStride + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(64)
k_reg_solve(TrackSolveK k, const double* __restrict__ slabs, RegDev* st, smx_register_result* out) {
  __shared__ double S[SMX_TRACK_RGBD_SUMS];
  const bool skip = reg_skips(st, k.level);
  if (!skip && threadIdx.x < SMX_TRACK_RGBD_SUMS) {
    double v = 0.0;
    if (threadIdx.x < SMX_REGISTER_SUMS)
      for (int b = 0; b < k.n_slabs; ++b) v += slabs[(size_t)b * kTrackSlabStride + threadIdx.x];   // (index order)
    S[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!skip) {
    const int slot = st->t.iterations_run;
    if (slot < kTrackRing)
      for (int i = 0; i < 12; ++i) st->ring_Tf[slot][i] = st->t.Tf[i];
    track_solve_step(S, k, &st->t);
  }
  if (k.final_launch) {
    track_finish(k, &st->t);                 // (the fraction test, the figures of the last iteration; its pose is not used)
    const smx_track_result& f = st->t.result.icp;
    smx_register_result res;
    for (int i = 0; i < 12; ++i) res.scene_T_points[i] = (float)st->t.T_rel[i];   // (nothing solved: T_init, bit for bit)
    res.status = f.status; res.iterations_run = f.iterations_run;
    res.inliers = f.inliers; res.points_used = f.pixels_with_depth;
    res.rms_residual = f.rms_residual; res.last_update_rotation = f.last_update_rotation;
    res.last_update_translation = f.last_update_translation;
    for (int i = 0; i < 36; ++i) res.information[i] = f.information[i];
    st->result = res;
    if (out) *out = res;
  }
}

// k_reg_reduce with the two new decisions per sample: the winner's rim byte joins the batch's gathers and reg_sample_robust takes
// reg_sample's place.  The 31 sums go to the same slabs in the same order, so that k_reg_solve serves both; the two new counts,
// sums [31] and [32], go to counts[workgroup][2] beside them (integers: their order does not matter).
__global__ void __launch_bounds__(kTrackBlock)
k_reg_reduce_robust(const RegDev* __restrict__ st, int level, const float* __restrict__ moved, const float* __restrict__ normals, uint32_t stride,
             uint32_t m, const uint32_t* __restrict__ nearest, const float* __restrict__ closest, const uint32_t* __restrict__ first_rec,
             const TgRec* __restrict__ recs, const TgRec* __restrict__ wide_recs, float cos_max, RegRobustK x, double* __restrict__ slabs, uint32_t* __restrict__ counts) {
  if (reg_skips(st, level)) return;
  float T[12];
  for (int i = 0; i < 12; ++i) T[i] = st->t.Tf[i];
  double acc[28];
  for (int i = 0; i < 28; ++i) acc[i] = 0.0;
  uint32_t n_in = 0, n_ok = 0, n_matched = 0, n_rim = 0, n_weight = 0;
  const bool with_normal = normals != nullptr;
  const uint32_t step = gridDim.x * kTrackBlock;
  // (m <= 2^28 and step <= 2^16: i + 3 step stays below 2^32)
  for (uint32_t i0 = blockIdx.x * kTrackBlock + threadIdx.x; i0 < m; i0 += kRegBatch * step) {
    uint32_t t[kRegBatch], word[kRegBatch], rim_byte[kRegBatch];
    TgVec P[kRegBatch], Q[kRegBatch], nrm[kRegBatch];
    float4 a[kRegBatch], b[kRegBatch], c[kRegBatch];
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      const uint32_t i = i0 + k * step;
      t[k] = i < m ? nearest[i] : kInvalid;
    }
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      const uint32_t i = i0 + k * step;
      word[k] = t[k] != kInvalid ? first_rec[t[k]] : kDsceneNoRec;
      rim_byte[k] = x.reject_rim && t[k] != kInvalid ? x.rim[t[k]] : 0u;
      // (a sample past the end is a BAD point: it adds to nothing)
      P[k] = Q[k] = nrm[k] = TgVec{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
      if (i < m) P[k] = TgVec{moved[3 * (size_t)i], moved[3 * (size_t)i + 1], moved[3 * (size_t)i + 2]};
      if (t[k] != kInvalid) {
        Q[k] = TgVec{closest[3 * (size_t)i], closest[3 * (size_t)i + 1], closest[3 * (size_t)i + 2]};
        if (with_normal) {
          const size_t p = (size_t)i * stride;
          nrm[k] = TgVec{normals[3 * p], normals[3 * p + 1], normals[3 * p + 2]};
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      // (a winner came out of a record, so it has a first one; if not: NaN corners, which end as collinear)
      const float nan = __builtin_nanf("");
      a[k] = b[k] = c[k] = make_float4(nan, nan, nan, nan);
      if (word[k] != kDsceneNoRec) {
        const TgRec* r = (word[k] & kDsceneWideBit) ? wide_recs + (word[k] & ~kDsceneWideBit) : recs + word[k];
        a[k] = r->a; b[k] = r->b; c[k] = r->c;
      }
    }
#pragma unroll
    for (int k = 0; k < kRegBatch; ++k) {
      const TgVec mk = with_normal ? reg_rotate(T, nrm[k]) : TgVec{0.0f, 0.0f, 0.0f};
      reg_sample_robust(P[k], t[k], Q[k], TgVec{a[k].x, a[k].y, a[k].z}, TgVec{b[k].x, b[k].y, b[k].z}, TgVec{c[k].x, c[k].y, c[k].z}, with_normal,
                        mk, cos_max, rim_byte[k], x.reject_rim != 0, x.kernel, x.c, acc, n_in, n_ok, n_matched, n_rim, n_weight);
    }
  }
  // wavefront: shifts towards lane 0; workgroup: one row of LDS per wavefront, added in wavefront order (k_track_reduce's)
  __shared__ double part[kTrackBlock / 64][kTrackSlabStride];
  __shared__ uint32_t part_counts[kTrackBlock / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 28; ++e) {
    double v = acc[e];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][e] = v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    n_in += __shfl_down(n_in, off, 64); n_ok += __shfl_down(n_ok, off, 64);
    n_matched += __shfl_down(n_matched, off, 64);
    n_rim += __shfl_down(n_rim, off, 64); n_weight += __shfl_down(n_weight, off, 64);
  }
  if (lane == 0) {
    part[wave][kSumInliers] = (double)n_in; part[wave][kSumPixels] = (double)n_ok;
    part[wave][kSumAssociated] = (double)n_matched;
    part_counts[wave][0] = n_rim; part_counts[wave][1] = n_weight;
  }
  __syncthreads();
  if (threadIdx.x < SMX_REGISTER_SUMS) {
    double v = part[0][threadIdx.x];
    for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part[wv][threadIdx.x];
    slabs[(size_t)blockIdx.x * kTrackSlabStride + threadIdx.x] = v;
  }
  if (threadIdx.x >= 64 && threadIdx.x < 66) {
    const int k = threadIdx.x - 64;
    uint32_t v = part_counts[0][k];
    for (int wv = 1; wv < kTrackBlock / 64; ++wv) v += part_counts[wv][k];
    counts[2 * (size_t)blockIdx.x + k] = v;
  }
}

// The two new counts of a robust iteration, before its solve: the workgroups' counts in index order into the record the solve
// is about to write (slot = iterations_run), if the iteration runs at all.
__global__ void k_reg_counts(RegDev* st, int level, int n_slabs, const uint32_t* __restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x >= 2 || reg_skips(st, level)) return;
  const int slot = st->t.iterations_run;
  if (slot >= kTrackRing) return;
  uint32_t v = 0;
  for (int b = 0; b < n_slabs; ++b) v += counts[2 * b + threadIdx.x];
  st->ring_counts[slot][threadIdx.x] = v;
}

struct RegLevel { uint32_t stride, m; int iters, grid; float q, cos_max; TrackSolveK sk; };

DistSceneIndex reg_index(const smx_distscene_s* sc) {
  return DistSceneIndex{reinterpret_cast<const TgCell*>(sc->table.get()), sc->mask, reinterpret_cast<const TgRec*>(sc->recs.get()),
                        reinterpret_cast<const TgRec*>(sc->wide_recs.get()), sc->n_wide, sc->first_rec.get(), sc->counters.get()};
}

template <typename T>
bool reg_fits(const DevBuf<T>& b, size_t want) { return want <= b.capacity(); }

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_register_params_default(smx_register_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  const int32_t stride[3] = {4, 2, 1}, iters[3] = {4, 5, 10};
  for (int l = 0; l < 3; ++l) { out->level_stride[l] = stride[l]; out->level_iterations[l] = iters[l]; out->level_max_distance[l] = 0.0f; }
  out->max_normal_angle_deg = 30.0f;
  out->convergence_rotation = 1e-5f; out->convergence_translation = 1e-5f;
  out->min_inliers = 50; out->min_inlier_fraction = 0.1f; out->min_pivot_ratio = 1e-6f;
  return SMX_OK;
}

// Both registration calls.  rp == nullptr, or one that asks for nothing (kernel 0, reject_rim 0): the plain call, its kernels,
// its allocations.
static int reg_run(smx_distscene sc, smx_stream s, const smx_register_params* params, const smx_register_robust_params* rp, const float* points,
                   const float* normals, uint32_t n_points, int32_t on_device, const float T_init[12], smx_register_result* result,
                   int32_t result_on_device) {
  SMX_CHECK_ARG(sc != nullptr && params != nullptr && T_init != nullptr && result != nullptr);
  const smx_register_params& p = *params;
  // (what does not need the scene first: a refusal of these comes before anything looks at it)
  SMX_CHECK_ARG(n_points <= (1u << 28));
  SMX_CHECK_ARG(points != nullptr || n_points == 0);
  for (int k = 0; k < 12; ++k) SMX_CHECK_ARG(finite_f(T_init[k]));
  RegLevel lv[kTrackLevels];
  int levels_used = 0, last_level = -1;
  uint32_t m_max = 0;
  SMX_CHECK_ARG(p.max_normal_angle_deg > 0 && p.max_normal_angle_deg <= 180.0f);
  SMX_CHECK_ARG(p.convergence_rotation >= 0 && p.convergence_translation >= 0 && p.min_inliers >= 0);
  SMX_CHECK_ARG(p.min_inlier_fraction >= 0 && p.min_inlier_fraction <= 1 && p.min_pivot_ratio >= 0);
  for (int l = 0; l < kTrackLevels; ++l) {
    SMX_CHECK_ARG(p.level_iterations[l] >= 0 && p.level_iterations[l] <= kTrackMaxIterationsPerLevel);
    RegLevel& t = lv[l];
    t.iters = p.level_iterations[l];
    if (t.iters == 0) continue;
    ++levels_used; last_level = l;
    SMX_CHECK_ARG(p.level_stride[l] >= 1 && p.level_stride[l] <= kRegMaxStride);
    const float q = p.level_max_distance[l];
    SMX_CHECK_ARG(q == 0.0f || (finite_f(q) && q >= 1e-3f && q <= 16.0f));
    t.q = q;
    t.stride = (uint32_t)p.level_stride[l];
    t.m = reg_samples(n_points, t.stride);
    m_max = std::max(m_max, t.m);
    t.grid = track_grid((long long)t.m);
    t.cos_max = (float)cos((double)p.max_normal_angle_deg * (M_PI / 180.0));
    TrackSolveK& sk = t.sk;
    sk.level = l; sk.stride = (int)t.stride; sk.n_slabs = t.grid; sk.final_launch = 0;
    sk.min_inliers = p.min_inliers; sk.photo = 0;
    sk.min_inlier_fraction = p.min_inlier_fraction; sk.min_pivot_ratio = p.min_pivot_ratio;
    sk.convergence_rotation = p.convergence_rotation; sk.convergence_translation = p.convergence_translation;
    for (int i = 0; i < 12; ++i) sk.pred[i] = (i == 0 || i == 5 || i == 10) ? 1.0 : 0.0;
  }
  SMX_CHECK_ARG(levels_used > 0);
  bool robust = false;
  if (rp) {
    SMX_CHECK_ARG(rp->kernel >= kRegKernelNone && rp->kernel <= kRegKernelTukey);
    SMX_CHECK_ARG(rp->reject_rim == 0 || rp->reject_rim == 1);
    if (rp->kernel != kRegKernelNone)
      for (int l = 0; l < kTrackLevels; ++l) {
        const float c = rp->level_scale[l];
        if (lv[l].iters > 0) SMX_CHECK_ARG(c == 0.0f || (finite_f(c) && c >= 1e-6f && c <= 16.0f));
      }
    robust = rp->kernel != kRegKernelNone || rp->reject_rim != 0;
  }
  if (!sc->built) {
    set_error("smx_distscene_register on an empty scene: build it first");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  if (rp && rp->reject_rim && !sc->has_rim) {
    set_error("smx_distscene_register_robust: reject_rim needs a scene built by smx_recon_build_distscene_rim");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  for (int l = 0; l < kTrackLevels; ++l) {
    if (lv[l].iters == 0) continue;
    if (lv[l].q > sc->max_distance) {
      set_error("smx_distscene_register: level_max_distance[%d] = %g is above the %g the scene was built for", l, (double)lv[l].q,
                (double)sc->max_distance);
      return SMX_ERR_INVALID_ARGUMENT;
    }
    if (lv[l].q == 0.0f) lv[l].q = sc->max_distance;
  }
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  const bool dev = on_device != 0;
  RegisterWork& w = sc->reg;
  DistQueryWork& qw = sc->query;

  // ---- every allocation of the call, before the first launch.  A block that has to grow may still be in use by the scene's
  // previous registration, which did not wait: then the host waits for it first; otherwise st does.
  const size_t n3 = (size_t)3 * n_points, m3 = (size_t)3 * m_max;
  const bool fits = w.state.get() && (!robust || w.robust_counts.get()) && qw.counters.get() && reg_fits(qw.best, m_max) && reg_fits(qw.keys[0], m_max) && reg_fits(qw.keys[1], m_max) &&
                    reg_fits(qw.vals[0], m_max) && reg_fits(qw.vals[1], m_max) && reg_fits(qw.hist, radix_sort_workspace_elems(m_max)) &&
                    (dev || (reg_fits(w.pts, n3) && (!normals || reg_fits(w.nrm, n3)))) && reg_fits(w.moved, m3) && reg_fits(w.nearest, m_max) &&
                    reg_fits(w.distance, m_max) && reg_fits(w.closest, m3);
  if (!fits) SMX_CALL(w.mark.sync());
  SMX_CALL(w.mark.wait(st));
  if (!w.state.get()) SMX_CALL(alloc_all(w.slabs, (size_t)kTrackMaxSlabs * kTrackSlabStride, w.state, 1));
  SMX_CALL(dist_scene_reserve(qw, m_max));
  SMX_CALL(w.moved.reserve(m3));
  SMX_CALL(w.nearest.reserve(m_max));
  SMX_CALL(w.distance.reserve(m_max));
  SMX_CALL(w.closest.reserve(m3));
  if (!dev && n_points > 0) {
    SMX_CALL(w.pts.reserve(n3));
    if (normals) SMX_CALL(w.nrm.reserve(n3));
  }
  if (robust && !w.robust_counts.get()) SMX_CALL(w.robust_counts.alloc((size_t)kTrackMaxSlabs * 2, false));
  const float *dpts = nullptr, *dnrm = nullptr;
  SMX_CALL(stage_in(w.pts, points, n3, dev, st, &dpts));
  SMX_CALL(stage_in(w.nrm, normals, normals ? n3 : 0, dev, st, &dnrm));
  if (n_points == 0) dnrm = nullptr;
  SMX_CALL(w.whole.begin(st));
  SMX_CALL(w.last.begin(st));             // (the events exist before the first launch; begun again at the last iteration)

  // ---- the schedule
  RegDev* state = w.state.get();
  const DistSceneIndex ix = reg_index(sc);
  RegPose T0;
  for (int k = 0; k < 12; ++k) T0.m[k] = T_init[k];
  hipLaunchKernelGGL(k_reg_begin, dim3(1), dim3(1), 0, st, state, T0);
  if (robust) SMX_HIP(hipMemsetAsync(state->ring_counts, 0, sizeof(state->ring_counts), st));
  w.last_robust = robust;
  SMX_LAUNCH_CHECK();
  for (int l = 0; l < kTrackLevels; ++l) {
    RegLevel& t = lv[l];
    for (int it = 0; it < t.iters; ++it) {
      const bool last = l == last_level && it == t.iters - 1;
      if (last) SMX_CALL(w.last.begin(st));
      if (t.m > 0)
        hipLaunchKernelGGL(k_reg_move, dim3((unsigned)div_up(t.m, kTrackBlock)), dim3(kTrackBlock), 0, st, state, l, dpts, t.stride, t.m, w.moved.get());
      if (last) SMX_CALL(w.last.mark(st));
      SMX_CALL(dist_scene_enqueue(qw, ix, w.moved.get(), t.m, t.q, 0, w.nearest.get(), w.distance.get(), w.closest.get(), st));
      if (last) SMX_CALL(w.last.mark(st));
      if (robust) {
        const RegRobustK x{sc->rim.get(), rp->reject_rim, rp->kernel, rp->kernel != kRegKernelNone ? rp->level_scale[l] : 0.0f};
        hipLaunchKernelGGL(k_reg_reduce_robust, dim3(t.grid), dim3(kTrackBlock), 0, st, state, l, w.moved.get(), dnrm, t.stride, t.m, w.nearest.get(),
                           w.closest.get(), ix.first_rec, ix.recs, ix.wide_recs, t.cos_max, x, w.slabs.get(), w.robust_counts.get());
        hipLaunchKernelGGL(k_reg_counts, dim3(1), dim3(64), 0, st, state, l, t.grid, w.robust_counts.get());
      } else {
        hipLaunchKernelGGL(k_reg_reduce, dim3(t.grid), dim3(kTrackBlock), 0, st, state, l, w.moved.get(), dnrm, t.stride, t.m, w.nearest.get(),
                           w.closest.get(), ix.first_rec, ix.recs, ix.wide_recs, t.cos_max, w.slabs.get());
      }
      if (last) SMX_CALL(w.last.mark(st));
      t.sk.final_launch = last ? 1 : 0;
      hipLaunchKernelGGL(k_reg_solve, dim3(1), dim3(64), 0, st, t.sk, w.slabs.get(), state, last && result_on_device ? result : nullptr);
      SMX_LAUNCH_CHECK();
      if (last) SMX_CALL(w.last.mark(st));
    }
  }
  SMX_CALL(w.whole.mark(st));
  SMX_CALL(w.mark.record(st));
  w.whole.publish(); w.last.publish();    // (reading them waits for their events)
  if (!result_on_device) {
    SMX_HIP(hipMemcpyAsync(result, &state->result, sizeof(*result), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
  }
  return SMX_OK;
}

int smx_distscene_register(smx_distscene sc, smx_stream s, const smx_register_params* params, const float* points, const float* normals,
                           uint32_t n_points, int32_t on_device, const float T_init[12], smx_register_result* result,
                           int32_t result_on_device) {
  return reg_run(sc, s, params, nullptr, points, normals, n_points, on_device, T_init, result, result_on_device);
}

int smx_register_robust_params_default(smx_register_robust_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->kernel = 0; out->reject_rim = 0;
  for (int l = 0; l < 3; ++l) out->level_scale[l] = 0.0f;
  return SMX_OK;
}

int smx_distscene_register_robust(smx_distscene sc, smx_stream s, const smx_register_params* params, const smx_register_robust_params* rp,
                                  const float* points, const float* normals, uint32_t n_points, int32_t on_device, const float T_init[12],
                                  smx_register_result* result, int32_t result_on_device) {
  SMX_CHECK_ARG(rp != nullptr);
  return reg_run(sc, s, params, rp, points, normals, n_points, on_device, T_init, result, result_on_device);
}

// By definition smx_recon_sample_mesh with its normals on r's map, then smx_distscene_register_robust of those points and
// normals: the two calls themselves, on device arrays of r's workspace.  Synchronous: the samples' buffers are free again on return.
int smx_recon_register_mesh(smx_recon r, smx_stream s, smx_distscene sc, const uint32_t* triangles, uint32_t n_in, int32_t on_device,
                            uint32_t n_samples, uint32_t seed, const smx_register_params* params, const smx_register_robust_params* rp,
                            const float T_init[12], smx_register_result* result, int32_t result_on_device) {
  SMX_CHECK_ARG(r != nullptr && sc != nullptr && rp != nullptr);
  SMX_CHECK_ARG(sc->device == r->device);
  SMX_CHECK_ARG(n_in <= (1u << 28) && n_samples <= (1u << 28));
  SMX_CHECK_ARG(triangles != nullptr || n_in == 0);
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  RegisterMeshWork& w = r->register_mesh;
  SMX_CALL(w.points.reserve((size_t)3 * n_samples));
  SMX_CALL(w.normals.reserve((size_t)3 * n_samples));
  SMX_CALL(w.tri.reserve(n_samples));
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(w.in, triangles, (size_t)3 * n_in, on_device != 0, st, &din));
  SMX_CALL(smx_recon_sample_mesh(r, s, din, n_in, n_samples, seed, w.points.get(), w.tri.get(), nullptr, w.normals.get(), 1, nullptr));
  const int rc = reg_run(sc, s, params, rp, w.points.get(), w.normals.get(), n_samples, 1, T_init, result, result_on_device);
  SMX_HIP(hipStreamSynchronize(st));
  return rc;
}

int smx_distscene_debug_register_robust_counts(smx_distscene sc, smx_stream s, uint32_t (*counts)[2], int32_t capacity, int32_t* count) {
  SMX_CHECK_ARG(sc != nullptr && count != nullptr && capacity >= 0 && (capacity == 0 || counts != nullptr));
  *count = 0;
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  const RegisterWork& w = sc->reg;
  if (!w.state.get() || !w.mark.busy()) return SMX_OK;
  SMX_CALL(w.mark.wait(st));
  int32_t n = 0;
  SMX_HIP(hipMemcpyAsync(&n, &w.state.get()->t.iterations_run, sizeof(n), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  n = std::max(0, std::min(n, (int32_t)kTrackRing));
  *count = n;
  const int32_t k = std::min(n, capacity);
  if (k == 0) return SMX_OK;
  if (!w.last_robust) {                  // (a plain registration has no such counts)
    for (int32_t i = 0; i < k; ++i) counts[i][0] = counts[i][1] = 0;
    return SMX_OK;
  }
  SMX_HIP(hipMemcpyAsync(counts, w.state.get()->ring_counts, sizeof(uint32_t) * 2 * (size_t)k, hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  return SMX_OK;
}

int smx_distscene_debug_register_iterations(smx_distscene sc, smx_stream s, smx_register_iteration* recs, int32_t capacity, int32_t* count) {
  SMX_CHECK_ARG(sc != nullptr && count != nullptr && capacity >= 0 && (capacity == 0 || recs != nullptr));
  *count = 0;
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  const RegisterWork& w = sc->reg;
  if (!w.state.get() || !w.mark.busy()) return SMX_OK;
  SMX_CALL(w.mark.wait(st));
  int32_t n = 0;
  SMX_HIP(hipMemcpyAsync(&n, &w.state.get()->t.iterations_run, sizeof(n), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  n = std::max(0, std::min(n, (int32_t)kTrackRing));
  *count = n;
  const int32_t k = std::min(n, capacity);
  if (k == 0) return SMX_OK;
  std::vector<smx_track_rgbd_iteration> ring((size_t)k);
  std::vector<float> Tf((size_t)k * 12);
  SMX_HIP(hipMemcpyAsync(ring.data(), w.state.get()->t.ring, sizeof(smx_track_rgbd_iteration) * (size_t)k, hipMemcpyDeviceToHost, st));
  SMX_HIP(hipMemcpyAsync(Tf.data(), w.state.get()->ring_Tf, sizeof(float) * 12 * (size_t)k, hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  for (int32_t i = 0; i < k; ++i) {
    const smx_track_rgbd_iteration& f = ring[(size_t)i];
    smx_register_iteration& t = recs[i];
    t.level = f.level; t.stride = f.stride; t.status = f.status; t.reserved = f.reserved;
    std::copy_n(&Tf[(size_t)i * 12], 12, t.Tf);
    std::copy_n(f.sums, SMX_REGISTER_SUMS, t.sums);
    std::copy_n(f.x, 6, t.x);
  }
  return SMX_OK;
}

int smx_distscene_debug_register_timings(smx_distscene sc, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(sc != nullptr && out_ms != nullptr && capacity >= SMX_REGISTER_PHASES);
  SMX_ON_DEVICE(sc->device);
  SMX_CALL(sc->reg.whole.elapsed_ms(out_ms, 1));
  return sc->reg.last.elapsed_ms(out_ms + 1, 4);
}

}  // extern "C"
