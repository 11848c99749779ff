// smx_global.hip -- registration without a start pose (gfx950): smx_register_pose_lattice, smx_distscene_score_poses and
// smx_distscene_register_global (the contract is in include/smx.h, the lattice, a sample's share of the score and
// the choice of the starts in smx_global.hpp, the association is the scene's own query in smx_distance.hip, a start is refined by
// smx_distscene_register(_robust) as it stands).  Per chunk of poses, all chunks of a call enqueued back to back:
//
//   k_glob_move    a workgroup per pose x 256 samples: the pose's 12 floats are uniform loads, the points are read at the stride,
//                  p' = T p goes into the query's point array at [pose][sample]
//   (the query)    dist_scene_enqueue over the chunk's poses x m points: k_dist_point_keys -> the sort -> k_dscene_query, unchanged
//   k_glob_score   a workgroup of 256 lanes per pose over its m samples: nearest, distance and p' read in sample order; with
//                  reject_rim the gather chain nearest -> first_rec -> the winner's record -> its rim byte is issued for four
//                  samples before the first is used, as k_reg_reduce does.  Four integer words per pose: wave shuffles, one LDS
//                  row per wavefront, one store per word.  No atomics, no floating-point sums.
//
// The host reads nothing before the last chunk is enqueued.  The entry points are at the end of the file.
#include <algorithm>
#include <chrono>
#include <vector>

#include "smx_recon_state.hpp"
#include "smx_global.hpp"
#include "smx_sort.hpp"

namespace smx {
namespace {

__global__ void __launch_bounds__(kGlobBlock)
k_glob_move(const float* __restrict__ poses, uint32_t blocks_per_pose, const float* __restrict__ points, uint32_t stride, uint32_t m,
            float* __restrict__ moved) {
  const uint32_t pose = blockIdx.x / blocks_per_pose;
  const uint32_t j = (blockIdx.x - pose * blocks_per_pose) * kGlobBlock + threadIdx.x;
  if (j >= m) return;
  float T[12];
  for (int i = 0; i < 12; ++i) T[i] = poses[12 * (size_t)pose + i];
  const size_t p = (size_t)j * stride;
  const TgVec out = reg_move(T, TgVec{points[3 * p], points[3 * p + 1], points[3 * p + 2]});
  const size_t o = 3 * ((size_t)pose * m + j);
  moved[o] = out.x; moved[o + 1] = out.y; moved[o + 2] = out.z;
}

template <bool kRim>
__global__ void __launch_bounds__(kGlobBlock)
k_glob_score(const float* __restrict__ moved, const uint32_t* __restrict__ nearest, const float* __restrict__ distance, uint32_t m, uint32_t q_word,
             const uint32_t* __restrict__ first_rec, const TgRec* __restrict__ recs, const TgRec* __restrict__ wide_recs, const uint8_t* __restrict__ rim,
             smx_pose_score* __restrict__ scores) {
  const size_t base = (size_t)blockIdx.x * m;
  unsigned long long cost = 0;
  uint32_t n_ok = 0, n_matched = 0, n_rim = 0;
  if (!kRim) {
    for (uint32_t i = threadIdx.x; i < m; i += kGlobBlock) {
      const size_t s = base + i;
      glob_sample(TgVec{moved[3 * s], moved[3 * s + 1], moved[3 * s + 2]}, nearest[s], distance[s], q_word, false, cost, n_ok, n_matched, n_rim);
    }
  } else {
    // (m <= 2^16: i0 + 3 * 256 stays far below 2^32)
    for (uint32_t i0 = threadIdx.x; i0 < m; i0 += kGlobBatch * kGlobBlock) {
      uint32_t t[kGlobBatch], word[kGlobBatch], rim_byte[kGlobBatch];
      float d[kGlobBatch];
      TgVec P[kGlobBatch];
      float4 a[kGlobBatch], b[kGlobBatch], c[kGlobBatch];
#pragma unroll
      for (int k = 0; k < kGlobBatch; ++k) {
        const uint32_t i = i0 + k * kGlobBlock;
        t[k] = i < m ? nearest[base + i] : kInvalid;
      }
#pragma unroll
      for (int k = 0; k < kGlobBatch; ++k) {
        const uint32_t i = i0 + k * kGlobBlock;
        word[k] = t[k] != kInvalid ? first_rec[t[k]] : kDsceneNoRec;
        rim_byte[k] = t[k] != kInvalid ? rim[t[k]] : 0u;
        P[k] = TgVec{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        d[k] = 0.0f;
        if (i < m) {
          const size_t s = base + i;
          P[k] = TgVec{moved[3 * s], moved[3 * s + 1], moved[3 * s + 2]};
          d[k] = distance[s];
        }
      }
#pragma unroll
      for (int k = 0; k < kGlobBatch; ++k) {
        // (a winner came out of a record, so it has a first one; if not: NaN corners, which have no area)
        const float nan = __builtin_nanf("");
        a[k] = b[k] = c[k] = make_float4(nan, nan, nan, nan);
        if (word[k] != kDsceneNoRec) {
          const TgRec* r = (word[k] & kDsceneWideBit) ? wide_recs + (word[k] & ~kDsceneWideBit) : recs + word[k];
          a[k] = r->a; b[k] = r->b; c[k] = r->c;
        }
      }
#pragma unroll
      for (int k = 0; k < kGlobBatch; ++k) {
        if (i0 + k * kGlobBlock >= m) continue;          // (a sample past the end pays nothing)
        const bool on_rim = t[k] != kInvalid && glob_on_rim(rim_byte[k], P[k], TgVec{a[k].x, a[k].y, a[k].z}, TgVec{b[k].x, b[k].y, b[k].z},
                                                            TgVec{c[k].x, c[k].y, c[k].z});
        glob_sample(P[k], t[k], d[k], q_word, on_rim, cost, n_ok, n_matched, n_rim);
      }
    }
  }
  // wavefront: shifts towards lane 0; workgroup: one row of LDS per wavefront.  Integers: the order does not matter.
  __shared__ unsigned long long part[kGlobBlock / 64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) {
    cost += __shfl_down(cost, off, 64);
    n_ok += __shfl_down(n_ok, off, 64); n_matched += __shfl_down(n_matched, off, 64); n_rim += __shfl_down(n_rim, off, 64);
  }
  if (lane == 0) { part[wave][0] = cost; part[wave][1] = n_ok; part[wave][2] = n_matched; part[wave][3] = n_rim; }
  __syncthreads();
  if (threadIdx.x < 5) {
    unsigned long long v = 0;
    if (threadIdx.x < 4)
      for (int wv = 0; wv < kGlobBlock / 64; ++wv) v += part[wv][threadIdx.x];
    smx_pose_score* o = scores + blockIdx.x;
    switch (threadIdx.x) {
      case 0: o->cost = v; break;
      case 1: o->n_ok = (uint32_t)v; break;
      case 2: o->n_matched = (uint32_t)v; break;
      case 3: o->n_rim = (uint32_t)v; break;
      default: o->reserved = 0u; break;
    }
  }
}

struct GlobScoreK { uint32_t stride, m; float q; int reject_rim; };

// What smx_distscene_score_poses refuses, with nothing launched and nothing written; fills *k.
int glob_check(smx_distscene sc, const smx_score_params* p, const float* points, uint32_t n_points, const float* poses, uint32_t P, GlobScoreK* k) {
  SMX_CHECK_ARG(sc != nullptr && p != nullptr && poses != nullptr);
  SMX_CHECK_ARG(P >= 1 && P <= kGlobMaxPoses);
  SMX_CHECK_ARG(n_points <= (1u << 28));
  SMX_CHECK_ARG(points != nullptr || n_points == 0);
  SMX_CHECK_ARG(p->stride >= 1 && p->stride <= kRegMaxStride);
  SMX_CHECK_ARG(p->reject_rim == 0 || p->reject_rim == 1);
  const float q = p->max_distance;
  SMX_CHECK_ARG(q == 0.0f || (finite_f(q) && q >= 1e-3f && q <= 16.0f));
  k->stride = (uint32_t)p->stride;
  k->m = reg_samples(n_points, k->stride);
  SMX_CHECK_ARG(k->m <= kGlobMaxSamples);
  for (size_t i = 0; i < 12 * (size_t)P; ++i) SMX_CHECK_ARG(finite_f(poses[i]));
  if (!sc->built) {
    set_error("smx_distscene_score_poses on an empty scene: build it first");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  if (p->reject_rim && !sc->has_rim) {
    set_error("smx_distscene_score_poses: reject_rim needs a scene built by smx_recon_build_distscene_rim");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  if (q > sc->max_distance) {
    set_error("smx_distscene_score_poses: max_distance = %g is above the %g the scene was built for", (double)q, (double)sc->max_distance);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  k->q = q == 0.0f ? sc->max_distance : q;
  k->reject_rim = p->reject_rim;
  return SMX_OK;
}

// The scores of P poses into `scores` (host), written once, after everything else.  stamp: keep the timings of this pass.
int glob_score(smx_distscene sc, hipStream_t st, const GlobScoreK& k, const float* points, bool dev, uint32_t n_points, const float* poses, uint32_t P,
               smx_pose_score* scores, bool stamp) {
  GlobalWork& w = sc->glob;
  DistQueryWork& qw = sc->query;
  SMX_CALL(sc->reg.mark.sync());           // (a registration still running uses the query's workspace, which may grow here)
  const uint32_t m = k.m;
  if (m == 0) {                            // (no samples: every word of every pose is 0)
    memset(scores, 0, sizeof(smx_pose_score) * (size_t)P);
    return SMX_OK;
  }
  const uint32_t chunk = std::min<uint32_t>(P, std::max<uint32_t>(1u, w.chunk_points / m));   // poses of a chunk
  const size_t nc = (size_t)chunk * m;                                                        // at most max(2^24, 2^16) points

  // ---- every allocation of the call, before the first launch
  SMX_CALL(dist_scene_reserve(qw, (uint32_t)nc));
  SMX_CALL(w.moved.reserve(3 * nc));
  SMX_CALL(w.nearest.reserve(nc));
  SMX_CALL(w.distance.reserve(nc));
  SMX_CALL(w.poses.reserve(12 * (size_t)P));
  SMX_CALL(w.scores.reserve(P));
  const float* dpts = nullptr;
  SMX_CALL(stage_in(w.pts, points, (size_t)3 * n_points, dev, st, &dpts));
  SMX_HIP(hipMemcpyAsync(w.poses.get(), poses, sizeof(float) * 12 * (size_t)P, hipMemcpyHostToDevice, st));
  if (stamp) {
    SMX_CALL(w.whole.begin(st));
    SMX_CALL(w.last.begin(st));            // (the events exist before the first launch; begun again at the last chunk)
  }

  // ---- the chunks
  const DistSceneIndex ix{reinterpret_cast<const TgCell*>(sc->table.get()), sc->mask, reinterpret_cast<const TgRec*>(sc->recs.get()),
                          reinterpret_cast<const TgRec*>(sc->wide_recs.get()), sc->n_wide, sc->first_rec.get(), sc->counters.get()};
  const uint32_t q_word = cmp_dq(k.q);
  const uint32_t blocks_per_pose = (uint32_t)div_up(m, kGlobBlock);
  for (uint32_t first = 0; first < P; first += chunk) {
    const uint32_t n = std::min(chunk, P - first);
    const bool last = first + n == P;
    if (stamp && last) SMX_CALL(w.last.begin(st));
    hipLaunchKernelGGL(k_glob_move, dim3(n * blocks_per_pose), dim3(kGlobBlock), 0, st, w.poses.get() + 12 * (size_t)first, blocks_per_pose, dpts, k.stride,
                       m, w.moved.get());
    SMX_LAUNCH_CHECK();
    if (stamp && last) SMX_CALL(w.last.mark(st));
    SMX_CALL(dist_scene_enqueue(qw, ix, w.moved.get(), n * m, k.q, 0, w.nearest.get(), w.distance.get(), nullptr, st));
    if (stamp && last) SMX_CALL(w.last.mark(st));
    if (k.reject_rim)
      hipLaunchKernelGGL(k_glob_score<true>, dim3(n), dim3(kGlobBlock), 0, st, w.moved.get(), w.nearest.get(), w.distance.get(), m, q_word, ix.first_rec,
                         ix.recs, ix.wide_recs, sc->rim.get(), w.scores.get() + first);
    else
      hipLaunchKernelGGL(k_glob_score<false>, dim3(n), dim3(kGlobBlock), 0, st, w.moved.get(), w.nearest.get(), w.distance.get(), m, q_word, ix.first_rec,
                         ix.recs, ix.wide_recs, (const uint8_t*)nullptr, w.scores.get() + first);
    SMX_LAUNCH_CHECK();
    if (stamp && last) SMX_CALL(w.last.mark(st));
  }
  if (stamp) SMX_CALL(w.whole.mark(st));
  SMX_HIP(hipStreamSynchronize(st));       // (the call's one look at the device; the copy below is its one write to the caller)
  if (stamp) { w.whole.publish(); w.last.publish(); }
  SMX_HIP(hipMemcpy(scores, w.scores.get(), sizeof(smx_pose_score) * (size_t)P, hipMemcpyDeviceToHost));
  return SMX_OK;
}

float ms_since(const std::chrono::steady_clock::time_point& t0) {
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_register_pose_lattice(int32_t k, const double centre[3], const double* anchors, uint32_t A, float* poses, uint32_t capacity, uint32_t* count) {
  SMX_CHECK_ARG(count != nullptr);
  *count = 0;
  SMX_CHECK_ARG(k >= 1 && k <= kGlobMaxK && centre != nullptr && anchors != nullptr);
  const uint32_t n_rot = glob_lattice_rotations(k);
  SMX_CHECK_ARG(A >= 1 && A <= kGlobMaxPoses / n_rot);
  *count = n_rot * A;
  SMX_CHECK_ARG(poses != nullptr && capacity >= *count);
  for (int i = 0; i < 3; ++i) SMX_CHECK_ARG(centre[i] - centre[i] == 0.0);
  for (size_t i = 0; i < 3 * (size_t)A; ++i) SMX_CHECK_ARG(anchors[i] - anchors[i] == 0.0);
  glob_lattice(k, centre, anchors, A, poses);
  return SMX_OK;
}

int smx_global_params_default(smx_global_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->score.stride = 1; out->score.max_distance = 0.0f; out->score.reject_rim = 0;
  out->n_starts = 8; out->min_matched_fraction = 0.5f;
  return SMX_OK;
}

int smx_distscene_score_poses(smx_distscene sc, smx_stream s, const smx_score_params* p, const float* points, uint32_t n_points, int32_t on_device,
                              const float* poses, uint32_t P, smx_pose_score* scores) {
  SMX_CHECK_ARG(scores != nullptr);
  GlobScoreK k;
  SMX_CALL(glob_check(sc, p, points, n_points, poses, P, &k));
  const size_t score_bytes = sizeof(smx_pose_score) * (size_t)P;
  if (ranges_overlap(scores, score_bytes, poses, sizeof(float) * 12 * (size_t)P) ||
      (!on_device && ranges_overlap(scores, score_bytes, points, sizeof(float) * 3 * (size_t)n_points))) {
    set_error("scores of smx_distscene_score_poses overlaps an input");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  SMX_ON_DEVICE(sc->device);
  for (float& v : sc->glob.host_ms) v = 0.0f;
  return glob_score(sc, (hipStream_t)s, k, points, on_device != 0, n_points, poses, P, scores, true);
}

int smx_distscene_register_global(smx_distscene sc, smx_stream s, const smx_global_params* gp, const smx_register_params* p,
                                  const smx_register_robust_params* rp, const float* points, const float* normals, uint32_t n_points,
                                  int32_t on_device, const float* poses, uint32_t P, smx_global_result* out, smx_pose_score* all_scores) {
  SMX_CHECK_ARG(gp != nullptr && p != nullptr && out != nullptr);
  SMX_CHECK_ARG(gp->n_starts >= 1 && gp->n_starts <= kGlobMaxStarts);
  SMX_CHECK_ARG(gp->min_matched_fraction >= 0.0f && gp->min_matched_fraction <= 1.0f);
  GlobScoreK k;
  SMX_CALL(glob_check(sc, &gp->score, points, n_points, poses, P, &k));
  {
    const void* outs[2] = {out, all_scores};
    const size_t out_bytes[2] = {sizeof(*out), sizeof(smx_pose_score) * (size_t)P};
    for (int o = 0; o < 2; ++o)
      if (ranges_overlap(outs[o], out_bytes[o], poses, sizeof(float) * 12 * (size_t)P) ||
          (!on_device && (ranges_overlap(outs[o], out_bytes[o], points, sizeof(float) * 3 * (size_t)n_points) ||
                          ranges_overlap(outs[o], out_bytes[o], normals, sizeof(float) * 3 * (size_t)n_points)))) {
        set_error("an output of smx_distscene_register_global overlaps an input");
        return SMX_ERR_INVALID_ARGUMENT;
      }
    if (ranges_overlap(out, sizeof(*out), all_scores, out_bytes[1])) {
      set_error("out and all_scores of smx_distscene_register_global overlap");
      return SMX_ERR_INVALID_ARGUMENT;
    }
  }
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  GlobalWork& w = sc->glob;
  for (float& v : w.host_ms) v = 0.0f;

  // 1. every pose's score; the caller's memory is written at the very end only, so that a refusal by a later step writes nothing
  std::vector<smx_pose_score> all(P);
  SMX_CALL(glob_score(sc, st, k, points, on_device != 0, n_points, poses, P, all.data(), true));

  // 2. the starts
  auto t0 = std::chrono::steady_clock::now();
  uint32_t order[kGlobMaxStarts];
  const uint32_t M = glob_select([&](uint32_t i) { return (unsigned long long)all[i].cost; }, P, (uint32_t)gp->n_starts, order);
  w.host_ms[0] = ms_since(t0);

  // 3. the registration itself from every start (what it refuses, its first call refuses)
  t0 = std::chrono::steady_clock::now();
  const bool robust = rp && (rp->kernel != 0 || rp->reject_rim != 0);      // (anything not 0: what is out of range that call refuses)
  std::vector<smx_register_result> res(M);
  std::vector<float> after(12 * (size_t)M);
  for (uint32_t r = 0; r < M; ++r) {
    const float* T_init = poses + 12 * (size_t)order[r];
    if (robust) SMX_CALL(smx_distscene_register_robust(sc, s, p, rp, points, normals, n_points, on_device, T_init, &res[r], 0));
    else SMX_CALL(smx_distscene_register(sc, s, p, points, normals, n_points, on_device, T_init, &res[r], 0));
    std::copy_n(res[r].scene_T_points, 12, &after[12 * (size_t)r]);
  }
  w.host_ms[1] = ms_since(t0);

  // 4. the result poses' scores
  t0 = std::chrono::steady_clock::now();
  for (float v : after) SMX_CHECK_ARG(finite_f(v));
  std::vector<smx_pose_score> again(M);
  SMX_CALL(glob_score(sc, st, k, points, on_device != 0, n_points, after.data(), M, again.data(), false));
  w.host_ms[2] = ms_since(t0);

  // 5. the winner
  uint32_t win = 0;
  for (uint32_t r = 1; r < M; ++r)
    if (glob_before(again[r].cost, r, again[win].cost, win)) win = r;
  smx_global_result g;
  memset(&g, 0, sizeof(g));
  g.result = res[win];
  g.found = glob_found(res[win].status, again[win].n_matched, again[win].n_ok, gp->min_matched_fraction) ? 1 : 0;
  g.winner_rank = (int32_t)win; g.n_starts_run = (int32_t)M;
  for (uint32_t r = 0; r < M; ++r) {
    smx_global_start& t = g.starts[r];
    t.pose_index = order[r]; t.status = res[r].status; t.iterations_run = res[r].iterations_run;
    t.n_matched_after = again[r].n_matched; t.cost_before = all[order[r]].cost; t.cost_after = again[r].cost;
  }
  *out = g;
  if (all_scores) memcpy(all_scores, all.data(), sizeof(smx_pose_score) * (size_t)P);
  return SMX_OK;
}

int smx_distscene_debug_set_score_chunk(smx_distscene sc, uint32_t chunk_points) {
  SMX_CHECK_ARG(sc != nullptr && chunk_points >= 1 && chunk_points <= (1u << 24));
  sc->glob.chunk_points = chunk_points;
  return SMX_OK;
}

int smx_distscene_debug_global_timings(smx_distscene sc, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(sc != nullptr && out_ms != nullptr && capacity >= SMX_GLOBAL_PHASES);
  SMX_ON_DEVICE(sc->device);
  SMX_CALL(sc->glob.whole.elapsed_ms(out_ms, 1));
  SMX_CALL(sc->glob.last.elapsed_ms(out_ms + 1, 3));
  for (int i = 0; i < 3; ++i) out_ms[4 + i] = sc->glob.host_ms[i];
  return SMX_OK;
}

}  // extern "C"
