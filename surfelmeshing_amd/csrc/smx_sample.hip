// smx_sample.hip -- the kernels of smx_recon_sample_mesh and smx_recon_compare_meshes (gfx950): points drawn on a triangle array
// over the surfel map in proportion to area, one per stratum of the total weight, and the two one-sided surface distances
// between two triangle arrays (the contract is in include/smx.h, its arithmetic in smx_sample.hpp).
//
//   weights: k_smp_weights (a lane per triangle: range check, step 1's classes, q_t; the sum of the block's weights up to the
//            lane by wave64 shuffles and across the wavefronts in LDS, the block's weight to blocks[]; the counts per wavefront)
//   scan:    k_smp_scan (one workgroup walks blocks[] in chunks of 256: the saturated sum of the blocks before each, and W)
//            -> the one read-back of the call: the error word, W and the counts.  A refused call has written nothing.
//   draw:    k_smp_draw (a lane per sample: u_k, the block by an upper-bound search in blocks[], the triangle by one in the
//            block's 256 sums, the point, the normal, the barycentrics, each output's rows staged in LDS and stored as
//            consecutive words; n_triangles_hit against the lane before)
//   sums:    k_cmp_sums (smx_recon_compare_meshes: d_q and the two halves of its square per matched sample, summed per
//            wavefront, one 64-bit atomic per wavefront and word)
//
// Why the result does not depend on the schedule: q_t is a function of the triangle, the prefix is a sum of integers (saturating,
// which is associative on [0, 2^62]), and a sample is a function of k, seed, S and the prefix.  The counters are integer sums.
#include <cmath>

#include "smx_recon_state.hpp"
#include "smx_distscene.hpp"
#include "smx_sample.hpp"

namespace smx {

namespace {

__device__ __forceinline__ bool smp_live(const TgMap& map, uint32_t i, const TgVec& p) {
  return dec_live(p.x, p.y, p.z, map.normal[(size_t)i * map.normal_stride].w);
}

// incl[t] = the weights of t's block up to and including t; block_sums[b] = the weight of block b (below 2^54: no saturation)
__global__ void __launch_bounds__(kSmpBlock)
k_smp_weights(TgMap map, const uint32_t* __restrict__ tri, uint32_t n_in, unsigned long long* __restrict__ incl,
              unsigned long long* __restrict__ block_sums, uint32_t* __restrict__ cnt) {
  __shared__ unsigned long long wave_tot[kSmpBlock / 64];
  const uint32_t t = blockIdx.x * kSmpBlock + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t cls = 0xFFu;
  unsigned long long q = 0;
  bool bad_index = false;
  if (t < n_in) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= map.n || i1 >= map.n || i2 >= map.n) {
      bad_index = true;
    } else {
      const TgVec a = tg_pos(map, i0), b = tg_pos(map, i1), c = tg_pos(map, i2);
      cls = tg_classify(i0, i1, i2, smp_live(map, i0, a), smp_live(map, i1, b), smp_live(map, i2, c), a, b, c);
      if (cls == kTgInR) q = smp_weight(smp_face(a, b, c).a);
    }
  }
  unsigned long long sum = q;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(sum, off);
    if (lane >= (uint32_t)off) sum += o;
  }
  if (lane == 63) wave_tot[wave] = sum;
  __syncthreads();
  unsigned long long before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kSmpBlock / 64; ++w) {
    if ((uint32_t)w < wave) before += wave_tot[w];
    total += wave_tot[w];
  }
  if (t < n_in) incl[t] = before + sum;
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
  if (__ballot(bad_index) != 0 && lane == 0) atomicOr(&cnt[kSmpError], 1u);                     // (one per wavefront)
  wave_count(&cnt[kSmpNotLive], cls == kTgDropNotLive);
  wave_count(&cnt[kSmpRepeated], cls == kTgDropRepeated);
  wave_count(&cnt[kSmpRange], cls == kTgDropRange);
  wave_count(&cnt[kSmpZero], cls == kTgInR && q == 0);
}

// blocks[b]: the weight of block b -> sat(the weights of the blocks before b); W to the counters.  One workgroup.
__global__ void __launch_bounds__(kSmpBlock)
k_smp_scan(unsigned long long* __restrict__ blocks, uint32_t n_blocks, uint32_t* __restrict__ cnt) {
  __shared__ unsigned long long wave_tot[kSmpBlock / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;                              // sat(the blocks of the chunks before)
  for (uint32_t base = 0; base < n_blocks; base += kSmpBlock) {
    const uint32_t b = base + threadIdx.x;
    const unsigned long long mine = b < n_blocks ? blocks[b] : 0ull;
    // 256 words below 2^54 on top of a carry of at most 2^62: the plain sums stay below 2^63, and sat of a plain sum of
    // non-negative words is the saturated sum
    unsigned long long sum = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long o = __shfl_up(sum, off);
      if (lane >= (uint32_t)off) sum += o;
    }
    if (lane == 63) wave_tot[wave] = sum;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSmpBlock / 64; ++w) {
      if ((uint32_t)w < wave) before += wave_tot[w];
      total += wave_tot[w];
    }
    if (b < n_blocks) blocks[b] = smp_sat_add(carry, before + sum - mine);
    carry = smp_sat_add(carry, total);
    __syncthreads();                                         // (wave_tot is written again by the next chunk)
  }
  if (threadIdx.x == 0) { cnt[kSmpTotalLo] = (uint32_t)carry; cnt[kSmpTotalHi] = (uint32_t)(carry >> 32); }
}

struct SmpWords {
  const unsigned long long* p;
  __device__ __forceinline__ unsigned long long operator()(uint32_t i) const { return p[i]; }
};

// One output of kPer floats per sample for the workgroup's `count` samples from sample `first` on, staged in LDS so that
// consecutive lanes store consecutive words.  Every lane of the workgroup calls it.
template <int kPer>
__device__ __forceinline__ void smp_store_rows(float* __restrict__ out, float* s_row, uint32_t first, uint32_t count, const float (&mine)[kPer]) {
  __syncthreads();                                           // (the rows staged before are stored)
#pragma unroll
  for (int c = 0; c < kPer; ++c) s_row[kPer * threadIdx.x + c] = mine[c];
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < kPer * count; j += kSmpBlock) out[(size_t)kPer * first + j] = s_row[j];
}

// none != 0 (W < n_samples): every sample is "none".  Otherwise 1 <= S and every u_k < W.
__global__ void __launch_bounds__(kSmpBlock)
k_smp_draw(TgMap map, const uint32_t* __restrict__ tri_in, uint32_t n_in, const unsigned long long* __restrict__ block_off, uint32_t n_blocks,
           const unsigned long long* __restrict__ incl, unsigned long long S, uint32_t n_samples, uint32_t seed, int none,
           float* __restrict__ points, uint32_t* __restrict__ tri, float* __restrict__ bary, float* __restrict__ normals, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_t[kSmpBlock + 1];                    // [1 + lane] the lane's triangle, [0] that of the sample before the workgroup's first
  __shared__ float s_row[3 * kSmpBlock];
  const uint32_t first = blockIdx.x * kSmpBlock, k = first + threadIdx.x;       // (first < n_samples: the grid)
  const uint32_t count = n_samples - first < (uint32_t)kSmpBlock ? n_samples - first : (uint32_t)kSmpBlock;
  const bool in = threadIdx.x < count;
  const float nan = __builtin_nanf("");
  uint32_t t = kSmpNone;
  float P[3] = {nan, nan, nan}, N[3] = {nan, nan, nan}, vw[2] = {nan, nan};
  if (!none) {                                               // (uniform)
    const SmpWords off{block_off}, sums{incl};
    if (in) t = smp_find(off, n_blocks, sums, n_in, smp_stratum(k, S, smp_rand(k, 0, seed)));
    s_t[threadIdx.x + 1] = t;
    if (threadIdx.x == 0) s_t[0] = k == 0 ? kSmpNone : smp_find(off, n_blocks, sums, n_in, smp_stratum(k - 1, S, smp_rand(k - 1, 0, seed)));
    __syncthreads();
    wave_count(&cnt[kSmpHit], in && s_t[threadIdx.x] != t);
    if (in) {
      const TgVec A = tg_pos(map, tri_in[3 * (size_t)t]), B = tg_pos(map, tri_in[3 * (size_t)t + 1]), C = tg_pos(map, tri_in[3 * (size_t)t + 2]);
      const SmpFace f = smp_face(A, B, C);
      smp_bary(smp_rand(k, 1, seed), smp_rand(k, 2, seed), &vw[0], &vw[1]);
      const TgVec p = smp_point(A, f, vw[0], vw[1]), nrm = smp_normal(f);
      P[0] = p.x; P[1] = p.y; P[2] = p.z;
      N[0] = nrm.x; N[1] = nrm.y; N[2] = nrm.z;
    }
  }
  if (in) tri[k] = t;
  smp_store_rows<3>(points, s_row, first, count, P);
  if (bary) smp_store_rows<2>(bary, s_row, first, count, vw);
  if (normals) smp_store_rows<3>(normals, s_row, first, count, N);
}

// the three sums over the matched samples of one side
__global__ void __launch_bounds__(kSmpBlock)
k_cmp_sums(const uint32_t* __restrict__ nearest, const float* __restrict__ distance, uint32_t n_samples, uint32_t* __restrict__ cnt) {
  const uint32_t k = blockIdx.x * kSmpBlock + threadIdx.x;
  unsigned long long d = 0, lo = 0, hi = 0;
  if (k < n_samples && nearest[k] != kInvalid) {
    const uint32_t dq = cmp_dq(distance[k]);
    d = dq;
    cmp_square(dq, &lo, &hi);
  }
  d = wave_sum(d); lo = wave_sum(lo); hi = wave_sum(hi);
  if ((threadIdx.x & 63) != 0) return;
  if (d != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kCmpSumD), d);
  if (lo != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kCmpSumSqLo), lo);
  if (hi != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kCmpSumSqHi), hi);
}

bool sample_limits_ok(uint32_t n_in, uint32_t n_samples) { return n_in <= (1u << 28) && n_samples <= (1u << 28); }

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_recon_sample_mesh(smx_recon r, smx_stream s, const uint32_t* triangles, uint32_t n_in, uint32_t n_samples, uint32_t seed,
                          float* points, uint32_t* tri, float* bary, float* normals, int32_t on_device, smx_sample_stats* stats) {
  SMX_CHECK_ARG(r != nullptr);
  SMX_CHECK_ARG(sample_limits_ok(n_in, n_samples));
  SMX_CHECK_ARG(triangles != nullptr || n_in == 0);
  SMX_CHECK_ARG((points != nullptr && tri != nullptr) || n_samples == 0);
  {
    const void* outs[4] = {points, tri, bary, normals};
    const size_t out_bytes[4] = {(size_t)n_samples * 12, (size_t)n_samples * 4, (size_t)n_samples * 8, (size_t)n_samples * 12};
    for (int o = 0; o < 4; ++o)
      if (ranges_overlap(triangles, (size_t)n_in * 12, outs[o], out_bytes[o])) {
        set_error("an output of smx_recon_sample_mesh overlaps triangles");
        return SMX_ERR_INVALID_ARGUMENT;
      }
  }
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; stats->n_samples = n_samples; }
  SampleWork& w = r->sample;
  SMX_CALL(w.stamps.begin(st));
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    w.stamps.publish();
    return rc;
  };

  // ---- every allocation of the call: the workspace, the input on the device, the outputs' staging
  const bool dev = on_device != 0;
  const uint32_t nb = (uint32_t)div_up(n_in, kSmpBlock);
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kSmpWords, false));
  SMX_CALL(w.incl.reserve(n_in));
  SMX_CALL(w.blocks.reserve(nb));
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(w.in, triangles, (size_t)3 * n_in, dev, st, &din));
  float *d_points = points, *d_bary = bary, *d_normals = normals;
  uint32_t* d_tri = tri;
  if (!dev && n_samples > 0) {
    SMX_CALL(w.out_points.reserve((size_t)3 * n_samples));
    SMX_CALL(w.out_tri.reserve(n_samples));
    if (bary) SMX_CALL(w.out_bary.reserve((size_t)2 * n_samples));
    if (normals) SMX_CALL(w.out_normals.reserve((size_t)3 * n_samples));
    d_points = w.out_points.get(); d_tri = w.out_tri.get();
    d_bary = bary ? w.out_bary.get() : nullptr; d_normals = normals ? w.out_normals.get() : nullptr;
  }
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kSmpWords * sizeof(uint32_t), st));

  // ---- weights
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const TgMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  const dim3 b(kSmpBlock);
  if (n_in > 0) {
    hipLaunchKernelGGL(k_smp_weights, dim3(nb), b, 0, st, map, din, n_in, w.incl.get(), w.blocks.get(), cnt);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- scan, and the one read-back: a refused call has published the weights and written nothing
  if (n_in > 0) {
    hipLaunchKernelGGL(k_smp_scan, dim3(1), b, 0, st, w.blocks.get(), nb, cnt);
    SMX_LAUNCH_CHECK();
  }
  uint32_t h[kSmpWords];
  SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (h[kSmpError] != 0) {
    set_error("triangles holds an index >= the %u slots of the map", n);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  const unsigned long long W = word64(h, kSmpTotalLo);
  if (W >= kSmpSat) {
    set_error("total area too large: the weights of smx_recon_sample_mesh sum to 2^62 units or more");
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- draw
  const bool none = W < n_samples;
  const unsigned long long S = n_samples > 0 ? W / n_samples : 0ull;
  if (n_samples > 0) {
    hipLaunchKernelGGL(k_smp_draw, dim3(blocks_for(n_samples)), b, 0, st, map, din, n_in, w.blocks.get(), nb, w.incl.get(), S, n_samples, seed,
                       none ? 1 : 0, d_points, d_tri, d_bary, d_normals, cnt);
    SMX_LAUNCH_CHECK();
    if (!dev) {
      SMX_HIP(hipMemcpyAsync(points, d_points, (size_t)n_samples * 12, hipMemcpyDeviceToHost, st));
      SMX_HIP(hipMemcpyAsync(tri, d_tri, (size_t)n_samples * 4, hipMemcpyDeviceToHost, st));
      if (bary) SMX_HIP(hipMemcpyAsync(bary, d_bary, (size_t)n_samples * 8, hipMemcpyDeviceToHost, st));
      if (normals) SMX_HIP(hipMemcpyAsync(normals, d_normals, (size_t)n_samples * 12, hipMemcpyDeviceToHost, st));
    }
  }
  uint32_t n_hit = 0;
  SMX_HIP(hipMemcpyAsync(&n_hit, cnt + kSmpHit, sizeof(n_hit), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (stats) {
    stats->n_not_live = h[kSmpNotLive]; stats->n_repeated = h[kSmpRepeated]; stats->n_out_of_range = h[kSmpRange];
    stats->n_zero_weight = h[kSmpZero];
    stats->n_none = none ? n_samples : 0u;
    stats->n_triangles_hit = n_hit;
    stats->total_weight = W; stats->stride = S;
  }
  SMX_CALL(w.stamps.mark(st));
  return finish(SMX_OK);
}

int smx_recon_debug_sample_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_SAMPLE_PHASES);
  SMX_ON_DEVICE(r->device);
  return r->sample.stamps.elapsed_ms(out_ms, SMX_SAMPLE_PHASES);
}

int smx_recon_compare_meshes(smx_recon r, smx_stream s, const smx_compare_params* p, const uint32_t* triangles_a, uint32_t n_a,
                             const uint32_t* triangles_b, uint32_t n_b, int32_t on_device, smx_compare_stats* out) {
  SMX_CHECK_ARG(out != nullptr);
  memset(out, 0, sizeof(*out));
  SMX_CHECK_ARG(r != nullptr && p != nullptr);
  SMX_CHECK_ARG(p->directions >= 1 && p->directions <= 3);
  // the limits of the two halves, before anything is allocated or launched
  SMX_CHECK_ARG(finite_f(p->max_distance) && p->max_distance >= 1e-3f && p->max_distance <= 16.0f);
  SMX_CHECK_ARG(finite_f(p->cell_size) && p->cell_size >= 0.0f);
  SMX_CHECK_ARG(sample_limits_ok(n_a, p->n_samples) && sample_limits_ok(n_b, p->n_samples));
  SMX_CHECK_ARG((triangles_a != nullptr || n_a == 0) && (triangles_b != nullptr || n_b == 0));
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  CompareWork& w = r->compare;
  const uint32_t ns = p->n_samples;
  const bool dev = on_device != 0;
  auto side_of = [&](int side, const uint32_t* from, uint32_t n_from, const uint32_t* onto, uint32_t n_onto, smx_compare_side* o) -> int {
    if (!(p->directions & (1 << side))) {                    // (its three phases read 0 ms: smx_recon_debug_compare_timings)
      for (int k = 0; k < 3; ++k) SMX_CALL(w.stamps.mark(st));
      return SMX_OK;
    }
    // the two calls the side is defined by, on device arrays: the samples stay in the workspace
    const smx_distance_params dp{p->max_distance, p->cell_size, 0};
    SMX_CALL(smx_recon_sample_mesh(r, s, from, n_from, ns, p->seed, w.points.get(), w.tri.get(), nullptr, nullptr, 1, &o->sample));
    SMX_CALL(w.stamps.mark(st));
    SMX_CALL(smx_recon_mesh_distance(r, s, &dp, onto, n_onto, w.points.get(), ns, w.nearest.get(), w.distance.get(), nullptr, 1, &o->distance));
    SMX_CALL(w.stamps.mark(st));
    uint32_t* cnt = w.counters.get();
    SMX_HIP(hipMemsetAsync(cnt, 0, kSmpWords * sizeof(uint32_t), st));
    if (ns > 0) {
      hipLaunchKernelGGL(k_cmp_sums, dim3(blocks_for(ns)), dim3(kSmpBlock), 0, st, w.nearest.get(), w.distance.get(), ns, cnt);
      SMX_LAUNCH_CHECK();
    }
    uint32_t h[kSmpWords];
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    o->sum_d = word64(h, kCmpSumD); o->sum_sq_lo = word64(h, kCmpSumSqLo); o->sum_sq_hi = word64(h, kCmpSumSqHi);
    return w.stamps.mark(st);
  };
  auto run = [&]() -> int {
    if (!w.counters.get()) SMX_CALL(w.counters.alloc(kSmpWords, false));
    SMX_CALL(w.points.reserve((size_t)3 * ns));
    SMX_CALL(w.tri.reserve(ns));
    SMX_CALL(w.nearest.reserve(ns));
    SMX_CALL(w.distance.reserve(ns));
    const uint32_t* da = nullptr;
    const uint32_t* db = nullptr;
    SMX_CALL(stage_in(w.in_a, triangles_a, (size_t)3 * n_a, dev, st, &da));
    SMX_CALL(stage_in(w.in_b, triangles_b, (size_t)3 * n_b, dev, st, &db));
    SMX_CALL(w.stamps.begin(st));
    w.directions = p->directions;
    SMX_CALL(side_of(0, da, n_a, db, n_b, &out->a_to_b));
    SMX_CALL(side_of(1, db, n_b, da, n_a, &out->b_to_a));
    SMX_HIP(hipStreamSynchronize(st));
    w.stamps.publish();
    return SMX_OK;
  };
  const int rc = run();
  if (rc != SMX_OK) {                                        // (a refusal by either half is the call's)
    (void)hipStreamSynchronize(st);
    memset(out, 0, sizeof(*out));
  }
  return rc;
}

// One side of the comparison against a kept index: the samples of `triangles` on r's map as it stands, measured against the
// scene's snapshot.  The two calls it is defined by, on device arrays: the samples stay in the comparison's workspace.
int smx_recon_compare_to_distscene(smx_recon r, smx_stream s, smx_distscene sc, float max_distance, uint32_t n_samples, uint32_t seed,
                                   const uint32_t* triangles, uint32_t n_in, int32_t on_device, smx_compare_side* out) {
  SMX_CHECK_ARG(out != nullptr);
  memset(out, 0, sizeof(*out));
  SMX_CHECK_ARG(r != nullptr && sc != nullptr);
  SMX_CHECK_ARG(sc->device == r->device);
  // the limits of the two halves, before anything is allocated or launched
  SMX_CHECK_ARG(finite_f(max_distance) && max_distance >= 1e-3f && max_distance <= 16.0f);
  SMX_CHECK_ARG(sample_limits_ok(n_in, n_samples));
  SMX_CHECK_ARG(triangles != nullptr || n_in == 0);
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  CompareWork& w = r->compare;
  auto run = [&]() -> int {
    if (!w.counters.get()) SMX_CALL(w.counters.alloc(kSmpWords, false));
    SMX_CALL(w.points.reserve((size_t)3 * n_samples));
    SMX_CALL(w.tri.reserve(n_samples));
    SMX_CALL(w.nearest.reserve(n_samples));
    SMX_CALL(w.distance.reserve(n_samples));
    const uint32_t* din = nullptr;
    SMX_CALL(stage_in(w.in_a, triangles, (size_t)3 * n_in, on_device != 0, st, &din));
    const smx_distance_params dp{max_distance, 0.0f, 0};
    SMX_CALL(smx_recon_sample_mesh(r, s, din, n_in, n_samples, seed, w.points.get(), w.tri.get(), nullptr, nullptr, 1, &out->sample));
    SMX_CALL(smx_distscene_query(sc, s, &dp, w.points.get(), n_samples, w.nearest.get(), w.distance.get(), nullptr, 1, &out->distance));
    uint32_t* cnt = w.counters.get();
    SMX_HIP(hipMemsetAsync(cnt, 0, kSmpWords * sizeof(uint32_t), st));
    if (n_samples > 0) {
      hipLaunchKernelGGL(k_cmp_sums, dim3(blocks_for(n_samples)), dim3(kSmpBlock), 0, st, w.nearest.get(), w.distance.get(), n_samples, cnt);
      SMX_LAUNCH_CHECK();
    }
    uint32_t h[kSmpWords];
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    out->sum_d = word64(h, kCmpSumD); out->sum_sq_lo = word64(h, kCmpSumSqLo); out->sum_sq_hi = word64(h, kCmpSumSqHi);
    return SMX_OK;
  };
  const int rc = run();
  if (rc != SMX_OK) {                                        // (a refusal by either half is the call's)
    (void)hipStreamSynchronize(st);
    memset(out, 0, sizeof(*out));
  }
  return rc;
}

int smx_recon_debug_compare_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_COMPARE_PHASES);
  SMX_ON_DEVICE(r->device);
  SMX_CALL(r->compare.stamps.elapsed_ms(out_ms, SMX_COMPARE_PHASES));
  for (int side = 0; side < 2; ++side)
    if (!(r->compare.directions & (1 << side)))
      for (int k = 0; k < 3; ++k) out_ms[3 * side + k] = 0.0f;
  return SMX_OK;
}

}  // extern "C"
