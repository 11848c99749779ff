// smx_distance.hip -- the kernels of smx_recon_mesh_distance (gfx950): for each of many points the closest point on a triangle
// array over the surfel map, exactly the minimum over all triangles (the contract is in include/smx.h, its
// distance arithmetic in smx_distance.hpp, the cell functions and the table operations in smx_trigrid.hpp).
//
//   mark:   tg_enqueue_mark of smx_trigrid.hip with the boxes as they are and c >= 1.125 max_distance
//   index:  tg_enqueue_index of smx_trigrid.hip, its sort buffers sized for the points' keys too
//   query:  k_dist_point_keys -> the same sort -> k_dist_query (a workgroup per tile of 256 points in cell order = a run of
//           occupied query cells: per cell 27 look-ups, the neighbour cells' packed records staged in LDS in chunks, the lanes
//           dealt out as walkers over the staged records with one 64-bit key each and an integer LDS minimum per point; the
//           wide list staged behind the cells; the answer goes to the point's place in the input order)
//   stats:  k_dist_stats (histogram, counts and maximum: integer atomics, one per wavefront and word)
//
// Why the result does not depend on the schedule: every output of a point is a function of the minimum of a set of 64-bit keys,
// and the set is the candidates of ALL of R whatever c is; the counters are integer sums and one integer
// maximum; c itself may depend on the order of nothing either (an integer sum), though the result would not care.
//
// One query body serves two kernels: k_dist_query for the call, which re-reads the winner's corners from the map, and
// k_dscene_query for a kept scene (smx_distscene.hip), which reads them from a record of the winner.
// dist_scene_query, behind the kernels, is the host side of a scene's query: the query and stats phases on a kept index.  Its
// enqueue-only half (dist_scene_reserve, then dist_scene_enqueue: keys, sort, walk) is what smx_distscene_register runs per
// iteration (smx_register.hip).
//
// smx_recon_mesh_distance itself is at the end of the file: it owns the order of the phases, the workspace (DistanceWork,
// smx_distance.hpp) and the second read of the counters (the first is tg_read_counts).
#include <cmath>

#include "smx_recon_state.hpp"
#include "smx_distscene.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

constexpr int kDBlock = kDistBlock;
constexpr unsigned long long kDistBadCell = 0x7FFFFFFFFFFFFFFFull;   // the sort key of a BAD point: behind every cell

__device__ __forceinline__ TgVec dist_point(const float* points, uint32_t p) {
  return TgVec{points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
}

// a BAD point gets the largest 63-bit key: it sorts behind every cell, and its lanes walk nothing
__global__ void __launch_bounds__(kDBlock)
k_dist_point_keys(const float* __restrict__ points, uint32_t n_points, const uint32_t* __restrict__ cnt, unsigned long long* __restrict__ keys,
                  uint32_t* __restrict__ vals) {
  const uint32_t p = blockIdx.x * kDBlock + threadIdx.x;
  if (p >= n_points) return;
  const TgVec P = dist_point(points, p);
  const float cell = tg_cell_of(cnt);
  keys[p] = tg_point_ok(P) ? dec_cell_key(tg_cell(P.x, cell), tg_cell(P.y, cell), tg_cell(P.z, cell)) : kDistBadCell;
  vals[p] = p;
}

constexpr uint32_t kDistChunk = 2 * kDBlock;                                // records staged at a time: two per lane, 24 KB

// the staged chunk: three 16-byte reads per record, the same address for the lanes that share a record (a broadcast)
struct DistLdsRecs {
  const float4 *a, *b, *c;
  __device__ __forceinline__ void load(uint32_t j, TgVec* A, TgVec* B, TgVec* C, uint32_t* t) const {
    const float4 x = a[j], y = b[j], z = c[j];
    *A = TgVec{x.x, x.y, x.z}; *B = TgVec{y.x, y.y, y.z}; *C = TgVec{z.x, z.y, z.z};
    *t = __float_as_uint(x.w);
  }
};
struct DistStage {                    // the workgroup's LDS as the helpers see it
  float4 *a, *b, *c;                  // [kDistChunk]
  unsigned long long* best;           // [kDBlock] the smallest key of every point of the tile so far
  const float *px, *py, *pz;          // [kDBlock] the tile's points
};

// `total` records, number g of them at src(g), tested for the `na` points [pos, pos + na) of the tile: staged in chunks, two
// loads per lane in flight before the first store; the lanes are dealt out as kDBlock / na walkers per point, walker q taking
// the staged records q, q + walkers, ..., and every walker folds its minimum into the point's key by an integer LDS minimum,
// which does not depend on the order.  Every lane of the workgroup reaches every barrier: total, pos and na are uniform.
template <class Src>
__device__ __forceinline__ void dist_stage_and_walk(const DistStage& st, const Src& src, uint32_t total, uint32_t pos, uint32_t na, float max2) {
  const uint32_t tid = threadIdx.x;
  const uint32_t walkers = na != 0 ? kDBlock / na : 0u, mine = na != 0 ? tid % na : 0u, q = na != 0 ? tid / na : 0u;
  const bool walking = na != 0 && q < walkers;
  TgVec P{0.0f, 0.0f, 0.0f};
  if (walking) P = TgVec{st.px[pos + mine], st.py[pos + mine], st.pz[pos + mine]};
  unsigned long long best = kTgNone;
  for (uint32_t base = 0; base < total; base += kDistChunk) {
    const uint32_t m = total - base < kDistChunk ? total - base : kDistChunk;
    const bool h0 = tid < m, h1 = tid + kDBlock < m;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 a0 = zero, b0 = zero, c0 = zero, a1 = zero, b1 = zero, c1 = zero;
    if (h0) { const TgRec* r = src(base + tid); a0 = r->a; b0 = r->b; c0 = r->c; }
    if (h1) { const TgRec* r = src(base + tid + kDBlock); a1 = r->a; b1 = r->b; c1 = r->c; }
    if (h0) { st.a[tid] = a0; st.b[tid] = b0; st.c[tid] = c0; }
    if (h1) { st.a[tid + kDBlock] = a1; st.b[tid + kDBlock] = b1; st.c[tid + kDBlock] = c1; }
    __syncthreads();
    if (walking) best = dist_walk(DistLdsRecs{st.a, st.b, st.c}, q, m, P, max2, best, walkers);
    __syncthreads();
  }
  if (walking && best != kTgNone) atomicMin(&st.best[pos + mine], best);
}

// the 27 neighbour runs of a cell as one sequence of records
struct DistCellSrc {
  const TgRec* recs;
  const uint32_t *first, *off;        // LDS: [27] first record of the run, [28] offsets of the runs in the sequence
  __device__ __forceinline__ const TgRec* operator()(uint32_t g) const {
    uint32_t k = 0;
    while (k < 26 && g >= off[k + 1]) ++k;
    return recs + first[k] + (g - off[k]);
  }
};
struct DistWideSrc {
  const TgRec* recs;
  __device__ __forceinline__ const TgRec* operator()(uint32_t g) const { return recs + g; }
};

// Where the winner's corners come from.  The call re-reads them through the caller's triangle array from the map; a kept scene
// reads any record of the winner (first_rec names one): the same float32 words, so the same Q and the same sign.
struct DistCornersFromMap {
  TgMap map;
  const uint32_t* tri;
  __device__ __forceinline__ void load(uint32_t t, TgVec* A, TgVec* B, TgVec* C) const {
    *A = tg_pos(map, tri[3 * (size_t)t]); *B = tg_pos(map, tri[3 * (size_t)t + 1]); *C = tg_pos(map, tri[3 * (size_t)t + 2]);
  }
};
struct DistCornersFromRecs {
  const uint32_t* first_rec;
  const TgRec *recs, *wide_recs;
  __device__ __forceinline__ void load(uint32_t t, TgVec* A, TgVec* B, TgVec* C) const {
    uint32_t held;
    const uint32_t word = first_rec[t];                      // (t came out of a record, so it has one; if not: NaN, which shows)
    *A = *B = *C = TgVec{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
    if (word != kDsceneNoRec) dscene_winner(word, TgDeviceRecs{recs}, TgDeviceRecs{wide_recs}, A, B, C, &held);
  }
};

// A workgroup per tile of 256 points in cell order = a run of occupied query cells.  Cell after cell: 27 lanes look the
// neighbour cells up, the workgroup stages their packed records in LDS in chunks and the lanes walk the staged records for the
// points of that cell; the wide list is staged the same way behind the cells, for all points of the tile.  (A cell whose points
// straddle two tiles is staged by both.)  Then every lane writes the answer of its own point to the point's place in the input.
// One body for the two kernels below.
template <class Corners>
__device__ __forceinline__ void
dist_query_tile(const Corners& corners, const float* __restrict__ points, uint32_t n_points, const unsigned long long* __restrict__ cell_keys,
                const uint32_t* __restrict__ order, const TgCell* __restrict__ table, uint32_t mask, const TgRec* __restrict__ recs,
                const TgRec* __restrict__ wide_recs, uint32_t n_wide, const uint32_t* __restrict__ cnt, float max2, int signed_distance,
                uint32_t* __restrict__ nearest, float* __restrict__ distance, float* __restrict__ closest, unsigned long long* __restrict__ best_out) {
  __shared__ float4 s_a[kDistChunk], s_b[kDistChunk], s_c[kDistChunk];
  __shared__ unsigned long long s_key[kDBlock], s_best[kDBlock];
  __shared__ float s_px[kDBlock], s_py[kDBlock], s_pz[kDBlock];
  __shared__ uint32_t s_first[27], s_count[27], s_off[28];
  const uint32_t tid = threadIdx.x, j = blockIdx.x * kDBlock + tid;
  const bool in = j < n_points;
  const uint32_t p = in ? order[j] : 0u;
  const TgVec P = in ? dist_point(points, p) : TgVec{0.0f, 0.0f, 0.0f};
  const unsigned long long my_cell = in ? cell_keys[j] : kDistBadCell;
  s_key[tid] = my_cell; s_best[tid] = kTgNone;
  s_px[tid] = P.x; s_py[tid] = P.y; s_pz[tid] = P.z;
  // the keys ascend, so the good points of the tile are its first n_good lanes
  const uint32_t n_good = (uint32_t)__syncthreads_count(my_cell != kDistBadCell);
  const float cell = tg_cell_of(cnt);
  const DistStage st{s_a, s_b, s_c, s_best, s_px, s_py, s_pz};
  uint32_t pos = 0;
  while (pos < n_good) {
    const unsigned long long cur = s_key[pos];
    const uint32_t na = (uint32_t)__syncthreads_count(my_cell == cur);       // (the lanes [pos, pos + na))
    if (tid < 27) {
      const TgDeviceTable tab{const_cast<TgCell*>(table)};
      uint32_t first = 0, end = 0;
      const bool found = tg_table_find(tab, mask, dist_neighbour_key(tg_cell(s_px[pos], cell), tg_cell(s_py[pos], cell),
                                                                      tg_cell(s_pz[pos], cell), tid), &first, &end);
      s_first[tid] = first; s_count[tid] = found ? end - first : 0u;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t sum = 0;
      for (int k = 0; k < 27; ++k) { s_off[k] = sum; sum += s_count[k]; }
      s_off[27] = sum;
    }
    __syncthreads();
    dist_stage_and_walk(st, DistCellSrc{recs, s_first, s_off}, s_off[27], pos, na, max2);
    pos += na;
  }
  dist_stage_and_walk(st, DistWideSrc{wide_recs}, n_wide, 0u, n_good, max2);
  __syncthreads();
  if (!in) return;
  const unsigned long long key = s_best[tid];
  uint32_t t = kInvalid;
  float d = __builtin_inff();
  TgVec Q{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if (key != kTgNone) {
    t = (uint32_t)key;
    TgVec A, B, C;
    corners.load(t, &A, &B, &C);
    uint32_t region;
    Q = dist_closest(P, A, B, C, &region);
    d = sqrtf(tg_key_float(key));
    if (signed_distance && dist_negative(P, Q, A, B, C)) d = -d;
  }
  best_out[p] = key;
  nearest[p] = t;
  distance[p] = d;
  if (closest) { closest[3 * (size_t)p] = Q.x; closest[3 * (size_t)p + 1] = Q.y; closest[3 * (size_t)p + 2] = Q.z; }
}

// The two kernels over it: the call's, and a kept scene's (smx_distscene), which reads neither the map nor the
// caller's triangle array.
__global__ void __launch_bounds__(kDBlock)
k_dist_query(TgMap map, const uint32_t* __restrict__ tri, const float* __restrict__ points, uint32_t n_points,
             const unsigned long long* __restrict__ cell_keys, const uint32_t* __restrict__ order, const TgCell* __restrict__ table,
             uint32_t mask, const TgRec* __restrict__ recs, const TgRec* __restrict__ wide_recs, uint32_t n_wide,
             const uint32_t* __restrict__ cnt, float max2, int signed_distance, uint32_t* __restrict__ nearest, float* __restrict__ distance,
             float* __restrict__ closest, unsigned long long* __restrict__ best_out) {
  dist_query_tile(DistCornersFromMap{map, tri}, points, n_points, cell_keys, order, table, mask, recs, wide_recs, n_wide, cnt, max2, signed_distance,
                  nearest, distance, closest, best_out);
}
__global__ void __launch_bounds__(kDBlock)
k_dscene_query(const uint32_t* __restrict__ first_rec, const float* __restrict__ points, uint32_t n_points,
               const unsigned long long* __restrict__ cell_keys, const uint32_t* __restrict__ order, const TgCell* __restrict__ table,
               uint32_t mask, const TgRec* __restrict__ recs, const TgRec* __restrict__ wide_recs, uint32_t n_wide,
               const uint32_t* __restrict__ cnt, float max2, int signed_distance, uint32_t* __restrict__ nearest, float* __restrict__ distance,
               float* __restrict__ closest, unsigned long long* __restrict__ best_out) {
  dist_query_tile(DistCornersFromRecs{first_rec, recs, wide_recs}, points, n_points, cell_keys, order, table, mask, recs, wide_recs, n_wide, cnt, max2,
                  signed_distance, nearest, distance, closest, best_out);
}

__global__ void __launch_bounds__(kDBlock)
k_dist_stats(const float* __restrict__ points, uint32_t n_points, const unsigned long long* __restrict__ best, float max_distance,
             uint32_t* __restrict__ cnt) {
  const uint32_t p = blockIdx.x * kDBlock + threadIdx.x;
  bool bad = false, matched = false;
  uint32_t bits = 0, bin = kDistBins;
  if (p < n_points) {
    bad = !tg_point_ok(dist_point(points, p));
    const unsigned long long key = best[p];
    matched = key != kTgNone;
    if (matched) { bits = (uint32_t)(key >> 32); bin = dist_bin(sqrtf(tg_key_float(key)), max_distance); }
  }
  wave_count(&cnt[kDistBadPoints], bad);
  wave_count(&cnt[kDistMatched], matched);
  if (__ballot(matched) == 0) return;                        // (uniform over the wavefront)
  for (uint32_t b = 0; b < kDistBins; ++b) wave_count(&cnt[kDistHist + b], bin == b);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)bits, off); bits = o > bits ? o : bits; }
  if ((threadIdx.x & 63) == 0) atomicMax(&cnt[kDistMaxBits], bits);    // (bits of non-negative floats order as the floats do)
}

}  // namespace

unsigned long long DistQueryWork::bytes() const {
  auto of = [](const auto& b) { return (unsigned long long)b.capacity() * sizeof(*b.get()); };
  return of(keys[0]) + of(keys[1]) + of(vals[0]) + of(vals[1]) + of(hist) + of(best) + of(pts) + of(out_distance) + of(out_closest) +
         of(out_nearest) + of(counters);
}

int dist_scene_reserve(DistQueryWork& w, uint32_t n_points) {
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kDistWords, false));
  SMX_CALL(w.best.reserve(n_points));
  for (int k = 0; k < 2; ++k) { SMX_CALL(w.keys[k].reserve(n_points)); SMX_CALL(w.vals[k].reserve(n_points)); }
  SMX_CALL(w.hist.reserve(radix_sort_workspace_elems(n_points)));
  return SMX_OK;
}

int dist_scene_enqueue(const DistQueryWork& w, const DistSceneIndex& ix, const float* dpts, uint32_t n_points, float max_distance,
                       int signed_distance, uint32_t* d_nearest, float* d_distance, float* d_closest, hipStream_t st) {
  if (n_points == 0) return SMX_OK;
  const dim3 g_pts(blocks_for(n_points)), b(kDistBlock);
  hipLaunchKernelGGL(k_dist_point_keys, g_pts, b, 0, st, dpts, n_points, ix.cnt, w.keys[0].get(), w.vals[0].get());
  SMX_LAUNCH_CHECK();
  const int cur = radix_sort(w.keys, w.vals, n_points, 63, w.hist.get(), st);
  hipLaunchKernelGGL(k_dscene_query, g_pts, b, 0, st, ix.first_rec, dpts, n_points, w.keys[cur].get(), w.vals[cur].get(), ix.table, ix.mask, ix.recs,
                     ix.wide_recs, ix.n_wide, ix.cnt, max_distance * max_distance, signed_distance, d_nearest, d_distance, d_closest, w.best.get());
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int dist_scene_query(DistQueryWork& w, const DistSceneIndex& ix, const smx_distance_params* p, const float* points, uint32_t n_points,
                     uint32_t* nearest, float* distance, float* closest, bool dev, hipStream_t st, PhaseStamps<2>& stamps,
                     smx_distance_stats* stats) {
  // ---- every allocation of the query: the counters, the keys, the sort's buffers, the staging
  SMX_CALL(dist_scene_reserve(w, n_points));
  const float* dpts = nullptr;
  SMX_CALL(stage_in(w.pts, points, (size_t)3 * n_points, dev, st, &dpts));
  uint32_t* d_nearest = nearest;
  float* d_distance = distance;
  float* d_closest = closest;
  if (!dev && n_points > 0) {
    SMX_CALL(w.out_nearest.reserve(n_points));
    SMX_CALL(w.out_distance.reserve(n_points));
    if (closest) SMX_CALL(w.out_closest.reserve((size_t)3 * n_points));
    d_nearest = w.out_nearest.get(); d_distance = w.out_distance.get(); d_closest = closest ? w.out_closest.get() : nullptr;
  }
  SMX_CALL(stamps.begin(st));
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    stamps.publish();
    return rc;
  };
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kDistWords * sizeof(uint32_t), st));
  const dim3 b(kDistBlock);

  // ---- query
  SMX_CALL(dist_scene_enqueue(w, ix, dpts, n_points, p->max_distance, (int)p->signed_distance, d_nearest, d_distance, d_closest, st));
  SMX_CALL(stamps.mark(st));

  // ---- stats
  if (n_points > 0) {
    hipLaunchKernelGGL(k_dist_stats, dim3(blocks_for(n_points)), b, 0, st, dpts, n_points, w.best.get(), p->max_distance, cnt);
    SMX_LAUNCH_CHECK();
    if (!dev) {
      SMX_HIP(hipMemcpyAsync(nearest, d_nearest, (size_t)n_points * 4, hipMemcpyDeviceToHost, st));
      SMX_HIP(hipMemcpyAsync(distance, d_distance, (size_t)n_points * 4, hipMemcpyDeviceToHost, st));
      if (closest) SMX_HIP(hipMemcpyAsync(closest, d_closest, (size_t)n_points * 12, hipMemcpyDeviceToHost, st));
    }
  }
  uint32_t h[kDistWords];
  SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (stats) {
    stats->n_bad_points = h[kDistBadPoints]; stats->n_matched = h[kDistMatched]; stats->max_dist2_bits = h[kDistMaxBits];
    for (uint32_t k = 0; k < kDistBins; ++k) stats->histogram[k] = h[kDistHist + k];
  }
  SMX_CALL(stamps.mark(st));
  return finish(SMX_OK);
}

}  // namespace smx

using namespace smx;

extern "C" {

int smx_distance_params_default(smx_distance_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->max_distance = 0.05f; out->cell_size = 0.0f; out->signed_distance = 0;
  return SMX_OK;
}

int smx_recon_mesh_distance(smx_recon r, smx_stream s, const smx_distance_params* p, const uint32_t* triangles, uint32_t n_in,
                            const float* points, uint32_t n_points, uint32_t* nearest, float* distance, float* closest,
                            int32_t on_device, smx_distance_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && p != nullptr);
  SMX_CHECK_ARG(finite_f(p->max_distance) && p->max_distance >= 1e-3f && p->max_distance <= 16.0f);
  SMX_CHECK_ARG(finite_f(p->cell_size) && p->cell_size >= 0.0f);
  SMX_CHECK_ARG(p->signed_distance == 0 || p->signed_distance == 1);
  SMX_CHECK_ARG(n_in <= (1u << 28) && n_points <= (1u << 28));
  SMX_CHECK_ARG(triangles != nullptr || n_in == 0);
  SMX_CHECK_ARG((points != nullptr && nearest != nullptr && distance != nullptr) || n_points == 0);
  {
    const void* ins[2] = {triangles, points};
    const size_t in_bytes[2] = {(size_t)n_in * 12, (size_t)n_points * 12};
    const void* outs[3] = {nearest, distance, closest};
    const size_t out_bytes[3] = {(size_t)n_points * 4, (size_t)n_points * 4, (size_t)n_points * 12};
    for (int i = 0; i < 2; ++i)
      for (int o = 0; o < 3; ++o)
        if (ranges_overlap(ins[i], in_bytes[i], outs[o], out_bytes[o])) {
          set_error("an output of smx_recon_mesh_distance overlaps %s", i == 0 ? "triangles" : "points");
          return SMX_ERR_INVALID_ARGUMENT;
        }
  }
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; stats->n_points = n_points; }
  DistanceWork& w = r->distance;
  SMX_CALL(w.stamps.begin(st));
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    w.stamps.publish();
    return rc;
  };

  // ---- workspace of the first phase; the inputs on the device; the outputs' staging
  const bool dev = on_device != 0;
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kDistWords, false));
  SMX_CALL(w.grid.reserve_mark(n_in));
  SMX_CALL(w.best.reserve(n_points));
  const uint32_t* din = nullptr;
  const float* dpts = nullptr;
  SMX_CALL(stage_in(w.in, triangles, (size_t)3 * n_in, dev, st, &din));
  SMX_CALL(stage_in(w.pts, points, (size_t)3 * n_points, dev, st, &dpts));
  uint32_t* d_nearest = nearest;
  float* d_distance = distance;
  float* d_closest = closest;
  if (!dev && n_points > 0) {
    SMX_CALL(w.out_nearest.reserve(n_points));
    SMX_CALL(w.out_distance.reserve(n_points));
    if (closest) SMX_CALL(w.out_closest.reserve((size_t)3 * n_points));
    d_nearest = w.out_nearest.get(); d_distance = w.out_distance.get(); d_closest = closest ? w.out_closest.get() : nullptr;
  }
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kDistWords * sizeof(uint32_t), st));
  uint32_t h[kDistWords];

  // ---- mark
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const TgMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  const dim3 b(kDistBlock);
  SMX_CALL(tg_enqueue_mark(w.grid, TgBoxes::kExact, map, din, n_in, p->cell_size, kDistMargin * p->max_distance, cnt, st));
  SMX_CALL(w.stamps.mark(st));
  uint32_t E = 0, Wd = 0;
  if (const int rc = tg_read_counts(cnt, h, kDistWords, n, st, &E, &Wd)) return finish(rc);

  // ---- index (every allocation of the call lies before the first write to an output; the sort's buffers hold the points' keys too)
  uint32_t mask = 0;
  SMX_CALL(tg_enqueue_index(w.grid, TgBoxes::kExact, map, din, n_in, E, Wd, n_points, cnt, w.recs, w.wide_recs, w.table, &mask, nullptr, st));
  const TgCell* table = reinterpret_cast<const TgCell*>(w.table.get());
  const TgRec* recs = reinterpret_cast<const TgRec*>(w.recs.get());
  const TgRec* wide_recs = reinterpret_cast<const TgRec*>(w.wide_recs.get());
  SMX_CALL(w.stamps.mark(st));

  // ---- query
  if (n_points > 0) {
    const dim3 g_pts(blocks_for(n_points));
    hipLaunchKernelGGL(k_dist_point_keys, g_pts, b, 0, st, dpts, n_points, cnt, w.grid.keys[0].get(), w.grid.vals[0].get());
    SMX_LAUNCH_CHECK();
    const int cur = radix_sort(w.grid.keys, w.grid.vals, n_points, 63, w.grid.hist.get(), st);
    hipLaunchKernelGGL(k_dist_query, g_pts, b, 0, st, map, din, dpts, n_points, w.grid.keys[cur].get(), w.grid.vals[cur].get(), table, mask, recs, wide_recs, Wd, cnt,
                       p->max_distance * p->max_distance, (int)p->signed_distance, d_nearest, d_distance, d_closest, w.best.get());
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- stats
  if (n_points > 0) {
    hipLaunchKernelGGL(k_dist_stats, dim3(blocks_for(n_points)), b, 0, st, dpts, n_points, w.best.get(), p->max_distance, cnt);
    SMX_LAUNCH_CHECK();
    if (!dev) {
      SMX_HIP(hipMemcpyAsync(nearest, d_nearest, (size_t)n_points * 4, hipMemcpyDeviceToHost, st));
      SMX_HIP(hipMemcpyAsync(distance, d_distance, (size_t)n_points * 4, hipMemcpyDeviceToHost, st));
      if (closest) SMX_HIP(hipMemcpyAsync(closest, d_closest, (size_t)n_points * 12, hipMemcpyDeviceToHost, st));
    }
  }
  SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (stats) {
    stats->n_not_live = h[kTgNotLive]; stats->n_repeated = h[kTgRepeated]; stats->n_out_of_range = h[kTgRange];
    stats->n_bad_points = h[kDistBadPoints]; stats->n_matched = h[kDistMatched]; stats->max_dist2_bits = h[kDistMaxBits];
    for (uint32_t k = 0; k < kDistBins; ++k) stats->histogram[k] = h[kDistHist + k];
    stats->n_wide = Wd; stats->n_entries = E; stats->n_cells = h[kTgCells];
    memcpy(&stats->cell_size_used, &h[kTgCellBits], sizeof(float));
  }
  SMX_CALL(w.stamps.mark(st));
  return finish(SMX_OK);
}

int smx_recon_debug_distance_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_DIST_PHASES);
  SMX_ON_DEVICE(r->device);
  return r->distance.stamps.elapsed_ms(out_ms, SMX_DIST_PHASES);
}

}  // extern "C"
