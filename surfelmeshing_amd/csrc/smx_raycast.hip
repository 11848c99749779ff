// smx_raycast.hip -- the kernels of smx_recon_raycast_mesh (gfx950): for each of many rays the first triangle of a triangle
// array over the surfel map it hits, exactly the minimum over all triangles (the contract is in include/smx.h,
// its arithmetic and the traversal in smx_raycast.hpp, the classes, the cell table and the records in smx_trigrid.hpp).
//
//   mark:   tg_enqueue_mark of smx_trigrid.hip with the boxes inflated by SLACK, the occupied cell box folded and c >= 2^-9 m
//           
//   index:  tg_enqueue_index of smx_trigrid.hip
//   cast:   k_ray_cast (a wavefront per ray: the wide list dealt to the lanes; then the layers of the dominant axis 64 at a
//           time, a lane per layer: its t interval, its cell rectangle and its look-ups; a ballot names the layers with
//           records; these in order: rectangle broadcast, look-ups a lane per cell, every run dealt to the 64 lanes by stride,
//           the 64-bit keys folded by a wave minimum, the exit test)
//   stats:  k_ray_stats (counts, the maximum and the work counters: integer atomics, one per wavefront and word)
//
// Why the result does not depend on the schedule: every output of a ray is a function of the minimum of a set of 64-bit keys,
// and that minimum is the minimum over the candidates of ALL of R whatever c is; the counters are integer sums
// and one integer maximum.
//
// smx_recon_raycast_mesh itself is at the end of the file: it owns the order of the phases, the workspace (RaycastWork,
// smx_raycast.hpp) and the second read of the counters (the first is tg_read_counts).  smx_recon_build_rayscene
// (smx_rayscene.hip) builds with the same workspace, into a scene's records and table.
#include <cmath>

#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

constexpr int kRBlock = kRayBlock;

// A wavefront per ray.  Everything that steers a loop (the ray, its axes, the layer count, the ballots, the broadcast
// rectangles and runs, the folded minimum) is uniform over the wavefront; a lane's own state is its layer's rectangle, one
// 64-bit key and three counts.  No LDS, no barrier.
__global__ void __launch_bounds__(kRBlock)
k_ray_cast(TgMap map, const uint32_t* __restrict__ tri, const float* __restrict__ rays, uint32_t n_rays, const TgCell* __restrict__ table,
           uint32_t mask, const TgRec* __restrict__ recs, const TgRec* __restrict__ wide_recs, uint32_t n_wide, uint32_t n_entries,
           const uint32_t* __restrict__ cnt, float t_min, float t_max, int cull, uint32_t* __restrict__ hit, float* __restrict__ t_out,
           float* __restrict__ uv, unsigned long long* __restrict__ best_out, uint4* __restrict__ work_out) {
  const uint32_t lane = threadIdx.x & 63, p = blockIdx.x * kRayWaves + (threadIdx.x >> 6);
  if (p >= n_rays) return;                                   // (the whole wavefront)
  TgVec O, D;
  ray_load(rays, p, &O, &D);
  const bool bad = ray_bad(O, D);
  unsigned long long best = kTgNone;
  uint32_t layers = 0, lookups = 0, tests = 0;
  if (!bad) {
    best = wave_min(ray_walk(TgDeviceRecs{wide_recs}, lane, n_wide, 64, O, D, t_min, t_max, cull, best, &tests));
    if (n_entries != 0) {
      const float cell = tg_cell_of(cnt);
      const int32_t* occ = reinterpret_cast<const int32_t*>(cnt);
      const RayAxes r = ray_axes(O, D, occ[kTgOccLo], occ[kTgOccLo + 1], occ[kTgOccLo + 2], occ[kTgOccHi], occ[kTgOccHi + 1],
                                 occ[kTgOccHi + 2], cell, t_min, t_max);
      const TgDeviceTable tab{const_cast<TgCell*>(table)};
      const TgDeviceRecs cell_recs{recs};
      bool stop = false;
      for (uint32_t base = 0; base < r.n_layers && !stop; base += 64) {
        if (ray_done(r, cell, best, base)) break;
        // a lane per layer: is there a record in any cell of its rectangle?
        const uint32_t m = base + lane;
        RayRect q{0, -1, 0, -1};
        uint32_t cells = 0;
        bool any = false;
        if (m < r.n_layers) {
          q = ray_layer_rect(r, cell, t_min, t_max, m);
          cells = ray_rect_cells(q);
          ++layers;
          for (uint32_t j = 0; j < cells && !any; ++j) {
            uint32_t first, end;
            ++lookups;
            any = tg_table_find(tab, mask, ray_rect_key(r, q, m, j), &first, &end);
          }
        }
        unsigned long long todo = __ballot(any);
        while (todo != 0) {
          const int k = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const RayRect qk{__shfl(q.b0, k), __shfl(q.b1, k), __shfl(q.c0, k), __shfl(q.c1, k)};
          const uint32_t nk = (uint32_t)__shfl((int)cells, k), mk = base + (uint32_t)k;
          for (uint32_t jb = 0; jb < nk; jb += 64) {         // a lane per cell of the rectangle
            uint32_t first = 0, end = 0;
            bool found = false;
            if (jb + lane < nk) {
              ++lookups;
              found = tg_table_find(tab, mask, ray_rect_key(r, qk, mk, jb + lane), &first, &end);
            }
            unsigned long long runs = __ballot(found);
            while (runs != 0) {
              const int s = __ffsll((long long)runs) - 1;
              runs &= runs - 1;
              const uint32_t f = (uint32_t)__shfl((int)first, s), e = (uint32_t)__shfl((int)end, s);
              best = ray_walk(cell_recs, f + lane, e, 64, O, D, t_min, t_max, cull, best, &tests);
            }
          }
          best = wave_min(best);
          if (ray_done(r, cell, best, mk + 1)) { stop = true; break; }
        }
      }
    }
  }
  const unsigned long long n_layers = wave_sum((unsigned long long)layers), n_lookups = wave_sum((unsigned long long)lookups),
                           n_tests = wave_sum((unsigned long long)tests);
  if (lane != 0) return;
  uint32_t i = kInvalid, flags = bad ? kRayFlagBad : 0u;
  float t = __builtin_inff(), u = __builtin_nanf(""), v = __builtin_nanf("");
  if (best != kTgNone) {
    i = (uint32_t)best;
    const TgVec A = tg_pos(map, tri[3 * (size_t)i]), B = tg_pos(map, tri[3 * (size_t)i + 1]), C = tg_pos(map, tri[3 * (size_t)i + 2]);
    RayHit h{0.0f, 0.0f, 0.0f, 0.0f};
    (void)ray_key(O, D, A, B, C, i, t_min, t_max, cull, &h);           // (the same expressions: the same key)
    t = tg_key_float(best); u = h.u; v = h.v;
    flags |= kRayFlagHit | (h.det > 0.0f ? kRayFlagFront : 0u);
  }
  best_out[p] = best;
  work_out[p] = make_uint4((uint32_t)n_layers, (uint32_t)n_lookups, (uint32_t)n_tests, flags);
  hit[p] = i;
  t_out[p] = t;
  if (uv) { uv[2 * (size_t)p] = u; uv[2 * (size_t)p + 1] = v; }
}

__global__ void __launch_bounds__(kRBlock)
k_ray_stats(uint32_t n_rays, const unsigned long long* __restrict__ best, const uint4* __restrict__ work, uint32_t* __restrict__ cnt) {
  const uint32_t p = blockIdx.x * kRBlock + threadIdx.x;
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  uint32_t bits = 0;
  if (p < n_rays) {
    w = work[p];
    if (w.w & kRayFlagHit) bits = (uint32_t)(best[p] >> 32);
  }
  wave_count(&cnt[kRayBadRays], (w.w & kRayFlagBad) != 0);
  wave_count(&cnt[kRayHits], (w.w & kRayFlagHit) != 0);
  wave_count(&cnt[kRayFrontHits], (w.w & kRayFlagFront) != 0);
  const unsigned long long layers = wave_sum((unsigned long long)w.x), lookups = wave_sum((unsigned long long)w.y),
                           tests = wave_sum((unsigned long long)w.z);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)bits, off); bits = o > bits ? o : bits; }
  if ((threadIdx.x & 63) != 0) return;
  if (layers) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayLayersLo), layers);
  if (lookups) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayLookupsLo), lookups);
  if (tests) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayTestsLo), tests);
  if (bits) atomicMax(&cnt[kRayMaxBits], bits);              // (bits of non-negative floats order as the floats do)
}

}  // namespace

}  // namespace smx

using namespace smx;

extern "C" {

int smx_raycast_params_default(smx_raycast_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->t_min = 0.0f; out->t_max = SMX_RAY_MAX_T; out->cell_size = 0.0f; out->cull = 0;
  return SMX_OK;
}

int smx_recon_raycast_mesh(smx_recon r, smx_stream s, const smx_raycast_params* p, const uint32_t* triangles, uint32_t n_in,
                           const float* rays, uint32_t n_rays, uint32_t* hit, float* t, float* uv, int32_t on_device,
                           smx_raycast_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && p != nullptr);
  SMX_CHECK_ARG(finite_f(p->t_min) && finite_f(p->t_max) && p->t_min >= 0.0f && p->t_min <= p->t_max && p->t_max <= SMX_RAY_MAX_T);
  SMX_CHECK_ARG(finite_f(p->cell_size) && p->cell_size >= 0.0f);
  SMX_CHECK_ARG(p->cull == 0 || p->cull == 1 || p->cull == 2);
  SMX_CHECK_ARG(n_in <= (1u << 28) && n_rays <= (1u << 28));
  SMX_CHECK_ARG(triangles != nullptr || n_in == 0);
  SMX_CHECK_ARG((rays != nullptr && hit != nullptr && t != nullptr) || n_rays == 0);
  {
    const void* ins[2] = {triangles, rays};
    const size_t in_bytes[2] = {(size_t)n_in * 12, (size_t)n_rays * 24};
    const void* outs[3] = {hit, t, uv};
    const size_t out_bytes[3] = {(size_t)n_rays * 4, (size_t)n_rays * 4, (size_t)n_rays * 8};
    for (int i = 0; i < 2; ++i)
      for (int o = 0; o < 3; ++o)
        if (ranges_overlap(ins[i], in_bytes[i], outs[o], out_bytes[o])) {
          set_error("an output of smx_recon_raycast_mesh overlaps %s", i == 0 ? "triangles" : "rays");
          return SMX_ERR_INVALID_ARGUMENT;
        }
  }
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; stats->n_rays = n_rays; }
  RaycastWork& w = r->raycast;
  SMX_CALL(w.stamps.begin(st));
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    w.stamps.publish();
    return rc;
  };

  // ---- workspace of the first phase; the inputs on the device; the outputs' staging
  const bool dev = on_device != 0;
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kRayWords, false));
  SMX_CALL(w.grid.reserve_mark(n_in));
  SMX_CALL(w.best.reserve(n_rays));
  SMX_CALL(w.work.reserve((size_t)4 * n_rays));
  const uint32_t* din = nullptr;
  const float* drays = nullptr;
  SMX_CALL(stage_in(w.in, triangles, (size_t)3 * n_in, dev, st, &din));
  SMX_CALL(stage_in(w.rays, rays, (size_t)6 * n_rays, dev, st, &drays));
  uint32_t* d_hit = hit;
  float* d_t = t;
  float* d_uv = uv;
  if (!dev && n_rays > 0) {
    SMX_CALL(w.out_hit.reserve(n_rays));
    SMX_CALL(w.out_t.reserve(n_rays));
    if (uv) SMX_CALL(w.out_uv.reserve((size_t)2 * n_rays));
    d_hit = w.out_hit.get(); d_t = w.out_t.get(); d_uv = uv ? w.out_uv.get() : nullptr;
  }
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kRayWords * sizeof(uint32_t), st));
  uint32_t h[kRayWords];

  // ---- mark
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const TgMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  const dim3 b(kRayBlock);
  SMX_CALL(tg_enqueue_mark(w.grid, TgBoxes::kForRays, map, din, n_in, p->cell_size, kRayMinCell, cnt, st));
  SMX_CALL(w.stamps.mark(st));
  uint32_t E = 0, Wd = 0;
  if (const int rc = tg_read_counts(cnt, h, kRayWords, n, st, &E, &Wd)) return finish(rc);

  // ---- index (every allocation of the call lies before the first write to an output)
  uint32_t mask = 0;
  SMX_CALL(tg_enqueue_index(w.grid, TgBoxes::kForRays, map, din, n_in, E, Wd, 0, cnt, w.recs, w.wide_recs, w.table, &mask, nullptr, st));
  const TgCell* table = reinterpret_cast<const TgCell*>(w.table.get());
  const TgRec* recs = reinterpret_cast<const TgRec*>(w.recs.get());
  const TgRec* wide_recs = reinterpret_cast<const TgRec*>(w.wide_recs.get());
  SMX_CALL(w.stamps.mark(st));

  // ---- cast
  uint4* work = reinterpret_cast<uint4*>(w.work.get());
  if (n_rays > 0) {
    hipLaunchKernelGGL(k_ray_cast, dim3((unsigned)div_up(n_rays, kRayWaves)), b, 0, st, map, din, drays, n_rays, table, mask, recs, wide_recs, Wd, E, cnt,
                       p->t_min, p->t_max, (int)p->cull, d_hit, d_t, d_uv, w.best.get(), work);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- stats
  if (n_rays > 0) {
    hipLaunchKernelGGL(k_ray_stats, dim3(blocks_for(n_rays)), b, 0, st, n_rays, w.best.get(), work, cnt);
    SMX_LAUNCH_CHECK();
    if (!dev) {
      SMX_HIP(hipMemcpyAsync(hit, d_hit, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      SMX_HIP(hipMemcpyAsync(t, d_t, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      if (uv) SMX_HIP(hipMemcpyAsync(uv, d_uv, (size_t)n_rays * 8, hipMemcpyDeviceToHost, st));
    }
  }
  SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (stats) {
    stats->n_not_live = h[kTgNotLive]; stats->n_repeated = h[kTgRepeated]; stats->n_out_of_range = h[kTgRange];
    stats->n_bad_rays = h[kRayBadRays]; stats->n_hit = h[kRayHits]; stats->n_front_hits = h[kRayFrontHits]; stats->max_t_bits = h[kRayMaxBits];
    stats->n_wide = Wd; stats->n_entries = E; stats->n_cells = h[kTgCells];
    memcpy(&stats->cell_size_used, &h[kTgCellBits], sizeof(float));
    stats->n_layers = word64(h, kRayLayersLo); stats->n_lookups = word64(h, kRayLookupsLo); stats->n_pair_tests = word64(h, kRayTestsLo);
  }
  SMX_CALL(w.stamps.mark(st));
  return finish(SMX_OK);
}

int smx_recon_debug_raycast_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_RAY_PHASES);
  SMX_ON_DEVICE(r->device);
  return r->raycast.stamps.elapsed_ms(out_ms, SMX_RAY_PHASES);
}

}  // extern "C"
