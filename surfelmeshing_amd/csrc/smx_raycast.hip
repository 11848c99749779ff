// smx_raycast.hip -- the ray cast (gfx950): for each of many rays the first triangle of a triangle array over the surfel map it
// hits, exactly the minimum over all triangles.  One traversal serves smx_recon_raycast_mesh, which builds its
// index, casts once and forgets it, and smx_rayscene_cast (smx_rayscene.hip), which casts an index it kept.  The
// contract is in include/smx.h, its arithmetic and the traversal in smx_raycast.hpp, the classes, the cell table and the records
// in smx_trigrid.hpp.
//
//   mark:   tg_enqueue_mark of smx_trigrid.hip with the boxes inflated by SLACK, the occupied cell box folded and c >= 2^-9 m
//           
//   index:  tg_enqueue_index of smx_trigrid.hip
//   cast:   k_ray_cast for a kept index, k_ray_cast_built for the call's, both thin over ray_cast_wave (a wavefront per ray:
//           the wide list dealt to the lanes; then the layers of the dominant axis 64 at a time, a lane per layer: its t interval, its cell rectangle and its look-ups, behind the bit grid where the index
//           has one; a ballot names the layers with records; these in order: rectangle broadcast, look-ups a lane per cell,
//           every run dealt to the 64 lanes by stride, the 64-bit keys folded by a wave minimum, the exit test; no read of the
//           map: the lane that holds the winning key hands its (u, v, det) to lane 0)
//   stats:  k_ray_stats (counts, the maximum and the work counters: at most 256 workgroups, integer atomics, one per wavefront
//           and word)
//
// Why the result does not depend on the schedule: every output of a ray is a function of the minimum of a set of 64-bit keys,
// and that minimum is the minimum over the candidates of ALL of R whatever c is and whatever the grid; the
// counters are integer sums and one integer maximum.
//
// The host side of a cast (ray_cast_overlap, ray_cast_stage, ray_cast_launch, ray_cast_finish) follows the kernels;
// smx_recon_raycast_mesh itself is at the end of the file: it owns the order of its phases and the workspace (RaycastWork,
// smx_raycast.hpp).  smx_recon_build_rayscene (smx_rayscene.hip) builds with the same workspace, into a scene's records and table.
#include <algorithm>
#include <cmath>

#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

// A wavefront per ray.  Everything that steers a loop (the ray, its axes, the layer count, the ballots, the broadcast
// rectangles and runs, the folded minimum, whether there is a grid) is uniform over the wavefront; a lane's own state is its
// layer's rectangle, one 64-bit key with what it came with, and five counts.  No LDS, no barrier, no read of the map.
__device__ __forceinline__ void
ray_cast_wave(const float* __restrict__ rays, uint32_t n_rays, const TgCell* __restrict__ table, uint32_t mask, const TgRec* __restrict__ recs,
              const TgRec* __restrict__ wide_recs, uint32_t n_wide, uint32_t n_entries, const RayGrid& grid, const uint32_t* __restrict__ bit_words,
              float cell, const RayBox& occ, float t_min, float t_max, int cull, uint32_t* __restrict__ hit, float* __restrict__ t_out,
              float* __restrict__ uv, unsigned long long* __restrict__ best_out, uint4* __restrict__ work_out) {
  const uint32_t lane = threadIdx.x & 63, p = blockIdx.x * kRayWaves + (threadIdx.x >> 6);
  if (p >= n_rays) return;                                   // (the whole wavefront)
  TgVec O, D;
  ray_load(rays, p, &O, &D);
  const bool bad = ray_bad(O, D);
  unsigned long long best = kTgNone;
  RayKeep keep{kTgNone, 0.0f, 0.0f, 0.0f};
  RayWork work{0, 0, 0, 0, 0};
  if (!bad) {
    best = wave_min(ray_walk(TgDeviceRecs{wide_recs}, lane, n_wide, 64, O, D, t_min, t_max, cull, best, &keep, &work.tests));
    if (n_entries != 0) {
      const RayAxes r = ray_axes(O, D, occ.lo[0], occ.lo[1], occ.lo[2], occ.hi[0], occ.hi[1], occ.hi[2], cell, t_min, t_max);
      const TgDeviceTable tab{const_cast<TgCell*>(table)};
      const TgDeviceRecs cell_recs{recs};
      const RayBits bits{bit_words};
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
          ++work.layers;
          for (uint32_t j = 0; j < cells && !any; ++j) {
            int32_t x, y, z;
            uint32_t first, end;
            ray_rect_cell(r, q, m, j, &x, &y, &z);
            any = ray_find(grid, bits, tab, mask, x, y, z, &first, &end, &work);
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
              int32_t x, y, z;
              ray_rect_cell(r, qk, mk, jb + lane, &x, &y, &z);
              found = ray_find(grid, bits, tab, mask, x, y, z, &first, &end, &work);
            }
            unsigned long long runs = __ballot(found);
            while (runs != 0) {
              const int s = __ffsll((long long)runs) - 1;
              runs &= runs - 1;
              const uint32_t f = (uint32_t)__shfl((int)first, s), e = (uint32_t)__shfl((int)end, s);
              best = ray_walk(cell_recs, f + lane, e, 64, O, D, t_min, t_max, cull, best, &keep, &work.tests);
            }
          }
          best = wave_min(best);
          if (ray_done(r, cell, best, mk + 1)) { stop = true; break; }
        }
      }
    }
  }
  const uint32_t n_layers = wave_sum(work.layers), n_bits = wave_sum(work.bit_tests), n_lookups = wave_sum(work.lookups),
                 n_misses = wave_sum(work.misses), n_tests = wave_sum(work.tests);
  // the winner's (u, v, det): from the first lane whose own key is the minimum (it was strictly below that lane's best when it
  // was computed, so the lane kept it, and no smaller key came after)
  const unsigned long long holders = __ballot(best != kTgNone && keep.own == best);
  const int src = holders != 0 ? __ffsll((long long)holders) - 1 : 0;
  const float wu = __shfl(keep.u, src), wv = __shfl(keep.v, src), wdet = __shfl(keep.det, src);
  if (lane != 0) return;
  uint32_t i = kInvalid, flags = bad ? kRayFlagBad : 0u;
  float t = __builtin_inff(), u = __builtin_nanf(""), v = __builtin_nanf("");
  if (best != kTgNone) {
    i = (uint32_t)best;
    t = tg_key_float(best); u = wu; v = wv;
    flags |= kRayFlagHit | (wdet > 0.0f ? kRayFlagFront : 0u);
  }
  best_out[p] = best;
  work_out[2 * (size_t)p] = make_uint4(n_layers, n_bits, n_lookups, n_misses);
  work_out[2 * (size_t)p + 1] = make_uint4(n_tests, flags, 0u, 0u);
  hit[p] = i;
  t_out[p] = t;
  if (uv) { uv[2 * (size_t)p] = u; uv[2 * (size_t)p + 1] = v; }
}

// The two kernels over it.  A kept index hands its grid, c and the occupied box by value.
__global__ void __launch_bounds__(kRayBlock)
k_ray_cast(const float* __restrict__ rays, uint32_t n_rays, const TgCell* __restrict__ table, uint32_t mask, const TgRec* __restrict__ recs,
           const TgRec* __restrict__ wide_recs, uint32_t n_wide, uint32_t n_entries, RayGrid grid, const uint32_t* __restrict__ bit_words,
           float cell, RayBox occ, float t_min, float t_max, int cull, uint32_t* __restrict__ hit, float* __restrict__ t_out,
           float* __restrict__ uv, unsigned long long* __restrict__ best_out, uint4* __restrict__ work_out) {
  ray_cast_wave(rays, n_rays, table, mask, recs, wide_recs, n_wide, n_entries, grid, bit_words, cell, occ, t_min, t_max, cull, hit, t_out, uv, best_out,
                work_out);
}
// The index the call has just built: never a grid, and c and the occupied box where the build left them, in its counter words.
__global__ void __launch_bounds__(kRayBlock)
k_ray_cast_built(const float* __restrict__ rays, uint32_t n_rays, const TgCell* __restrict__ table, uint32_t mask, const TgRec* __restrict__ recs,
                 const TgRec* __restrict__ wide_recs, uint32_t n_wide, uint32_t n_entries, const uint32_t* __restrict__ cnt, float t_min, float t_max,
                 int cull, uint32_t* __restrict__ hit, float* __restrict__ t_out, float* __restrict__ uv, unsigned long long* __restrict__ best_out,
                 uint4* __restrict__ work_out) {
  const int32_t* c = reinterpret_cast<const int32_t*>(cnt);
  const RayBox occ{{c[kTgOccLo], c[kTgOccLo + 1], c[kTgOccLo + 2]}, {c[kTgOccHi], c[kTgOccHi + 1], c[kTgOccHi + 2]}};
  ray_cast_wave(rays, n_rays, table, mask, recs, wide_recs, n_wide, n_entries, RayGrid{{0, 0, 0}, {0, 0, 0}, -1}, nullptr, tg_cell_of(cnt), occ, t_min,
                t_max, cull, hit, t_out, uv, best_out, work_out);
}

// A lane sums several rays before the wavefront folds: at most kRayStatsBlocks workgroups, so the atomics on the few counter
// words stay few however many rays there are (a wavefront per 64 rays took 0.27 ms for 307 200 rays, this takes 0.11 ms).
constexpr unsigned kRayStatsBlocks = 256;
__global__ void __launch_bounds__(kRayBlock)
k_ray_stats(uint32_t n_rays, const unsigned long long* __restrict__ best, const uint4* __restrict__ work, uint32_t* __restrict__ cnt) {
  unsigned long long layers = 0, bit_tests = 0, lookups = 0, misses = 0, tests = 0;
  uint32_t bits = 0, n_bad = 0, n_hit = 0, n_front = 0;
  for (uint32_t p = blockIdx.x * kRayBlock + threadIdx.x; p < n_rays; p += gridDim.x * kRayBlock) {
    const uint4 a = work[2 * (size_t)p], b = work[2 * (size_t)p + 1];
    layers += a.x; bit_tests += a.y; lookups += a.z; misses += a.w; tests += b.x;
    n_bad += (b.y & kRayFlagBad) != 0; n_hit += (b.y & kRayFlagHit) != 0; n_front += (b.y & kRayFlagFront) != 0;
    if (b.y & kRayFlagHit) { const uint32_t t_bits = (uint32_t)(best[p] >> 32); bits = t_bits > bits ? t_bits : bits; }
  }
  layers = wave_sum(layers); bit_tests = wave_sum(bit_tests); lookups = wave_sum(lookups); misses = wave_sum(misses);
  tests = wave_sum(tests);
  n_bad = wave_sum(n_bad); n_hit = wave_sum(n_hit); n_front = wave_sum(n_front);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)bits, off); bits = o > bits ? o : bits; }
  if ((threadIdx.x & 63) != 0) return;
  if (n_bad) atomicAdd(&cnt[kRayBadRays], n_bad);
  if (n_hit) atomicAdd(&cnt[kRayHits], n_hit);
  if (n_front) atomicAdd(&cnt[kRayFrontHits], n_front);
  if (layers) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayLayersLo), layers);
  if (bit_tests) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayBitTestsLo), bit_tests);
  if (lookups) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayLookupsLo), lookups);
  if (misses) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayMissesLo), misses);
  if (tests) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayTestsLo), tests);
  if (bits) atomicMax(&cnt[kRayMaxBits], bits);           // (bits of non-negative floats order as the floats do)
}

}  // namespace

unsigned long long RayCastWork::bytes() const {
  auto of = [](const auto& b) { return (unsigned long long)b.capacity() * sizeof(*b.get()); };
  return of(best) + of(work) + of(rays) + of(out_t) + of(out_uv) + of(out_hit) + of(counters);
}

int ray_cast_overlap(const char* fn, const char* what, const void* in, size_t in_bytes, uint32_t n_rays, const uint32_t* hit, const float* t,
                     const float* uv) {
  const void* outs[3] = {hit, t, uv};
  const size_t out_bytes[3] = {(size_t)n_rays * 4, (size_t)n_rays * 4, (size_t)n_rays * 8};
  for (int o = 0; o < 3; ++o)
    if (ranges_overlap(in, in_bytes, outs[o], out_bytes[o])) {
      set_error("an output of %s overlaps %s", fn, what);
      return SMX_ERR_INVALID_ARGUMENT;
    }
  return SMX_OK;
}

int ray_cast_stage(RayCastWork& w, const float* rays, uint32_t n_rays, uint32_t* hit, float* t, float* uv, bool on_device, hipStream_t st,
                   RayCastArrays* d) {
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kRayWords, false));
  SMX_CALL(w.best.reserve(n_rays));
  SMX_CALL(w.work.reserve((size_t)kRayWorkWords * n_rays));
  SMX_CALL(stage_in(w.rays, rays, (size_t)6 * n_rays, on_device, st, &d->rays));
  d->hit = hit; d->t = t; d->uv = uv;
  if (!on_device && n_rays > 0) {
    SMX_CALL(w.out_hit.reserve(n_rays));
    SMX_CALL(w.out_t.reserve(n_rays));
    if (uv) SMX_CALL(w.out_uv.reserve((size_t)2 * n_rays));
    d->hit = w.out_hit.get(); d->t = w.out_t.get(); d->uv = uv ? w.out_uv.get() : nullptr;
  }
  SMX_HIP(hipMemsetAsync(w.counters.get(), 0, kRayWords * sizeof(uint32_t), st));
  return SMX_OK;
}

int ray_cast_launch(RayCastWork& w, const RayIndex& ix, const smx_raycast_params* p, const RayCastArrays& d, uint32_t n_rays, hipStream_t st) {
  if (n_rays > 0) {
    const dim3 g((unsigned)div_up(n_rays, kRayWaves)), b(kRayBlock);
    uint4* work = reinterpret_cast<uint4*>(w.work.get());
    if (ix.built)
      hipLaunchKernelGGL(k_ray_cast_built, g, b, 0, st, d.rays, n_rays, ix.table, ix.mask, ix.recs, ix.wide_recs, ix.n_wide, ix.n_entries, ix.built,
                         p->t_min, p->t_max, (int)p->cull, d.hit, d.t, d.uv, w.best.get(), work);
    else
      hipLaunchKernelGGL(k_ray_cast, g, b, 0, st, d.rays, n_rays, ix.table, ix.mask, ix.recs, ix.wide_recs, ix.n_wide, ix.n_entries, ix.grid, ix.bits,
                         ix.cell, ix.occ, p->t_min, p->t_max, (int)p->cull, d.hit, d.t, d.uv, w.best.get(), work);
    SMX_LAUNCH_CHECK();
  }
  return SMX_OK;
}

int ray_cast_finish(RayCastWork& w, const RayIndex& ix, const RayCastArrays& d, uint32_t n_rays, uint32_t* hit, float* t, float* uv, bool on_device,
                    hipStream_t st, smx_rayscene_cast_stats* out, uint32_t* built_cells) {
  uint32_t* cnt = w.counters.get();
  if (n_rays > 0) {
    hipLaunchKernelGGL(k_ray_stats, dim3(std::min(blocks_for(n_rays), kRayStatsBlocks)), dim3(kRayBlock), 0, st, n_rays, w.best.get(),
                       reinterpret_cast<const uint4*>(w.work.get()), cnt);
    SMX_LAUNCH_CHECK();
    if (!on_device) {
      SMX_HIP(hipMemcpyAsync(hit, d.hit, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      SMX_HIP(hipMemcpyAsync(t, d.t, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      if (uv) SMX_HIP(hipMemcpyAsync(uv, d.uv, (size_t)n_rays * 8, hipMemcpyDeviceToHost, st));
    }
  }
  uint32_t h[kRayWords];
  SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  if (built_cells) SMX_HIP(hipMemcpyAsync(built_cells, ix.built + kTgCells, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  memset(out, 0, sizeof(*out));
  out->n_rays = n_rays; out->n_bad_rays = h[kRayBadRays]; out->n_hit = h[kRayHits]; out->n_front_hits = h[kRayFrontHits];
  out->max_t_bits = h[kRayMaxBits];
  out->n_layers = word64(h, kRayLayersLo); out->n_bit_tests = word64(h, kRayBitTestsLo);
  out->n_lookups = word64(h, kRayLookupsLo); out->n_lookup_misses = word64(h, kRayMissesLo);
  out->n_pair_tests = word64(h, kRayTestsLo);
  return SMX_OK;
}

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
  SMX_CALL(ray_cast_overlap("smx_recon_raycast_mesh", "triangles", triangles, (size_t)n_in * 12, n_rays, hit, t, uv));
  SMX_CALL(ray_cast_overlap("smx_recon_raycast_mesh", "rays", rays, (size_t)n_rays * 24, n_rays, hit, t, uv));
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
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kTgWords, false));
  SMX_CALL(w.grid.reserve_mark(n_in));
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(w.in, triangles, (size_t)3 * n_in, dev, st, &din));
  RayCastArrays d;
  SMX_CALL(ray_cast_stage(w.cast, rays, n_rays, hit, t, uv, dev, st, &d));
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kTgWords * sizeof(uint32_t), st));
  uint32_t h[kTgWords];

  // ---- mark
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const TgMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  SMX_CALL(tg_enqueue_mark(w.grid, TgBoxes::kForRays, map, din, n_in, p->cell_size, kRayMinCell, cnt, st));
  SMX_CALL(w.stamps.mark(st));
  uint32_t E = 0, Wd = 0;
  if (const int rc = tg_read_counts(cnt, h, kTgWords, n, st, &E, &Wd)) return finish(rc);

  // ---- index (every allocation of the call lies before the first write to an output)
  RayIndex ix{};
  SMX_CALL(tg_enqueue_index(w.grid, TgBoxes::kForRays, map, din, n_in, E, Wd, 0, cnt, w.recs, w.wide_recs, w.table, &ix.mask, nullptr, st));
  ix.table = reinterpret_cast<const TgCell*>(w.table.get());
  ix.recs = reinterpret_cast<const TgRec*>(w.recs.get());
  ix.wide_recs = reinterpret_cast<const TgRec*>(w.wide_recs.get());
  ix.n_entries = E; ix.n_wide = Wd;
  ray_index_read(&ix, h);
  ix.grid = RayGrid{{0, 0, 0}, {0, 0, 0}, -1};           // no grid: every cell goes to the table
  ix.built = cnt;
  SMX_CALL(w.stamps.mark(st));

  // ---- cast, stats
  smx_rayscene_cast_stats cs;
  uint32_t n_cells = 0;                  // (the index phase counted them after the first read of the counters)
  SMX_CALL(ray_cast_launch(w.cast, ix, p, d, n_rays, st));
  SMX_CALL(w.stamps.mark(st));
  SMX_CALL(ray_cast_finish(w.cast, ix, d, n_rays, hit, t, uv, dev, st, &cs, &n_cells));
  if (stats) {
    stats->n_not_live = h[kTgNotLive]; stats->n_repeated = h[kTgRepeated]; stats->n_out_of_range = h[kTgRange];
    stats->n_bad_rays = cs.n_bad_rays; stats->n_hit = cs.n_hit; stats->n_front_hits = cs.n_front_hits; stats->max_t_bits = cs.max_t_bits;
    stats->n_wide = Wd; stats->n_entries = E; stats->n_cells = n_cells;
    memcpy(&stats->cell_size_used, &h[kTgCellBits], sizeof(float));
    stats->n_layers = cs.n_layers; stats->n_lookups = cs.n_lookups; stats->n_pair_tests = cs.n_pair_tests;
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
