// smx_rayscene.hip -- smx_rayscene (gfx950): the search structure of smx_recon_raycast_mesh built once and kept, with an
// occupancy bit grid in front of its cell table (the contract is in include/smx.h, the grid's arithmetic and the
// filtered walk in smx_rayscene.hpp).
//
//   build:  tg_enqueue_mark and tg_enqueue_index of smx_trigrid.hip as smx_recon_raycast_mesh calls them, writing
//           the records and the cell table into the scene's own buffers -> k_scene_occupancy (a lane per sorted entry; the head
//           of a run sets its block's bit, one atomic per distinct bit of the wavefront) -> k_scene_popcount (the set bits,
//           counted from the bits)
//   cast:   k_scene_cast (k_ray_cast's structure: a wavefront per ray, 64 layers per round, a ballot of the non-empty ones, the
//           runs dealt to the lanes, a wave minimum of 64-bit keys; the bit test in front of both look-up sites; no read of the
//           map: the lane that holds the winning key hands its (u, v, det) to lane 0) -> k_scene_stats
//
// A cast's outputs are a function of the minimum of a set of 64-bit keys over the records, which are copies of the corners as
// the map held them at the build: the bytes of smx_recon_raycast_mesh on that map, whatever the schedule and the grid.
#include <memory>

#include "smx_recon_state.hpp"
#include "smx_rayscene.hpp"

namespace smx {

namespace {

// occupancy 0: the smallest block that fits.  DESIGN.md 5m "Measured" holds the numbers behind this: on an MI355X the grid pays.
constexpr bool kSceneAutoGrid = true;

struct SceneBox { int32_t lo[3], hi[3]; };

// bits is all zeros before.  At k > 0 the heads of one block lie near each other in the sorted order (z runs fastest in the
// cell key), so a wavefront issues one atomic per distinct bit, and none where a plain read already sees the bit (a stale
// read costs one atomic).
__global__ void __launch_bounds__(kRayBlock)
k_scene_occupancy(const unsigned long long* __restrict__ keys, uint32_t n_entries, SceneGrid grid, uint32_t* bits) {
  const uint32_t j = blockIdx.x * kRayBlock + threadIdx.x, lane = threadIdx.x & 63;
  unsigned long long bit64 = 0;
  const bool active = j < n_entries && scene_entry_bit(grid, keys, j, &bit64);
  const uint32_t bit = (uint32_t)bit64;                      // (below 2^31)
  if (grid.k == 0) {                                         // (every head has a bit of its own)
    if (active) atomicOr(&bits[bit >> 5], 1u << (bit & 31u));
    return;
  }
  unsigned long long todo = __ballot(active);
  while (todo != 0) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t lb = (uint32_t)__shfl((int)bit, leader);
    todo &= ~__ballot(active && bit == lb);
    if (lane == (uint32_t)leader) {
      const volatile uint32_t* seen = bits;
      if (!((seen[lb >> 5] >> (lb & 31u)) & 1u)) atomicOr(&bits[lb >> 5], 1u << (lb & 31u));
    }
  }
}

__global__ void __launch_bounds__(kRayBlock)
k_scene_popcount(const uint32_t* __restrict__ bits, uint32_t n_words, uint32_t* __restrict__ cnt) {
  uint32_t sum = 0;
  for (uint32_t i = blockIdx.x * kRayBlock + threadIdx.x; i < n_words; i += gridDim.x * kRayBlock) sum += (uint32_t)__popc(bits[i]);
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(&cnt[kSceneBlocksSet], sum);
}

// A wavefront per ray, as k_ray_cast: everything that steers a loop is uniform over the wavefront; a lane's own state is its
// layer's rectangle, one 64-bit key with what it came with, and five counts.  No LDS, no barrier, no read of the map.
__global__ void __launch_bounds__(kRayBlock)
k_scene_cast(const float* __restrict__ rays, uint32_t n_rays, const TgCell* __restrict__ table, uint32_t mask, const TgRec* __restrict__ recs,
             const TgRec* __restrict__ wide_recs, uint32_t n_wide, uint32_t n_entries, SceneGrid grid, const uint32_t* __restrict__ bit_words,
             float cell, SceneBox occ, float t_min, float t_max, int cull, uint32_t* __restrict__ hit, float* __restrict__ t_out,
             float* __restrict__ uv, unsigned long long* __restrict__ best_out, uint4* __restrict__ work_out) {
  const uint32_t lane = threadIdx.x & 63, p = blockIdx.x * kRayWaves + (threadIdx.x >> 6);
  if (p >= n_rays) return;                                   // (the whole wavefront)
  TgVec O, D;
  ray_load(rays, p, &O, &D);
  const bool bad = ray_bad(O, D);
  unsigned long long best = kTgNone;
  SceneKeep keep{kTgNone, 0.0f, 0.0f, 0.0f};
  SceneWork work{0, 0, 0, 0, 0};
  if (!bad) {
    best = wave_min(scene_walk(TgDeviceRecs{wide_recs}, lane, n_wide, 64, O, D, t_min, t_max, cull, best, &keep, &work.tests));
    if (n_entries != 0) {
      const RayAxes r = ray_axes(O, D, occ.lo[0], occ.lo[1], occ.lo[2], occ.hi[0], occ.hi[1], occ.hi[2], cell, t_min, t_max);
      const TgDeviceTable tab{const_cast<TgCell*>(table)};
      const TgDeviceRecs cell_recs{recs};
      const SceneBits bits{bit_words};
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
            scene_rect_cell(r, q, m, j, &x, &y, &z);
            any = scene_find(grid, bits, tab, mask, x, y, z, &first, &end, &work);
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
              scene_rect_cell(r, qk, mk, jb + lane, &x, &y, &z);
              found = scene_find(grid, bits, tab, mask, x, y, z, &first, &end, &work);
            }
            unsigned long long runs = __ballot(found);
            while (runs != 0) {
              const int s = __ffsll((long long)runs) - 1;
              runs &= runs - 1;
              const uint32_t f = (uint32_t)__shfl((int)first, s), e = (uint32_t)__shfl((int)end, s);
              best = scene_walk(cell_recs, f + lane, e, 64, O, D, t_min, t_max, cull, best, &keep, &work.tests);
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

// A lane sums several rays before the wavefront folds: at most kSceneStatsBlocks workgroups, so the atomics on the few counter
// words stay few however many rays there are (one per ray's wavefront made this phase slower than the cast's gain allowed).
constexpr unsigned kSceneStatsBlocks = 256;
__global__ void __launch_bounds__(kRayBlock)
k_scene_stats(uint32_t n_rays, const unsigned long long* __restrict__ best, const uint4* __restrict__ work, uint32_t* __restrict__ cnt) {
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
  if (n_bad) atomicAdd(&cnt[kSceneBadRays], n_bad);
  if (n_hit) atomicAdd(&cnt[kSceneHits], n_hit);
  if (n_front) atomicAdd(&cnt[kSceneFrontHits], n_front);
  if (layers) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kSceneLayersLo), layers);
  if (bit_tests) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kSceneBitTestsLo), bit_tests);
  if (lookups) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kSceneLookupsLo), lookups);
  if (misses) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kSceneMissesLo), misses);
  if (tests) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kSceneTestsLo), tests);
  if (bits) atomicMax(&cnt[kSceneMaxTBits], bits);           // (bits of non-negative floats order as the floats do)
}

// empty: the build's buffers go; the cast workspace and the counters stay for the next build
void scene_clear(smx_rayscene_s* sc) {
  sc->built = false;
  sc->recs.reset(); sc->wide_recs.reset(); sc->table.reset(); sc->bits.reset();
  sc->mask = sc->n_entries = sc->n_wide = 0;
  sc->grid = SceneGrid{{0, 0, 0}, {0, 0, 0}, -1};
}

template <typename T>
unsigned long long scene_bytes(const DevBuf<T>& b) { return (unsigned long long)b.capacity() * sizeof(T); }

int scene_build(smx_recon r, hipStream_t st, smx_rayscene_s* sc, const smx_rayscene_params* p, const uint32_t* triangles, uint32_t n_in,
                bool dev, uint32_t n, smx_rayscene_stats* stats) {
  SMX_CALL(sc->build_stamps.begin(st));
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    sc->build_stamps.publish();
    return rc;
  };
  TgWork& w = r->raycast.grid;
  if (!sc->counters.get()) SMX_CALL(sc->counters.alloc(kSceneBuildWords, false));
  SMX_CALL(w.reserve_mark(n_in));
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(r->raycast.in, triangles, (size_t)3 * n_in, dev, st, &din));
  uint32_t* cnt = sc->counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kSceneBuildWords * sizeof(uint32_t), st));
  uint32_t* h = sc->h;

  // ---- mark
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const TgMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  SMX_CALL(tg_enqueue_mark(w, TgBoxes::kForRays, map, din, n_in, p->cell_size, kRayMinCell, cnt, st));
  SMX_CALL(sc->build_stamps.mark(st));
  uint32_t E = 0, Wd = 0;
  if (const int rc = tg_read_counts(cnt, h, kSceneBuildWords, n, st, &E, &Wd)) return finish(rc);
  int32_t lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = (int32_t)h[kTgOccLo + a]; hi[a] = (int32_t)h[kTgOccHi + a]; }
  int k = -1;
  if (p->occupancy > 0) {
    k = p->occupancy - 1;
    if (!scene_grid_fits(lo, hi, k)) {
      set_error("an occupancy grid of 2^%d cells per block has %llu bits, above the 2^31 allowed", k, scene_grid_bits(lo, hi, k));
      return finish(SMX_ERR_INVALID_ARGUMENT);
    }
  } else if (p->occupancy == 0 && kSceneAutoGrid && E != 0) {
    k = scene_grid_smallest(lo, hi);
  }
  const SceneGrid grid = scene_grid_make(lo, hi, k);
  const unsigned long long n_bits = k < 0 ? 0ull : scene_grid_bits(lo, hi, k);
  const uint32_t n_words = (uint32_t)((n_bits + 31) >> 5);

  // ---- index, into the scene's own records and table
  uint32_t mask = 0;
  const unsigned long long* sorted_keys = nullptr;
  SMX_CALL(tg_enqueue_index(w, TgBoxes::kForRays, map, din, n_in, E, Wd, 0, cnt, sc->recs, sc->wide_recs, sc->table, &mask, &sorted_keys, st));
  SMX_CALL(sc->build_stamps.mark(st));

  // ---- occupancy
  if (k >= 0) {
    SMX_CALL(sc->bits.alloc(n_words, false));
    SMX_HIP(hipMemsetAsync(sc->bits.get(), 0, (size_t)std::max<uint32_t>(n_words, 1u) * sizeof(uint32_t), st));
    if (E > 0 && n_words > 0) {
      hipLaunchKernelGGL(k_scene_occupancy, dim3(blocks_for(E)), dim3(kRayBlock), 0, st, sorted_keys, E, grid, sc->bits.get());
      hipLaunchKernelGGL(k_scene_popcount, dim3(std::min<unsigned>(blocks_for(n_words), 4096u)), dim3(kRayBlock), 0, st, sc->bits.get(), n_words, cnt);
      SMX_LAUNCH_CHECK();
    }
  }
  SMX_CALL(sc->build_stamps.mark(st));
  SMX_HIP(hipMemcpyAsync(h, cnt, kSceneBuildWords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  sc->mask = mask; sc->n_entries = E; sc->n_wide = Wd; sc->grid = grid;
  sc->built = true;
  if (stats) {
    stats->n_not_live = h[kTgNotLive]; stats->n_repeated = h[kTgRepeated]; stats->n_out_of_range = h[kTgRange];
    stats->n_wide = Wd; stats->n_entries = E; stats->n_cells = h[kTgCells];
    memcpy(&stats->cell_size_used, &h[kTgCellBits], sizeof(float));
    stats->occupancy_log2 = k; stats->n_blocks_set = h[kSceneBlocksSet];
    stats->occupancy_bytes = (unsigned long long)n_words * sizeof(uint32_t);
    stats->device_bytes = scene_bytes(sc->recs) + scene_bytes(sc->wide_recs) + scene_bytes(sc->table) + scene_bytes(sc->bits) +
                          scene_bytes(sc->counters) + scene_bytes(sc->cast_counters) + scene_bytes(sc->best) + scene_bytes(sc->work) +
                          scene_bytes(sc->rays) + scene_bytes(sc->out_t) + scene_bytes(sc->out_uv) + scene_bytes(sc->out_hit);
  }
  return finish(SMX_OK);
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_rayscene_params_default(smx_rayscene_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->cell_size = 0.0f; out->occupancy = 0;
  return SMX_OK;
}

int smx_rayscene_create(int32_t device_id, smx_rayscene* out) {
  SMX_CHECK_ARG(out != nullptr);
  int device = 0;
  SMX_CALL(resolve_device(device_id, &device));
  SMX_ON_DEVICE(device);
  std::unique_ptr<smx_rayscene_s> sc(new smx_rayscene_s());
  sc->device = device;
  *out = sc.release();
  return SMX_OK;
}

int smx_rayscene_destroy(smx_rayscene sc) {
  if (!sc) return SMX_OK;
  SMX_ON_DEVICE(sc->device);
  (void)hipDeviceSynchronize();
  delete sc;
  return SMX_OK;
}

int smx_recon_build_rayscene(smx_recon r, smx_stream s, smx_rayscene sc, const smx_rayscene_params* p, const uint32_t* triangles, uint32_t n_in,
                             int32_t on_device, smx_rayscene_stats* stats) {
  SMX_CHECK_ARG(sc != nullptr);
  SMX_ON_DEVICE(sc->device);
  scene_clear(sc);                       // (a refused build leaves the scene empty too; casts are synchronous: nothing reads what goes)
  SMX_CHECK_ARG(r != nullptr && p != nullptr);
  SMX_CHECK_ARG(sc->device == r->device);
  SMX_CHECK_ARG(finite_f(p->cell_size) && p->cell_size >= 0.0f);
  SMX_CHECK_ARG(p->occupancy >= -1 && p->occupancy <= 1 + kSceneMaxLog2);
  SMX_CHECK_ARG(n_in <= (1u << 28));
  SMX_CHECK_ARG(triangles != nullptr || n_in == 0);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; stats->occupancy_log2 = -1; }
  const int rc = scene_build(r, st, sc, p, triangles, n_in, on_device != 0, n, stats);
  if (rc != SMX_OK) {
    (void)hipStreamSynchronize(st);      // (a failed build leaves the scene empty)
    scene_clear(sc);
  }
  return rc;
}

int smx_rayscene_cast(smx_rayscene sc, smx_stream s, const smx_raycast_params* p, const float* rays, uint32_t n_rays, uint32_t* hit, float* t,
                      float* uv, int32_t on_device, smx_rayscene_cast_stats* stats) {
  SMX_CHECK_ARG(sc != nullptr && p != nullptr);
  SMX_CHECK_ARG(finite_f(p->t_min) && finite_f(p->t_max) && p->t_min >= 0.0f && p->t_min <= p->t_max && p->t_max <= SMX_RAY_MAX_T);
  SMX_CHECK_ARG(p->cell_size == 0.0f);
  SMX_CHECK_ARG(p->cull == 0 || p->cull == 1 || p->cull == 2);
  SMX_CHECK_ARG(n_rays <= (1u << 28));
  SMX_CHECK_ARG((rays != nullptr && hit != nullptr && t != nullptr) || n_rays == 0);
  if (!sc->built) {
    set_error("smx_rayscene_cast on an empty scene: build it first");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  {
    const void* outs[3] = {hit, t, uv};
    const size_t out_bytes[3] = {(size_t)n_rays * 4, (size_t)n_rays * 4, (size_t)n_rays * 8};
    for (int o = 0; o < 3; ++o)
      if (ranges_overlap(rays, (size_t)n_rays * 24, outs[o], out_bytes[o])) {
        set_error("an output of smx_rayscene_cast overlaps rays");
        return SMX_ERR_INVALID_ARGUMENT;
      }
  }
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  // ---- every allocation of the call lies before the first write to an output
  const bool dev = on_device != 0;
  if (!sc->cast_counters.get()) SMX_CALL(sc->cast_counters.alloc(kSceneWords, false));
  SMX_CALL(sc->best.reserve(n_rays));
  SMX_CALL(sc->work.reserve((size_t)kSceneWorkWords * n_rays));
  const float* drays = nullptr;
  SMX_CALL(stage_in(sc->rays, rays, (size_t)6 * n_rays, dev, st, &drays));
  uint32_t* d_hit = hit;
  float* d_t = t;
  float* d_uv = uv;
  if (!dev && n_rays > 0) {
    SMX_CALL(sc->out_hit.reserve(n_rays));
    SMX_CALL(sc->out_t.reserve(n_rays));
    if (uv) SMX_CALL(sc->out_uv.reserve((size_t)2 * n_rays));
    d_hit = sc->out_hit.get(); d_t = sc->out_t.get(); d_uv = uv ? sc->out_uv.get() : nullptr;
  }
  uint32_t* cnt = sc->cast_counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kSceneWords * sizeof(uint32_t), st));
  SMX_CALL(sc->cast_stamps.begin(st));   // (the phases are the kernels', as smx_recon_raycast_mesh stamps them)
  auto finish = [&](int rc) -> int {
    SMX_HIP(hipStreamSynchronize(st));
    sc->cast_stamps.publish();
    return rc;
  };

  // ---- cast
  const dim3 b(kRayBlock);
  uint4* work = reinterpret_cast<uint4*>(sc->work.get());
  if (n_rays > 0) {
    float cell;
    memcpy(&cell, &sc->h[kTgCellBits], sizeof(float));
    SceneBox occ;
    for (int a = 0; a < 3; ++a) { occ.lo[a] = (int32_t)sc->h[kTgOccLo + a]; occ.hi[a] = (int32_t)sc->h[kTgOccHi + a]; }
    hipLaunchKernelGGL(k_scene_cast, dim3((unsigned)div_up(n_rays, kRayWaves)), b, 0, st, drays, n_rays, reinterpret_cast<const TgCell*>(sc->table.get()),
                       sc->mask, reinterpret_cast<const TgRec*>(sc->recs.get()), reinterpret_cast<const TgRec*>(sc->wide_recs.get()), sc->n_wide,
                       sc->n_entries, sc->grid, sc->bits.get(), cell, occ, p->t_min, p->t_max, (int)p->cull, d_hit, d_t, d_uv, sc->best.get(), work);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(sc->cast_stamps.mark(st));

  // ---- stats
  if (n_rays > 0) {
    hipLaunchKernelGGL(k_scene_stats, dim3(std::min(blocks_for(n_rays), kSceneStatsBlocks)), b, 0, st, n_rays, sc->best.get(), work, cnt);
    SMX_LAUNCH_CHECK();
    if (!dev) {
      SMX_HIP(hipMemcpyAsync(hit, d_hit, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      SMX_HIP(hipMemcpyAsync(t, d_t, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      if (uv) SMX_HIP(hipMemcpyAsync(uv, d_uv, (size_t)n_rays * 8, hipMemcpyDeviceToHost, st));
    }
  }
  uint32_t h[kSceneWords];
  SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->n_rays = n_rays; stats->n_bad_rays = h[kSceneBadRays]; stats->n_hit = h[kSceneHits]; stats->n_front_hits = h[kSceneFrontHits];
    stats->max_t_bits = h[kSceneMaxTBits];
    stats->n_layers = word64(h, kSceneLayersLo); stats->n_bit_tests = word64(h, kSceneBitTestsLo);
    stats->n_lookups = word64(h, kSceneLookupsLo); stats->n_lookup_misses = word64(h, kSceneMissesLo);
    stats->n_pair_tests = word64(h, kSceneTestsLo);
  }
  SMX_CALL(sc->cast_stamps.mark(st));
  return finish(SMX_OK);
}

int smx_rayscene_debug_timings(smx_rayscene sc, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(sc != nullptr && out_ms != nullptr && capacity >= SMX_RAYSCENE_PHASES);
  SMX_ON_DEVICE(sc->device);
  SMX_CALL(sc->build_stamps.elapsed_ms(out_ms, 3));
  return sc->cast_stamps.elapsed_ms(out_ms + 3, 2);
}

}  // extern "C"
