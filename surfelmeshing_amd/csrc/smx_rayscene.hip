// smx_rayscene.hip -- smx_rayscene (gfx950): the search structure of smx_recon_raycast_mesh built once and kept, with an
// occupancy bit grid in front of its cell table (the contract is in include/smx.h, the grid's sizes in
// smx_rayscene.hpp, its index function and the filtered walk in smx_raycast.hpp).
//
//   build:  tg_enqueue_mark and tg_enqueue_index of smx_trigrid.hip as smx_recon_raycast_mesh calls them, writing
//           the records and the cell table into the scene's own buffers -> k_scene_occupancy (a lane per sorted entry; the head
//           of a run sets its block's bit, one atomic per distinct bit of the wavefront) -> k_scene_popcount (the set bits,
//           counted from the bits)
//   cast:   the cast of smx_raycast.hip (k_ray_cast -> k_ray_stats) on the index the scene keeps, with the bit test in front
//           of both look-up sites
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

// bits is all zeros before.  At k > 0 the heads of one block lie near each other in the sorted order (z runs fastest in the
// cell key), so a wavefront issues one atomic per distinct bit, and none where a plain read already sees the bit (a stale
// read costs one atomic).
__global__ void __launch_bounds__(kRayBlock)
k_scene_occupancy(const unsigned long long* __restrict__ keys, uint32_t n_entries, RayGrid grid, uint32_t* bits) {
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

// empty: the build's buffers go; the cast workspace and the counters stay for the next build
void scene_clear(smx_rayscene_s* sc) {
  sc->built = false;
  sc->recs.reset(); sc->wide_recs.reset(); sc->table.reset(); sc->bits.reset();
  sc->mask = sc->n_entries = sc->n_wide = 0;
  sc->grid = RayGrid{{0, 0, 0}, {0, 0, 0}, -1};
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
  const RayGrid grid = scene_grid_make(lo, hi, k);
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
                          scene_bytes(sc->counters) + sc->cast.bytes();
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
  SMX_CALL(ray_cast_overlap("smx_rayscene_cast", "rays", rays, (size_t)n_rays * 24, n_rays, hit, t, uv));
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  // ---- every allocation of the call lies before the first write to an output
  const bool dev = on_device != 0;
  RayCastArrays d;
  SMX_CALL(ray_cast_stage(sc->cast, rays, n_rays, hit, t, uv, dev, st, &d));
  SMX_CALL(sc->cast_stamps.begin(st));   // (the phases are the kernels', as smx_recon_raycast_mesh stamps them)
  auto finish = [&](int rc) -> int {
    SMX_HIP(hipStreamSynchronize(st));
    sc->cast_stamps.publish();
    return rc;
  };
  RayIndex ix{reinterpret_cast<const TgCell*>(sc->table.get()), sc->mask, reinterpret_cast<const TgRec*>(sc->recs.get()),
              reinterpret_cast<const TgRec*>(sc->wide_recs.get()), sc->n_entries, sc->n_wide, 0.0f, {}, sc->grid, sc->bits.get(), nullptr};
  ray_index_read(&ix, sc->h);
  smx_rayscene_cast_stats cs;
  SMX_CALL(ray_cast_launch(sc->cast, ix, p, d, n_rays, st));
  SMX_CALL(sc->cast_stamps.mark(st));
  SMX_CALL(ray_cast_finish(sc->cast, ix, d, n_rays, hit, t, uv, dev, st, &cs));
  if (stats) *stats = cs;
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
