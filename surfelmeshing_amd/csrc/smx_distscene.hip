// smx_distscene.hip -- smx_distscene (gfx950): the search structure of smx_recon_mesh_distance built once and kept, with a way
// from a triangle to one of its records so that a query needs neither the map nor the triangle array (the
// contract is in include/smx.h, the first-record rule in smx_distscene.hpp, the query's kernels in smx_distance.hip).
//
//   build:  tg_enqueue_mark and tg_enqueue_index of smx_trigrid.hip as smx_recon_mesh_distance calls them, writing
//           the records and the cell table into the scene's own buffers -> k_dscene_first (a lane per record, cell records and
//           wide records alike: one integer minimum into first_rec[t])
//   rim:    smx_recon_build_distscene_rim = the build, then rim_run of smx_rim.hip on the same array, its bytes copied into the scene
//   query:  dist_scene_query of smx_distance.hip (k_dist_point_keys -> the sort -> k_dscene_query -> k_dist_stats) on the index
//           the scene keeps
//
// A query's outputs are a function of the minimum of a set of 64-bit keys over the records and of the winner's corners, which
// are copies of the corners as the map held them at the build: the bytes of smx_recon_mesh_distance on that map, whatever the
// schedule.  first_rec is a minimum of integers, so the scene's own bytes do not depend on the schedule either.
#include <memory>

#include "smx_recon_state.hpp"
#include "smx_distscene.hpp"

namespace smx {

namespace {

// first_rec is all kDsceneNoRec before.  sorted_t[j] = the triangle of cell record j, wide_t[j] = the triangle of wide record j
// (the lists the records were written from).  One atomic per record: neighbouring records of one cell never share a triangle, so
// there is nothing to fold within a wavefront but the few runs of neighbouring cells.
__global__ void __launch_bounds__(kTgBlock)
k_dscene_first(const uint32_t* __restrict__ sorted_t, uint32_t n_entries, const uint32_t* __restrict__ wide_t, uint32_t n_wide, uint32_t n_in,
               uint32_t* first_rec) {
  const uint32_t j = blockIdx.x * kTgBlock + threadIdx.x;
  if (j >= n_entries + n_wide) return;
  const bool wide = j >= n_entries;
  const uint32_t position = wide ? j - n_entries : j;
  const uint32_t t = wide ? wide_t[position] : sorted_t[position];
  if (t < n_in) atomicMin(&first_rec[t], dscene_first_word(position, wide));
}

// empty: the build's buffers go; the query workspace and the counters stay for the next build
void dscene_clear(smx_distscene_s* sc) {
  sc->built = false;
  sc->recs.reset(); sc->wide_recs.reset(); sc->table.reset(); sc->first_rec.reset(); sc->rim.reset();
  sc->has_rim = false;
  sc->mask = sc->n_entries = sc->n_wide = sc->n_in = 0;
  sc->max_distance = 0.0f;
}

template <typename T>
unsigned long long dscene_bytes(const DevBuf<T>& b) { return (unsigned long long)b.capacity() * sizeof(T); }

int dscene_build(smx_recon r, hipStream_t st, smx_distscene_s* sc, const smx_distscene_params* p, const uint32_t* triangles, uint32_t n_in,
                 bool dev, uint32_t n, smx_distscene_stats* stats) {
  SMX_CALL(sc->build_stamps.begin(st));
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    sc->build_stamps.publish();
    return rc;
  };
  TgWork& w = r->distance.grid;
  if (!sc->counters.get()) SMX_CALL(sc->counters.alloc(kDsceneBuildWords, false));
  SMX_CALL(w.reserve_mark(n_in));
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(r->distance.in, triangles, (size_t)3 * n_in, dev, st, &din));
  uint32_t* cnt = sc->counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kDsceneBuildWords * sizeof(uint32_t), st));
  uint32_t* h = sc->h;

  // ---- mark
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const TgMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  SMX_CALL(tg_enqueue_mark(w, TgBoxes::kExact, map, din, n_in, p->cell_size, kDistMargin * p->max_distance, cnt, st));
  SMX_CALL(sc->build_stamps.mark(st));
  uint32_t E = 0, Wd = 0;
  if (const int rc = tg_read_counts(cnt, h, kDsceneBuildWords, n, st, &E, &Wd)) return finish(rc);

  // ---- index, into the scene's own records and table
  uint32_t mask = 0;
  const uint32_t* sorted_t = nullptr;
  SMX_CALL(tg_enqueue_index(w, TgBoxes::kExact, map, din, n_in, E, Wd, 0, cnt, sc->recs, sc->wide_recs, sc->table, &mask, nullptr, st, &sorted_t));
  SMX_CALL(sc->build_stamps.mark(st));

  // ---- first: the triangles of the sorted entries lie beside their keys in the build's workspace
  SMX_CALL(sc->first_rec.alloc(n_in, false));
  SMX_HIP(hipMemsetAsync(sc->first_rec.get(), 0xFF, (size_t)std::max<uint32_t>(n_in, 1u) * sizeof(uint32_t), st));
  if (E + Wd > 0) {
    hipLaunchKernelGGL(k_dscene_first, dim3(blocks_for(E + Wd)), dim3(kTgBlock), 0, st, sorted_t, E, w.wide_t.get(), Wd, n_in, sc->first_rec.get());
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(sc->build_stamps.mark(st));
  SMX_HIP(hipMemcpyAsync(h, cnt, kDsceneBuildWords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  sc->mask = mask; sc->n_entries = E; sc->n_wide = Wd; sc->n_in = n_in; sc->max_distance = p->max_distance;
  sc->built = true;
  if (stats) {
    stats->n_not_live = h[kTgNotLive]; stats->n_repeated = h[kTgRepeated]; stats->n_out_of_range = h[kTgRange];
    stats->n_wide = Wd; stats->n_entries = E; stats->n_cells = h[kTgCells];
    memcpy(&stats->cell_size_used, &h[kTgCellBits], sizeof(float));
    stats->max_distance = p->max_distance;
    stats->device_bytes = dscene_bytes(sc->recs) + dscene_bytes(sc->wide_recs) + dscene_bytes(sc->table) + dscene_bytes(sc->first_rec) +
                          dscene_bytes(sc->counters) + sc->query.bytes();
  }
  return finish(SMX_OK);
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_distscene_params_default(smx_distscene_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->max_distance = 0.05f; out->cell_size = 0.0f;
  return SMX_OK;
}

int smx_distscene_create(int32_t device_id, smx_distscene* out) {
  SMX_CHECK_ARG(out != nullptr);
  int device = 0;
  SMX_CALL(resolve_device(device_id, &device));
  SMX_ON_DEVICE(device);
  std::unique_ptr<smx_distscene_s> sc(new smx_distscene_s());
  sc->device = device;
  *out = sc.release();
  return SMX_OK;
}

int smx_distscene_destroy(smx_distscene sc) {
  if (!sc) return SMX_OK;
  SMX_ON_DEVICE(sc->device);
  (void)hipDeviceSynchronize();
  delete sc;
  return SMX_OK;
}

int smx_recon_build_distscene(smx_recon r, smx_stream s, smx_distscene sc, const smx_distscene_params* p, const uint32_t* triangles, uint32_t n_in,
                              int32_t on_device, smx_distscene_stats* stats) {
  SMX_CHECK_ARG(sc != nullptr);
  SMX_ON_DEVICE(sc->device);
  SMX_CALL(sc->reg.mark.sync());         // (a registration may still be running: the one call on a scene that does not wait)
  dscene_clear(sc);                      // (a refused build leaves the scene empty too; queries are synchronous: nothing reads what goes)
  SMX_CHECK_ARG(r != nullptr && p != nullptr);
  SMX_CHECK_ARG(finite_f(p->max_distance) && p->max_distance >= 1e-3f && p->max_distance <= 16.0f);
  SMX_CHECK_ARG(finite_f(p->cell_size) && p->cell_size >= 0.0f);
  SMX_CHECK_ARG(n_in <= (1u << 28));
  SMX_CHECK_ARG(triangles != nullptr || n_in == 0);
  SMX_CHECK_ARG(sc->device == r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; }
  const int rc = dscene_build(r, st, sc, p, triangles, n_in, on_device != 0, n, stats);
  if (rc != SMX_OK) {
    (void)hipStreamSynchronize(st);      // (a failed build leaves the scene empty)
    dscene_clear(sc);
  }
  return rc;
}

// By definition smx_recon_build_distscene followed by smx_recon_mesh_rim of the same array, the bytes kept with the scene.
int smx_recon_build_distscene_rim(smx_recon r, smx_stream s, smx_distscene sc, const smx_distscene_params* p, const uint32_t* triangles,
                                  uint32_t n_in, int32_t on_device, smx_distscene_stats* stats, smx_rim_stats* rim_stats) {
  SMX_CALL(smx_recon_build_distscene(r, s, sc, p, triangles, n_in, on_device, stats));
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  auto rim = [&]() -> int {
    uint32_t n = 0;
    SMX_CALL(read_surfel_count(r, st, &n));
    SMX_CALL(sc->rim.alloc(n_in, false));
    smx_rim_stats out;
    memset(&out, 0, sizeof(out));
    const uint8_t* d_rim = nullptr;
    SMX_CALL(rim_run(r, st, triangles, n_in, on_device != 0, n, &d_rim, &out));
    if (n_in > 0) {
      SMX_HIP(hipMemcpyAsync(sc->rim.get(), d_rim, n_in, hipMemcpyDeviceToDevice, st));
      SMX_HIP(hipStreamSynchronize(st));
    }
    if (rim_stats) *rim_stats = out;
    return SMX_OK;
  };
  const int rc = rim();
  if (rc != SMX_OK) {                    // (if either half fails the scene is left empty)
    (void)hipStreamSynchronize(st);
    dscene_clear(sc);
    if (stats) memset(stats, 0, sizeof(*stats));
    return rc;
  }
  sc->has_rim = true;
  if (stats) stats->device_bytes += dscene_bytes(sc->rim);
  return SMX_OK;
}

int smx_distscene_query(smx_distscene sc, smx_stream s, const smx_distance_params* p, const float* points, uint32_t n_points, uint32_t* nearest,
                        float* distance, float* closest, int32_t on_device, smx_distance_stats* stats) {
  SMX_CHECK_ARG(sc != nullptr && p != nullptr);
  SMX_CHECK_ARG(finite_f(p->max_distance) && p->max_distance >= 1e-3f && p->max_distance <= 16.0f);
  SMX_CHECK_ARG(p->cell_size == 0.0f);
  SMX_CHECK_ARG(p->signed_distance == 0 || p->signed_distance == 1);
  SMX_CHECK_ARG(n_points <= (1u << 28));
  SMX_CHECK_ARG((points != nullptr && nearest != nullptr && distance != nullptr) || n_points == 0);
  if (!sc->built) {
    set_error("smx_distscene_query on an empty scene: build it first");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  if (p->max_distance > sc->max_distance) {
    set_error("smx_distscene_query: max_distance %g is above the %g the scene was built for", (double)p->max_distance, (double)sc->max_distance);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  {
    const void* outs[3] = {nearest, distance, closest};
    const size_t out_bytes[3] = {(size_t)n_points * 4, (size_t)n_points * 4, (size_t)n_points * 12};
    for (int o = 0; o < 3; ++o)
      if (ranges_overlap(points, (size_t)n_points * 12, outs[o], out_bytes[o])) {
        set_error("an output of smx_distscene_query overlaps points");
        return SMX_ERR_INVALID_ARGUMENT;
      }
  }
  SMX_ON_DEVICE(sc->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(sc->reg.mark.sync());         // (a registration still running uses the query's workspace, which may grow here)
  smx_distance_stats out;
  memset(&out, 0, sizeof(out));
  const DistSceneIndex ix{reinterpret_cast<const TgCell*>(sc->table.get()), sc->mask, reinterpret_cast<const TgRec*>(sc->recs.get()),
                          reinterpret_cast<const TgRec*>(sc->wide_recs.get()), sc->n_wide, sc->first_rec.get(), sc->counters.get()};
  SMX_CALL(dist_scene_query(sc->query, ix, p, points, n_points, nearest, distance, closest, on_device != 0, st, sc->query_stamps, &out));
  if (stats) {
    const uint32_t* h = sc->h;
    out.n_in = sc->n_in; out.n_points = n_points;
    out.n_not_live = h[kTgNotLive]; out.n_repeated = h[kTgRepeated]; out.n_out_of_range = h[kTgRange];
    out.n_wide = sc->n_wide; out.n_entries = sc->n_entries; out.n_cells = h[kTgCells];
    memcpy(&out.cell_size_used, &h[kTgCellBits], sizeof(float));
    *stats = out;
  }
  return SMX_OK;
}

int smx_distscene_debug_timings(smx_distscene sc, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(sc != nullptr && out_ms != nullptr && capacity >= SMX_DISTSCENE_PHASES);
  SMX_ON_DEVICE(sc->device);
  SMX_CALL(sc->build_stamps.elapsed_ms(out_ms, 3));
  return sc->query_stamps.elapsed_ms(out_ms + 3, 2);
}

}  // extern "C"
