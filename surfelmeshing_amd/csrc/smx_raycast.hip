// smx_raycast.hip -- the kernels of smx_recon_raycast_mesh (gfx950): for each of many rays the first triangle of a triangle
// array over the surfel map it hits, exactly the minimum over all triangles (the contract is in include/smx.h,
// its arithmetic and the traversal in smx_raycast.hpp, the classes, the cell table and the records in smx_distance.hpp).
//
//   mark:   k_ray_classify (a lane per triangle: range check, step 1's classes, the extents summed per wavefront in fixed
//           point) -> k_ray_cell (one lane: c, the occupied box set to empty) -> k_ray_mark (a lane per triangle of R: its
//           box inflated by SLACK, the entry count or the wide list by ballot compaction, the occupied box by one integer
//           minimum / maximum per wavefront and axis, entries counted per workgroup) -> enqueue_segment_scan
//   index:  k_ray_entries ((cell key, i) per cell of every box) -> the stable radix sort of smx_nn.hip -> k_ray_records (the
//           packed corner records in the sorted order, and the wide list's) -> k_ray_table (the head and the tail of every
//           run add its bounds to the cell's entry of an open-addressing table)
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
// smx_raycast.hpp) and the two reads of the counters.  The mark and the index phase are ray_enqueue_mark and ray_enqueue_index,
// which smx_recon_build_rayscene (smx_rayscene.hip) calls too, with a scene's records and table in place of the workspace's.
#include <cmath>

#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

constexpr int kRBlock = kRayBlock;

__device__ __forceinline__ DistVec ray_pos(const DistMap& map, uint32_t i) {
  const float4 s = map.smooth[(size_t)i * map.smooth_stride];
  return DistVec{s.x, s.y, s.z};
}
__device__ __forceinline__ bool ray_live(const DistMap& map, uint32_t i, const DistVec& p) {
  return dec_live(p.x, p.y, p.z, map.normal[(size_t)i * map.normal_stride].w);
}
__device__ __forceinline__ float ray_cell_of(const uint32_t* cnt) { return __uint_as_float(cnt[kRayCellBits]); }

// mark[i] = 1 for a triangle of R, else 0.  (A triangle with an index out of range reads nothing; the call is refused.)
__global__ void __launch_bounds__(kRBlock)
k_ray_classify(DistMap map, const uint32_t* __restrict__ tri, uint32_t n_in, uint32_t* __restrict__ mark, uint32_t* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * kRBlock + threadIdx.x;
  uint32_t cls = 0xFFu;
  unsigned long long extent = 0;
  bool bad_index = false;
  if (t < n_in) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= map.n || i1 >= map.n || i2 >= map.n) {
      bad_index = true;
    } else {
      const DistVec a = ray_pos(map, i0), b = ray_pos(map, i1), c = ray_pos(map, i2);
      cls = dist_classify(i0, i1, i2, ray_live(map, i0, a), ray_live(map, i1, b), ray_live(map, i2, c), a, b, c);
      if (cls == kDistInR) extent = (unsigned long long)(dist_extent(a, b, c) * 1048576.0f);     // (at most 128 m: 2^27)
    }
    mark[t] = cls == kDistInR ? 1u : 0u;
  }
  extent = ray_wave_sum(extent);
  if ((threadIdx.x & 63) == 0 && extent != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayExtentLo), extent);
  if (__ballot(bad_index) != 0 && (threadIdx.x & 63) == 0) atomicOr(&cnt[kRayError], 1u);      // (one per wavefront)
  ray_wave_count(&cnt[kRayNotLive], cls == kDistDropNotLive);
  ray_wave_count(&cnt[kRayRepeated], cls == kDistDropRepeated);
  ray_wave_count(&cnt[kRayRange], cls == kDistDropRange);
  ray_wave_count(&cnt[kRayInRCount], cls == kDistInR);
}

__global__ void k_ray_cell(float cell_size, uint32_t* cnt) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float given = cell_size;
  if (!(cell_size > 0.0f)) {
    const unsigned long long sum = *reinterpret_cast<const unsigned long long*>(cnt + kRayExtentLo);
    const uint32_t r = cnt[kRayInRCount];
    given = r != 0 ? (float)((double)sum / (double)r * (1.0 / 1048576.0)) : 0.0f;
  }
  cnt[kRayCellBits] = __float_as_uint(ray_cell_size(given));
  for (int k = 0; k < 3; ++k) { cnt[kRayOccLo + k] = 0x7FFFFFFFu; cnt[kRayOccHi + k] = 0x80000000u; }      // (int32: empty)
}

__device__ __forceinline__ DistBox ray_box_of(const DistMap& map, const uint32_t* tri, uint32_t t, float cell) {
  const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
  return ray_box(ray_pos(map, i0), ray_pos(map, i1), ray_pos(map, i2), cell);
}

// mark[i]: 1 -> the entry count of the triangle or kDistWide.  wide_t has n_in entries.
__global__ void __launch_bounds__(kRBlock)
k_ray_mark(DistMap map, const uint32_t* __restrict__ tri, uint32_t n_in, uint32_t* __restrict__ mark, uint32_t* __restrict__ wide_t,
           uint32_t* __restrict__ block_sums, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t wave_tot[kRayWaves];
  const uint32_t t = blockIdx.x * kRBlock + threadIdx.x;
  const float cell = ray_cell_of(cnt);
  uint32_t word = 0;
  int32_t lx = 0x7FFFFFFF, ly = 0x7FFFFFFF, lz = 0x7FFFFFFF, hx = -0x7FFFFFFF - 1, hy = -0x7FFFFFFF - 1, hz = -0x7FFFFFFF - 1;
  if (t < n_in && mark[t] != 0) {
    const DistBox box = ray_box_of(map, tri, t, cell);
    word = dist_mark(box);
    mark[t] = word;
    if (word != kDistWide) { lx = box.lo[0]; ly = box.lo[1]; lz = box.lo[2]; hx = box.hi[0]; hy = box.hi[1]; hz = box.hi[2]; }
  }
  const bool wide = word == kDistWide;
  const uint32_t lane = threadIdx.x & 63;
  if (__ballot(word != 0 && !wide) != 0) {                   // (uniform over the wavefront)
    lx = ray_wave_imin(lx); ly = ray_wave_imin(ly); lz = ray_wave_imin(lz);
    hx = ray_wave_imax(hx); hy = ray_wave_imax(hy); hz = ray_wave_imax(hz);
    if (lane == 0) {
      // the box only grows: a plain read that already holds this wavefront's bound saves the atomic (a stale read costs one)
      int32_t* occ = reinterpret_cast<int32_t*>(cnt);
      const volatile int32_t* seen = occ;
      if (lx < seen[kRayOccLo]) atomicMin(&occ[kRayOccLo], lx);
      if (ly < seen[kRayOccLo + 1]) atomicMin(&occ[kRayOccLo + 1], ly);
      if (lz < seen[kRayOccLo + 2]) atomicMin(&occ[kRayOccLo + 2], lz);
      if (hx > seen[kRayOccHi]) atomicMax(&occ[kRayOccHi], hx);
      if (hy > seen[kRayOccHi + 1]) atomicMax(&occ[kRayOccHi + 1], hy);
      if (hz > seen[kRayOccHi + 2]) atomicMax(&occ[kRayOccHi + 2], hz);
    }
  }
  const unsigned long long m = __ballot(wide);
  if (m != 0) {
    const uint32_t leader = (uint32_t)(__ffsll((long long)m) - 1);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&cnt[kRayNWide], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader);
    if (wide) wide_t[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = t;      // (at most n_in wide triangles in all)
  }
  uint32_t total;
  (void)block_excl_scan<kRayWaves>(wide ? 0u : word, wave_tot, total);
  if (threadIdx.x == 0) {
    block_sums[blockIdx.x] = total;
    if (total != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayEntries64Lo), (unsigned long long)total);
  }
}

__global__ void __launch_bounds__(kRBlock)
k_ray_entries(DistMap map, const uint32_t* __restrict__ tri, uint32_t n_in, const uint32_t* __restrict__ mark,
              const uint32_t* __restrict__ block_off, const uint32_t* __restrict__ cnt, uint32_t n_entries,
              unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ uint32_t wave_tot[kRayWaves];
  const uint32_t t = blockIdx.x * kRBlock + threadIdx.x;
  uint32_t count = t < n_in ? mark[t] : 0u;
  if (count == kDistWide) count = 0;
  uint32_t total;
  const uint32_t off = block_off[blockIdx.x] + block_excl_scan<kRayWaves>(count, wave_tot, total);
  if (count == 0 || off + count > n_entries) return;         // (the second never holds: off + count <= the scan's total)
  const DistBox box = ray_box_of(map, tri, t, ray_cell_of(cnt));
  for (uint32_t j = 0; j < count; ++j) { keys[off + j] = dist_box_key(box, j); vals[off + j] = t; }
}

// recs[j] = the corners of triangle list[j]
__global__ void __launch_bounds__(kRBlock)
k_ray_records(DistMap map, const uint32_t* __restrict__ tri, const uint32_t* __restrict__ list, uint32_t m, DistRec* __restrict__ recs) {
  const uint32_t j = blockIdx.x * kRBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t t = list[j];
  const DistVec a = ray_pos(map, tri[3 * (size_t)t]), b = ray_pos(map, tri[3 * (size_t)t + 1]), c = ray_pos(map, tri[3 * (size_t)t + 2]);
  DistRec r;
  r.a = make_float4(a.x, a.y, a.z, __uint_as_float(t)); r.b = make_float4(b.x, b.y, b.z, 0.0f); r.c = make_float4(c.x, c.y, c.z, 0.0f);
  recs[j] = r;
}

// the table is all zeros before: empty
__global__ void __launch_bounds__(kRBlock)
k_ray_table(const unsigned long long* __restrict__ keys, uint32_t n_entries, DistCell* table, uint32_t mask, uint32_t* __restrict__ cnt) {
  const uint32_t j = blockIdx.x * kRBlock + threadIdx.x;
  bool head = false;
  if (j < n_entries) {
    RayDeviceTable tab{table};
    head = dist_table_entry(tab, mask, keys, n_entries, j);
  }
  ray_wave_count(&cnt[kRayCells], head);
}

// A wavefront per ray.  Everything that steers a loop (the ray, its axes, the layer count, the ballots, the broadcast
// rectangles and runs, the folded minimum) is uniform over the wavefront; a lane's own state is its layer's rectangle, one
// 64-bit key and three counts.  No LDS, no barrier.
__global__ void __launch_bounds__(kRBlock)
k_ray_cast(DistMap map, const uint32_t* __restrict__ tri, const float* __restrict__ rays, uint32_t n_rays, const DistCell* __restrict__ table,
           uint32_t mask, const DistRec* __restrict__ recs, const DistRec* __restrict__ wide_recs, uint32_t n_wide, uint32_t n_entries,
           const uint32_t* __restrict__ cnt, float t_min, float t_max, int cull, uint32_t* __restrict__ hit, float* __restrict__ t_out,
           float* __restrict__ uv, unsigned long long* __restrict__ best_out, uint4* __restrict__ work_out) {
  const uint32_t lane = threadIdx.x & 63, p = blockIdx.x * kRayWaves + (threadIdx.x >> 6);
  if (p >= n_rays) return;                                   // (the whole wavefront)
  DistVec O, D;
  ray_load(rays, p, &O, &D);
  const bool bad = ray_bad(O, D);
  unsigned long long best = kDistNone;
  uint32_t layers = 0, lookups = 0, tests = 0;
  if (!bad) {
    best = ray_wave_min(ray_walk(RayDeviceRecs{wide_recs}, lane, n_wide, 64, O, D, t_min, t_max, cull, best, &tests));
    if (n_entries != 0) {
      const float cell = ray_cell_of(cnt);
      const int32_t* occ = reinterpret_cast<const int32_t*>(cnt);
      const RayAxes r = ray_axes(O, D, occ[kRayOccLo], occ[kRayOccLo + 1], occ[kRayOccLo + 2], occ[kRayOccHi], occ[kRayOccHi + 1],
                                 occ[kRayOccHi + 2], cell, t_min, t_max);
      const RayDeviceTable tab{const_cast<DistCell*>(table)};
      const RayDeviceRecs cell_recs{recs};
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
            any = dist_table_find(tab, mask, ray_rect_key(r, q, m, j), &first, &end);
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
              found = dist_table_find(tab, mask, ray_rect_key(r, qk, mk, jb + lane), &first, &end);
            }
            unsigned long long runs = __ballot(found);
            while (runs != 0) {
              const int s = __ffsll((long long)runs) - 1;
              runs &= runs - 1;
              const uint32_t f = (uint32_t)__shfl((int)first, s), e = (uint32_t)__shfl((int)end, s);
              best = ray_walk(cell_recs, f + lane, e, 64, O, D, t_min, t_max, cull, best, &tests);
            }
          }
          best = ray_wave_min(best);
          if (ray_done(r, cell, best, mk + 1)) { stop = true; break; }
        }
      }
    }
  }
  const unsigned long long n_layers = ray_wave_sum(layers), n_lookups = ray_wave_sum(lookups), n_tests = ray_wave_sum(tests);
  if (lane != 0) return;
  uint32_t i = kInvalid, flags = bad ? kRayFlagBad : 0u;
  float t = __builtin_inff(), u = __builtin_nanf(""), v = __builtin_nanf("");
  if (best != kDistNone) {
    i = (uint32_t)best;
    const DistVec A = ray_pos(map, tri[3 * (size_t)i]), B = ray_pos(map, tri[3 * (size_t)i + 1]), C = ray_pos(map, tri[3 * (size_t)i + 2]);
    RayHit h{0.0f, 0.0f, 0.0f, 0.0f};
    (void)ray_key(O, D, A, B, C, i, t_min, t_max, cull, &h);           // (the same expressions: the same key)
    t = dist_key_dist2(best); u = h.u; v = h.v;
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
  ray_wave_count(&cnt[kRayBadRays], (w.w & kRayFlagBad) != 0);
  ray_wave_count(&cnt[kRayHits], (w.w & kRayFlagHit) != 0);
  ray_wave_count(&cnt[kRayFrontHits], (w.w & kRayFlagFront) != 0);
  const unsigned long long layers = ray_wave_sum(w.x), lookups = ray_wave_sum(w.y), tests = ray_wave_sum(w.z);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)bits, off); bits = o > bits ? o : bits; }
  if ((threadIdx.x & 63) != 0) return;
  if (layers) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayLayersLo), layers);
  if (lookups) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayLookupsLo), lookups);
  if (tests) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kRayTestsLo), tests);
  if (bits) atomicMax(&cnt[kRayMaxBits], bits);              // (bits of non-negative floats order as the floats do)
}

}  // namespace

int ray_enqueue_mark(RaycastWork& w, const DistMap& map, const uint32_t* din, uint32_t n_in, float cell_size, uint32_t* cnt, hipStream_t st) {
  const int nb = div_up(n_in, kRayBlock);
  const dim3 b(kRayBlock), g_in(nb);
  if (n_in > 0) hipLaunchKernelGGL(k_ray_classify, g_in, b, 0, st, map, din, n_in, w.mark.get(), cnt);
  hipLaunchKernelGGL(k_ray_cell, dim3(1), dim3(64), 0, st, cell_size, cnt);
  if (n_in > 0) {
    hipLaunchKernelGGL(k_ray_mark, g_in, b, 0, st, map, din, n_in, w.mark.get(), w.wide_t.get(), w.blocks.get(), cnt);
    enqueue_segment_scan(st, w.blocks.get(), nb, cnt + kRayEntries);
  }
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int ray_enqueue_index(RaycastWork& w, const DistMap& map, const uint32_t* din, uint32_t n_in, uint32_t E, uint32_t Wd, uint32_t* cnt,
                      DevBuf<float>& recs_buf, DevBuf<float>& wide_buf, DevBuf<unsigned long long>& table_buf, uint32_t* mask_out,
                      const unsigned long long** sorted_keys, hipStream_t st) {
  const dim3 b(kRayBlock), g_in(div_up(n_in, kRayBlock));
  const uint32_t entries = dec_table_size(E), mask = entries - 1;
  for (int k = 0; k < 2; ++k) { SMX_CALL(w.keys[k].reserve(E)); SMX_CALL(w.vals[k].reserve(E)); }
  SMX_CALL(w.hist.reserve(radix_sort_workspace_elems(E)));
  SMX_CALL(recs_buf.reserve((size_t)E * 12));
  SMX_CALL(wide_buf.reserve((size_t)Wd * 12));
  SMX_CALL(table_buf.reserve((size_t)2 * entries));
  DistCell* table = reinterpret_cast<DistCell*>(table_buf.get());
  DistRec* recs = reinterpret_cast<DistRec*>(recs_buf.get());
  DistRec* wide_recs = reinterpret_cast<DistRec*>(wide_buf.get());
  *mask_out = mask;
  *sorted_keys = nullptr;
  SMX_HIP(hipMemsetAsync(table, 0, (size_t)entries * sizeof(DistCell), st));
  if (E > 0) {
    hipLaunchKernelGGL(k_ray_entries, g_in, b, 0, st, map, din, n_in, w.mark.get(), w.blocks.get(), cnt, E, w.keys[0].get(), w.vals[0].get());
    SMX_LAUNCH_CHECK();
    const int cur = radix_sort(w.keys, w.vals, E, 63, w.hist.get(), st);
    hipLaunchKernelGGL(k_ray_records, dim3(ray_blocks(E)), b, 0, st, map, din, w.vals[cur].get(), E, recs);
    hipLaunchKernelGGL(k_ray_table, dim3(ray_blocks(E)), b, 0, st, w.keys[cur].get(), E, table, mask, cnt);
    *sorted_keys = w.keys[cur].get();
  }
  if (Wd > 0) hipLaunchKernelGGL(k_ray_records, dim3(ray_blocks(Wd)), b, 0, st, map, din, w.wide_t.get(), Wd, wide_recs);
  SMX_LAUNCH_CHECK();
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
  SMX_CHECK_ARG(ray_finite_f(p->t_min) && ray_finite_f(p->t_max) && p->t_min >= 0.0f && p->t_min <= p->t_max && p->t_max <= SMX_RAY_MAX_T);
  SMX_CHECK_ARG(ray_finite_f(p->cell_size) && p->cell_size >= 0.0f);
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
        if (ray_overlap(ins[i], in_bytes[i], outs[o], out_bytes[o])) {
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
  const int nb = div_up(n_in, kRayBlock);
  const bool dev = on_device != 0;
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kRayWords, false));
  SMX_CALL(w.mark.reserve(n_in));
  SMX_CALL(w.blocks.reserve((size_t)nb));
  SMX_CALL(w.wide_t.reserve(n_in));
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
  auto read_counters = [&]() -> int {
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    return SMX_OK;
  };

  // ---- mark
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const DistMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  const dim3 b(kRayBlock);
  SMX_CALL(ray_enqueue_mark(w, map, din, n_in, p->cell_size, cnt, st));
  SMX_CALL(w.stamps.mark(st));
  SMX_CALL(read_counters());
  if (h[kRayError] != 0) {
    set_error("triangles holds an index >= the %u slots of the map", n);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  if (ray_word64(h, kRayEntries64Lo) > (1ull << 30)) {
    set_error("more than 2^30 (cell, triangle) entries: choose a larger cell_size");
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  const uint32_t E = h[kRayEntries], Wd = h[kRayNWide];

  // ---- index (every allocation of the call lies before the first write to an output)
  uint32_t mask = 0;
  const unsigned long long* sorted_keys = nullptr;
  SMX_CALL(ray_enqueue_index(w, map, din, n_in, E, Wd, cnt, w.recs, w.wide_recs, w.table, &mask, &sorted_keys, st));
  const DistCell* table = reinterpret_cast<const DistCell*>(w.table.get());
  const DistRec* recs = reinterpret_cast<const DistRec*>(w.recs.get());
  const DistRec* wide_recs = reinterpret_cast<const DistRec*>(w.wide_recs.get());
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
    hipLaunchKernelGGL(k_ray_stats, dim3(ray_blocks(n_rays)), b, 0, st, n_rays, w.best.get(), work, cnt);
    SMX_LAUNCH_CHECK();
    if (!dev) {
      SMX_HIP(hipMemcpyAsync(hit, d_hit, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      SMX_HIP(hipMemcpyAsync(t, d_t, (size_t)n_rays * 4, hipMemcpyDeviceToHost, st));
      if (uv) SMX_HIP(hipMemcpyAsync(uv, d_uv, (size_t)n_rays * 8, hipMemcpyDeviceToHost, st));
    }
  }
  SMX_CALL(read_counters());
  if (stats) {
    stats->n_not_live = h[kRayNotLive]; stats->n_repeated = h[kRayRepeated]; stats->n_out_of_range = h[kRayRange];
    stats->n_bad_rays = h[kRayBadRays]; stats->n_hit = h[kRayHits]; stats->n_front_hits = h[kRayFrontHits]; stats->max_t_bits = h[kRayMaxBits];
    stats->n_wide = Wd; stats->n_entries = E; stats->n_cells = h[kRayCells];
    memcpy(&stats->cell_size_used, &h[kRayCellBits], sizeof(float));
    stats->n_layers = ray_word64(h, kRayLayersLo); stats->n_lookups = ray_word64(h, kRayLookupsLo); stats->n_pair_tests = ray_word64(h, kRayTestsLo);
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
