// smx_trigrid.hip -- the build of the triangle grid (gfx950): the cell table and the packed corner records that
// smx_recon_mesh_distance, smx_recon_raycast_mesh and smx_recon_build_rayscene search (the cell functions and
// the table operations are in smx_trigrid.hpp).
//
//   mark:   k_tg_classify (a lane per triangle: range check, step 1's classes, the extents summed per wavefront in fixed
//           point) -> k_tg_cell (one lane: c, the occupied box set to empty) -> k_tg_mark (a lane per triangle of R: its box,
//           the entry count or the wide list by ballot compaction, entries counted per workgroup) -> enqueue_segment_scan
//   index:  k_tg_entries ((cell key, t) per cell of every box) -> the stable radix sort of smx_nn.hip -> k_tg_records (the
//           packed corner records in the sorted order, and the wide list's) -> k_tg_table (the head and the tail of every
//           run add its bounds to the cell's entry of an open-addressing table)
//
// k_tg_mark and k_tg_entries exist in two compile-time variants (TgBoxes): for rays the box is inflated by SMX_RAY_BOX_SLACK
// and k_tg_mark folds the occupied cell box, by one integer minimum / maximum per wavefront and axis.  The other four kernels
// do not depend on the variant.  Between mark and index the caller reads the counters back (tg_read_counts).
#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

template <TgBoxes kBoxes> struct Variant;
template <> struct Variant<TgBoxes::kExact> { static constexpr bool kSlack = false, kOccupied = false; };
template <> struct Variant<TgBoxes::kForRays> { static constexpr bool kSlack = true, kOccupied = true; };

__device__ __forceinline__ bool tg_live(const TgMap& map, uint32_t i, const TgVec& p) {
  return dec_live(p.x, p.y, p.z, map.normal[(size_t)i * map.normal_stride].w);
}

// mark[t] = 1 for a triangle of R, else 0.  (A triangle with an index out of range reads nothing; the call is refused.)
__global__ void __launch_bounds__(kTgBlock)
k_tg_classify(TgMap map, const uint32_t* __restrict__ tri, uint32_t n_in, uint32_t* __restrict__ mark, uint32_t* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * kTgBlock + threadIdx.x;
  uint32_t cls = 0xFFu;
  unsigned long long extent = 0;
  bool bad_index = false;
  if (t < n_in) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= map.n || i1 >= map.n || i2 >= map.n) {
      bad_index = true;
    } else {
      const TgVec a = tg_pos(map, i0), b = tg_pos(map, i1), c = tg_pos(map, i2);
      cls = tg_classify(i0, i1, i2, tg_live(map, i0, a), tg_live(map, i1, b), tg_live(map, i2, c), a, b, c);
      if (cls == kTgInR) extent = (unsigned long long)(tg_extent(a, b, c) * 1048576.0f);       // (at most 128 m: 2^27)
    }
    mark[t] = cls == kTgInR ? 1u : 0u;
  }
  extent = wave_sum(extent);
  if ((threadIdx.x & 63) == 0 && extent != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kTgExtentLo), extent);
  if (__ballot(bad_index) != 0 && (threadIdx.x & 63) == 0) atomicOr(&cnt[kTgError], 1u);       // (one per wavefront)
  wave_count(&cnt[kTgNotLive], cls == kTgDropNotLive);
  wave_count(&cnt[kTgRepeated], cls == kTgDropRepeated);
  wave_count(&cnt[kTgRange], cls == kTgDropRange);
  wave_count(&cnt[kTgInRCount], cls == kTgInR);
}

__global__ void k_tg_cell(float cell_size, float least, uint32_t* cnt) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float given = cell_size;
  if (!(cell_size > 0.0f)) {
    const unsigned long long sum = *reinterpret_cast<const unsigned long long*>(cnt + kTgExtentLo);
    const uint32_t r = cnt[kTgInRCount];
    given = r != 0 ? (float)((double)sum / (double)r * (1.0 / 1048576.0)) : 0.0f;
  }
  cnt[kTgCellBits] = __float_as_uint(tg_cell_size(given, least));
  for (int k = 0; k < 3; ++k) { cnt[kTgOccLo + k] = 0x7FFFFFFFu; cnt[kTgOccHi + k] = 0x80000000u; }        // (int32: empty)
}

template <class V>
__device__ __forceinline__ TgBox tg_box_of(const TgMap& map, const uint32_t* tri, uint32_t t, float cell) {
  const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
  if constexpr (V::kSlack) return tg_box_slack(tg_pos(map, i0), tg_pos(map, i1), tg_pos(map, i2), cell, kRayBoxSlack);
  else return tg_box(tg_pos(map, i0), tg_pos(map, i1), tg_pos(map, i2), cell);
}

// mark[t]: 1 -> the entry count of the triangle or kTgWide.  wide_t has n_in entries.
template <class V>
__global__ void __launch_bounds__(kTgBlock)
k_tg_mark(TgMap map, const uint32_t* __restrict__ tri, uint32_t n_in, uint32_t* __restrict__ mark, uint32_t* __restrict__ wide_t,
          uint32_t* __restrict__ block_sums, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t wave_tot[kTgBlock / 64];
  const uint32_t t = blockIdx.x * kTgBlock + threadIdx.x, lane = threadIdx.x & 63;
  const float cell = tg_cell_of(cnt);
  uint32_t word = 0;
  int32_t lx = 0x7FFFFFFF, ly = 0x7FFFFFFF, lz = 0x7FFFFFFF, hx = -0x7FFFFFFF - 1, hy = -0x7FFFFFFF - 1, hz = -0x7FFFFFFF - 1;
  if (t < n_in && mark[t] != 0) {
    const TgBox box = tg_box_of<V>(map, tri, t, cell);
    word = tg_mark(box);
    mark[t] = word;
    if (V::kOccupied && word != kTgWide) { lx = box.lo[0]; ly = box.lo[1]; lz = box.lo[2]; hx = box.hi[0]; hy = box.hi[1]; hz = box.hi[2]; }
  }
  const bool wide = word == kTgWide;
  if constexpr (V::kOccupied) {
    if (__ballot(word != 0 && !wide) != 0) {                 // (uniform over the wavefront)
      lx = wave_imin(lx); ly = wave_imin(ly); lz = wave_imin(lz);
      hx = wave_imax(hx); hy = wave_imax(hy); hz = wave_imax(hz);
      if (lane == 0) {
        // the box only grows: a plain read that already holds this wavefront's bound saves the atomic (a stale read costs one)
        int32_t* occ = reinterpret_cast<int32_t*>(cnt);
        const volatile int32_t* seen = occ;
        if (lx < seen[kTgOccLo]) atomicMin(&occ[kTgOccLo], lx);
        if (ly < seen[kTgOccLo + 1]) atomicMin(&occ[kTgOccLo + 1], ly);
        if (lz < seen[kTgOccLo + 2]) atomicMin(&occ[kTgOccLo + 2], lz);
        if (hx > seen[kTgOccHi]) atomicMax(&occ[kTgOccHi], hx);
        if (hy > seen[kTgOccHi + 1]) atomicMax(&occ[kTgOccHi + 1], hy);
        if (hz > seen[kTgOccHi + 2]) atomicMax(&occ[kTgOccHi + 2], hz);
      }
    }
  }
  const unsigned long long m = __ballot(wide);
  if (m != 0) {
    const uint32_t leader = (uint32_t)(__ffsll((long long)m) - 1);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&cnt[kTgNWide], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader);
    if (wide) wide_t[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = t;      // (at most n_in wide triangles in all)
  }
  uint32_t total;
  (void)block_excl_scan(wide ? 0u : word, wave_tot, total);
  if (threadIdx.x == 0) {
    block_sums[blockIdx.x] = total;
    if (total != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + kTgEntries64Lo), (unsigned long long)total);
  }
}

template <class V>
__global__ void __launch_bounds__(kTgBlock)
k_tg_entries(TgMap map, const uint32_t* __restrict__ tri, uint32_t n_in, const uint32_t* __restrict__ mark,
             const uint32_t* __restrict__ block_off, const uint32_t* __restrict__ cnt, uint32_t n_entries,
             unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ uint32_t wave_tot[kTgBlock / 64];
  const uint32_t t = blockIdx.x * kTgBlock + threadIdx.x;
  uint32_t count = t < n_in ? mark[t] : 0u;
  if (count == kTgWide) count = 0;
  uint32_t total;
  const uint32_t off = block_off[blockIdx.x] + block_excl_scan(count, wave_tot, total);
  if (count == 0 || off + count > n_entries) return;         // (the second never holds: off + count <= the scan's total)
  const TgBox box = tg_box_of<V>(map, tri, t, tg_cell_of(cnt));
  for (uint32_t j = 0; j < count; ++j) { keys[off + j] = tg_box_key(box, j); vals[off + j] = t; }
}

// recs[j] = the corners of triangle list[j]
__global__ void __launch_bounds__(kTgBlock)
k_tg_records(TgMap map, const uint32_t* __restrict__ tri, const uint32_t* __restrict__ list, uint32_t m, TgRec* __restrict__ recs) {
  const uint32_t j = blockIdx.x * kTgBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t t = list[j];
  const TgVec a = tg_pos(map, tri[3 * (size_t)t]), b = tg_pos(map, tri[3 * (size_t)t + 1]), c = tg_pos(map, tri[3 * (size_t)t + 2]);
  TgRec r;
  r.a = make_float4(a.x, a.y, a.z, __uint_as_float(t)); r.b = make_float4(b.x, b.y, b.z, 0.0f); r.c = make_float4(c.x, c.y, c.z, 0.0f);
  recs[j] = r;
}

// the table is all zeros before: empty
__global__ void __launch_bounds__(kTgBlock)
k_tg_table(const unsigned long long* __restrict__ keys, uint32_t n_entries, TgCell* table, uint32_t mask, uint32_t* __restrict__ cnt) {
  const uint32_t j = blockIdx.x * kTgBlock + threadIdx.x;
  bool head = false;
  if (j < n_entries) {
    TgDeviceTable tab{table};
    head = tg_table_entry(tab, mask, keys, n_entries, j);
  }
  wave_count(&cnt[kTgCells], head);
}

}  // namespace

int TgWork::reserve_mark(uint32_t n_in) {
  SMX_CALL(mark.reserve(n_in));
  SMX_CALL(blocks.reserve((size_t)div_up(n_in, kTgBlock)));
  SMX_CALL(wide_t.reserve(n_in));
  return SMX_OK;
}

int tg_enqueue_mark(TgWork& w, TgBoxes boxes, const TgMap& map, const uint32_t* din, uint32_t n_in, float cell_size, float least_cell,
                    uint32_t* cnt, hipStream_t st) {
  const int nb = div_up(n_in, kTgBlock);
  const dim3 b(kTgBlock), g_in(nb);
  if (n_in > 0) hipLaunchKernelGGL(k_tg_classify, g_in, b, 0, st, map, din, n_in, w.mark.get(), cnt);
  hipLaunchKernelGGL(k_tg_cell, dim3(1), dim3(64), 0, st, cell_size, least_cell, cnt);
  if (n_in > 0) {
    const auto mark = boxes == TgBoxes::kForRays ? k_tg_mark<Variant<TgBoxes::kForRays>> : k_tg_mark<Variant<TgBoxes::kExact>>;
    hipLaunchKernelGGL(mark, g_in, b, 0, st, map, din, n_in, w.mark.get(), w.wide_t.get(), w.blocks.get(), cnt);
    enqueue_segment_scan(st, w.blocks.get(), nb, cnt + kTgEntries);
  }
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int tg_read_counts(const uint32_t* cnt, uint32_t* h, int n_words, uint32_t n_slots, hipStream_t st, uint32_t* E, uint32_t* Wd) {
  SMX_HIP(hipMemcpyAsync(h, cnt, (size_t)n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (h[kTgError] != 0) {
    set_error("triangles holds an index >= the %u slots of the map", n_slots);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  if (word64(h, kTgEntries64Lo) > (1ull << 30)) {
    set_error("more than 2^30 (cell, triangle) entries: choose a larger cell_size");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  *E = h[kTgEntries]; *Wd = h[kTgNWide];
  return SMX_OK;
}

int tg_enqueue_index(TgWork& w, TgBoxes boxes, const TgMap& map, const uint32_t* din, uint32_t n_in, uint32_t E, uint32_t Wd, uint32_t min_sort,
                     uint32_t* cnt, DevBuf<float>& recs_buf, DevBuf<float>& wide_buf, DevBuf<unsigned long long>& table_buf, uint32_t* mask_out,
                     const unsigned long long** sorted_keys, hipStream_t st, const uint32_t** sorted_vals) {
  const dim3 b(kTgBlock), g_in(div_up(n_in, kTgBlock));
  const uint32_t sort_n = E > min_sort ? E : min_sort;
  const uint32_t entries = dec_table_size(E), mask = entries - 1;
  for (int k = 0; k < 2; ++k) { SMX_CALL(w.keys[k].reserve(sort_n)); SMX_CALL(w.vals[k].reserve(sort_n)); }
  SMX_CALL(w.hist.reserve(radix_sort_workspace_elems(sort_n)));
  SMX_CALL(recs_buf.reserve((size_t)E * 12));
  SMX_CALL(wide_buf.reserve((size_t)Wd * 12));
  SMX_CALL(table_buf.reserve((size_t)2 * entries));
  TgCell* table = reinterpret_cast<TgCell*>(table_buf.get());
  TgRec* recs = reinterpret_cast<TgRec*>(recs_buf.get());
  TgRec* wide_recs = reinterpret_cast<TgRec*>(wide_buf.get());
  *mask_out = mask;
  if (sorted_keys) *sorted_keys = nullptr;
  if (sorted_vals) *sorted_vals = nullptr;
  SMX_HIP(hipMemsetAsync(table, 0, (size_t)entries * sizeof(TgCell), st));
  if (E > 0) {
    const auto fill = boxes == TgBoxes::kForRays ? k_tg_entries<Variant<TgBoxes::kForRays>> : k_tg_entries<Variant<TgBoxes::kExact>>;
    hipLaunchKernelGGL(fill, g_in, b, 0, st, map, din, n_in, w.mark.get(), w.blocks.get(), cnt, E, w.keys[0].get(), w.vals[0].get());
    SMX_LAUNCH_CHECK();
    const int cur = radix_sort(w.keys, w.vals, E, 63, w.hist.get(), st);
    hipLaunchKernelGGL(k_tg_records, dim3(blocks_for(E)), b, 0, st, map, din, w.vals[cur].get(), E, recs);
    hipLaunchKernelGGL(k_tg_table, dim3(blocks_for(E)), b, 0, st, w.keys[cur].get(), E, table, mask, cnt);
    if (sorted_keys) *sorted_keys = w.keys[cur].get();
    if (sorted_vals) *sorted_vals = w.vals[cur].get();
  }
  if (Wd > 0) hipLaunchKernelGGL(k_tg_records, dim3(blocks_for(Wd)), b, 0, st, map, din, w.wide_t.get(), Wd, wide_recs);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

}  // namespace smx
