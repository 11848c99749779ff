// smx_decimate.hip -- the kernels of smx_recon_decimate_mesh (gfx950): vertex clustering of a triangle array over the
// surfel map (the contract is in include/smx.h, its arithmetic in smx_decimate.hpp).
//
//   cluster:  k_dec_mark (a lane per triangle: range check, live test, marks U in vmap) -> k_dec_insert (a lane per slot
//             of U: cell key and value word into an open-addressing table, 64-bit CAS on the key, 64-bit min on the word)
//             -> k_dec_lookup (vmap = the slot in the cell's word)
//   remap:    k_dec_remap (a lane per triangle: corners through vmap, collapse test, canonical triple) -> k_dec_dups (the
//             table of triangle indices: an empty entry is claimed, an entry whose resident has the same corners takes the
//             minimum of the two indices)
//   survive:  k_dec_count -> enqueue_segment_scan (the caller's) -> k_dec_write (no cursor: the list is in input order)
//   order:    two stable radix sorts of smx_nn.hip, by (a, b) and then by p, k_dec_keys_p between them, k_dec_emit after.
//
// Every result is independent of the order in which lanes arrive: a cell's key never changes once claimed and its word
// only decreases towards the minimum over the cell; an entry of the triangle table only ever holds triangles of one corner
// set and decreases towards the earliest of them.  A kernel reads with plain loads only what an EARLIER kernel wrote;
// within a kernel, lanes meet through the atomics' return values alone.
//
// smx_recon_decimate_mesh itself is at the end of the file: it owns the order of the phases, the workspace (DecimateWork,
// smx_decimate.hpp) and the three reads of the counters.
#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

constexpr int kBlock = kDecBlock;

// one atomic per wavefront: the number of its lanes with `pred`
__device__ __forceinline__ void wave_count_add(uint32_t* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m != 0 && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(counter, (uint32_t)__popcll(m));
}

__device__ __forceinline__ bool slot_live(const DecMap& map, uint32_t i) {
  const float4 s = map.smooth[(size_t)i * map.smooth_stride];
  const float rs = map.normal[(size_t)i * map.normal_stride].w;
  return dec_live(s.x, s.y, s.z, rs);
}

__global__ void __launch_bounds__(kBlock)
k_dec_mark(DecMap map, const uint32_t* __restrict__ tri_in, uint32_t n_in, uint32_t* __restrict__ vmap, uint32_t* __restrict__ counters) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  bool not_live = false;
  if (t < n_in) {
    const uint32_t i0 = tri_in[3 * (size_t)t], i1 = tri_in[3 * (size_t)t + 1], i2 = tri_in[3 * (size_t)t + 2];
    if (i0 >= map.n || i1 >= map.n || i2 >= map.n) {
      atomicOr(&counters[kDecError], kDecErrIndex);
    } else if (slot_live(map, i0) && slot_live(map, i1) && slot_live(map, i2)) {
      vmap[i0] = 0; vmap[i1] = 0; vmap[i2] = 0;      // "in U" (any value but kDecNoSlot; k_dec_insert replaces it)
    } else {
      not_live = true;
    }
  }
  wave_count_add(&counters[kDecNotLive], not_live);
}

__global__ void __launch_bounds__(kBlock)
k_dec_insert(DecMap map, float cell_size, float inv, uint32_t* __restrict__ vmap, DecCell* __restrict__ table, uint32_t mask,
             uint32_t* __restrict__ counters) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool used = i < map.n && vmap[i] != kDecNoSlot;
  bool claimed = false;
  if (used) {
    const float4 s = map.smooth[(size_t)i * map.smooth_stride];
    int32_t cx = 0, cy = 0, cz = 0;
    const bool ok = dec_cell_coord(s.x, inv, &cx) && dec_cell_coord(s.y, inv, &cy) && dec_cell_coord(s.z, inv, &cz);
    if (!ok) {
      atomicOr(&counters[kDecError], kDecErrRange);
    } else {
      const unsigned long long key = dec_cell_key(cx, cy, cz);
      const unsigned long long word = dec_value_word(dec_d2(s.x, s.y, s.z, cx, cy, cz, cell_size), i);
      uint32_t h = dec_hash(key, mask);
      // (the table has at least twice as many entries as U has slots: an empty one ends every chain)
      for (;;) {
        const unsigned long long prev = atomicCAS(&table[h].key, kDecEmpty, key);
        if (prev == kDecEmpty) claimed = true;
        if (prev == kDecEmpty || prev == key) break;
        h = (h + 1) & mask;
      }
      atomicMin(&table[h].word, word);
      vmap[i] = h;                                    // (k_dec_lookup replaces it)
    }
  }
  wave_count_add(&counters[kDecUsed], used);
  wave_count_add(&counters[kDecCells], claimed);
}

__global__ void __launch_bounds__(kBlock)
k_dec_lookup(uint32_t n, uint32_t* __restrict__ vmap, const DecCell* __restrict__ table) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t h = vmap[i];
  if (h != kDecNoSlot) vmap[i] = dec_word_slot(table[h].word);
}

__global__ void __launch_bounds__(kBlock)
k_dec_remap(const uint32_t* __restrict__ tri_in, uint32_t n_in, const uint32_t* __restrict__ vmap, DecTri* __restrict__ canon,
            uint32_t* __restrict__ counters) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  bool collapsed = false, alive = false;
  if (t < n_in) {
    const uint32_t r0 = vmap[tri_in[3 * (size_t)t]], r1 = vmap[tri_in[3 * (size_t)t + 1]], r2 = vmap[tri_in[3 * (size_t)t + 2]];
    DecTri c{kDecNoSlot, kDecNoSlot, kDecNoSlot};
    // (a live corner of a dropped triangle may be in U through another triangle: all three decide)
    if (r0 != kDecNoSlot && r1 != kDecNoSlot && r2 != kDecNoSlot) {
      collapsed = dec_collapsed(r0, r1, r2);
      alive = !collapsed;
      if (alive) c = dec_canonical(r0, r1, r2);
    }
    canon[t] = c;
  }
  wave_count_add(&counters[kDecCollapsed], collapsed);
  wave_count_add(&counters[kDecAlive], alive);
}

__global__ void __launch_bounds__(kBlock)
k_dec_dups(uint32_t n_in, const DecTri* __restrict__ canon, uint32_t* __restrict__ own, uint32_t* __restrict__ table, uint32_t mask) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_in) return;
  const DecTri c = canon[t];
  uint32_t h = kDecNoSlot;
  if (c.p != kDecNoSlot) {
    h = dec_tri_hash(c, mask);
    for (;;) {
      const uint32_t prev = atomicCAS(&table[h], kDecNoSlot, t);
      if (prev == kDecNoSlot) break;
      // (whoever holds the entry has this entry's corner set, now and later: its triple was written by k_dec_remap)
      if (dec_same_corners(canon[prev], c)) { if (t < prev) atomicMin(&table[h], t); break; }
      h = (h + 1) & mask;
    }
  }
  own[t] = h;
}

__device__ __forceinline__ bool survives(uint32_t t, uint32_t n_in, const uint32_t* __restrict__ own, const uint32_t* __restrict__ table) {
  if (t >= n_in) return false;
  const uint32_t h = own[t];
  return h != kDecNoSlot && table[h] == t;
}

__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* wave_tot /* LDS [kBlock / 64] */, uint32_t* total) {
  const unsigned long long m = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) { if ((uint32_t)w < wave) off += wave_tot[w]; tot += wave_tot[w]; }
  *total = tot;
  return off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(kBlock)
k_dec_count(uint32_t n_in, const uint32_t* __restrict__ own, const uint32_t* __restrict__ table, uint32_t* __restrict__ block_sums) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  uint32_t total;
  (void)block_rank(survives(blockIdx.x * kBlock + threadIdx.x, n_in, own, table), wave_tot, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock)
k_dec_write(uint32_t n_in, const uint32_t* __restrict__ own, const uint32_t* __restrict__ table, const uint32_t* __restrict__ block_off,
            const DecTri* __restrict__ canon, int bits, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  const bool s = survives(t, n_in, own, table);
  uint32_t total;
  const uint32_t j = block_off[blockIdx.x] + block_rank(s, wave_tot, &total);
  if (s) { keys[j] = dec_key_ab(canon[t], bits); vals[j] = t; }
}

__global__ void __launch_bounds__(kBlock)
k_dec_keys_p(uint32_t m, const uint32_t* vals_in, const DecTri* __restrict__ canon, unsigned long long* __restrict__ keys_out,
             uint32_t* vals_out) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t t = vals_in[j];      // (vals_out may be vals_in: each lane reads its entry before it writes it)
  keys_out[j] = canon[t].p;
  vals_out[j] = t;
}

__global__ void __launch_bounds__(kBlock)
k_dec_emit(uint32_t m, const uint32_t* __restrict__ vals, const DecTri* __restrict__ canon, uint32_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  const DecTri c = canon[vals[j]];
  out[3 * (size_t)j] = c.p; out[3 * (size_t)j + 1] = c.a; out[3 * (size_t)j + 2] = c.b;
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_recon_decimate_mesh(smx_recon r, smx_stream s, float cell_size, const uint32_t* triangles_in, uint32_t n_in,
                            uint32_t* triangles_out, uint32_t capacity, uint32_t* vertex_map, int32_t on_device,
                            uint32_t* n_triangles, smx_decimate_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && n_triangles != nullptr);
  SMX_CHECK_ARG(cell_size > 0.0f && cell_size - cell_size == 0.0f);
  SMX_CHECK_ARG(triangles_in != nullptr || n_in == 0);
  SMX_CHECK_ARG(triangles_out != nullptr || capacity == 0);
  if (n_in > 0 && capacity > 0) {
    const uintptr_t i0 = (uintptr_t)triangles_in, i1 = i0 + (size_t)n_in * 12, o0 = (uintptr_t)triangles_out, o1 = o0 + (size_t)capacity * 12;
    if (i0 < o1 && o0 < i1) {
      set_error("triangles_out overlaps triangles_in");
      return SMX_ERR_INVALID_ARGUMENT;
    }
  }
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  *n_triangles = 0;
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; }
  DecimateWork& w = r->decimate;
  SMX_CALL(w.stamps.begin(st));
  // Every way out below that has marked a phase goes through finish: it publishes exactly the phases marked so far, which
  // is what a refused call's getter returns (1 after a bad index or range, 2 after the capacity rule, 4 after a full call).
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    w.stamps.publish();
    return rc;
  };

  // ---- workspace of the first two phases; the input on the device
  const uint32_t cell_entries = dec_table_size((uint32_t)std::min<unsigned long long>(n, 3ull * n_in));
  const uint32_t dup_entries = dec_table_size(n_in);
  const int nb = div_up(n_in, kDecBlock);
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kDecWords, false));
  SMX_CALL(w.vmap.reserve(n));
  if (n_in > 0) {
    SMX_CALL(w.cells.reserve((size_t)2 * cell_entries));
    SMX_CALL(w.canon.reserve((size_t)3 * n_in));
    SMX_CALL(w.own.reserve(n_in));
    SMX_CALL(w.dup.reserve(dup_entries));
    SMX_CALL(w.blocks.reserve((size_t)nb));
  }
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(w.in, triangles_in, (size_t)3 * n_in, on_device != 0, st, &din));
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kDecWords * sizeof(uint32_t), st));
  uint32_t h[kDecWords];
  auto read_counters = [&]() -> int {
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    return SMX_OK;
  };

  // ---- clustering: U, the cell table, the vertex map.  (An index out of range marks nothing and is read by nothing.)
  const float inv = 1.0f / cell_size;
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const DecMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  DecCell* cells = reinterpret_cast<DecCell*>(w.cells.get());   // (dec_table_size(min(n, 3 n_in)) entries)
  DecTri* canon = reinterpret_cast<DecTri*>(w.canon.get());
  uint32_t* vmap = w.vmap.get();                                // (ends as the contract's vertex_map)
  const dim3 b(kDecBlock), g_in(nb), g_map(blocks_for(n));
  if (n > 0) SMX_HIP(hipMemsetAsync(vmap, 0xFF, (size_t)n * sizeof(uint32_t), st));
  if (n_in > 0) {
    hipLaunchKernelGGL(k_dec_mark, g_in, b, 0, st, map, din, n_in, vmap, cnt);
    if (n > 0) {      // (an empty map: every index is out of range, which k_dec_mark has just said)
      SMX_HIP(hipMemsetAsync(cells, 0xFF, (size_t)cell_entries * sizeof(DecCell), st));
      hipLaunchKernelGGL(k_dec_insert, g_map, b, 0, st, map, cell_size, inv, vmap, cells, cell_entries - 1, cnt);
      hipLaunchKernelGGL(k_dec_lookup, g_map, b, 0, st, n, vmap, cells);
    }
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));
  SMX_CALL(read_counters());
  if (h[kDecError] & kDecErrIndex) {
    set_error("triangles_in holds an index >= the %u slots of the map", n);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  if (h[kDecError] & kDecErrRange) {
    set_error("cell_size %g is too small for the extent of the map: a cell coordinate is outside [-2^20, 2^20)", (double)cell_size);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }

  // ---- remap and duplicates: canon gets the canonical triples (p = kDecNoSlot: dropped), own each triangle's entry of the
  // table dup, which ends holding the earliest triangle of each corner set; survivors counted and scanned
  if (n_in > 0) {
    SMX_HIP(hipMemsetAsync(w.dup.get(), 0xFF, (size_t)dup_entries * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_dec_remap, g_in, b, 0, st, din, n_in, vmap, canon, cnt);
    hipLaunchKernelGGL(k_dec_dups, g_in, b, 0, st, n_in, canon, w.own.get(), w.dup.get(), dup_entries - 1);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));
  if (n_in > 0) {
    hipLaunchKernelGGL(k_dec_count, g_in, b, 0, st, n_in, w.own.get(), w.dup.get(), w.blocks.get());
    enqueue_segment_scan(st, w.blocks.get(), nb, cnt + kDecTotal);   // (survivors per workgroup -> their offsets, and the total)
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(read_counters());
  const uint32_t T = h[kDecTotal];
  *n_triangles = T;
  if (stats) {
    stats->n_not_live = h[kDecNotLive]; stats->n_used_vertices = h[kDecUsed]; stats->n_cells = h[kDecCells];
    stats->n_collapsed = h[kDecCollapsed]; stats->n_duplicates = h[kDecAlive] - T; stats->n_triangles = T;
  }
  if (capacity < T) {
    if (triangles_out != nullptr || capacity != 0) set_error("triangles_out holds %u entries, the decimated mesh has %u", capacity, T);
    else set_error("count only: the decimated mesh has %u triangles", T);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }

  // ---- the survivors in input order as sort records, ordered by (a, b) and then, stably, by p
  if (T > 0) {
    int bits = 1;
    while (bits < 32 && ((uint32_t)(n - 1) >> bits) != 0) ++bits;
    for (int k = 0; k < 2; ++k) { SMX_CALL(w.keys[k].reserve(T)); SMX_CALL(w.vals[k].reserve(T)); }
    SMX_CALL(w.hist.reserve(radix_sort_workspace_elems(T)));
    const dim3 gt(blocks_for(T));
    // (keys[j] = (a << bits) | b, vals[j] = the triangle's index in canon)
    hipLaunchKernelGGL(k_dec_write, g_in, b, 0, st, n_in, w.own.get(), w.dup.get(), w.blocks.get(), canon, bits, w.keys[0].get(),
                       w.vals[0].get());
    SMX_LAUNCH_CHECK();
    SMX_CALL(w.stamps.mark(st));
    int cur = radix_sort(w.keys, w.vals, T, 2 * bits, w.hist.get(), st);
    // (between the two stable sorts: keys[j] = p of triangle vals[j]; after them out[j] = canon[vals[j]])
    hipLaunchKernelGGL(k_dec_keys_p, gt, b, 0, st, T, w.vals[cur].get(), canon, w.keys[0].get(), w.vals[0].get());
    cur = radix_sort(w.keys, w.vals, T, bits, w.hist.get(), st);
    SMX_LAUNCH_CHECK();
    uint32_t* dst = triangles_out;
    if (!on_device) {
      SMX_CALL(w.out.reserve((size_t)3 * T));
      dst = w.out.get();
    }
    hipLaunchKernelGGL(k_dec_emit, gt, b, 0, st, T, w.vals[cur].get(), canon, dst);
    SMX_LAUNCH_CHECK();
    if (!on_device) SMX_HIP(hipMemcpyAsync(triangles_out, dst, (size_t)T * 12, hipMemcpyDeviceToHost, st));
  } else {
    SMX_CALL(w.stamps.mark(st));
  }
  if (vertex_map && n > 0)
    SMX_HIP(hipMemcpyAsync(vertex_map, vmap, (size_t)n * sizeof(uint32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  SMX_CALL(w.stamps.mark(st));
  return finish(SMX_OK);
}

int smx_recon_debug_decimate_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_DECIMATE_PHASES);
  SMX_ON_DEVICE(r->device);
  return r->decimate.stamps.elapsed_ms(out_ms, SMX_DECIMATE_PHASES);
}

}  // extern "C"
