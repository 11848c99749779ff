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
#include "smx_decimate.hpp"

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

inline unsigned blocks_for(uint32_t n) { return (unsigned)div_up(n, kBlock); }

}  // namespace

int dec_enqueue_cluster(hipStream_t st, const DecMap& map, const uint32_t* tri_in, uint32_t n_in, float cell_size, float inv,
                        uint32_t* vmap, DecCell* table, uint32_t table_size, uint32_t* counters) {
  if (map.n > 0) SMX_HIP(hipMemsetAsync(vmap, 0xFF, (size_t)map.n * sizeof(uint32_t), st));
  if (n_in == 0) return SMX_OK;
  hipLaunchKernelGGL(k_dec_mark, dim3(blocks_for(n_in)), dim3(kBlock), 0, st, map, tri_in, n_in, vmap, counters);
  if (map.n > 0) {      // (an empty map: every index is out of range, which k_dec_mark has just said)
    SMX_HIP(hipMemsetAsync(table, 0xFF, (size_t)table_size * sizeof(DecCell), st));
    hipLaunchKernelGGL(k_dec_insert, dim3(blocks_for(map.n)), dim3(kBlock), 0, st, map, cell_size, inv, vmap, table, table_size - 1, counters);
    hipLaunchKernelGGL(k_dec_lookup, dim3(blocks_for(map.n)), dim3(kBlock), 0, st, map.n, vmap, table);
  }
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int dec_enqueue_remap(hipStream_t st, const uint32_t* tri_in, uint32_t n_in, const uint32_t* vmap, DecTri* canon, uint32_t* own,
                      uint32_t* dup_table, uint32_t table_size, uint32_t* counters) {
  if (n_in == 0) return SMX_OK;
  SMX_HIP(hipMemsetAsync(dup_table, 0xFF, (size_t)table_size * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_dec_remap, dim3(blocks_for(n_in)), dim3(kBlock), 0, st, tri_in, n_in, vmap, canon, counters);
  hipLaunchKernelGGL(k_dec_dups, dim3(blocks_for(n_in)), dim3(kBlock), 0, st, n_in, canon, own, dup_table, table_size - 1);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int dec_enqueue_count(hipStream_t st, uint32_t n_in, const uint32_t* own, const uint32_t* dup_table, uint32_t* block_sums) {
  if (n_in == 0) return SMX_OK;
  hipLaunchKernelGGL(k_dec_count, dim3(blocks_for(n_in)), dim3(kBlock), 0, st, n_in, own, dup_table, block_sums);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int dec_enqueue_write(hipStream_t st, uint32_t n_in, const uint32_t* own, const uint32_t* dup_table, const uint32_t* block_off,
                      const DecTri* canon, int bits, unsigned long long* keys, uint32_t* vals) {
  if (n_in == 0) return SMX_OK;
  hipLaunchKernelGGL(k_dec_write, dim3(blocks_for(n_in)), dim3(kBlock), 0, st, n_in, own, dup_table, block_off, canon, bits, keys, vals);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int dec_enqueue_keys_p(hipStream_t st, uint32_t m, const uint32_t* vals_in, const DecTri* canon, unsigned long long* keys_out,
                       uint32_t* vals_out) {
  if (m == 0) return SMX_OK;
  hipLaunchKernelGGL(k_dec_keys_p, dim3(blocks_for(m)), dim3(kBlock), 0, st, m, vals_in, canon, keys_out, vals_out);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int dec_enqueue_emit(hipStream_t st, uint32_t m, const uint32_t* vals, const DecTri* canon, uint32_t* out) {
  if (m == 0) return SMX_OK;
  hipLaunchKernelGGL(k_dec_emit, dim3(blocks_for(m)), dim3(kBlock), 0, st, m, vals, canon, out);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

}  // namespace smx
