// smx_components.hip -- the kernels of smx_recon_mesh_components (gfx950): connected components of a triangle array over the
// surfel map, their measures, and the array without the small ones (the contract is in include/smx.h, its
// arithmetic and the union-find in smx_components.hpp).
//
//   mark + link:       k_cc_mark (a lane per triangle: range check, live test, parent[corner] = corner, tcomp = remaining or
//                      not) -> k_cc_link (a lane per remaining triangle: unite (p, a) and (p, b); ONE launch)
//   flatten + number:  k_cc_flatten (a lane per slot: label = find, roots counted per workgroup) -> enqueue_segment_scan (the
//                      caller's) -> k_cc_number (parent[root] = its dense number: roots ascending)
//   measure:           k_cc_measure_vertices / _triangles (counts and box keys into the dense accumulators, aggregated within
//                      the wavefront and along its run of chunks first) -> k_cc_pass (a lane per component: box, diag2,
//                      pass bit, rank record) -> with keep_largest the radix sort of smx_nn.hip and k_cc_rank
//   write:             k_cc_count -> enqueue_segment_scan -> k_cc_write (no cursor: the output is in input order)
//
// Why the result does not depend on the schedule: parent[x] <= x throughout (the invariants are listed at cc_find), so the
// root a component ends with is its smallest slot; counts are integer sums and the box is a minimum / maximum of integer
// keys.  Within k_cc_link and k_cc_flatten every access to parent is an agent-scope atomic; every other kernel reads with
// plain loads only what an EARLIER kernel wrote.
//
// smx_recon_mesh_components itself is at the end of the file: it owns the order of the phases, the workspace
// (ComponentsWork, smx_components.hpp) and the two reads of the counters.
#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

constexpr int kBlock = kCcBlock;

// parent[] as the union-find sees it on the device: relaxed agent-scope atomics, nothing cached in a register
struct CcDeviceWords {
  uint32_t* parent;
  __device__ __forceinline__ uint32_t load(uint32_t i) const {
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t expected, uint32_t desired) const {
    return atomicCAS(parent + i, expected, desired);
  }
  __device__ __forceinline__ void min(uint32_t i, uint32_t v) const { atomicMin(parent + i, v); }
};

// one atomic per wavefront: the number of its lanes with `pred`
__device__ __forceinline__ void wave_count_add(uint32_t* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m != 0 && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(counter, (uint32_t)__popcll(m));
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
  return v;
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

__device__ __forceinline__ bool slot_live(const CcMap& map, uint32_t i) {
  const float4 s = map.smooth[(size_t)i * map.smooth_stride];
  const float rs = map.normal[(size_t)i * map.normal_stride].w;
  return cc_live(s.x, s.y, s.z, rs);
}

// parent is all ones before: the corners of the remaining triangles become roots (every writer of a word writes the same value)
__global__ void __launch_bounds__(kBlock)
k_cc_mark(CcMap map, const uint32_t* __restrict__ tri_in, uint32_t n_in, uint32_t* __restrict__ parent, uint32_t* __restrict__ tcomp,
          uint32_t* __restrict__ counters) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  bool not_live = false;
  if (t < n_in) {
    const uint32_t i0 = tri_in[3 * (size_t)t], i1 = tri_in[3 * (size_t)t + 1], i2 = tri_in[3 * (size_t)t + 2];
    uint32_t remaining = kCcNoSlot;
    if (i0 >= map.n || i1 >= map.n || i2 >= map.n) {
      atomicOr(&counters[kCcError], 1u);
    } else if (slot_live(map, i0) && slot_live(map, i1) && slot_live(map, i2)) {
      parent[i0] = i0; parent[i1] = i1; parent[i2] = i2;
      remaining = 0;
    } else {
      not_live = true;
    }
    tcomp[t] = remaining;
  }
  wave_count_add(&counters[kCcNotLive], not_live);
}

// (a triangle k_cc_mark has let through has three indices in range whose words are roots or below)
__global__ void __launch_bounds__(kBlock)
k_cc_link(const uint32_t* __restrict__ tri_in, uint32_t n_in, const uint32_t* __restrict__ tcomp, uint32_t* parent) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_in || tcomp[t] == kCcNoSlot) return;
  const uint32_t p = tri_in[3 * (size_t)t], a = tri_in[3 * (size_t)t + 1], b = tri_in[3 * (size_t)t + 2];
  CcDeviceWords m{parent};
  cc_unite(m, p, a);
  cc_unite(m, p, b);
}

__global__ void __launch_bounds__(kBlock)
k_cc_flatten(uint32_t n, uint32_t* parent, uint32_t* __restrict__ label, uint32_t* __restrict__ block_sums, uint32_t* __restrict__ counters) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  CcDeviceWords m{parent};
  uint32_t l = kCcNoSlot;
  if (i < n && m.load(i) != kCcNoSlot) l = cc_find(m, i);   // (halving goes on beside the other lanes' finds: still only ancestors)
  if (i < n) label[i] = l;
  uint32_t total;
  (void)block_rank(l == i && i < n, wave_tot, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
  wave_count_add(&counters[kCcUsed], l != kCcNoSlot);
}

// parent[root] = the root's rank among the roots: the dense number of its component, ascending by label
__global__ void __launch_bounds__(kBlock)
k_cc_number(uint32_t n, const uint32_t* __restrict__ label, const uint32_t* __restrict__ block_off, uint32_t* __restrict__ parent) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool root = i < n && label[i] == i;
  uint32_t total;
  const uint32_t d = block_off[blockIdx.x] + block_rank(root, wave_tot, &total);
  if (root) parent[i] = d;
}

// A value of lane `leader` (wave-uniform) or, with `many`, the maximum over the wavefront: the same word in every lane.
__device__ __forceinline__ uint32_t wave_pick_max(uint32_t v, bool many, int leader) {
  return many ? wave_max(v) : (uint32_t)__builtin_amdgcn_readlane((int)v, leader);
}

// Counts and box keys of the used slots into acc (zeroed before; lo is kept as ~key, so that zero is the identity of both
// maxima).  The usual mesh is one component holding nearly everything, and atomics on one 32-byte row retire one after the
// other: one set per lane would be millions of them in a single queue.  So (a) the lanes of a wavefront that share the first
// remaining lane's component reduce among themselves -- one or two trips on a sorted array, at most 64 -- and (b) a
// wavefront measures kCcRun chunks of 64 slots in a row and keeps the aggregate of the component it is in (wave-uniform
// registers) until the component changes: the seven atomics are issued once per run of one component, not once per chunk.
constexpr int kCcRun = 16;
constexpr uint32_t kCcSlotsPerBlock = kBlock * kCcRun;

__global__ void __launch_bounds__(kBlock)
k_cc_measure_vertices(CcMap map, const uint32_t* __restrict__ label, const uint32_t* __restrict__ dense, CcAcc* __restrict__ acc,
                      smx_mesh_component* __restrict__ table) {
  const uint32_t lane = threadIdx.x & 63;
  const size_t base = ((size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * (64 * kCcRun) + lane;
  uint32_t pc = kCcNoSlot, pn = 0, pnlo[3] = {0, 0, 0}, phi[3] = {0, 0, 0};      // the pending aggregate: the same in every lane
  auto flush = [&]() {
    if (pc != kCcNoSlot && lane == 0) {
      CcAcc* a = acc + pc;
      atomicAdd(&a->n_vertices, pn);
#pragma unroll
      for (int q = 0; q < 3; ++q) { atomicMax(&a->lo[q], pnlo[q]); atomicMax(&a->hi[q], phi[q]); }
    }
  };
  for (int j = 0; j < kCcRun; ++j) {
    const size_t i = base + (size_t)j * 64;
    const uint32_t l = i < map.n ? label[i] : kCcNoSlot;
    const bool active = l != kCcNoSlot;
    uint32_t c = 0, k[3] = {0, 0, 0};
    if (active) {
      c = dense[l];
      const float4 s = map.smooth[i * map.smooth_stride];
      k[0] = cc_key(s.x); k[1] = cc_key(s.y); k[2] = cc_key(s.z);
      if (l == (uint32_t)i) table[c].label = l;
    }
    unsigned long long rem = __ballot(active);
    while (rem != 0) {
      const int leader = __ffsll((long long)rem) - 1;
      const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)c, leader);
      const bool mine = active && c == c0;
      const unsigned long long m = __ballot(mine);
      const bool many = (m & (m - 1)) != 0;
      if (c0 != pc) {
        flush();
        pc = c0; pn = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) { pnlo[q] = 0; phi[q] = 0; }
      }
      pn += (uint32_t)__popcll(m);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        pnlo[q] = max(pnlo[q], wave_pick_max(mine ? ~k[q] : 0u, many, leader));
        phi[q] = max(phi[q], wave_pick_max(mine ? k[q] : 0u, many, leader));
      }
      rem &= ~m;
    }
  }
  flush();
}

// tcomp = the dense component of every remaining triangle, and the triangle counts (aggregated as above)
__global__ void __launch_bounds__(kBlock)
k_cc_measure_triangles(const uint32_t* __restrict__ tri_in, uint32_t n_in, const uint32_t* __restrict__ label,
                       const uint32_t* __restrict__ dense, uint32_t* __restrict__ tcomp, CcAcc* __restrict__ acc) {
  const uint32_t lane = threadIdx.x & 63;
  const size_t base = ((size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * (64 * kCcRun) + lane;
  uint32_t pc = kCcNoSlot, pn = 0;
  for (int j = 0; j < kCcRun; ++j) {
    const size_t t = base + (size_t)j * 64;
    const bool active = t < n_in && tcomp[t] != kCcNoSlot;
    uint32_t c = 0;
    if (active) {
      c = dense[label[tri_in[3 * t]]];
      tcomp[t] = c;
    }
    unsigned long long rem = __ballot(active);
    while (rem != 0) {
      const int leader = __ffsll((long long)rem) - 1;
      const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)c, leader);
      const unsigned long long m = __ballot(active && c == c0);
      if (c0 != pc) {
        if (pc != kCcNoSlot && lane == 0) atomicAdd(&acc[pc].n_triangles, pn);
        pc = c0; pn = 0;
      }
      pn += (uint32_t)__popcll(m);
      rem &= ~m;
    }
  }
  if (pc != kCcNoSlot && lane == 0) atomicAdd(&acc[pc].n_triangles, pn);
}

__global__ void __launch_bounds__(kBlock)
k_cc_pass(uint32_t n_components, const CcAcc* __restrict__ acc, smx_components_params p, smx_mesh_component* __restrict__ table,
          unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ counters) {
  const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
  bool pass = false;
  uint32_t nt = 0;
  if (d < n_components) {
    const CcAcc a = acc[d];
    smx_mesh_component row;
    row.label = table[d].label;
    row.n_vertices = a.n_vertices; row.n_triangles = nt = a.n_triangles;
#pragma unroll
    for (int q = 0; q < 3; ++q) { row.lo[q] = cc_unkey(~a.lo[q]); row.hi[q] = cc_unkey(a.hi[q]); }
    pass = cc_passes(nt, cc_diag2(row.lo, row.hi), p.min_triangles, p.min_diagonal);
    row.kept = pass ? 1u : 0u;
    table[d] = row;
    if (p.keep_largest > 0) {       // (k_cc_rank decides kept and counts)
      keys[d] = pass ? cc_rank_record(nt, row.label) : kCcNoRecord;
      vals[d] = d;
    }
  }
  const uint32_t most = wave_max(nt);
  if ((threadIdx.x & 63) == 0 && most > 0) atomicMax(&counters[kCcLargest], most);
  if (p.keep_largest == 0) wave_count_add(&counters[kCcKept], pass);
}

// the records in rank order: the first keep_largest of those that pass stay
__global__ void __launch_bounds__(kBlock)
k_cc_rank(uint32_t n_components, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t keep_largest,
          smx_mesh_component* __restrict__ table, uint32_t* __restrict__ counters) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  bool kept = false;
  if (j < n_components) {
    kept = j < keep_largest && keys[j] != kCcNoRecord;
    table[vals[j]].kept = kept ? 1u : 0u;
  }
  wave_count_add(&counters[kCcKept], kept);
}

__device__ __forceinline__ bool survives(uint32_t t, uint32_t n_in, const uint32_t* __restrict__ tcomp,
                                         const smx_mesh_component* __restrict__ table) {
  if (t >= n_in) return false;
  const uint32_t c = tcomp[t];
  return c != kCcNoSlot && table[c].kept != 0;
}

__global__ void __launch_bounds__(kBlock)
k_cc_count(uint32_t n_in, const uint32_t* __restrict__ tcomp, const smx_mesh_component* __restrict__ table, uint32_t* __restrict__ block_sums) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  uint32_t total;
  (void)block_rank(survives(blockIdx.x * kBlock + threadIdx.x, n_in, tcomp, table), wave_tot, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock)
k_cc_write(const uint32_t* __restrict__ tri_in, uint32_t n_in, const uint32_t* __restrict__ tcomp, const smx_mesh_component* __restrict__ table,
           const uint32_t* __restrict__ block_off, uint32_t* __restrict__ out) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  const bool s = survives(t, n_in, tcomp, table);
  uint32_t total;
  const size_t j = block_off[blockIdx.x] + block_rank(s, wave_tot, &total);
  if (s) {
    out[3 * j] = tri_in[3 * (size_t)t]; out[3 * j + 1] = tri_in[3 * (size_t)t + 1]; out[3 * j + 2] = tri_in[3 * (size_t)t + 2];
  }
}

}  // namespace
}  // namespace smx

using namespace smx;

extern "C" {

int smx_components_params_default(smx_components_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->min_triangles = 0; out->min_diagonal = 0.0f; out->keep_largest = 0;
  return SMX_OK;
}

int smx_recon_mesh_components(smx_recon r, smx_stream s, const smx_components_params* p, const uint32_t* triangles_in, uint32_t n_in,
                              uint32_t* triangles_out, uint32_t capacity, uint32_t* vertex_labels, smx_mesh_component* components,
                              uint32_t component_capacity, int32_t on_device, uint32_t* n_triangles, uint32_t* n_components,
                              smx_components_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && p != nullptr && n_triangles != nullptr && n_components != nullptr);
  SMX_CHECK_ARG(p->min_diagonal >= 0.0f && p->min_diagonal - p->min_diagonal == 0.0f);
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
  *n_triangles = 0; *n_components = 0;
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; }
  ComponentsWork& w = r->components;
  SMX_CALL(w.stamps.begin(st));
  // Every way out below that has marked a phase goes through finish: it publishes exactly the phases marked so far (2 after
  // a bad index, 3 after the capacity rule, 4 after a full call).
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    w.stamps.publish();
    return rc;
  };

  // ---- workspace of the first two phases; the input on the device
  const int nb = div_up(n_in, kCcBlock), nbv = div_up(n, kCcBlock);
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kCcWords, false));
  SMX_CALL(w.parent.reserve(n));
  SMX_CALL(w.label.reserve(n));
  SMX_CALL(w.tcomp.reserve(n_in));
  SMX_CALL(w.blocks.reserve((size_t)std::max(nb, nbv)));
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(w.in, triangles_in, (size_t)3 * n_in, on_device != 0, st, &din));
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kCcWords * sizeof(uint32_t), st));
  uint32_t h[kCcWords];
  auto read_counters = [&]() -> int {
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    return SMX_OK;
  };

  // ---- mark and link.  (An index out of range marks nothing, and its triangle is linked by nobody.)
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const CcMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  uint32_t* parent = w.parent.get();
  uint32_t* label = w.label.get();
  uint32_t* tcomp = w.tcomp.get();
  const dim3 b(kCcBlock), g_in(nb), g_map(nbv);
  if (n > 0) SMX_HIP(hipMemsetAsync(parent, 0xFF, (size_t)n * sizeof(uint32_t), st));
  if (n_in > 0) {
    hipLaunchKernelGGL(k_cc_mark, g_in, b, 0, st, map, din, n_in, parent, tcomp, cnt);
    hipLaunchKernelGGL(k_cc_link, g_in, b, 0, st, din, n_in, tcomp, parent);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- flatten and number: label (the contract's vertex_labels), then parent[root] = the component's dense number
  if (n > 0) {
    hipLaunchKernelGGL(k_cc_flatten, g_map, b, 0, st, n, parent, label, w.blocks.get(), cnt);
    enqueue_segment_scan(st, w.blocks.get(), nbv, cnt + kCcComponents);
    hipLaunchKernelGGL(k_cc_number, g_map, b, 0, st, n, label, w.blocks.get(), parent);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));
  SMX_CALL(read_counters());
  if (h[kCcError] != 0) {
    set_error("triangles_in holds an index >= the %u slots of the map", n);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  const uint32_t C = h[kCcComponents];
  *n_components = C;

  // ---- measure: the accumulators, the table (box, diag2, pass), the ranking
  SMX_CALL(w.acc.reserve((size_t)C * (sizeof(CcAcc) / sizeof(uint32_t))));
  SMX_CALL(w.table.reserve((size_t)C * (sizeof(smx_mesh_component) / sizeof(uint32_t))));
  CcAcc* acc = reinterpret_cast<CcAcc*>(w.acc.get());
  smx_mesh_component* table = reinterpret_cast<smx_mesh_component*>(w.table.get());
  if (C > 0) {
    const dim3 gc(blocks_for(C));
    if (p->keep_largest > 0) {
      for (int k = 0; k < 2; ++k) { SMX_CALL(w.keys[k].reserve(C)); SMX_CALL(w.vals[k].reserve(C)); }
      SMX_CALL(w.hist.reserve(radix_sort_workspace_elems(C)));
    }
    SMX_HIP(hipMemsetAsync(acc, 0, (size_t)C * sizeof(CcAcc), st));
    hipLaunchKernelGGL(k_cc_measure_vertices, dim3(div_up(n, kCcSlotsPerBlock)), b, 0, st, map, label, parent, acc, table);
    hipLaunchKernelGGL(k_cc_measure_triangles, dim3(div_up(n_in, kCcSlotsPerBlock)), b, 0, st, din, n_in, label, parent, tcomp, acc);
    hipLaunchKernelGGL(k_cc_pass, gc, b, 0, st, C, acc, *p, table, w.keys[0].get(), w.vals[0].get(), cnt);
    SMX_LAUNCH_CHECK();
    if (p->keep_largest > 0) {
      const int cur = radix_sort(w.keys, w.vals, C, 64, w.hist.get(), st);
      hipLaunchKernelGGL(k_cc_rank, gc, b, 0, st, C, w.keys[cur].get(), w.vals[cur].get(), p->keep_largest, table, cnt);
      SMX_LAUNCH_CHECK();
    }
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- write: survivors counted and scanned, then everything the caller asked for
  if (n_in > 0 && C > 0) {
    hipLaunchKernelGGL(k_cc_count, g_in, b, 0, st, n_in, tcomp, table, w.blocks.get());
    enqueue_segment_scan(st, w.blocks.get(), nb, cnt + kCcTotal);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(read_counters());
  const uint32_t T = h[kCcTotal];
  *n_triangles = T;
  if (stats) {
    stats->n_not_live = h[kCcNotLive]; stats->n_used_vertices = h[kCcUsed]; stats->n_components = C;
    stats->n_kept_components = h[kCcKept]; stats->n_largest_triangles = h[kCcLargest]; stats->n_triangles = T;
  }
  if (capacity < T) {
    if (triangles_out != nullptr || capacity != 0) set_error("triangles_out holds %u entries, the kept components have %u triangles", capacity, T);
    else set_error("count only: the kept components have %u triangles in %u components", T, C);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  if (components != nullptr && component_capacity < C) {
    set_error("components holds %u entries, the mesh has %u components", component_capacity, C);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  uint32_t* dst = triangles_out;
  if (T > 0 && !on_device) {      // (the last allocation of the call: nothing has been written to the caller's arrays yet)
    SMX_CALL(w.out.reserve((size_t)3 * T));
    dst = w.out.get();
  }
  const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (T > 0) {
    hipLaunchKernelGGL(k_cc_write, g_in, b, 0, st, din, n_in, tcomp, table, w.blocks.get(), dst);
    SMX_LAUNCH_CHECK();
    if (!on_device) SMX_HIP(hipMemcpyAsync(triangles_out, dst, (size_t)T * 12, hipMemcpyDeviceToHost, st));
  }
  if (vertex_labels && n > 0) SMX_HIP(hipMemcpyAsync(vertex_labels, label, (size_t)n * sizeof(uint32_t), back, st));
  if (components && C > 0) SMX_HIP(hipMemcpyAsync(components, table, (size_t)C * sizeof(smx_mesh_component), back, st));
  SMX_CALL(w.stamps.mark(st));
  return finish(SMX_OK);
}

int smx_recon_debug_components_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_COMPONENTS_PHASES);
  SMX_ON_DEVICE(r->device);
  return r->components.stamps.elapsed_ms(out_ms, SMX_COMPONENTS_PHASES);
}

}  // extern "C"
