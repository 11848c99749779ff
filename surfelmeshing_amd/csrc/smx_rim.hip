// smx_rim.hip -- the kernels of smx_recon_mesh_rim (gfx950): per triangle of an array over the surfel map one byte that says
// which of its corners and edges lie on the boundary of the surface (the contract is in include/smx.h, its
// integer rules in smx_rim.hpp, the edge table in smx_fill.hpp).
//
//   edges:     k_rim_edges (a lane per triangle: range check, the classes of smx_recon_mesh_distance's step 1, three inserts
//              into the edge table, the pairs counted by who claimed their entry)
//   vertices:  k_rim_vertices (a lane per triangle of R: the three counts, the edge bits, the slots that end a rim edge ored
//              into the bitmap, one atomic per word a wavefront touches; rim edges, rim vertices and non-manifold pairs counted)
//   bytes:     k_rim_bytes (a lane per triangle of R: the corners' bits from the bitmap beside the edge bits)
//
// Why the result does not depend on the schedule: the counters of a pair are integer sums; the bitmap is an or of bits; a
// pair is counted by the lane that claimed its entry, a rim vertex by the atomic that set its bit, a non-manifold pair by the
// lane that marked its entry: each exactly once, whoever it is.  No float arithmetic beyond the comparisons of step 1.
//
// smx_recon_mesh_rim itself is at the end of the file: it owns the order of the passes, the workspace (RimWork, smx_rim.hpp)
// and the one read of the counters.
#include "smx_recon_state.hpp"
#include "smx_rim.hpp"

namespace smx {

namespace {

constexpr int kBlock = kRimBlock;

// the edge table as the kernels see it
struct RimDeviceTable {
  FillEdge* e;
  __device__ __forceinline__ unsigned long long key(uint32_t h) const { return e[h].key; }
  __device__ __forceinline__ unsigned long long value(uint32_t h) const { return e[h].value; }
  __device__ __forceinline__ unsigned long long claim(uint32_t h, unsigned long long expected, unsigned long long desired) const {
    return atomicCAS(&e[h].key, expected, desired);
  }
  __device__ __forceinline__ void bump(uint32_t h, unsigned long long inc) const { atomicAdd(&e[h].value, inc); }
  __device__ __forceinline__ unsigned long long mark(uint32_t h, unsigned long long bits) const { return atomicOr(&e[h].value, bits); }
};

__device__ __forceinline__ bool rim_live(const TgMap& map, uint32_t i, const TgVec& p) {
  return dec_live(p.x, p.y, p.z, map.normal[(size_t)i * map.normal_stride].w);
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off);
  return v;
}

// bitmap[word] |= bits for every lane with bits != 0, one atomic per word the wavefront touches: the lanes that share the
// first waiting lane's word fold their bits, that lane issues the atomic, and so on until nobody waits.  Every lane of the
// wavefront calls it.  Returns, in the issuing lanes, the bits the atomic found clear: slots that became rim vertices here.
__device__ __forceinline__ uint32_t wave_or_into(uint32_t* bitmap, uint32_t word, uint32_t bits) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t fresh = 0;
  unsigned long long waiting = __ballot(bits != 0);
  while (waiting != 0) {
    const uint32_t first = (uint32_t)__ffsll((long long)waiting) - 1u;
    const uint32_t w = (uint32_t)__shfl((int)word, (int)first);
    const bool mine = bits != 0 && word == w;
    const uint32_t all = wave_or(mine ? bits : 0u);
    if (lane == first) fresh |= all & ~atomicOr(&bitmap[w], all);
    waiting &= ~__ballot(mine);
  }
  return fresh;
}

// the table is all zeros before: empty.  bytes[t] = kRimInR for a triangle of R, else 0.  (A triangle with an index out of
// range reads and inserts nothing; the call is refused.)
__global__ void __launch_bounds__(kBlock)
k_rim_edges(TgMap map, const uint32_t* __restrict__ tri, uint32_t n_in, FillEdge* table, uint32_t mask, uint8_t* __restrict__ bytes,
            uint32_t* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  uint32_t cls = 0xFFu, claimed = 0;
  bool bad_index = false;
  if (t < n_in) {
    const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if (i0 >= map.n || i1 >= map.n || i2 >= map.n) {
      bad_index = true;
    } else {
      const TgVec a = tg_pos(map, i0), b = tg_pos(map, i1), c = tg_pos(map, i2);
      cls = tg_classify(i0, i1, i2, rim_live(map, i0, a), rim_live(map, i1, b), rim_live(map, i2, c), a, b, c);
      if (cls == kTgInR) {
        RimDeviceTable tab{table};
        claimed = (fill_insert(tab, mask, i0, i1) ? 1u : 0u) + (fill_insert(tab, mask, i1, i2) ? 1u : 0u) + (fill_insert(tab, mask, i2, i0) ? 1u : 0u);
      }
    }
    bytes[t] = cls == kTgInR ? (uint8_t)kRimInR : (uint8_t)0;
  }
  if (__ballot(bad_index) != 0 && (threadIdx.x & 63) == 0) atomicOr(&cnt[kRimError], 1u);       // (one per wavefront)
  wave_count(&cnt[kRimNotLive], cls == kTgDropNotLive);
  wave_count(&cnt[kRimRepeated], cls == kTgDropRepeated);
  wave_count(&cnt[kRimRange], cls == kTgDropRange);
  claimed = wave_sum(claimed);
  if ((threadIdx.x & 63) == 0 && claimed != 0) atomicAdd(&cnt[kRimEdges], claimed);
}

// the bitmap is all zeros before.  bytes[t] = kRimInR | the edge bits for a triangle of R.
__global__ void __launch_bounds__(kBlock)
k_rim_vertices(const uint32_t* __restrict__ tri, uint32_t n_in, FillEdge* table, uint32_t mask, uint8_t* __restrict__ bytes,
               uint32_t* __restrict__ bitmap, uint32_t* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  uint32_t i[3] = {0, 0, 0}, marks = 0, rim_edges = 0, nonmanifold = 0;
  if (t < n_in && bytes[t] != 0) {
    i[0] = tri[3 * (size_t)t]; i[1] = tri[3 * (size_t)t + 1]; i[2] = tri[3 * (size_t)t + 2];
    RimDeviceTable tab{table};
    bool first[3];
    const uint32_t c_ab = rim_edge(tab, mask, i[0], i[1], &first[0]), c_bc = rim_edge(tab, mask, i[1], i[2], &first[1]),
                   c_ca = rim_edge(tab, mask, i[2], i[0], &first[2]);
    const uint32_t edge_bits = rim_edge_bits(c_ab, c_bc, c_ca);
    bytes[t] = (uint8_t)(kRimInR | edge_bits);
    marks = rim_corner_marks(edge_bits);
    rim_edges = (uint32_t)__popc(edge_bits);
    nonmanifold = (first[0] ? 1u : 0u) + (first[1] ? 1u : 0u) + (first[2] ? 1u : 0u);
  }
  uint32_t fresh = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) fresh += (uint32_t)__popc(wave_or_into(bitmap, rim_word(i[k]), (marks >> k) & 1u ? rim_bit(i[k]) : 0u));
  fresh = wave_sum(fresh); rim_edges = wave_sum(rim_edges); nonmanifold = wave_sum(nonmanifold);
  if ((threadIdx.x & 63) == 0) {
    if (fresh != 0) atomicAdd(&cnt[kRimVertices], fresh);
    if (rim_edges != 0) atomicAdd(&cnt[kRimRimEdges], rim_edges);
    if (nonmanifold != 0) atomicAdd(&cnt[kRimNonManifold], nonmanifold);
  }
}

__global__ void __launch_bounds__(kBlock)
k_rim_bytes(const uint32_t* __restrict__ tri, uint32_t n_in, const uint32_t* __restrict__ bitmap, uint8_t* __restrict__ bytes,
            uint32_t* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  uint32_t byte = 0;
  if (t < n_in) {
    const uint32_t held = bytes[t];
    if (held != 0) {
      const uint32_t i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
      byte = rim_byte(held & ~kRimInR, rim_vertex(bitmap, i0), rim_vertex(bitmap, i1), rim_vertex(bitmap, i2));
      bytes[t] = (uint8_t)byte;
    }
  }
  wave_count(&cnt[kRimTriangles], byte != 0);
}

}  // namespace

// The three passes on st, into w.bytes; din is device memory.  Every allocation lies before the first launch.
static int rim_enqueue(smx_recon r, RimWork& w, const uint32_t* din, uint32_t n_in, uint32_t n, hipStream_t st) {
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kRimWords * sizeof(uint32_t), st));
  if (n_in == 0) return SMX_OK;
  const uint32_t entries = dec_table_size(3 * n_in), mask = entries - 1;
  FillEdge* table = reinterpret_cast<FillEdge*>(w.table.get());
  SMX_HIP(hipMemsetAsync(table, 0, (size_t)entries * sizeof(FillEdge), st));
  SMX_HIP(hipMemsetAsync(w.bitmap.get(), 0, ((size_t)n / 32 + 1) * sizeof(uint32_t), st));
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const TgMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  const dim3 b(kRimBlock), g(div_up(n_in, kRimBlock));
  hipLaunchKernelGGL(k_rim_edges, g, b, 0, st, map, din, n_in, table, mask, w.bytes.get(), cnt);
  hipLaunchKernelGGL(k_rim_vertices, g, b, 0, st, din, n_in, table, mask, w.bytes.get(), w.bitmap.get(), cnt);
  hipLaunchKernelGGL(k_rim_bytes, g, b, 0, st, din, n_in, w.bitmap.get(), w.bytes.get(), cnt);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int rim_run(smx_recon r, hipStream_t st, const uint32_t* triangles, uint32_t n_in, bool on_device, uint32_t n, const uint8_t** d_rim,
            smx_rim_stats* stats) {
  RimWork& w = r->rim;
  // ---- the workspace; the input on the device
  const uint32_t entries = dec_table_size(3 * n_in);
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kRimWords, false));
  SMX_CALL(w.table.reserve((size_t)2 * entries));
  SMX_CALL(w.bitmap.reserve((size_t)n / 32 + 1));
  SMX_CALL(w.bytes.reserve(n_in));
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(w.in, triangles, (size_t)3 * n_in, on_device, st, &din));
  SMX_CALL(rim_enqueue(r, w, din, n_in, n, st));
  uint32_t h[kRimWords];
  SMX_HIP(hipMemcpyAsync(h, w.counters.get(), sizeof(h), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (h[kRimError] != 0) {
    set_error("triangles holds an index >= the %u slots of the map", n);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  if (stats) {
    stats->n_in = n_in; stats->n_not_live = h[kRimNotLive]; stats->n_repeated = h[kRimRepeated]; stats->n_out_of_range = h[kRimRange];
    stats->n_edges = h[kRimEdges]; stats->n_rim_edges = h[kRimRimEdges]; stats->n_nonmanifold_edges = h[kRimNonManifold];
    stats->n_rim_vertices = h[kRimVertices]; stats->n_rim_triangles = h[kRimTriangles];
  }
  *d_rim = w.bytes.get();
  return SMX_OK;
}

}  // namespace smx

using namespace smx;

extern "C" {

int smx_recon_mesh_rim(smx_recon r, smx_stream s, const uint32_t* triangles, uint32_t n_in, int32_t on_device, uint8_t* rim, smx_rim_stats* stats) {
  SMX_CHECK_ARG(r != nullptr);
  SMX_CHECK_ARG(n_in <= (1u << 28));
  SMX_CHECK_ARG((triangles != nullptr && rim != nullptr) || n_in == 0);
  if (ranges_overlap(triangles, (size_t)n_in * 12, rim, n_in)) {
    set_error("rim overlaps triangles");
    return SMX_ERR_INVALID_ARGUMENT;
  }
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  smx_rim_stats out;
  memset(&out, 0, sizeof(out));
  const uint8_t* d_rim = nullptr;
  SMX_CALL(rim_run(r, st, triangles, n_in, on_device != 0, n, &d_rim, &out));
  if (n_in > 0) {
    SMX_HIP(hipMemcpyAsync(rim, d_rim, n_in, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
  }
  if (stats) *stats = out;
  return SMX_OK;
}

}  // extern "C"
