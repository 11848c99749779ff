// smx_fill.hip -- the kernels of smx_recon_fill_holes (gfx950): the edge table of a triangle array over the surfel map, its
// boundary loops, and the small ones closed by fans (the contract is in include/smx.h, its arithmetic and the
// table operations in smx_fill.hpp).
//
//   edges:  k_fill_edges (a lane per triangle: range check, live test, keep flag, three inserts into the edge table, triangles
//           of R counted per workgroup) -> enqueue_segment_scan -> k_fill_classify (a lane per table entry: interior,
//           boundary or non-manifold; a boundary entry adds its gap to out / in and stores next)
//   loops:  k_fill_walk (a lane per slot: pinched or not, the bounded walk along next, owners counted per workgroup) ->
//           enqueue_segment_scan -> k_fill_list (the table of listed loops, ascending by label)
//   fill:   k_fill_loops (32 lanes per loop: vertices staged in LDS, cost per lane, packed-key minimum, one fan triangle and
//           one diagonal per lane, status, the new triangles appended) -> two stable radix sorts of smx_nn.hip, by (a, b) and
//           then by p, as smx_decimate.hip orders its output
//   write:  k_fill_write (R by its offsets) and k_fill_emit (the new run behind it)
//
// Why the result does not depend on the schedule: the counters of a pair are integer sums; out / in are integer sums; next[w]
// is read only where out(w) = 1, that is where one lane stored it; a loop has one owner (its smallest slot) found without
// atomics; the new triangles are appended through a cursor in arrival order, but the loops are vertex-disjoint, so no two of
// them share (p, a, b) and the sorted run is unique.
//
// smx_recon_fill_holes itself is at the end of the file: it owns the order of the phases, the workspace (FillWork,
// smx_fill.hpp) and the two reads of the counters.
#include <cmath>

#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

namespace smx {

namespace {

constexpr int kBlock = kFillBlock;
constexpr int kLoopsPerBlock = kBlock / 32;

// the edge table as the kernels see it
struct FillDeviceTable {
  FillEdge* e;
  __device__ __forceinline__ unsigned long long key(uint32_t h) const { return e[h].key; }
  __device__ __forceinline__ unsigned long long claim(uint32_t h, unsigned long long expected, unsigned long long desired) const {
    return atomicCAS(&e[h].key, expected, desired);
  }
  __device__ __forceinline__ void bump(uint32_t h, unsigned long long inc) const { atomicAdd(&e[h].value, inc); }
};

// one atomic per wavefront: the number of its lanes with `pred`
__device__ __forceinline__ void wave_count_add(uint32_t* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m != 0 && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(counter, (uint32_t)__popcll(m));
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

__device__ __forceinline__ bool slot_live(const FillMap& map, uint32_t i) {
  const float4 s = map.smooth[(size_t)i * map.smooth_stride];
  const float rs = map.normal[(size_t)i * map.normal_stride].w;
  return dec_live(s.x, s.y, s.z, rs);
}

// the table is all zeros before: empty.  (A triangle with an index out of range inserts nothing; the call is refused.)
__global__ void __launch_bounds__(kBlock)
k_fill_edges(FillMap map, const uint32_t* __restrict__ tri_in, uint32_t n_in, uint32_t* __restrict__ keep, FillEdge* table, uint32_t mask,
             uint32_t* __restrict__ block_sums, uint32_t* __restrict__ counters) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  bool not_live = false, in_r = false;
  if (t < n_in) {
    const uint32_t i0 = tri_in[3 * (size_t)t], i1 = tri_in[3 * (size_t)t + 1], i2 = tri_in[3 * (size_t)t + 2];
    if (i0 >= map.n || i1 >= map.n || i2 >= map.n) {
      atomicOr(&counters[kFillError], 1u);
    } else if (slot_live(map, i0) && slot_live(map, i1) && slot_live(map, i2)) {
      in_r = true;
      FillDeviceTable tab{table};
      (void)fill_insert(tab, mask, i0, i1);
      (void)fill_insert(tab, mask, i1, i2);
      (void)fill_insert(tab, mask, i2, i0);
    } else {
      not_live = true;
    }
    keep[t] = in_r ? 1u : 0u;
  }
  uint32_t total;
  (void)block_rank(in_r, wave_tot, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
  wave_count_add(&counters[kFillNotLive], not_live);
}

// deg is all zeros before.  Two gaps that leave one vertex both store its next: that vertex has out = 2 and nobody reads it.
__global__ void __launch_bounds__(kBlock)
k_fill_classify(const FillEdge* __restrict__ table, uint32_t entries, uint32_t* __restrict__ deg, uint32_t* __restrict__ next,
                uint32_t* __restrict__ counters) {
  const uint32_t h = blockIdx.x * kBlock + threadIdx.x;
  bool used = false, boundary = false, bad = false;
  if (h < entries) {
    const FillEdge e = table[h];
    if (e.key != kFillEmpty) {
      used = true;
      const unsigned long long key = e.key - 1;
      const uint32_t lo = (uint32_t)(key >> 32), hi = (uint32_t)key;
      const uint32_t c = fill_classify(e.value);
      bad = c == kFillNonManifold;
      boundary = c == kFillBoundaryUp || c == kFillBoundaryDown;
      if (boundary) {
        const uint32_t from = c == kFillBoundaryUp ? hi : lo, to = c == kFillBoundaryUp ? lo : hi;
        atomicAdd(&deg[2 * (size_t)from], 1u);
        atomicAdd(&deg[2 * (size_t)to + 1], 1u);
        next[from] = to;
      }
    }
  }
  wave_count_add(&counters[kFillEdges], used);
  wave_count_add(&counters[kFillBoundary], boundary);
  wave_count_add(&counters[kFillNonManifoldEdges], bad);
}

__global__ void __launch_bounds__(kBlock)
k_fill_walk(uint32_t n, const uint32_t* __restrict__ deg, const uint32_t* __restrict__ next, uint32_t max_edges, uint32_t* __restrict__ len,
            uint32_t* __restrict__ block_sums, uint32_t* __restrict__ counters) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool pinched = false;
  uint32_t L = 0;
  if (i < n) {
    const uint32_t o = deg[2 * (size_t)i], in = deg[2 * (size_t)i + 1];
    pinched = (o | in) != 0 && !(o == 1 && in == 1);
    L = fill_walk(deg, next, i, max_edges);
    if (L < 3) L = 0;
    len[i] = L;
  }
  uint32_t total;
  (void)block_rank(L != 0, wave_tot, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
  wave_count_add(&counters[kFillPinched], pinched);
}

__global__ void __launch_bounds__(kBlock)
k_fill_list(uint32_t n, const uint32_t* __restrict__ len, const uint32_t* __restrict__ block_off, smx_mesh_hole* __restrict__ holes) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t L = i < n ? len[i] : 0;
  uint32_t total;
  const uint32_t j = block_off[blockIdx.x] + block_rank(L != 0, wave_tot, &total);
  if (L != 0) holes[j] = smx_mesh_hole{i, L, 0u};
}

struct LdsVecs {
  const float4* p;
  __device__ __forceinline__ MeshVec operator[](uint32_t j) const { const float4 v = p[j]; return MeshVec{v.x, v.y, v.z}; }
};

// the bits of a ballot that belong to this lane's group of 32
__device__ __forceinline__ uint32_t group_ballot(bool pred) {
  const unsigned long long m = __ballot(pred);
  return (uint32_t)(m >> (threadIdx.x & 32));
}

// A group of 32 lanes per listed loop, two groups per wavefront.  Lane j holds w_j; then lane i evaluates cost(i), and lane k
// tests fan triangle k and diagonal k.  All lanes of the workgroup reach every barrier, ballot and shuffle.
__global__ void __launch_bounds__(kBlock)
k_fill_loops(FillMap map, smx_mesh_hole* __restrict__ holes, uint32_t n_listed, const uint32_t* __restrict__ next,
             const FillEdge* __restrict__ table, uint32_t mask, float cos_min_angle, float cos_max_angle, DecTri* __restrict__ fresh,
             uint32_t* __restrict__ counters) {
  __shared__ float4 s_pos[kLoopsPerBlock][kFillMaxHoleEdges], s_nrm[kLoopsPerBlock][kFillMaxHoleEdges];
  __shared__ uint32_t s_w[kLoopsPerBlock][kFillMaxHoleEdges];
  const uint32_t g = threadIdx.x >> 5, j = threadIdx.x & 31;
  const uint32_t loop = blockIdx.x * kLoopsPerBlock + g;
  const bool active = loop < n_listed;
  uint32_t L = 0, w = 0;
  if (active) { const smx_mesh_hole row = holes[loop]; L = row.n_edges; w = row.label; }
  for (uint32_t s = 0; s + 1 < L; ++s) if (s < j) w = next[w];       // (L <= 32: lane j < L ends at w_j)
  if (j < L) {
    s_w[g][j] = w;
    s_pos[g][j] = map.smooth[(size_t)w * map.smooth_stride];
    s_nrm[g][j] = map.normal[(size_t)w * map.normal_stride];
  }
  __syncthreads();
  const LdsVecs pos{s_pos[g]}, nrm{s_nrm[g]};
  unsigned long long key = ~0ull;
  if (j < L) key = dec_value_word(fill_cost(pos, L, j), w);
  unsigned long long best = key;
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(best, off);
    best = other < best ? other : best;
  }
  const uint32_t winners = group_ballot(j < L && key == best);       // (the slots of a loop differ: one bit)
  const uint32_t ia = winners != 0 ? (uint32_t)__ffs((int)winners) - 1u : 0u;
  const uint32_t k = j;
  const bool fan = active && k >= 1 && k + 2 <= L;
  bool diagonal = false, rejected = false;
  if (fan) {
    const FillDeviceTable tab{const_cast<FillEdge*>(table)};
    if (k >= 2) diagonal = fill_has_edge(tab, mask, s_w[g][ia], s_w[g][(ia + k) % L]);
    rejected = !fill_fan_ok(pos, nrm, L, ia, k, cos_min_angle, cos_max_angle);
  }
  const uint32_t any_diagonal = group_ballot(diagonal), any_rejected = group_ballot(rejected);
  const uint32_t status = any_diagonal != 0 ? (uint32_t)SMX_HOLE_DIAGONAL : any_rejected != 0 ? (uint32_t)SMX_HOLE_FILTER : (uint32_t)SMX_HOLE_FILLED;
  const bool filled = active && status == SMX_HOLE_FILLED;
  uint32_t base = 0;
  if (filled && j == 0) base = atomicAdd(&counters[kFillNew], L - 2);
  base = (uint32_t)__shfl((int)base, (int)(threadIdx.x & 32));
  if (filled && fan) fresh[base + k - 1] = dec_canonical(s_w[g][ia], s_w[g][(ia + k) % L], s_w[g][(ia + k + 1) % L]);
  if (active && j == 0) holes[loop].status = status;
  wave_count_add(&counters[kFillFilled], filled && j == 0);
  wave_count_add(&counters[kFillDiagonal], active && j == 0 && status == SMX_HOLE_DIAGONAL);
  wave_count_add(&counters[kFillFilter], active && j == 0 && status == SMX_HOLE_FILTER);
}

__global__ void __launch_bounds__(kBlock)
k_fill_keys_ab(uint32_t m, const DecTri* __restrict__ fresh, int bits, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  keys[j] = dec_key_ab(fresh[j], bits);
  vals[j] = j;
}

__global__ void __launch_bounds__(kBlock)
k_fill_keys_p(uint32_t m, const uint32_t* vals_in, const DecTri* __restrict__ fresh, unsigned long long* __restrict__ keys_out,
              uint32_t* vals_out) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t t = vals_in[j];      // (vals_out may be vals_in: each lane reads its entry before it writes it)
  keys_out[j] = fresh[t].p;
  vals_out[j] = t;
}

__global__ void __launch_bounds__(kBlock)
k_fill_emit(uint32_t m, const uint32_t* __restrict__ vals, const DecTri* __restrict__ fresh, uint32_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  const DecTri c = fresh[vals[j]];
  out[3 * (size_t)j] = c.p; out[3 * (size_t)j + 1] = c.a; out[3 * (size_t)j + 2] = c.b;
}

__global__ void __launch_bounds__(kBlock)
k_fill_write(const uint32_t* __restrict__ tri_in, uint32_t n_in, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ block_off,
             uint32_t* __restrict__ out) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  const bool s = t < n_in && keep[t] != 0;
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

int smx_fill_params_default(smx_fill_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->max_hole_edges = 8; out->min_triangle_angle_deg = 10.0f; out->max_triangle_angle_deg = 170.0f;
  return SMX_OK;
}

int smx_recon_fill_holes(smx_recon r, smx_stream s, const smx_fill_params* p, const uint32_t* triangles_in, uint32_t n_in,
                         uint32_t* triangles_out, uint32_t capacity, smx_mesh_hole* holes, uint32_t hole_capacity, int32_t on_device,
                         uint32_t* n_triangles, uint32_t* n_kept, uint32_t* n_holes, smx_fill_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && p != nullptr && n_triangles != nullptr && n_kept != nullptr && n_holes != nullptr);
  SMX_CHECK_ARG(p->max_hole_edges >= 3 && p->max_hole_edges <= SMX_FILL_MAX_HOLE_EDGES);
  SMX_CHECK_ARG(finite_f(p->min_triangle_angle_deg) && finite_f(p->max_triangle_angle_deg));
  SMX_CHECK_ARG(p->min_triangle_angle_deg >= 0.0f && p->min_triangle_angle_deg < p->max_triangle_angle_deg &&
                p->max_triangle_angle_deg <= 180.0f);
  SMX_CHECK_ARG(n_in <= (1u << 28));
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
  *n_triangles = 0; *n_kept = 0; *n_holes = 0;
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_in = n_in; }
  FillWork& w = r->fill;
  SMX_CALL(w.stamps.begin(st));
  // Every way out below that has marked a phase goes through finish: it publishes exactly the phases marked so far (2 after
  // a bad index, 3 after the capacity rule, 4 after a full call).
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    w.stamps.publish();
    return rc;
  };

  // ---- workspace of the first two phases; the input on the device
  const int nb = div_up(n_in, kFillBlock), nbv = div_up(n, kFillBlock);
  const uint32_t entries = dec_table_size(3 * n_in), mask = entries - 1;
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kFillWords, false));
  SMX_CALL(w.table.reserve((size_t)2 * entries));
  SMX_CALL(w.keep.reserve(n_in));
  SMX_CALL(w.deg.reserve((size_t)2 * n));
  SMX_CALL(w.next.reserve(n));
  SMX_CALL(w.len.reserve(n));
  SMX_CALL(w.tblocks.reserve((size_t)nb));
  SMX_CALL(w.vblocks.reserve((size_t)nbv));
  SMX_CALL(w.holes.reserve(((size_t)n / 3 + 1) * 3));      // (the listed loops are vertex-disjoint and have three vertices at least)
  const uint32_t* din = nullptr;
  SMX_CALL(stage_in(w.in, triangles_in, (size_t)3 * n_in, on_device != 0, st, &din));
  uint32_t* cnt = w.counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kFillWords * sizeof(uint32_t), st));
  uint32_t h[kFillWords];
  auto read_counters = [&]() -> int {
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    return SMX_OK;
  };

  // ---- edges
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  const FillMap map{sv.p, sv.stride, nv.p, nv.stride, n};
  FillEdge* table = reinterpret_cast<FillEdge*>(w.table.get());
  smx_mesh_hole* rows = reinterpret_cast<smx_mesh_hole*>(w.holes.get());
  const dim3 b(kFillBlock), g_in(nb), g_map(nbv);
  if (n_in > 0) {
    SMX_HIP(hipMemsetAsync(table, 0, (size_t)entries * sizeof(FillEdge), st));
    if (n > 0) SMX_HIP(hipMemsetAsync(w.deg.get(), 0, (size_t)2 * n * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_fill_edges, g_in, b, 0, st, map, din, n_in, w.keep.get(), table, mask, w.tblocks.get(), cnt);
    enqueue_segment_scan(st, w.tblocks.get(), nb, cnt + kFillKept);
    hipLaunchKernelGGL(k_fill_classify, dim3(blocks_for(entries)), b, 0, st, table, entries, w.deg.get(), w.next.get(), cnt);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- loops
  if (n_in > 0 && n > 0) {
    hipLaunchKernelGGL(k_fill_walk, g_map, b, 0, st, n, w.deg.get(), w.next.get(), p->max_hole_edges, w.len.get(), w.vblocks.get(), cnt);
    enqueue_segment_scan(st, w.vblocks.get(), nbv, cnt + kFillListed);
    hipLaunchKernelGGL(k_fill_list, g_map, b, 0, st, n, w.len.get(), w.vblocks.get(), rows);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));
  SMX_CALL(read_counters());
  if (h[kFillError] != 0) {
    set_error("triangles_in holds an index >= the %u slots of the map", n);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  const uint32_t R = h[kFillKept], H = h[kFillListed];
  *n_kept = R; *n_holes = H;

  // ---- fill: status and new triangles of every listed loop, then the new run's order
  uint32_t n_new = 0;
  DecTri* fresh = nullptr;
  int cur = 0;
  if (H > 0) {
    const double rad = 3.14159265358979323846 / 180.0;
    const float cos_min_angle = (float)std::cos((double)p->min_triangle_angle_deg * rad);
    const float cos_max_angle = (float)std::cos((double)p->max_triangle_angle_deg * rad);
    SMX_CALL(w.fresh.reserve((size_t)H * (p->max_hole_edges - 2) * 3));
    fresh = reinterpret_cast<DecTri*>(w.fresh.get());
    hipLaunchKernelGGL(k_fill_loops, dim3(div_up(H, kLoopsPerBlock)), b, 0, st, map, rows, H, w.next.get(), table, mask, cos_min_angle,
                       cos_max_angle, fresh, cnt);
    SMX_LAUNCH_CHECK();
    SMX_CALL(read_counters());
    n_new = h[kFillNew];
  }
  if (n_new > 0) {
    for (int k = 0; k < 2; ++k) { SMX_CALL(w.keys[k].reserve(n_new)); SMX_CALL(w.vals[k].reserve(n_new)); }
    SMX_CALL(w.hist.reserve(radix_sort_workspace_elems(n_new)));
    int bits = 1;
    while (bits < 32 && ((uint32_t)(n - 1) >> bits) != 0) ++bits;
    const dim3 gt(blocks_for(n_new));
    hipLaunchKernelGGL(k_fill_keys_ab, gt, b, 0, st, n_new, fresh, bits, w.keys[0].get(), w.vals[0].get());
    SMX_LAUNCH_CHECK();
    cur = radix_sort(w.keys, w.vals, n_new, 2 * bits, w.hist.get(), st);
    hipLaunchKernelGGL(k_fill_keys_p, gt, b, 0, st, n_new, w.vals[cur].get(), fresh, w.keys[0].get(), w.vals[0].get());
    SMX_LAUNCH_CHECK();
    cur = radix_sort(w.keys, w.vals, n_new, bits, w.hist.get(), st);
  }
  SMX_CALL(w.stamps.mark(st));
  const uint32_t T = R + n_new;
  *n_triangles = T;
  if (stats) {
    stats->n_not_live = h[kFillNotLive]; stats->n_edges = h[kFillEdges]; stats->n_boundary_edges = h[kFillBoundary];
    stats->n_nonmanifold_edges = h[kFillNonManifoldEdges]; stats->n_pinched_vertices = h[kFillPinched]; stats->n_listed_loops = H;
    stats->n_filled_loops = h[kFillFilled]; stats->n_rejected_diagonal = h[kFillDiagonal]; stats->n_rejected_filter = h[kFillFilter];
    stats->n_new_triangles = n_new; stats->n_triangles = T;
  }
  if (capacity < T) {
    if (triangles_out != nullptr || capacity != 0) set_error("triangles_out holds %u entries, the filled mesh has %u triangles", capacity, T);
    else set_error("count only: the filled mesh has %u triangles, %u listed loops", T, H);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  if (holes != nullptr && hole_capacity < H) {
    set_error("holes holds %u entries, the mesh has %u listed loops", hole_capacity, H);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }

  // ---- write: R in input order, the new run behind it, the table
  uint32_t* dst = triangles_out;
  if (T > 0 && !on_device) {      // (the last allocation of the call: nothing has been written to the caller's arrays yet)
    SMX_CALL(w.out.reserve((size_t)3 * T));
    dst = w.out.get();
  }
  const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (T > 0) {
    if (R > 0) hipLaunchKernelGGL(k_fill_write, g_in, b, 0, st, din, n_in, w.keep.get(), w.tblocks.get(), dst);
    if (n_new > 0) hipLaunchKernelGGL(k_fill_emit, dim3(blocks_for(n_new)), b, 0, st, n_new, w.vals[cur].get(), fresh, dst + (size_t)3 * R);
    SMX_LAUNCH_CHECK();
    if (!on_device) SMX_HIP(hipMemcpyAsync(triangles_out, dst, (size_t)T * 12, hipMemcpyDeviceToHost, st));
  }
  if (holes && H > 0) SMX_HIP(hipMemcpyAsync(holes, rows, (size_t)H * sizeof(smx_mesh_hole), back, st));
  SMX_CALL(w.stamps.mark(st));
  return finish(SMX_OK);
}

int smx_recon_debug_fill_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_FILL_PHASES);
  SMX_ON_DEVICE(r->device);
  return r->fill.stamps.elapsed_ms(out_ms, SMX_FILL_PHASES);
}

}  // extern "C"
