// smx_mesh.hip -- localized Delaunay triangulation of the surfel map (smx_recon_triangulate).
//
//   k_mesh_prepare   a lane per slot: the RadiusSquared row smx_nn_query_self reads, the live count
//   (smx_nn_query_self: the [n][K] candidate lists)
//   k_mesh_star      a wavefront per slot, a lane per candidate: projection into the slot's tangent plane, the star of
//                    the origin by mesh_star_successor (O(K^2) broadcast reads of 768 bytes of LDS per wavefront, no
//                    per-lane arrays), ring order by counting, one 64-byte ring row and a meta word per slot
//   k_mesh_agree     a lane per slot, twice: <false> counts the triangles the slot owns (smallest corner) after
//                    agreement and filters and scans the counts inside the workgroup; <true> finds them again and
//                    writes them at (workgroup offset + local offset), then orders its own few entries
//   k_mesh_scan      one workgroup: exclusive scan of the workgroup totals
// The arithmetic is in smx_mesh.hpp; nothing here decides a sign by itself.
#include <algorithm>
#include <cmath>

#include "smx_mesh.hpp"

namespace smx {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
enum : int { kStLive = 0, kStStar, kStOverflow, kStTruncated, kStTotal, kStWords = 8 };

struct MeshK {
  const float4* smooth; size_t smooth_stride;
  const float4* normal; size_t normal_stride;
  uint32_t n;
  int K;                      // row length of the lists
  float cos_max_normal, cos_min_angle, cos_max_angle;
};

__device__ __forceinline__ MeshVec v3(const float4& f) { return MeshVec{f.x, f.y, f.z}; }
__device__ __forceinline__ bool slot_live(const float4& s, const float4& nr) {
  return !(nr.w < 0.0f) && mesh_finite(s.x) && mesh_finite(s.y) && mesh_finite(s.z);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void __launch_bounds__(kBlock)
k_mesh_prepare(MeshK k, float* __restrict__ r2, uint32_t* __restrict__ stat) {
  uint32_t live = 0;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < k.n; i += gridDim.x * kBlock) {
    const float4 s = k.smooth[(size_t)i * k.smooth_stride];
    const float4 nr = k.normal[(size_t)i * k.normal_stride];
    r2[i] = nr.w;
    live += slot_live(s, nr) ? 1u : 0u;
  }
  live = wave_sum(live);
  if ((threadIdx.x & 63) == 0 && live) atomicAdd(&stat[kStLive], live);   // (integer: any order gives the same sum)
}

__global__ void __launch_bounds__(kBlock)
k_mesh_star(MeshK k, const uint32_t* __restrict__ lists, const int32_t* __restrict__ counts, uint32_t* __restrict__ rings,
            uint32_t* __restrict__ meta, uint32_t* __restrict__ stat) {
  __shared__ float sx[kWaves][64], sy[kWaves][64], sq[kWaves][64];
  __shared__ uint32_t s_ring[kWaves][kMeshMaxStarDegree];
  __shared__ uint32_t s_mask[kWaves];
  __shared__ uint8_t s_is_succ[kWaves][64], s_rank[kWaves][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // (every wavefront of the workgroup makes the same number of trips, so that the barriers below are uniform)
  for (uint32_t base = blockIdx.x * kWaves; base < k.n; base += gridDim.x * kWaves) {
    const uint32_t p = base + w;
    const bool valid = p < k.n;
    float4 ps = make_float4(0, 0, 0, 0), pn = make_float4(0, 0, 0, -1.0f);
    int cnt = 0;
    if (valid) {
      ps = k.smooth[(size_t)p * k.smooth_stride];
      pn = k.normal[(size_t)p * k.normal_stride];
      cnt = counts[p];
    }
    const bool live = valid && slot_live(ps, pn);
    cnt = live ? min(max(cnt, 0), k.K) : 0;
    // projection of candidate `lane`
    uint32_t j = kInvalid;
    float x = 0.0f, y = 0.0f, q = -1.0f;
    if (lane < cnt) {
      j = lists[(size_t)p * k.K + lane];
      if (j < k.n) {
        const float4 js = k.smooth[(size_t)j * k.smooth_stride];
        const float4 jn = k.normal[(size_t)j * k.normal_stride];
        MeshVec u, v;
        mesh_basis(v3(pn), &u, &v);
        const MeshVec d = mesh_sub(v3(js), v3(ps));
        x = mesh_dot(d, u); y = mesh_dot(d, v);
        if (mesh_candidate_ok(p, j, v3(pn), v3(jn), k.cos_max_normal, x, y, pn.w)) q = x * x + y * y;
      }
    }
    sx[w][lane] = x; sy[w][lane] = y; sq[w][lane] = q;
    s_is_succ[w][lane] = 0;
    if (lane < kMeshMaxStarDegree) s_ring[w][lane] = kInvalid;
    if (lane == 0) s_mask[w] = 0;
    __syncthreads();
    int succ = -1;
    if (q > 0.0f) succ = mesh_star_successor(lane, cnt, sx[w], sy[w], sq[w]);
    if (succ >= 0) s_is_succ[w][succ] = 1;
    __syncthreads();
    const bool in_star = succ >= 0 || s_is_succ[w][lane] != 0;
    const unsigned long long star = __ballot(in_star);
    const int deg = __popcll(star);
    const bool overflow = deg > kMeshMaxStarDegree;
    int rank = 0;
    if (in_star && !overflow) {
      const float ang = mesh_pseudo_angle(x, y);
      for (unsigned long long m = star; m; m &= m - 1) {
        const int c = __ffsll((long long)m) - 1;
        if (c != lane && mesh_ring_before(mesh_pseudo_angle(sx[w][c], sy[w][c]), c, ang, lane)) ++rank;
      }
      s_ring[w][rank] = j;
      s_rank[w][lane] = (uint8_t)rank;
    }
    __syncthreads();
    if (succ >= 0 && !overflow && (int)s_rank[w][succ] == (rank + 1 == deg ? 0 : rank + 1)) atomicOr(&s_mask[w], 1u << rank);
    __syncthreads();
    if (valid) {
      if (lane < kMeshMaxStarDegree) rings[(size_t)p * kMeshMaxStarDegree + lane] = overflow ? kInvalid : s_ring[w][lane];
      if (lane == 0) {
        meta[p] = overflow ? kMeshOverflowBit : ((uint32_t)deg | (s_mask[w] << 8));
        if (overflow) atomicAdd(&stat[kStOverflow], 1u);
        if (live && cnt == k.K) atomicAdd(&stat[kStTruncated], 1u);
      }
    }
    __syncthreads();   // (the next trip rewrites the rows)
  }
}

__device__ __forceinline__ void load_ring(const uint32_t* __restrict__ rings, uint32_t slot, uint32_t out[kMeshMaxStarDegree]) {
  const uint4* row = reinterpret_cast<const uint4*>(rings + (size_t)slot * kMeshMaxStarDegree);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint4 v = row[t];
    out[4 * t] = v.x; out[4 * t + 1] = v.y; out[4 * t + 2] = v.z; out[4 * t + 3] = v.w;
  }
}

// Exclusive scan of one value per lane over the workgroup; *total = the workgroup's sum.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t s_wave[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int t = 0; t < kWaves; ++t) { if (t < w) before += s_wave[t]; all += s_wave[t]; }
  *total = all;
  return before + inc - v;
}

// One lane per slot p (no grid stride: the workgroup index is the scan's unit).  Every star triangle of p is looked up
// in the rings of its other two corners; p owns it iff p is its smallest corner.
template <bool kWrite>
__global__ void __launch_bounds__(kBlock)
k_mesh_agree(MeshK k, const uint32_t* __restrict__ rings, const uint32_t* __restrict__ meta, uint32_t* __restrict__ local_off,
             uint32_t* __restrict__ block_sums, const uint32_t* __restrict__ block_off, uint32_t* __restrict__ tri,
             uint32_t total, uint32_t* __restrict__ stat) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  uint32_t own = 0, distinct = 0;
  uint32_t* out = nullptr;
  uint32_t room = 0;     // (entries from the slot's offset to the end of the output: the write pass never leaves the buffer)
  if (kWrite && p < k.n) {
    const uint32_t first = block_off[blockIdx.x] + local_off[p];
    out = tri + 3 * (size_t)first;
    room = first < total ? total - first : 0u;
  }
  const uint32_t mp = p < k.n ? meta[p] : 0u;
  const uint32_t deg = mesh_meta_degree(mp);
  if (deg >= 2 && !(mp & kMeshOverflowBit)) {
    const uint32_t* ring_p = rings + (size_t)p * kMeshMaxStarDegree;
    for (uint32_t i = 0; i < deg; ++i) {
      if (!((mp >> (8 + i)) & 1u)) continue;
      const uint32_t a = ring_p[i], b = ring_p[i + 1 == deg ? 0 : i + 1];
      if (a >= k.n || b >= k.n) continue;
      if (kWrite && !(p < a && p < b)) continue;
      uint32_t ra[kMeshMaxStarDegree];
      load_ring(rings, a, ra);
      const bool in_a = mesh_ring_has_triangle(ra, meta[a], b, p);
      load_ring(rings, b, ra);
      const bool in_b = mesh_ring_has_triangle(ra, meta[b], p, a);
      // counted once: by the smallest of the corners whose star holds it
      if (!kWrite && !(a < p && in_a) && !(b < p && in_b)) ++distinct;
      if (!(p < a && p < b && in_a && in_b)) continue;
      const float4 Ps = k.smooth[(size_t)p * k.smooth_stride], Pn = k.normal[(size_t)p * k.normal_stride];
      const float4 As = k.smooth[(size_t)a * k.smooth_stride], An = k.normal[(size_t)a * k.normal_stride];
      const float4 Bs = k.smooth[(size_t)b * k.smooth_stride], Bn = k.normal[(size_t)b * k.normal_stride];
      const int f = mesh_triangle_filter(v3(Ps), v3(As), v3(Bs), v3(Pn), v3(An), v3(Bn), k.cos_min_angle, k.cos_max_angle);
      if (f == 0) continue;
      if (kWrite && own >= room) break;
      if (kWrite) {
        // insertion into the slot's own (a, b)-ordered run of the output (it owns two triangles on average)
        const uint32_t na = f == 1 ? a : b, nb = f == 1 ? b : a;
        uint32_t at = own;
        while (at > 0) {
          const uint32_t ea = out[3 * (at - 1) + 1], eb = out[3 * (at - 1) + 2];
          if (ea < na || (ea == na && eb <= nb)) break;
          out[3 * at + 1] = ea; out[3 * at + 2] = eb;
          --at;
        }
        out[3 * own] = p;
        out[3 * at + 1] = na; out[3 * at + 2] = nb;
      }
      ++own;
    }
  }
  if (!kWrite) {
    uint32_t total;
    const uint32_t off = block_exclusive_scan(own, &total);
    if (p < k.n) local_off[p] = off;
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
    distinct = wave_sum(distinct);
    if ((threadIdx.x & 63) == 0 && distinct) atomicAdd(&stat[kStStar], distinct);
  }
}

// One workgroup: exclusive scan of the nb workgroup totals, in place order; the grand total goes to stat[kStTotal].
__global__ void __launch_bounds__(kBlock)
k_mesh_scan(const uint32_t* __restrict__ block_sums, uint32_t nb, uint32_t* __restrict__ block_off, uint32_t* __restrict__ stat) {
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += kBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? block_sums[i] : 0u;
    uint32_t total;
    const uint32_t off = block_exclusive_scan(v, &total);
    if (i < nb) block_off[i] = carry + off;
    carry += total;
    __syncthreads();   // (block_exclusive_scan's LDS row is rewritten by the next trip)
  }
  if (threadIdx.x == 0) stat[kStTotal] = carry;
}

template <typename T>
int grow(T** p, size_t* cap, size_t want) {
  if (want <= *cap) return SMX_OK;
  if (*p) { SMX_HIP(hipFree(*p)); *p = nullptr; }
  *cap = 0;
  const size_t c = want + want / 8 + 1024;
  SMX_HIP(hipMalloc(reinterpret_cast<void**>(p), c * sizeof(T)));
  *cap = c;
  return SMX_OK;
}

}  // namespace

struct MeshWorkspace {
  uint32_t* lists; float* d2; size_t lists_cap, d2_cap;          // [n][K]
  int32_t* counts; float* r2; uint32_t* meta; uint32_t* local_off; size_t counts_cap, r2_cap, meta_cap, local_cap;   // [n]
  uint32_t* rings; size_t rings_cap;                             // [n][16]
  uint32_t* block_sums; uint32_t* block_off; size_t sums_cap, off_cap;
  uint32_t* tri; size_t tri_cap;                                 // [T][3] when the caller's buffer is host memory
  uint32_t* stat;
  hipEvent_t ev[5];
  bool timed;
};

int mesh_workspace_create(MeshWorkspace** out) {
  MeshWorkspace* w = new MeshWorkspace();
  memset(w, 0, sizeof(*w));
  *out = w;
  SMX_HIP(hipMalloc(reinterpret_cast<void**>(&w->stat), kStWords * sizeof(uint32_t)));
  for (int i = 0; i < 5; ++i) SMX_HIP(hipEventCreate(&w->ev[i]));
  return SMX_OK;
}

void mesh_workspace_destroy(MeshWorkspace* w) {
  if (!w) return;
  void* ptrs[] = {w->lists, w->d2, w->counts, w->r2, w->meta, w->local_off, w->rings, w->block_sums, w->block_off, w->tri, w->stat};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  for (int i = 0; i < 5; ++i) if (w->ev[i]) (void)hipEventDestroy(w->ev[i]);
  delete w;
}

int mesh_check_params(const smx_mesh_params& p) {
  SMX_CHECK_ARG(p.max_neighbors >= 1 && p.max_neighbors <= kMeshMaxNeighbors);
  SMX_CHECK_ARG(p.search_radius_factor >= 1.0f && p.search_radius_factor <= 2.0f);
  SMX_CHECK_ARG(p.max_angle_between_normals_deg > 0.0f && p.max_angle_between_normals_deg <= 180.0f);
  SMX_CHECK_ARG(p.min_triangle_angle_deg >= 0.0f && p.max_triangle_angle_deg <= 180.0f &&
                p.min_triangle_angle_deg <= p.max_triangle_angle_deg);
  SMX_CHECK_ARG(p.max_star_degree == kMeshMaxStarDegree);
  return SMX_OK;
}

int mesh_stamp_begin(MeshWorkspace* w, hipStream_t st) {
  w->timed = false;
  SMX_HIP(hipEventRecord(w->ev[0], st));
  return SMX_OK;
}

int mesh_phase_ms(MeshWorkspace* w, float out_ms[4]) {
  for (int i = 0; i < 4; ++i) out_ms[i] = 0.0f;
  if (!w || !w->timed) return SMX_OK;
  for (int i = 0; i < 4; ++i) SMX_HIP(hipEventElapsedTime(&out_ms[i], w->ev[i], w->ev[i + 1]));
  return SMX_OK;
}

int mesh_triangulate(MeshWorkspace* w, hipStream_t st, smx_nn nn, const float4* smooth, size_t smooth_stride,
                     const float4* normal, size_t normal_stride, uint32_t n, const smx_mesh_params& p, uint32_t* triangles,
                     uint32_t capacity, int32_t on_device, uint32_t* n_triangles, smx_mesh_stats* stats) {
  SMX_HIP(hipEventRecord(w->ev[1], st));   // (the index is built)
  *n_triangles = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (n == 0) return SMX_OK;
  const int K = p.max_neighbors;
  const uint32_t nb = (uint32_t)div_up(n, kBlock);
  // (a buffer that has to grow is freed first: the previous call ended with a synchronisation, nothing reads it)
  int rc = grow(&w->lists, &w->lists_cap, (size_t)n * K);
  if (rc == SMX_OK) rc = grow(&w->d2, &w->d2_cap, (size_t)n * K);
  if (rc == SMX_OK) rc = grow(&w->counts, &w->counts_cap, (size_t)n);
  if (rc == SMX_OK) rc = grow(&w->r2, &w->r2_cap, (size_t)n);
  if (rc == SMX_OK) rc = grow(&w->meta, &w->meta_cap, (size_t)n);
  if (rc == SMX_OK) rc = grow(&w->local_off, &w->local_cap, (size_t)n);
  if (rc == SMX_OK) rc = grow(&w->rings, &w->rings_cap, (size_t)n * kMeshMaxStarDegree);
  if (rc == SMX_OK) rc = grow(&w->block_sums, &w->sums_cap, (size_t)nb);
  if (rc == SMX_OK) rc = grow(&w->block_off, &w->off_cap, (size_t)nb);
  if (rc != SMX_OK) return rc;
  MeshK k;
  k.smooth = smooth; k.smooth_stride = smooth_stride; k.normal = normal; k.normal_stride = normal_stride;
  k.n = n; k.K = K;
  const double rad = 3.14159265358979323846 / 180.0;
  k.cos_max_normal = (float)std::cos((double)p.max_angle_between_normals_deg * rad);
  k.cos_min_angle = (float)std::cos((double)p.min_triangle_angle_deg * rad);
  k.cos_max_angle = (float)std::cos((double)p.max_triangle_angle_deg * rad);
  SMX_HIP(hipMemsetAsync(w->stat, 0, kStWords * sizeof(uint32_t), st));
  const unsigned grid = (unsigned)std::min<uint32_t>(nb, 8192u);
  hipLaunchKernelGGL(k_mesh_prepare, dim3(grid), dim3(kBlock), 0, st, k, w->r2, w->stat);
  SMX_LAUNCH_CHECK();
  // (a slot without finite coordinates is not indexed and gets count 0; a merged one was left out of the build)
  rc = smx_nn_query_self(nn, (smx_stream)st, w->r2, p.search_radius_factor * p.search_radius_factor, K, nullptr, 0, w->lists,
                         w->d2, w->counts);
  if (rc != SMX_OK) return rc;
  SMX_HIP(hipEventRecord(w->ev[2], st));
  const unsigned star_grid = (unsigned)std::min<uint32_t>((uint32_t)div_up(n, kWaves), 16384u);
  hipLaunchKernelGGL(k_mesh_star, dim3(star_grid), dim3(kBlock), 0, st, k, w->lists, w->counts, w->rings, w->meta, w->stat);
  SMX_LAUNCH_CHECK();
  SMX_HIP(hipEventRecord(w->ev[3], st));
  hipLaunchKernelGGL(k_mesh_agree<false>, dim3(nb), dim3(kBlock), 0, st, k, w->rings, w->meta, w->local_off, w->block_sums,
                     nullptr, nullptr, 0u, w->stat);
  hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kBlock), 0, st, w->block_sums, nb, w->block_off, w->stat);
  SMX_LAUNCH_CHECK();
  uint32_t h[kStWords];
  SMX_HIP(hipMemcpyAsync(h, w->stat, sizeof(h), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  const uint32_t T = h[kStTotal];
  *n_triangles = T;
  if (stats) {
    stats->n_live = h[kStLive]; stats->n_star_triangles = h[kStStar]; stats->n_triangles = T;
    stats->star_overflow = h[kStOverflow]; stats->truncated_lists = h[kStTruncated];
  }
  if (capacity < T) {
    if (triangles != nullptr || capacity != 0) set_error("triangles holds %u entries, the mesh has %u", capacity, T);
    else set_error("count only: the mesh has %u triangles", T);
    SMX_HIP(hipEventRecord(w->ev[4], st));
    SMX_HIP(hipStreamSynchronize(st));
    w->timed = true;
    return SMX_ERR_INVALID_ARGUMENT;
  }
  if (T > 0) {
    uint32_t* dst = triangles;
    if (!on_device) {
      rc = grow(&w->tri, &w->tri_cap, (size_t)3 * T);
      if (rc != SMX_OK) return rc;
      dst = w->tri;
    }
    hipLaunchKernelGGL(k_mesh_agree<true>, dim3(nb), dim3(kBlock), 0, st, k, w->rings, w->meta, w->local_off, nullptr,
                       w->block_off, dst, T, nullptr);
    SMX_LAUNCH_CHECK();
    if (!on_device) SMX_HIP(hipMemcpyAsync(triangles, dst, (size_t)T * 12, hipMemcpyDeviceToHost, st));
  }
  SMX_HIP(hipEventRecord(w->ev[4], st));
  SMX_HIP(hipStreamSynchronize(st));
  w->timed = true;
  return SMX_OK;
}

}  // namespace smx

extern "C" int smx_mesh_params_default(smx_mesh_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  out->max_angle_between_normals_deg = 90.0f;
  out->min_triangle_angle_deg = 10.0f;
  out->max_triangle_angle_deg = 170.0f;
  out->search_radius_factor = 1.0f;
  out->max_neighbors = smx::kMeshMaxNeighbors;
  out->max_star_degree = smx::kMeshMaxStarDegree;
  return SMX_OK;
}
