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
// smx_recon_triangulate_update adds
//   k_mesh_diff      a lane per slot, twice: <false> compares the slot's seven words bitwise with the kept snapshot, writes
//                    the changed byte and counts the ghosts (snapshot positions of changed slots that were live) per
//                    workgroup; <true> writes the rows of the two index builds, the ghosts at (workgroup offset + local
//                    offset), the state bytes and radii of the reverse test, and the new snapshot
//   k_mesh_worklist  a lane per slot, twice: counts / writes the ascending list of the slots whose star is recomputed
//   k_mesh_star<true>   the star kernel over that list; marks the members of the old and of the new ring in a byte row
//   k_mesh_agree<.., true>   slots with the byte set recount and rewrite, the others reuse their kept counts and copy
//                    their kept run of the previous output
// The arithmetic is in smx_mesh.hpp; nothing here decides a sign by itself.
#include <algorithm>
#include <memory>
#include <cmath>

#include "smx_mesh.hpp"

namespace smx {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
enum : int { kStLive = 0, kStStar, kStOverflow, kStTruncated, kStTotal, kStChanged, kStKept, kStReagreed, kStNoFilter,
             kStWords = 16 };

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

// What the update adds to the kernels' arguments.  kept[p]: bits 0-7 the triangles slot p owns, bits 8-15 the distinct star
// triangles counted at p, bit 16 "p's candidate list came back full".
constexpr uint32_t kKeptFullBit = 1u << 16;
struct MeshU {
  const uint32_t* work; uint32_t n_work;   // ascending slots whose star is recomputed; list row = position in this list
  uint32_t n_prev;                         // slots below it have a kept ring row
  uint8_t* in_a;                           // [n] 1 = owned triangles and star-triangle count are recomputed
  uint32_t* kept;                          // [n]
  const uint32_t* prev_tri; const uint32_t* prev_local; const uint32_t* prev_block;   // the previous output and its offsets
};

// kSubset = false: the slot is the work item (u is not read).  kSubset = true: the slot comes from u.work.
template <bool kSubset>
__global__ void __launch_bounds__(kBlock)
k_mesh_star(MeshK k, const uint32_t* __restrict__ lists, const int32_t* __restrict__ counts, uint32_t* __restrict__ rings,
            uint32_t* __restrict__ meta, uint32_t* __restrict__ stat, MeshU u) {
  __shared__ float sx[kWaves][64], sy[kWaves][64], sq[kWaves][64];
  __shared__ uint32_t s_ring[kWaves][kMeshMaxStarDegree];
  __shared__ uint32_t s_mask[kWaves];
  __shared__ uint8_t s_is_succ[kWaves][64], s_rank[kWaves][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // (every wavefront of the workgroup makes the same number of trips, so that the barriers below are uniform)
  const uint32_t n_items = kSubset ? u.n_work : k.n;
  for (uint32_t base = blockIdx.x * kWaves; base < n_items; base += gridDim.x * kWaves) {
    const uint32_t item = base + w;
    const bool valid = item < n_items;
    const uint32_t p = !kSubset ? item : (valid ? u.work[item] : 0u);
    float4 ps = make_float4(0, 0, 0, 0), pn = make_float4(0, 0, 0, -1.0f);
    int cnt = 0;
    if (valid) {
      ps = k.smooth[(size_t)p * k.smooth_stride];
      pn = k.normal[(size_t)p * k.normal_stride];
      cnt = counts[item];
    }
    const bool live = valid && slot_live(ps, pn);
    cnt = live ? min(max(cnt, 0), k.K) : 0;
    // projection of candidate `lane`
    uint32_t j = kInvalid;
    float x = 0.0f, y = 0.0f, q = -1.0f;
    if (lane < cnt) {
      j = lists[(size_t)item * k.K + lane];
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
      if (lane < kMeshMaxStarDegree) {
        const uint32_t now = overflow ? kInvalid : s_ring[w][lane];
        if (kSubset) {
          // (plain byte stores of 1: every racing store writes the same value)
          if (p < u.n_prev) {
            const uint32_t old = rings[(size_t)p * kMeshMaxStarDegree + lane];
            if (old < k.n) u.in_a[old] = 1;
          }
          if (now < k.n) u.in_a[now] = 1;
        }
        rings[(size_t)p * kMeshMaxStarDegree + lane] = now;
      }
      if (lane == 0) {
        meta[p] = overflow ? kMeshOverflowBit : ((uint32_t)deg | (s_mask[w] << 8));
        if (kSubset) {
          u.in_a[p] = 1;
          u.kept[p] = (live && cnt == k.K) ? kKeptFullBit : 0u;   // (the counts follow in k_mesh_agree: p is in A)
        } else {
          if (overflow) atomicAdd(&stat[kStOverflow], 1u);
          if (live && cnt == k.K) atomicAdd(&stat[kStTruncated], 1u);
        }
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
// kUpdate: only the slots with u.in_a set do that; the others take their two counts from u.kept and, in the write pass, copy
// their run of the previous output (same workgroup, previous offsets) to the new offset.  The statistics that the star
// kernel sums in the full call are summed here from the per-slot values.
template <bool kWrite, bool kUpdate>
__global__ void __launch_bounds__(kBlock)
k_mesh_agree(MeshK k, const uint32_t* __restrict__ rings, const uint32_t* __restrict__ meta, uint32_t* __restrict__ local_off,
             uint32_t* __restrict__ block_sums, const uint32_t* __restrict__ block_off, uint32_t* __restrict__ tri,
             uint32_t total, uint32_t* __restrict__ stat, MeshU u) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool redo = !kUpdate || (p < k.n && u.in_a[p] != 0);
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
  if (redo && deg >= 2 && !(mp & kMeshOverflowBit)) {
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
  if (kUpdate) {
    const uint32_t word = p < k.n ? u.kept[p] : 0u;
    if (p >= k.n) {
    } else if (redo) {
      if (!kWrite) u.kept[p] = (word & kKeptFullBit) | own | (distinct << 8);
    } else {
      own = word & 0xFFu; distinct = (word >> 8) & 0xFFu;
      if (kWrite) {
        // (p is below the kept slot count, so its workgroup had an offset in the previous call)
        const uint32_t* src = u.prev_tri + 3 * (size_t)(u.prev_block[blockIdx.x] + u.prev_local[p]);
        const uint32_t m = own < room ? own : room;
        for (uint32_t t = 0; t < 3 * m; ++t) out[t] = src[t];
      }
    }
    if (!kWrite) {
      const uint32_t ov = wave_sum((mp & kMeshOverflowBit) ? 1u : 0u), full = wave_sum((word & kKeptFullBit) ? 1u : 0u);
      const uint32_t keep = wave_sum(redo ? 0u : own), again = wave_sum(redo && p < k.n ? 1u : 0u);
      if ((threadIdx.x & 63) == 0) {
        if (ov) atomicAdd(&stat[kStOverflow], ov);
        if (full) atomicAdd(&stat[kStTruncated], full);
        if (keep) atomicAdd(&stat[kStKept], keep);
        if (again) atomicAdd(&stat[kStReagreed], again);
      }
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

// The diff of smx_recon_triangulate_update: one lane per slot (no grid stride: the workgroup is the scan's unit).
struct MeshDiff {
  uint32_t n_prev;
  float4* snap_s; float4* snap_n;     // [n] the kept seven words: (smooth x, y, z, 0) and (normal x, y, z, RadiusSquared)
  uint8_t* changed;                   // [n]
  float* rows; size_t row_len;        // [3][row_len]: the n current positions (NaN where merged), then the ghosts
  float* reverse_r2; uint8_t* state;  // [row_len] the reverse test's radii (0 unless unchanged and live) and state bytes
  float* r2;                          // [n] RadiusSquared, the row smx_nn_query_self reads on the full path
  uint32_t* near_bits; float inv_h;   // the coarse filter of the reverse test (mesh_coarse_cell); null = not used
};
// (an integer atomic whose result does not depend on the order: the bit is set, whoever sets it)
__device__ __forceinline__ void mark_near(const MeshDiff& d, float x, float y, float z, uint32_t* stat) {
  int ix, iy, iz;
  if (!mesh_coarse_cell(x, y, z, d.inv_h, &ix, &iy, &iz)) { atomicOr(&stat[kStNoFilter], 1u); return; }
  const uint32_t b = mesh_coarse_bit(ix, iy, iz);
  atomicOr(&d.near_bits[b >> 5], 1u << (b & 31u));
}
template <bool kWrite>
__global__ void __launch_bounds__(kBlock)
k_mesh_diff(MeshK k, MeshDiff d, uint32_t* __restrict__ block_sums, const uint32_t* __restrict__ block_off,
            uint32_t* __restrict__ stat) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < k.n;
  float4 s = make_float4(0, 0, 0, 0), nr = make_float4(0, 0, 0, -1.0f), os = s, on = nr;
  if (valid) {
    s = k.smooth[(size_t)i * k.smooth_stride];
    nr = k.normal[(size_t)i * k.normal_stride];
    if (i < d.n_prev) { os = d.snap_s[i]; on = d.snap_n[i]; }
  }
  const float now[7] = {s.x, s.y, s.z, nr.w, nr.x, nr.y, nr.z}, kept[7] = {os.x, os.y, os.z, on.w, on.x, on.y, on.z};
  const bool chg = valid && mesh_slot_changed(i, d.n_prev, now, kept);
  const bool live = valid && slot_live(s, nr);
  const bool ghost = chg && i < d.n_prev && slot_live(os, on);
  uint32_t total;
  const uint32_t off = block_exclusive_scan(ghost ? 1u : 0u, &total);
  if (!kWrite) {
    if (valid) d.changed[i] = chg ? 1 : 0;
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
    const uint32_t nl = wave_sum(live ? 1u : 0u), nc = wave_sum(chg ? 1u : 0u);
    if ((threadIdx.x & 63) == 0) {
      if (nl) atomicAdd(&stat[kStLive], nl);
      if (nc) atomicAdd(&stat[kStChanged], nc);
    }
    return;
  }
  if (!valid) return;
  const float nanv = __builtin_nanf("");
  const bool merged = nr.w < 0.0f;
  d.rows[i] = merged ? nanv : s.x;
  d.rows[d.row_len + i] = merged ? nanv : s.y;
  d.rows[2 * d.row_len + i] = merged ? nanv : s.z;
  d.reverse_r2[i] = (!chg && live) ? nr.w : 0.0f;
  d.state[i] = chg ? 0 : 1;
  d.r2[i] = nr.w;
  if (d.near_bits != nullptr) {
    if (chg && live) mark_near(d, s.x, s.y, s.z, stat);
    if (ghost) mark_near(d, os.x, os.y, os.z, stat);
  }
  if (ghost) {
    const size_t g = (size_t)k.n + block_off[blockIdx.x] + off;
    if (g < d.row_len) {
      d.rows[g] = os.x; d.rows[d.row_len + g] = os.y; d.rows[2 * d.row_len + g] = os.z;
      d.reverse_r2[g] = 0.0f;
      d.state[g] = 0;
    }
  }
  d.snap_s[i] = make_float4(s.x, s.y, s.z, 0.0f);
  d.snap_n[i] = nr;
}

// The rows the reverse test's index is built over: the map's rows and the ghosts, without (NaN) every unchanged slot that
// the coarse filter shows to have no changed point and no ghost in its ball.  A slot that is left out neither queries nor
// is found; its count stays 0.
__global__ void __launch_bounds__(kBlock)
k_mesh_reverse_rows(uint32_t n, size_t row_len, const float* __restrict__ rows, float* __restrict__ out,
                    const uint8_t* __restrict__ changed, const float* __restrict__ reverse_r2, float f2, float inv_h,
                    float max_r2, const uint32_t* __restrict__ near_bits, const uint32_t* __restrict__ stat) {
  const bool filter = stat[kStNoFilter] == 0;
  const float nanv = __builtin_nanf("");
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < row_len; i += (size_t)gridDim.x * kBlock) {
    const float x = rows[i], y = rows[row_len + i], z = rows[2 * row_len + i];
    bool keep = true;
    int ix, iy, iz;
    if (filter && i < n && changed[i] == 0 && f2 * reverse_r2[i] <= max_r2 && mesh_coarse_cell(x, y, z, inv_h, &ix, &iy, &iz)) {
      keep = false;
      for (int c = 0; c < 27 && !keep; ++c) {
        const uint32_t b = mesh_coarse_bit(ix + c % 3 - 1, iy + (c / 3) % 3 - 1, iz + c / 9 - 1);
        keep = (near_bits[b >> 5] >> (b & 31u)) & 1u;
      }
    }
    out[i] = keep ? x : nanv; out[row_len + i] = keep ? y : nanv; out[2 * row_len + i] = keep ? z : nanv;
  }
}

// D as an ascending slot list: every changed slot, and every slot whose reverse query found a changed point or a ghost
// (only an unchanged live slot asks with a radius, and unchanged points are skipped by their state byte).
template <bool kWrite>
__global__ void __launch_bounds__(kBlock)
k_mesh_worklist(uint32_t n, const uint8_t* __restrict__ changed, const int32_t* __restrict__ reverse_count, int32_t all,
                uint32_t* __restrict__ block_sums, const uint32_t* __restrict__ block_off, uint32_t* __restrict__ work) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool in_d = i < n && (all || changed[i] != 0 || (reverse_count != nullptr && reverse_count[i] > 0));
  uint32_t total;
  const uint32_t off = block_exclusive_scan(in_d ? 1u : 0u, &total);
  if (!kWrite) {
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
  } else if (in_d) {
    work[block_off[blockIdx.x] + off] = i;
  }
}

}  // namespace

// The kept state of smx_recon_triangulate_update and its workspace (rings and meta of the workspace belong to it while
// `have` is set).  mesh_update_reset puts a fresh one in its place.
struct MeshUpdate {
  bool have = false;
  bool utimed = false;
  uint32_t n_prev = 0, t_prev = 0;
  smx_mesh_params prm{};
  smx_mesh_stats last_stats{};
  int cur = 0;                                                   // which of the double-buffered sets holds the kept output
  DevBuf<float4> snap_s, snap_n; DevBuf<uint32_t> kept;          // [n]
  DevBuf<uint32_t> utri[2], ulocal[2], ublock[2];
  DevBuf<uint8_t> changed, in_a; DevBuf<uint32_t> work;          // [n]
  DevBuf<float> rows, reverse_r2; DevBuf<uint8_t> state;         // [n + ghosts]
  DevBuf<float> reverse_rows; DevBuf<uint32_t> near_bits;        // the coarse filter
  DevBuf<uint32_t> reverse_idx; DevBuf<float> reverse_d2; DevBuf<int32_t> reverse_count;   // [n + ghosts]
  smx_nn reverse_nn = nullptr;                                   // the index of the reverse test
};

// (created value-initialised: events null, buffers empty)
struct MeshWorkspace {
  DevBuf<uint32_t> lists; DevBuf<float> d2;                      // [n][K]
  DevBuf<int32_t> counts; DevBuf<float> r2; DevBuf<uint32_t> meta, local_off;   // [n]
  DevBuf<uint32_t> rings;                                        // [n][16]
  DevBuf<uint32_t> block_sums, block_off;
  DevBuf<uint32_t> tri;                                          // [T][3] when the caller's buffer is host memory
  DevBuf<uint32_t> stat;
  hipEvent_t ev[5];
  bool timed;
  MeshUpdate upd;
  hipEvent_t uev[8];
  ~MeshWorkspace() {
    (void)mesh_update_reset(this);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : uev) if (e) (void)hipEventDestroy(e);
  }
};

int mesh_workspace_create(MeshWorkspace** out) {
  std::unique_ptr<MeshWorkspace> w(new MeshWorkspace());
  SMX_CALL(w->stat.alloc(kStWords, false));
  for (int i = 0; i < 5; ++i) SMX_HIP(hipEventCreate(&w->ev[i]));
  for (int i = 0; i < 8; ++i) SMX_HIP(hipEventCreate(&w->uev[i]));
  *out = w.release();   // (a complete workspace or none)
  return SMX_OK;
}

void mesh_workspace_destroy(MeshWorkspace* w) { delete w; }

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
  w->upd.have = false;                     // (the rings are shared with smx_recon_triangulate_update: its kept state is gone)
  *n_triangles = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (n == 0) return SMX_OK;
  const int K = p.max_neighbors;
  const uint32_t nb = (uint32_t)div_up(n, kBlock);
  // (a buffer that has to grow is freed first: the previous call ended with a synchronisation, nothing reads it)
  SMX_CALL(w->lists.reserve((size_t)n * K));
  SMX_CALL(w->d2.reserve((size_t)n * K));
  SMX_CALL(w->counts.reserve((size_t)n));
  SMX_CALL(w->r2.reserve((size_t)n));
  SMX_CALL(w->meta.reserve((size_t)n));
  SMX_CALL(w->local_off.reserve((size_t)n));
  SMX_CALL(w->rings.reserve((size_t)n * kMeshMaxStarDegree));
  SMX_CALL(w->block_sums.reserve((size_t)nb));
  SMX_CALL(w->block_off.reserve((size_t)nb));
  int rc = SMX_OK;
  MeshK k;
  k.smooth = smooth; k.smooth_stride = smooth_stride; k.normal = normal; k.normal_stride = normal_stride;
  k.n = n; k.K = K;
  const double rad = 3.14159265358979323846 / 180.0;
  k.cos_max_normal = (float)std::cos((double)p.max_angle_between_normals_deg * rad);
  k.cos_min_angle = (float)std::cos((double)p.min_triangle_angle_deg * rad);
  k.cos_max_angle = (float)std::cos((double)p.max_triangle_angle_deg * rad);
  SMX_HIP(hipMemsetAsync(w->stat.get(), 0, kStWords * sizeof(uint32_t), st));
  const unsigned grid = (unsigned)std::min<uint32_t>(nb, 8192u);
  hipLaunchKernelGGL(k_mesh_prepare, dim3(grid), dim3(kBlock), 0, st, k, w->r2.get(), w->stat.get());
  SMX_LAUNCH_CHECK();
  // (a slot without finite coordinates is not indexed and gets count 0; a merged one was left out of the build)
  rc = smx_nn_query_self(nn, (smx_stream)st, w->r2.get(), p.search_radius_factor * p.search_radius_factor, K, nullptr, 0, w->lists.get(),
                         w->d2.get(), w->counts.get());
  if (rc != SMX_OK) return rc;
  SMX_HIP(hipEventRecord(w->ev[2], st));
  const unsigned star_grid = (unsigned)std::min<uint32_t>((uint32_t)div_up(n, kWaves), 16384u);
  hipLaunchKernelGGL(k_mesh_star<false>, dim3(star_grid), dim3(kBlock), 0, st, k, w->lists.get(), w->counts.get(), w->rings.get(), w->meta.get(), w->stat.get(),
                     MeshU{});
  SMX_LAUNCH_CHECK();
  SMX_HIP(hipEventRecord(w->ev[3], st));
  hipLaunchKernelGGL((k_mesh_agree<false, false>), dim3(nb), dim3(kBlock), 0, st, k, w->rings.get(), w->meta.get(), w->local_off.get(),
                     w->block_sums.get(), nullptr, nullptr, 0u, w->stat.get(), MeshU{});
  hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kBlock), 0, st, w->block_sums.get(), nb, w->block_off.get(), w->stat.get());
  SMX_LAUNCH_CHECK();
  uint32_t h[kStWords];
  SMX_HIP(hipMemcpyAsync(h, w->stat.get(), sizeof(h), hipMemcpyDeviceToHost, st));
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
      SMX_CALL(w->tri.reserve((size_t)3 * T));
      dst = w->tri.get();
    }
    hipLaunchKernelGGL((k_mesh_agree<true, false>), dim3(nb), dim3(kBlock), 0, st, k, w->rings.get(), w->meta.get(), w->local_off.get(), nullptr,
                       w->block_off.get(), dst, T, nullptr, MeshU{});
    SMX_LAUNCH_CHECK();
    if (!on_device) SMX_HIP(hipMemcpyAsync(triangles, dst, (size_t)T * 12, hipMemcpyDeviceToHost, st));
  }
  SMX_HIP(hipEventRecord(w->ev[4], st));
  SMX_HIP(hipStreamSynchronize(st));
  w->timed = true;
  return SMX_OK;
}

int mesh_update_reset(MeshWorkspace* w) {
  if (!w) return SMX_OK;
  if (w->upd.reverse_nn) (void)smx_nn_destroy(w->upd.reverse_nn);
  w->upd = MeshUpdate{};
  return SMX_OK;
}

int mesh_update_phase_ms(MeshWorkspace* w, float out_ms[6]) {
  for (int i = 0; i < 6; ++i) out_ms[i] = 0.0f;
  if (!w || !w->upd.utimed) return SMX_OK;
  float d[7];
  for (int i = 0; i < 7; ++i) SMX_HIP(hipEventElapsedTime(&d[i], w->uev[i], w->uev[i + 1]));
  // stamps: diff | reverse index build | reverse query and work list | index build over the map | lists | stars | agreement
  out_ms[0] = d[0]; out_ms[1] = d[1] + d[3]; out_ms[2] = d[2]; out_ms[3] = d[4]; out_ms[4] = d[5]; out_ms[5] = d[6];
  return SMX_OK;
}

namespace {
bool same_params(const smx_mesh_params& a, const smx_mesh_params& b) {
  return a.max_angle_between_normals_deg == b.max_angle_between_normals_deg && a.min_triangle_angle_deg == b.min_triangle_angle_deg &&
         a.max_triangle_angle_deg == b.max_triangle_angle_deg && a.search_radius_factor == b.search_radius_factor &&
         a.max_neighbors == b.max_neighbors && a.max_star_degree == b.max_star_degree;
}
}  // namespace

int mesh_triangulate_update(MeshWorkspace* w, int device, hipStream_t st, smx_nn nn, float cell_size, const float4* smooth,
                            size_t smooth_stride, const float4* normal, size_t normal_stride, uint32_t n,
                            const smx_mesh_params& p, float full_above_fraction, MeshSubsetLists lists, void* lists_ctx,
                            uint32_t* triangles, uint32_t capacity, int32_t on_device, uint32_t* n_triangles,
                            smx_mesh_stats* stats, smx_mesh_update_stats* update_stats) {
  MeshUpdate& up = w->upd;
  up.utimed = false;
  SMX_HIP(hipEventRecord(w->uev[0], st));
  *n_triangles = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  smx_mesh_update_stats us;
  memset(&us, 0, sizeof(us));
  us.mode = !up.have ? 1u : !same_params(p, up.prm) ? 2u : n < up.n_prev ? 3u : 0u;
  if (update_stats) *update_stats = us;
  if (n == 0) {
    up.have = false;
    return smx_nn_build(nn, (smx_stream)st, nullptr, nullptr, nullptr, 0, cell_size, 1);
  }
  const float fraction = full_above_fraction < 0.0f ? kMeshUpdateDefaultFullAboveFraction : full_above_fraction;
  const uint32_t n_prev = us.mode == 0 ? up.n_prev : 0u;  // (the full path: every slot is changed, nothing was live)
  const int K = p.max_neighbors;
  const uint32_t nb = (uint32_t)div_up(n, kBlock);
  const int nw = up.cur ^ 1;                               // the set this call writes
  up.have = false;                                         // (until this call has gone through)
  SMX_CALL(w->rings.reserve_keep((size_t)n * kMeshMaxStarDegree, (size_t)n_prev * kMeshMaxStarDegree, st));
  SMX_CALL(w->meta.reserve_keep((size_t)n, (size_t)n_prev, st));
  SMX_CALL(up.kept.reserve_keep((size_t)n, (size_t)n_prev, st));
  SMX_CALL(up.snap_s.reserve_keep((size_t)n, (size_t)n_prev, st));
  SMX_CALL(up.snap_n.reserve_keep((size_t)n, (size_t)n_prev, st));
  SMX_CALL(w->r2.reserve((size_t)n));
  SMX_CALL(up.changed.reserve((size_t)n));
  SMX_CALL(up.in_a.reserve((size_t)n));
  SMX_CALL(up.work.reserve((size_t)n));
  SMX_CALL(w->block_sums.reserve((size_t)nb));
  SMX_CALL(w->block_off.reserve((size_t)nb));
  SMX_CALL(up.ulocal[nw].reserve((size_t)n));
  SMX_CALL(up.ublock[nw].reserve((size_t)nb));
  int rc = SMX_OK;
  MeshK k;
  k.smooth = smooth; k.smooth_stride = smooth_stride; k.normal = normal; k.normal_stride = normal_stride;
  k.n = n; k.K = K;
  const double rad = 3.14159265358979323846 / 180.0;
  k.cos_max_normal = (float)std::cos((double)p.max_angle_between_normals_deg * rad);
  k.cos_min_angle = (float)std::cos((double)p.min_triangle_angle_deg * rad);
  k.cos_max_angle = (float)std::cos((double)p.max_triangle_angle_deg * rad);
  const float f2 = p.search_radius_factor * p.search_radius_factor;
  uint32_t h[kStWords];
  auto read_stat = [&]() -> int {
    SMX_HIP(hipMemcpyAsync(h, w->stat.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    return SMX_OK;
  };

  // ---- diff: changed bytes, ghost count, live count; then the rows, the reverse test's inputs and the new snapshot
  MeshDiff d;
  memset(&d, 0, sizeof(d));
  d.n_prev = n_prev; d.snap_s = up.snap_s.get(); d.snap_n = up.snap_n.get(); d.changed = up.changed.get();
  SMX_HIP(hipMemsetAsync(w->stat.get(), 0, kStWords * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_mesh_diff<false>, dim3(nb), dim3(kBlock), 0, st, k, d, w->block_sums.get(), nullptr, w->stat.get());
  hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kBlock), 0, st, w->block_sums.get(), nb, w->block_off.get(), w->stat.get());
  SMX_LAUNCH_CHECK();
  if ((rc = read_stat()) != SMX_OK) return rc;
  const uint32_t n_live = h[kStLive], n_changed = h[kStChanged], n_ghosts = h[kStTotal];
  const size_t M = (size_t)n + n_ghosts;
  SMX_CALL(up.rows.reserve(3 * M));
  SMX_CALL(up.reverse_r2.reserve(M));
  SMX_CALL(up.state.reserve(M));
  d.rows = up.rows.get(); d.row_len = M; d.reverse_r2 = up.reverse_r2.get(); d.state = up.state.get(); d.r2 = w->r2.get();
  const bool reverse = us.mode == 0 && n_changed > 0;
  constexpr size_t kNearWords = (size_t)1 << (kMeshNearBitsLog2 - 5);
  if (reverse) {
    if (!up.near_bits.get()) SMX_CALL(up.near_bits.alloc(kNearWords, false));
    SMX_HIP(hipMemsetAsync(up.near_bits.get(), 0, kNearWords * sizeof(uint32_t), st));
    d.near_bits = up.near_bits.get(); d.inv_h = 1.0f / cell_size;
  }
  hipLaunchKernelGGL(k_mesh_diff<true>, dim3(nb), dim3(kBlock), 0, st, k, d, nullptr, w->block_off.get(), w->stat.get());
  SMX_LAUNCH_CHECK();
  SMX_HIP(hipEventRecord(w->uev[1], st));
  us.n_changed = n_changed;

  // ---- nothing changed: the kept array is the answer
  if (us.mode == 0 && n_changed == 0) {
    for (int e = 2; e <= 3; ++e) SMX_HIP(hipEventRecord(w->uev[e], st));
    rc = smx_nn_build(nn, (smx_stream)st, up.rows.get(), up.rows.get() + M, up.rows.get() + 2 * M, n, cell_size, 1);
    if (rc != SMX_OK) return rc;
    for (int e = 4; e <= 6; ++e) SMX_HIP(hipEventRecord(w->uev[e], st));
    const uint32_t T = up.t_prev;
    us.n_kept_triangles = T;
    *n_triangles = T;
    if (stats) *stats = up.last_stats;
    if (update_stats) *update_stats = us;
    up.have = true;
    int out_rc = SMX_OK;
    if (capacity < T) {
      set_error("triangles holds %u entries, the mesh has %u", capacity, T);
      out_rc = SMX_ERR_INVALID_ARGUMENT;
    } else if (T > 0) {
      SMX_HIP(hipMemcpyAsync(triangles, up.utri[up.cur].get(), (size_t)T * 12, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    }
    SMX_HIP(hipEventRecord(w->uev[7], st));
    SMX_HIP(hipStreamSynchronize(st));
    up.utimed = true;
    return out_rc;
  }

  // ---- reverse test: which unchanged live slots have a changed point, or the kept position of one, in their ball
  if (us.mode == 0) {
    if (!up.reverse_nn) { rc = smx_nn_create(device, &up.reverse_nn); if (rc != SMX_OK) return rc; }
    SMX_CALL(up.reverse_idx.reserve(M));
    SMX_CALL(up.reverse_d2.reserve(M));
    SMX_CALL(up.reverse_count.reserve(M));
    SMX_CALL(up.reverse_rows.reserve(3 * M));
    // (a ball of radius <= cell_size / 2 stays within the 27 cells around its centre's)
    hipLaunchKernelGGL(k_mesh_reverse_rows, dim3((unsigned)std::min<size_t>((size_t)div_up((long long)M, kBlock), 8192)), dim3(kBlock), 0, st,
                       n, M, up.rows.get(), up.reverse_rows.get(), up.changed.get(), up.reverse_r2.get(), f2, 1.0f / cell_size, 0.25f * cell_size * cell_size,
                       up.near_bits.get(), w->stat.get());
    SMX_LAUNCH_CHECK();
    rc = smx_nn_build(up.reverse_nn, (smx_stream)st, up.reverse_rows.get(), up.reverse_rows.get() + M, up.reverse_rows.get() + 2 * M, (uint32_t)M,
                      cell_size, 1);
    if (rc != SMX_OK) return rc;
  }
  SMX_HIP(hipEventRecord(w->uev[2], st));
  auto count_work = [&](int32_t all) -> int {
    hipLaunchKernelGGL(k_mesh_worklist<false>, dim3(nb), dim3(kBlock), 0, st, n, up.changed.get(), all ? nullptr : up.reverse_count.get(), all,
                       w->block_sums.get(), nullptr, nullptr);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kBlock), 0, st, w->block_sums.get(), nb, w->block_off.get(), w->stat.get());
    SMX_LAUNCH_CHECK();
    return read_stat();
  };
  uint32_t n_work = n;
  if (us.mode == 0) {
    // (the index holds the changed points and the ghosts for this query: unchanged points carry state 1 and are skipped)
    rc = smx_nn_query_self(up.reverse_nn, (smx_stream)st, up.reverse_r2.get(), f2, 1, up.state.get(), 1, up.reverse_idx.get(), up.reverse_d2.get(),
                           up.reverse_count.get());
    if (rc != SMX_OK) return rc;
    if ((rc = count_work(0)) != SMX_OK) return rc;
    n_work = h[kStTotal];
    us.n_dirty = n_work;
    if ((double)n_work > (double)fraction * (double)n) us.mode = 4;
  }
  const bool incremental = us.mode == 0;
  if (!incremental) {
    if ((rc = count_work(1)) != SMX_OK) return rc;
    n_work = n;
    if (us.mode != 4) us.n_dirty = n;
  }
  hipLaunchKernelGGL(k_mesh_worklist<true>, dim3(nb), dim3(kBlock), 0, st, n, up.changed.get(), incremental ? up.reverse_count.get() : nullptr,
                     incremental ? 0 : 1, nullptr, w->block_off.get(), up.work.get());
  SMX_LAUNCH_CHECK();
  SMX_HIP(hipEventRecord(w->uev[3], st));

  // ---- the caller's index over the map, and the candidate lists of the work list
  rc = smx_nn_build(nn, (smx_stream)st, up.rows.get(), up.rows.get() + M, up.rows.get() + 2 * M, n, cell_size, 1);
  if (rc != SMX_OK) return rc;
  SMX_HIP(hipEventRecord(w->uev[4], st));
  SMX_CALL(w->lists.reserve((size_t)n_work * K));
  SMX_CALL(w->d2.reserve((size_t)n_work * K));
  SMX_CALL(w->counts.reserve((size_t)n_work));
  if (n_work > 0) {
    if (incremental) rc = lists(lists_ctx, st, nn, up.work.get(), n_work, f2, K, w->lists.get(), w->d2.get(), w->counts.get());
    else rc = smx_nn_query_self(nn, (smx_stream)st, w->r2.get(), f2, K, nullptr, 0, w->lists.get(), w->d2.get(), w->counts.get());
    if (rc != SMX_OK) return rc;
  }
  SMX_HIP(hipEventRecord(w->uev[5], st));

  // ---- stars of the work list; A = D + old rings + new rings
  MeshU u;
  memset(&u, 0, sizeof(u));
  u.work = up.work.get(); u.n_work = n_work; u.n_prev = n_prev; u.in_a = up.in_a.get(); u.kept = up.kept.get();
  u.prev_tri = up.utri[up.cur].get(); u.prev_local = up.ulocal[up.cur].get(); u.prev_block = up.ublock[up.cur].get();
  SMX_HIP(hipMemsetAsync(up.in_a.get(), 0, (size_t)n, st));
  if (n_work > 0) {
    const unsigned star_grid = (unsigned)std::min<uint32_t>((uint32_t)div_up(n_work, kWaves), 16384u);
    hipLaunchKernelGGL(k_mesh_star<true>, dim3(star_grid), dim3(kBlock), 0, st, k, w->lists.get(), w->counts.get(), w->rings.get(), w->meta.get(), w->stat.get(), u);
    SMX_LAUNCH_CHECK();
  }
  SMX_HIP(hipEventRecord(w->uev[6], st));

  // ---- agreement: count, scan, write into the other output set
  SMX_HIP(hipMemsetAsync(w->stat.get(), 0, kStWords * sizeof(uint32_t), st));
  hipLaunchKernelGGL((k_mesh_agree<false, true>), dim3(nb), dim3(kBlock), 0, st, k, w->rings.get(), w->meta.get(), up.ulocal[nw].get(), w->block_sums.get(),
                     nullptr, nullptr, 0u, w->stat.get(), u);
  hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kBlock), 0, st, w->block_sums.get(), nb, up.ublock[nw].get(), w->stat.get());
  SMX_LAUNCH_CHECK();
  if ((rc = read_stat()) != SMX_OK) return rc;
  const uint32_t T = h[kStTotal];
  smx_mesh_stats ms;
  ms.n_live = n_live; ms.n_star_triangles = h[kStStar]; ms.n_triangles = T;
  ms.star_overflow = h[kStOverflow]; ms.truncated_lists = h[kStTruncated];
  us.n_reagreed = h[kStReagreed]; us.n_kept_triangles = h[kStKept];
  SMX_CALL(up.utri[nw].reserve((size_t)3 * T));
  if (T > 0) {
    hipLaunchKernelGGL((k_mesh_agree<true, true>), dim3(nb), dim3(kBlock), 0, st, k, w->rings.get(), w->meta.get(), up.ulocal[nw].get(), nullptr,
                       up.ublock[nw].get(), up.utri[nw].get(), T, nullptr, u);
    SMX_LAUNCH_CHECK();
  }
  // (the state has advanced, whether or not the caller's buffer holds the result)
  up.cur = nw; up.n_prev = n; up.t_prev = T; up.prm = p; up.last_stats = ms; up.have = true;
  *n_triangles = T;
  if (stats) *stats = ms;
  if (update_stats) *update_stats = us;
  int out_rc = SMX_OK;
  if (capacity < T) {
    if (triangles != nullptr || capacity != 0) set_error("triangles holds %u entries, the mesh has %u", capacity, T);
    else set_error("count only: the mesh has %u triangles", T);
    out_rc = SMX_ERR_INVALID_ARGUMENT;
  } else if (T > 0) {
    SMX_HIP(hipMemcpyAsync(triangles, up.utri[nw].get(), (size_t)T * 12, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  }
  SMX_HIP(hipEventRecord(w->uev[7], st));
  SMX_HIP(hipStreamSynchronize(st));
  up.utimed = true;
  return out_rc;
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
