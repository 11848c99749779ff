// smx_recon_map.hip -- map services of the surfel reconstruction object: the entry points that are called outside the
// frame loop and only read or rewrite the finished map, and their gfx950 kernels.
//
// TransferAllToCPU, ExportVertices, the viewer buffers, the splat render (and the front end it shares with the mesh
// render, smx_render.hpp), the glue of smx_recon_triangulate / _triangulate_update, the mesher's candidate lists and
// triangle tests, map compaction, the loop-closure deformation and the debug row upload / download.  Tracking, decimation
// and the mesh render are with their kernels (smx_track.hip, smx_decimate.hip, smx_mesh_raster.hip).  The frame loop itself
// (Integrate, Regularize, their kernels, the timing readers, and the changed-surfel delta whose marks those kernels write)
// is smx_recon.hip; what they all share is smx_recon_state.hpp.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "smx_recon_state.hpp"
#include "smx_mesh.hpp"
#include "smx_splat.hpp"

using namespace smx;

namespace {

// ---- map compaction (smx_recon_compact; not in the reference) -----------------------------------------------------
// Count / scan / map / scatter over kSeg-slot segments, four slots per lane as in the delta kernels (smx_recon.hip): per-segment
// counts of the kept slots (!(RadiusSquared < 0): the merge mark), enqueue_segment_scan over the counts, old_to_new for every
// old slot, then one scatter launch per record group.  A stable compaction IN PLACE races (a workgroup would overwrite
// source records that an earlier workgroup has not read yet), so each group is scattered into the staging buffer
// (16 B per old slot) and copied back before the next group is scattered: peak extra memory 16 B + 4 B per slot.
// The G record (rows 11-13, the parked next smooth position) is scratch within a call and does not move.
__global__ void __launch_bounds__(kBlock)
k_compact_count(Surfels S, uint32_t n, uint8_t* __restrict__ keep4, uint32_t* __restrict__ seg_count) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t lane_id = blockIdx.x * kBlock + threadIdx.x, i0 = lane_id * 4;
  uint32_t bits = 0;
  if (i0 < n) {   // (i0 + 3 < pitch: the group arrays are padded to a multiple of 64 slots)
    const float r0 = S.f(kRadiusSq, i0), r1 = S.f(kRadiusSq, i0 + 1), r2 = S.f(kRadiusSq, i0 + 2), r3 = S.f(kRadiusSq, i0 + 3);
    bits = (!(r0 < 0) ? 1u : 0u) | ((i0 + 1 < n && !(r1 < 0)) ? 2u : 0u) | ((i0 + 2 < n && !(r2 < 0)) ? 4u : 0u) |
           ((i0 + 3 < n && !(r3 < 0)) ? 8u : 0u);
    keep4[lane_id] = (uint8_t)bits;
  }
  uint32_t total;
  (void)block_excl_scan((uint32_t)__popc(bits), wave_tot, total);
  if (threadIdx.x == 0) seg_count[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kBlock)
k_compact_map(const uint8_t* __restrict__ keep4, const uint32_t* __restrict__ seg_offset, uint32_t n, uint32_t* __restrict__ map) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t lane_id = blockIdx.x * kBlock + threadIdx.x, i0 = lane_id * 4;
  const uint32_t bits = i0 < n ? keep4[lane_id] : 0u;
  uint32_t seg_total;
  uint32_t off = seg_offset[blockIdx.x] + block_excl_scan((uint32_t)__popc(bits), wave_tot, seg_total);
  if (i0 >= n) return;
  uint32_t m[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = (bits & (1u << j)) ? off++ : kInvalid;
  *reinterpret_cast<uint4*>(&map[i0]) = make_uint4(m[0], m[1], m[2], m[3]);   // (map has pitch entries)
}
// One record group: the records of the kept slots go to out[old_to_new[i]] (one 16-byte load and store per record).
// Lane l of a segment's workgroup takes the slots l, l + 256, l + 512, l + 768 of it, so that every load instruction of
// a wavefront reads 1 KB in one piece and the stores (ascending destinations with gaps) stay nearly contiguous.  (Four
// consecutive slots per lane, as in the count kernel, left every instruction 64 B-strided: 75 us per group at C2.)
// kLinks (group T): the four links go through the map as well, and the links that compaction drops are counted --
// those of removed slots and those of kept slots into removed ones.
template <bool kLinks>
__global__ void __launch_bounds__(kBlock)
k_compact_scatter(Surfels S, int g, const uint32_t* __restrict__ map, uint32_t n, float4* __restrict__ out,
                  uint32_t* __restrict__ dropped) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t base = blockIdx.x * kSeg + threadIdx.x;
  uint32_t dst[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dst[j] = base + j * kBlock < n ? map[base + j * kBlock] : kInvalid;
  uint32_t drop = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t i = base + j * kBlock;
    if (i >= n) continue;
    if (kLinks) {
      const uint4 t = *reinterpret_cast<const uint4*>(S.group(kGroupT, i));
      uint32_t nb[4] = {t.x, t.y, t.z, t.w};
      if (dst[j] == kInvalid) {
#pragma unroll
        for (int q = 0; q < 4; ++q) drop += nb[q] != kInvalid ? 1u : 0u;
        continue;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (nb[q] == kInvalid) continue;
        nb[q] = nb[q] < n ? map[nb[q]] : kInvalid;   // (the map is read-mostly and small: these gathers hit the caches)
        drop += nb[q] == kInvalid ? 1u : 0u;
      }
      out[dst[j]] = make_float4(__uint_as_float(nb[0]), __uint_as_float(nb[1]), __uint_as_float(nb[2]), __uint_as_float(nb[3]));
    } else if (dst[j] != kInvalid) {
      out[dst[j]] = *S.group(g, i);
    }
  }
  if (kLinks) {
    uint32_t total;
    (void)block_excl_scan(drop, wave_tot, total);
    if (threadIdx.x == 0 && total) atomicAdd(dropped, total);
  }
}
__global__ void __launch_bounds__(kBlock)
k_compact_copy(Surfels S, int g, const float4* __restrict__ src, const uint32_t* __restrict__ total) {
  const uint32_t K = *total;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < K; i += gridDim.x * kBlock) *S.group(g, i) = src[i];
}
// The device state after compaction: the new count, no merged slots, every other counter reset (as a state upload does).
__global__ void k_compact_finish(DevState* st, const uint32_t* __restrict__ total) {
  if (threadIdx.x != 0) return;
  DevState h;
  memset(&h, 0, sizeof(h));
  h.surfel_count = *total;
  *st = h;
}
// Delta tracking: every slot of the compacted map counts as changed, the marks at and above the new count are cleared.
__global__ void __launch_bounds__(kBlock)
k_compact_dirty(uint8_t* __restrict__ dirty8, uint32_t bytes, const uint32_t* __restrict__ total) {
  const uint32_t K = *total;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < bytes; i += gridDim.x * kBlock) dirty8[i] = i < K ? 1 : 0;
}

// Boundary conversion between the grouped records and the reference's row layout: out[k][i] = row rows[k] of
// slot i (pack) and back (unpack).  Rows without storage read as 0.
struct RowList { int n; int rows[kRows]; };
RowList all_rows() {   // (every row in the reference's order: the debug upload and download)
  RowList rl;
  rl.n = kRows;
  for (int k = 0; k < kRows; ++k) rl.rows[k] = k;
  return rl;
}
__global__ void __launch_bounds__(kBlock)
k_pack_rows(Surfels S, RowList rl, float* __restrict__ out, uint32_t count) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock)
    for (int k = 0; k < rl.n; ++k) {
      const int g = row_group(rl.rows[k]), sub = row_sub(rl.rows[k]);
      out[(size_t)k * count + i] = g < 0 ? 0.0f : S.base[S.quad(g, i) * 4 + sub];
    }
}
__global__ void __launch_bounds__(kBlock)
k_unpack_rows(Surfels S, RowList rl, const float* __restrict__ in, uint32_t count) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock)
    for (int k = 0; k < rl.n; ++k) {
      const int g = row_group(rl.rows[k]), sub = row_sub(rl.rows[k]);
      if (g >= 0) S.base[S.quad(g, i) * 4 + sub] = in[(size_t)k * count + i];
    }
}

// ExportVerticesCUDAKernel, kernels.cu:2412-2433
__global__ void __launch_bounds__(kBlock)
k_export(Surfels S, float* __restrict__ pos, uint8_t* __restrict__ col, const DevState* st) {
  const uint32_t N = st->surfel_count;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
    const bool merged = S.f(kRadiusSq, i) < 0;
    const float nanv = __builtin_nanf("");
    pos[3 * (size_t)i + 0] = merged ? nanv : S.f(kSmoothX, i);
    pos[3 * (size_t)i + 1] = merged ? nanv : S.f(kSmoothY, i);
    pos[3 * (size_t)i + 2] = merged ? nanv : S.f(kSmoothZ, i);
    const uint32_t c = S.u(kColor, i);
    col[3 * (size_t)i + 0] = (uint8_t)(c & 255u);
    col[3 * (size_t)i + 1] = (uint8_t)((c >> 8) & 255u);
    col[3 * (size_t)i + 2] = (uint8_t)((c >> 16) & 255u);
  }
}

// ---- viewer buffers (UpdateVisualizationBuffers) and headless rendering (smx_recon_render) ----
// (VisColor and vis_color, shared with the mesh rasteriser: smx_recon_state.hpp)

// The three fill kernels of UpdateVisualizationBuffers (kernels.cu:278-351, 434-449, 498-514) in one pass over the
// slots; each buffer stops at its own capacity.  (The reference writes vertex components one float at a time; one
// 16-byte record per slot here, 32 for the neighbour pairs.)
__global__ void __launch_bounds__(kBlock)
k_vis_fill(Surfels S, VisColor vc, uint32_t latest_triangulated, uint32_t latest_mesh_count,
           float4* __restrict__ vtx, uint32_t vtx_cap, uint4* __restrict__ nbr, uint32_t nbr_cap,
           float2* __restrict__ nvb, uint32_t nvb_cap, const DevState* st) {
  const uint32_t N = min(st->surfel_count, max(vtx ? vtx_cap : 0u, max(nbr ? nbr_cap : 0u, nvb ? nvb_cap : 0u)));
  const float nanv = __builtin_nanf("");
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
    const float4 s = *S.group(kGroupS, i);
    if (vtx && i < vtx_cap) {
      const bool output_vertex = S.u(kCreationStamp, i) <= latest_triangulated || i >= latest_mesh_count;
      vtx[i] = make_float4(output_vertex ? s.x : nanv, s.y, s.z, __uint_as_float(vis_color(S, i, vc)));
    }
    if (nbr && i < nbr_cap) {
      const uint4 t = *reinterpret_cast<const uint4*>(S.group(kGroupT, i));
      nbr[2 * (size_t)i + 0] = make_uint4(i, t.x == kInvalid ? i : t.x, i, t.y == kInvalid ? i : t.y);
      nbr[2 * (size_t)i + 1] = make_uint4(i, t.z == kInvalid ? i : t.z, i, t.w == kInvalid ? i : t.w);
    }
    if (nvb && i < nvb_cap) {
      const float4 n = *S.group(kGroupN, i);
      const float radius = sqrtf(n.w);
      nvb[3 * (size_t)i + 0] = make_float2(s.x, s.y);
      nvb[3 * (size_t)i + 1] = make_float2(s.z, s.x + radius * n.x);
      nvb[3 * (size_t)i + 2] = make_float2(s.y + radius * n.y, s.z + radius * n.z);
    }
  }
}

// z-test: the smaller (depth bits, slot) key wins; a plain load first, so that a hidden splat costs no atomic
__device__ __forceinline__ void render_zmin(unsigned long long* p, unsigned long long key) {
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

// One thread per live slot: project, find the candidate pixel rectangle, z-test every covered pixel.  Streams the S
// and N records (32 B per slot).  (No segment culling: the segment boxes bound the raw positions, not the smooth ones.)
// The geometry is evaluated in double precision: neighbouring discs of one surface meet a pixel's ray at depths only
// 1e-6 apart, and a float evaluation would order them by its rounding errors; the key then holds the depth as a float.
__global__ void __launch_bounds__(kBlock)
k_render_splat(Surfels S, SplatCam rc, unsigned long long* __restrict__ zbuf, const DevState* st) {
  const uint32_t N = st->surfel_count;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
    const float4 nr = *S.group(kGroupN, i);
    if (!sp_live(nr.w)) continue;                        // merged
    const float4 sp = *S.group(kGroupS, i);
    const double cz = sp_depth(rc, sp.x, sp.y, sp.z);
    if (!sp_in_range(rc, cz)) continue;
    SplatSlot s;
    if (!sp_project(rc, sp.x, sp.y, sp.z, cz, &s)) continue;   // (far outside any image)
    sp_extent(rc, nr.w, &s);
    sp_rect(rc, &s);
    if (rc.mode == SMX_SPLAT_SQUARE) {
      const unsigned long long key = sp_key(cz, i);
      for (int y = s.y0; y <= s.y1; ++y)
        for (int x = s.x0; x <= s.x1; ++x) render_zmin(&zbuf[(size_t)y * rc.W + x], key);
    } else {
      const SplatDisc d = sp_disc(rc, s, nr.x, nr.y, nr.z);
      for (int y = s.y0; y <= s.y1; ++y) {
        const double dy = sp_ray_y(rc, y);
        for (int x = s.x0; x <= s.x1; ++x) {
          const double dx = sp_ray_x(rc, x);
          const double n_dot_d = sp_n_dot_d(d, dx, dy);
          if (sp_edge_on(n_dot_d)) continue;
          const double t = sp_plane_depth(d, n_dot_d);
          if (!sp_in_front(rc, t)) continue;
          if (sp_within_disc(s, d, t, dx, dy)) render_zmin(&zbuf[(size_t)y * rc.W + x], sp_key(t, i));
        }
      }
    }
  }
}

// One thread per pixel: decode the key, gather only the winner's records.
__global__ void __launch_bounds__(kBlock)
k_render_resolve(Surfels S, SplatCam rc, VisColor vc, const unsigned long long* __restrict__ zbuf,
                 Img<float> depth, Img<uint32_t> index, Img<float4> normal, Img<uint32_t> color) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= rc.W || y >= rc.H) return;
  const unsigned long long key = zbuf[(size_t)y * rc.W + x];
  const bool empty = sp_key_empty(key);
  const uint32_t slot = sp_key_slot(key);
  if (depth.address) depth(y, x) = sp_key_depth(key);
  if (index.address) index(y, x) = slot;
  if (normal.address) {
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!empty) {
      const float4 nr = *S.group(kGroupN, slot);
      float n[3];
      sp_rotate_normal(rc.Lf, nr.x, nr.y, nr.z, n);
      o = make_float4(n[0], n[1], n[2], 0.0f);
    }
    normal(y, x) = o;
  }
  if (color.address) color(y, x) = empty ? 0u : ((vis_color(S, slot, vc) & 0x00FFFFFFu) | 0xFF000000u);
}

// Candidate lists for the mesher: the rows the neighbour index is built from (smooth position,
// NaN for merged slots so that the index leaves them out) and the per-query (position, radius^2) of a list of slots.
__global__ void __launch_bounds__(kBlock)
k_index_rows(Surfels S, float* __restrict__ out, uint32_t count) {
  const float nanv = __builtin_nanf("");
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
    const float4 s = *S.group(kGroupS, i);
    const bool merged = S.f(kRadiusSq, i) < 0;
    out[i] = merged ? nanv : s.x;
    out[(size_t)count + i] = merged ? nanv : s.y;
    out[(size_t)2 * count + i] = merged ? nanv : s.z;
  }
}
__global__ void __launch_bounds__(kBlock)
k_candidate_queries(Surfels S, const uint32_t* __restrict__ slots, uint32_t nq, const DevState* st,
                    float radius_factor_sq, float* __restrict__ q /* [4][nq]: x, y, z, r^2 */) {
  const uint32_t N = st->surfel_count;
  for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < nq; k += gridDim.x * kBlock) {
    const uint32_t i = slots[k];
    float4 s = make_float4(0, 0, 0, 0);
    float r2 = -1.0f;  // out of range or merged: an empty ball
    if (i < N) {
      s = *S.group(kGroupS, i);
      const float rs = S.f(kRadiusSq, i);
      if (!(rs < 0)) r2 = radius_factor_sq * rs;  // surfel_meshing.cc:359-360
    }
    q[k] = s.x; q[(size_t)nq + k] = s.y; q[(size_t)2 * nq + k] = s.z; q[(size_t)3 * nq + k] = r2;
  }
}

// The per-triangle tests of SurfelMeshing::CheckRemeshing (APP/surfel_meshing.cc:590-650) over the device-resident
// map: one thread per triangle, three (S, N) record gathers.  Flag bits: see smx.h.
__global__ void __launch_bounds__(kBlock)
k_check_triangles(Surfels S, const uint32_t* __restrict__ tri, uint32_t n_tri, const DevState* st,
                  float factor_sq, uint8_t* __restrict__ flags) {
  const uint32_t N = st->surfel_count;
  for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t < n_tri; t += gridDim.x * kBlock) {
    const uint32_t v[3] = {tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2]};
    if (v[0] >= N || v[1] >= N || v[2] >= N) { flags[t] = 16; continue; }
    Vec3 p[3], nrm[3];
    float maxsq[3];
    uint32_t f = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 s = *S.group(kGroupS, v[k]);
      const float4 n = *S.group(kGroupN, v[k]);
      p[k] = Vec3{s.x, s.y, s.z};
      nrm[k] = Vec3{n.x, n.y, n.z};
      maxsq[k] = factor_sq * n.w;   // :556-557, 593-596
      if (n.w < 0) f |= 16u;        // :559
    }
    float e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int b = (k + 1) % 3;
      const float dx = p[b].x - p[k].x, dy = p[b].y - p[k].y, dz = p[b].z - p[k].z;
      e[k] = dx * dx + dy * dy + dz * dz;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // :605-617
      const int b = (k + 1) % 3, c = (k + 2) % 3;
      if (e[k] > maxsq[k] && e[k] > maxsq[b] && (e[b] > maxsq[c] || e[c] > maxsq[c])) f |= 1u;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // :632-635, pivot k
      const int r = (k + 1) % 3, l = (k + 2) % 3;
      const float rx = p[r].x - p[k].x, ry = p[r].y - p[k].y, rz = p[r].z - p[k].z;
      const float lx = p[l].x - p[k].x, ly = p[l].y - p[k].y, lz = p[l].z - p[k].z;
      const float cx = ry * lz - rz * ly, cy = rz * lx - rx * lz, cz = rx * ly - ry * lx;
      const float d0 = cx * nrm[k].x + cy * nrm[k].y + cz * nrm[k].z;
      const float d1 = cx * nrm[r].x + cy * nrm[r].y + cz * nrm[r].z;
      const float d2 = cx * nrm[l].x + cy * nrm[l].y + cz * nrm[l].z;
      if (d0 <= 0 && d1 <= 0 && d2 <= 0) f |= (2u << k);
    }
    flags[t] = (uint8_t)f;
  }
}

// The loop-closure hook the reference describes but does not ship (README.md:152-176, main.cc:1194-1200): a rigid
// correction per creation frame.  Streams the C records (creation stamp); only moved slots touch P, S, N.
__global__ void __launch_bounds__(kBlock)
k_deform_by_creation_frame(Surfels S, const float* __restrict__ frame_T, uint32_t n_frames,
                           const uint8_t* __restrict__ reactivate, uint32_t frame_index, uint8_t* __restrict__ dirty8,
                           const DevState* st) {
  const uint32_t N = st->surfel_count;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
    const uint32_t c = S.u(kCreationStamp, i);
    if (c >= n_frames) continue;
    float4 nr = *S.group(kGroupN, i);
    if (nr.w < 0) continue;  // merged
    Mat34 T;
#pragma unroll
    for (int k = 0; k < 12; ++k) T.m[k] = frame_T[12 * (size_t)c + k];
    float4 pr = *S.group(kGroupP, i);
    float4 sr = *S.group(kGroupS, i);
    const Vec3 p = {pr.x, pr.y, pr.z};
    const Vec3 q = mul(T, p);
    const float ox = q.x - p.x, oy = q.y - p.y, oz = q.z - p.z;  // README.md:160-165: one offset for both positions
    const Vec3 nn = rotate(T, Vec3{nr.x, nr.y, nr.z});            // README.md:166-168
    const bool restamp = reactivate != nullptr && reactivate[c] && __float_as_uint(pr.w) != frame_index;
    // a correction that leaves the slot as it is (identity rows) is not a change for the delta hand-off
    if (ox == 0 && oy == 0 && oz == 0 && nn.x == nr.x && nn.y == nr.y && nn.z == nr.z && !restamp) continue;
    pr.x = p.x + ox; pr.y = p.y + oy; pr.z = p.z + oz;
    sr.x = sr.x + ox; sr.y = sr.y + oy; sr.z = sr.z + oz;
    nr.x = nn.x; nr.y = nn.y; nr.z = nn.z;
    if (restamp) pr.w = __uint_as_float(frame_index);             // README.md:172-174
    *S.group(kGroupP, i) = pr;
    *S.group(kGroupS, i) = sr;
    *S.group(kGroupN, i) = nr;
    if (dirty8) dirty8[i] = 1;
  }
}

// A temporary device buffer of one call: freed on every way out of the function, behind a synchronisation of the
// stream whose work uses it.
template <typename T>
struct DevTemp {
  hipStream_t st;
  DevBuf<T> buf;   // (freed after the destructor's body)
  explicit DevTemp(hipStream_t st_) : st(st_) {}
  ~DevTemp() { if (buf.get()) (void)hipStreamSynchronize(st); }
  int alloc(size_t count) { return buf.alloc(count, false); }
  T* get() const { return buf.get(); }
};

}  // namespace

// The regulariser's accumulators and the merge marks, as a state upload leaves them.
int smx::reset_accumulators(smx_recon r, hipStream_t st) {
  SMX_HIP(hipMemsetAsync(r->grad_acc, 0, 2 * r->S.pitch * sizeof(long long), st));
  SMX_HIP(hipMemsetAsync(r->fb.count, 0, (size_t)r->nsegB * kCountStride * sizeof(uint32_t), st));
  SMX_HIP(hipMemsetAsync(r->merge_flag, 0, r->S.pitch, st));
  return SMX_OK;
}

// After slots were rewritten, moved or added behind the frame loop's back (compaction, a map merge).
// Derived state: everything a state upload resets (smx_recon_debug_upload_surfels), and the state an upload of the
// same slots never had to care about, because these calls change WHICH SLOT a byte belongs to:
//  * both copies of the double-buffered flag table: zeroed, the current one rebuilt from the records, and copied
//    into the other (pass A of the next call reads the current copy; the other one is relied on through seg_streak);
//  * seg_streak = 0: a streak >= 2 means "the copy written two calls ago already holds this segment's bytes";
//  * hot_epoch = this call's epoch: every group counts as hot for the next calls (a group that looks hot only costs
//    gathers; the hold-off of invalidate_derived keeps pass B unfiltered for two calls in any case, after which
//    every mark it reads has been written after the call);
//  * seg_targets = all groups: a superset of the groups a segment's links point into, which is all the skip test
//    of pass B needs (the first unfiltered pass rebuilds the bitmaps).
// The boxes and visible lists are dropped by invalidate_derived (count 0 = no box: no segment is culled before it
// has been read again, and reading a segment resets its streak).
int smx::reset_derived_after_rewrite(smx_recon r, hipStream_t st) {
  SMX_CALL(reset_accumulators(r, st));
  SMX_HIP(hipMemsetAsync(r->flags_buf[0], 0, (size_t)r->nsegB * kSegB, st));
  SMX_HIP(hipMemsetAsync(r->flags_buf[1], 0, (size_t)r->nsegB * kSegB, st));
  SMX_HIP(hipMemsetAsync(r->L.seg_streak, 0, (size_t)r->nseg, st));
  SMX_HIP(hipMemsetAsync(r->L.hot_epoch, (int)(r->L.epoch & 255u), (size_t)r->L.n_hot_groups + 64, st));
  SMX_HIP(hipMemsetAsync(r->L.seg_targets, 0xFF, (size_t)r->nsegB * kBlockB * sizeof(uint16_t), st));
  SMX_CALL(invalidate_derived(r, st));   // (rebuilds the current flag table)
  uint8_t* other_flags = (r->L.flags8 == r->flags_buf[0]) ? r->flags_buf[1] : r->flags_buf[0];
  SMX_HIP(hipMemcpyAsync(other_flags, r->L.flags8, (size_t)r->nsegB * kSegB, hipMemcpyDeviceToDevice, st));
  return SMX_OK;
}

// ---- the render front end (smx_render.hpp) ----
int smx::render_begin(smx_recon r, hipStream_t st, size_t px, bool caller_grows) {
  SMX_CALL(join_regularizer(r, st));
  RenderWork& w = r->render;
  if (w.zbuf.capacity() < px || caller_grows) {
    if (w.mark.busy()) SMX_HIP(hipDeviceSynchronize());
    w.mark.clear();
    if (w.zbuf.capacity() < px) SMX_CALL(w.zbuf.alloc(px, false));
  }
  return w.mark.wait(st);
}
int smx::render_end(smx_recon r, hipStream_t st) { return r->render.mark.record(st); }

extern "C" {

int smx_recon_transfer_all_to_cpu(smx_recon r, smx_stream s, uint32_t frame_index, smx_surfel_buffers_cpu* buf) {
  SMX_CHECK_ARG(r != nullptr && buf != nullptr);
  SMX_ON_DEVICE(r->device);
  SMX_CALL(join_regularizer(r, (hipStream_t)s));
  hipStream_t st = (hipStream_t)s;
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  buf->frame_index = frame_index;  // cc:345-346
  buf->surfel_count = n;
  if (n == 0) return SMX_OK;
  const size_t bytes = (size_t)n * 4;
  // the 8 rows are packed out of the grouped records into a row-layout staging buffer, then copied row by row
  SMX_CALL(acquire_staging(r, st, (size_t)8 * n));
  RowList rl;
  rl.n = 8;
  const int want[8] = {kSmoothX, kSmoothY, kSmoothZ, kRadiusSq, kNormalX, kNormalY, kNormalZ, kLastUpdateStamp};
  for (int k = 0; k < 8; ++k) rl.rows[k] = want[k];
  hipLaunchKernelGGL(k_pack_rows, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, rl, r->staging.buf.get(), n);
  SMX_LAUNCH_CHECK();
  struct { int row; void* dst; } rows[8] = {
      {kSmoothX, buf->surfel_x_buffer}, {kSmoothY, buf->surfel_y_buffer}, {kSmoothZ, buf->surfel_z_buffer},
      {kRadiusSq, buf->surfel_radius_squared_buffer},
      {kNormalX, buf->surfel_normal_x_buffer}, {kNormalY, buf->surfel_normal_y_buffer}, {kNormalZ, buf->surfel_normal_z_buffer},
      {kLastUpdateStamp, buf->surfel_last_update_stamp_buffer}};  // cc:348-358
  int k = 0;
  for (auto& q : rows) {
    SMX_CHECK_ARG(q.dst != nullptr);
    SMX_HIP(hipMemcpyAsync(q.dst, r->staging.buf.get() + (size_t)k * n, bytes, hipMemcpyDeviceToHost, st));
    ++k;
  }
  return release_staging(r, st);  // (the copies are still in flight: the caller synchronises, main.cc:1266-1267)
}

int smx_recon_export_vertices(smx_recon r, smx_stream s, const smx_buffer_desc* position_buffer,
                              const smx_buffer_desc* color_buffer) {
  SMX_CHECK_ARG(r && position_buffer && color_buffer);
  SMX_ON_DEVICE(r->device);
  SMX_CALL(join_regularizer(r, (hipStream_t)s));
  hipLaunchKernelGGL(k_export, dim3(r->grid_surfels), dim3(kBlock), 0, (hipStream_t)s, r->S,
                     (float*)position_buffer->address, (uint8_t*)color_buffer->address, r->st);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int smx_recon_update_visualization_buffers(smx_recon r, smx_stream s, uint32_t frame_index,
    uint32_t latest_triangulated_frame_index, uint32_t latest_mesh_surfel_count,
    int32_t surfel_integration_active_window_size, int32_t flags,
    float* vertex_buffer, uint32_t vertex_capacity,
    uint32_t* neighbor_index_buffer, uint32_t neighbor_capacity,
    float* normal_vertex_buffer, uint32_t normal_capacity) {
  SMX_CHECK_ARG(r != nullptr && (flags & ~15) == 0);
  // (one 16-byte record per slot for the vertex and neighbour buffers, 8-byte stores for the normal vertices)
  SMX_CHECK_ARG(((uintptr_t)vertex_buffer & 15u) == 0 && ((uintptr_t)neighbor_index_buffer & 15u) == 0 &&
                ((uintptr_t)normal_vertex_buffer & 7u) == 0);
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  const uint32_t vc_ = vertex_buffer ? vertex_capacity : 0u, nc_ = neighbor_index_buffer ? neighbor_capacity : 0u;
  const uint32_t nvc_ = normal_vertex_buffer ? normal_capacity : 0u;
  if (vc_ == 0 && nc_ == 0 && nvc_ == 0) return SMX_OK;
  SMX_CALL(join_regularizer(r, st));
  VisColor vc;
  vc.frame = frame_index; vc.window = surfel_integration_active_window_size; vc.flags = flags;
  hipLaunchKernelGGL(k_vis_fill, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, vc, latest_triangulated_frame_index,
                     latest_mesh_surfel_count, vc_ ? reinterpret_cast<float4*>(vertex_buffer) : nullptr, vc_,
                     nc_ ? reinterpret_cast<uint4*>(neighbor_index_buffer) : nullptr, nc_,
                     nvc_ ? reinterpret_cast<float2*>(normal_vertex_buffer) : nullptr, nvc_, r->st);
  SMX_LAUNCH_CHECK();
  return SMX_OK;
}

int smx_recon_render(smx_recon r, smx_stream s, const smx_render_params* p, const smx_buffer_desc* depth,
                     const smx_buffer_desc* index, const smx_buffer_desc* normal, const smx_buffer_desc* color) {
  SMX_CHECK_ARG(r != nullptr && p != nullptr);
  SMX_CALL(check_view(*p));
  SMX_CHECK_ARG(p->splat_mode == SMX_SPLAT_SQUARE || p->splat_mode == SMX_SPLAT_DISC);
  // (a splat's pixel rectangle is bounded by these: at most (2 x 1024 + 1)^2 pixels for one thread)
  SMX_CHECK_ARG(p->splat_half_extent_in_pixels >= 0 && p->splat_half_extent_in_pixels <= 1024);
  SMX_CHECK_ARG(p->max_splat_extent_in_pixels > 0 && p->max_splat_extent_in_pixels <= 1024);
  SMX_CHECK_ARG(std::isfinite(p->disc_radius_factor) && p->disc_radius_factor > 0);
  const int W = p->width, H = p->height;
  SMX_CHECK_ARG(image_desc_ok_or_null(depth, W, H, 4) && image_desc_ok_or_null(index, W, H, 4) &&
                image_desc_ok_or_null(normal, W, H, 16) && image_desc_ok_or_null(color, W, H, 4));
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  const size_t px = (size_t)W * H;
  SMX_CALL(render_begin(r, st, px));
  unsigned long long* zbuf = r->render.zbuf.get();
  SplatCam rc;
  sp_make_cam(*p, &rc);   // (float fields widened to double)
  VisColor vc;
  vc.frame = p->frame_index; vc.window = p->surfel_integration_active_window_size; vc.flags = p->color_flags;
  SMX_HIP(hipMemsetAsync(zbuf, 0xFF, px * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_render_splat, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, rc, zbuf, r->st);
  hipLaunchKernelGGL(k_render_resolve, dim3(div_up(W, 64), div_up(H, 4)), dim3(kBlock), 0, st, r->S, rc, vc, zbuf,
                     img_or_null<float>(depth), img_or_null<uint32_t>(index), img_or_null<float4>(normal), img_or_null<uint32_t>(color));
  SMX_LAUNCH_CHECK();
  return render_end(r, st);
}

int smx_recon_build_neighbor_index(smx_recon r, smx_stream s, smx_nn nn, float cell_size) {
  SMX_CHECK_ARG(r != nullptr && nn != nullptr && cell_size > 0);
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  if (n == 0) return smx_nn_build(nn, s, nullptr, nullptr, nullptr, 0, cell_size, 1);
  SMX_CALL(acquire_staging(r, st, (size_t)3 * n));
  hipLaunchKernelGGL(k_index_rows, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, r->staging.buf.get(), n);
  SMX_LAUNCH_CHECK();
  SMX_CALL(smx_nn_build(nn, s, r->staging.buf.get(), r->staging.buf.get() + n, r->staging.buf.get() + (size_t)2 * n, n, cell_size, 1));
  return release_staging(r, st);
}

int smx_recon_neighbor_candidates(smx_recon r, smx_stream s, smx_nn nn, const uint32_t* surfel_indices,
                                  uint32_t n_indices, float radius_factor_squared, int32_t k,
                                  const uint8_t* state, uint8_t skip_mask, int32_t inputs_on_device,
                                  uint32_t* out_idx, float* out_d2, int32_t* out_count, int32_t outputs_on_device) {
  SMX_CHECK_ARG(r != nullptr && nn != nullptr && radius_factor_squared >= 0 && k >= 1 && k <= 64);
  SMX_ON_DEVICE(r->device);
  SMX_CHECK_ARG(n_indices == 0 || (surfel_indices && out_idx && out_d2 && out_count));
  if (n_indices == 0) return SMX_OK;
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  // workspace owned by the object, grown only when a batch is larger than any before it (then, and only then, the
  // device is synchronised: earlier batches may still be reading the old buffers)
  CandidateWork& w = r->candidates;
  if (n_indices > w.slots.capacity()) {
    SMX_HIP(hipDeviceSynchronize());
    w.q.reset(); w.slots.reset();   // (first, so that the old and the new pair never exist together)
    const size_t cap = (size_t)n_indices + n_indices / 8 + 1024;
    SMX_CALL(alloc_all(w.q, 4 * cap, w.slots, cap));
  }
  const uint8_t* dstate = state;
  const uint32_t* dslots = nullptr;
  SMX_CALL(stage_in(w.slots, surfel_indices, n_indices, inputs_on_device != 0, st, &dslots));   // (there is room: no allocation)
  if (!inputs_on_device && state) {
    uint32_t n = 0;
    SMX_CALL(read_surfel_count(r, st, &n));
    if (n > w.state.capacity()) {
      SMX_HIP(hipDeviceSynchronize());
      SMX_CALL(w.state.alloc((size_t)r->S.pitch, false));
    }
    if (n > 0) SMX_HIP(hipMemcpyAsync(w.state.get(), state, n, hipMemcpyHostToDevice, st));
    dstate = w.state.get();
  }
  float* q = w.q.get();
  const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_indices + kBlock - 1) / kBlock, 4096);
  hipLaunchKernelGGL(k_candidate_queries, dim3(blocks), dim3(kBlock), 0, st, r->S, dslots, n_indices, r->st,
                     radius_factor_squared, q);
  SMX_LAUNCH_CHECK();
  // (device inputs and outputs: nothing below allocates or synchronises either)
  return smx_nn_query_batch(nn, s, n_indices, q, q + n_indices, q + (size_t)2 * n_indices, q + (size_t)3 * n_indices, k,
                            dstate, skip_mask, 1, out_idx, out_d2, out_count, outputs_on_device);
}

int smx_recon_check_triangles(smx_recon r, smx_stream s, const uint32_t* triangles, uint32_t n_triangles,
                              float long_edge_total_factor_squared, uint8_t* flags, int32_t on_device) {
  SMX_CHECK_ARG(r != nullptr && (n_triangles == 0 || (triangles && flags)));
  SMX_ON_DEVICE(r->device);
  if (n_triangles == 0) return SMX_OK;
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  DevTemp<uint32_t> dtri(st);
  DevTemp<uint8_t> dflags(st);
  const uint32_t* tri = nullptr;
  SMX_CALL(stage_in(dtri.buf, triangles, (size_t)n_triangles * 3, on_device != 0, st, &tri));
  if (!on_device) SMX_CALL(dflags.alloc(n_triangles));
  const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_triangles + kBlock - 1) / kBlock, 8192);
  hipLaunchKernelGGL(k_check_triangles, dim3(blocks), dim3(kBlock), 0, st, r->S, tri, n_triangles, r->st,
                     long_edge_total_factor_squared, on_device ? flags : dflags.get());
  SMX_LAUNCH_CHECK();
  if (!on_device) {
    SMX_HIP(hipMemcpyAsync(flags, dflags.get(), n_triangles, hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
  }
  return SMX_OK;
}

int smx_recon_triangulate(smx_recon r, smx_stream s, smx_nn nn, float cell_size, const smx_mesh_params* p,
                          uint32_t* triangles, uint32_t capacity, int32_t on_device, uint32_t* n_triangles,
                          smx_mesh_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && nn != nullptr && p != nullptr && n_triangles != nullptr && cell_size > 0);
  SMX_CHECK_ARG(triangles != nullptr || capacity == 0);
  SMX_CALL(mesh_check_params(*p));
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  if (!r->mesh) SMX_CALL(mesh_workspace_create(&r->mesh));
  SMX_CALL(join_regularizer(r, st));
  SMX_CALL(mesh_stamp_begin(r->mesh, st));
  // (the build orders st behind the pipelined regulariser, reads the slot count back and leaves merged slots out)
  SMX_CALL(smx_recon_build_neighbor_index(r, s, nn, cell_size));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  return mesh_triangulate(r->mesh, st, nn, sv.p, sv.stride, nv.p, nv.stride, n, *p, triangles, capacity, on_device, n_triangles,
                          stats);
}

int smx_recon_debug_mesh_timings(smx_recon r, float out_ms[4]) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr);
  SMX_ON_DEVICE(r->device);
  return mesh_phase_ms(r->mesh, out_ms);
}

namespace {
// the candidate lists of a device list of slots, by the route of smx_recon_neighbor_candidates
int mesh_subset_lists(void* ctx, hipStream_t st, smx_nn nn, const uint32_t* slots, uint32_t n_slots, float factor_squared, int K,
                      uint32_t* out_idx, float* out_d2, int32_t* out_count) {
  return smx_recon_neighbor_candidates(static_cast<smx_recon>(ctx), (smx_stream)st, nn, slots, n_slots, factor_squared, K, nullptr,
                                       0, 1, out_idx, out_d2, out_count, 1);
}
}  // namespace

int smx_recon_triangulate_update(smx_recon r, smx_stream s, smx_nn nn, float cell_size, const smx_mesh_params* p,
                                 float full_above_fraction, uint32_t* triangles, uint32_t capacity, int32_t on_device,
                                 uint32_t* n_triangles, smx_mesh_stats* stats, smx_mesh_update_stats* update_stats) {
  SMX_CHECK_ARG(r != nullptr && nn != nullptr && p != nullptr && n_triangles != nullptr && cell_size > 0);
  SMX_CHECK_ARG(triangles != nullptr || capacity == 0);
  SMX_CHECK_ARG(full_above_fraction < 0.0f || full_above_fraction <= 1.0f);
  SMX_CALL(mesh_check_params(*p));
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  if (!r->mesh) SMX_CALL(mesh_workspace_create(&r->mesh));
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  const Surfels::View sv = r->S.view(kGroupS), nv = r->S.view(kGroupN);
  return mesh_triangulate_update(r->mesh, r->device, st, nn, cell_size, sv.p, sv.stride, nv.p, nv.stride, n, *p,
                                 full_above_fraction, mesh_subset_lists, r, triangles, capacity, on_device, n_triangles, stats,
                                 update_stats);
}

int smx_recon_triangulate_reset(smx_recon r) {
  SMX_CHECK_ARG(r != nullptr);
  SMX_ON_DEVICE(r->device);
  SMX_HIP(hipDeviceSynchronize());
  return mesh_update_reset(r->mesh);
}

int smx_recon_debug_mesh_update_timings(smx_recon r, float out_ms[6]) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr);
  SMX_ON_DEVICE(r->device);
  return mesh_update_phase_ms(r->mesh, out_ms);
}

int smx_recon_debug_download_surfels(smx_recon r, smx_stream s, float* rows, uint32_t count) {
  SMX_CHECK_ARG(r != nullptr && rows != nullptr && count <= r->max_surfels);
  SMX_ON_DEVICE(r->device);
  if (count == 0) return SMX_OK;
  SMX_CALL(join_regularizer(r, (hipStream_t)s));
  SMX_CALL(acquire_staging(r, (hipStream_t)s, (size_t)kRows * count));
  hipLaunchKernelGGL(k_pack_rows, dim3(r->grid_surfels), dim3(kBlock), 0, (hipStream_t)s, r->S, all_rows(), r->staging.buf.get(), count);
  SMX_HIP(hipMemcpyAsync(rows, r->staging.buf.get(), (size_t)kRows * count * 4, hipMemcpyDeviceToHost, (hipStream_t)s));
  SMX_HIP(hipStreamSynchronize((hipStream_t)s));
  return SMX_OK;
}

int smx_recon_debug_upload_surfels(smx_recon r, smx_stream s, const float* rows, uint32_t count, uint32_t merge_count) {
  SMX_CHECK_ARG(r != nullptr && count <= r->max_surfels && (rows != nullptr || count == 0));
  SMX_ON_DEVICE(r->device);
  SMX_CALL(join_regularizer(r, (hipStream_t)s));
  hipStream_t st = (hipStream_t)s;
  if (count) {
    SMX_CALL(acquire_staging(r, st, (size_t)kRows * count));
    SMX_HIP(hipMemcpyAsync(r->staging.buf.get(), rows, (size_t)kRows * count * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_unpack_rows, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, all_rows(), r->staging.buf.get(), count);
  }
  DevState h;
  memset(&h, 0, sizeof(h));
  h.surfel_count = count; h.merge_count = merge_count;
  SMX_HIP(hipMemcpyAsync(r->st, &h, sizeof(h), hipMemcpyHostToDevice, st));
  SMX_CALL(reset_accumulators(r, st));
  if (r->L.dirty8) SMX_HIP(hipMemsetAsync(r->L.dirty8, 1, (size_t)r->nseg * kSeg, st));
  SMX_CALL(invalidate_derived(r, st));
  SMX_HIP(hipStreamSynchronize(st));
  return SMX_OK;
}

int smx_recon_compact(smx_recon r, smx_stream s, uint32_t* old_to_new, uint32_t capacity, int32_t on_device,
                      uint32_t* new_size, uint32_t* links_dropped) {
  SMX_CHECK_ARG(r != nullptr);
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t n = 0;
  SMX_CALL(read_surfel_count(r, st, &n));
  if (old_to_new && capacity < n) {   // (nothing has been changed yet)
    set_error("old_to_new holds %u entries, the map has %u slots", capacity, n);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  CompactWork& w = r->compact;
  if (!w.out.get()) SMX_CALL(alloc_all(w.map, r->S.pitch, w.seg, (size_t)r->nseg, w.out, 2));
  SMX_HIP(hipMemsetAsync(w.out.get(), 0, 2 * sizeof(uint32_t), st));
  const dim3 b(kBlock);
  if (n) {
    const int nseg_used = div_up((long long)n, kSeg);
    // (merge_flag -- one byte per slot, reset below -- holds the keep bits: a byte per four slots)
    hipLaunchKernelGGL(k_compact_count, dim3(nseg_used), b, 0, st, r->S, n, r->merge_flag, w.seg.get());
    enqueue_segment_scan(st, w.seg.get(), nseg_used, w.out.get());
    hipLaunchKernelGGL(k_compact_map, dim3(nseg_used), b, 0, st, r->merge_flag, w.seg.get(), n, w.map.get());
    SMX_LAUNCH_CHECK();
    SMX_CALL(acquire_staging(r, st, (size_t)4 * n));
    float4* tmp = reinterpret_cast<float4*>(r->staging.buf.get());
    const int groups[5] = {kGroupP, kGroupS, kGroupN, kGroupC, kGroupT};
    for (int g : groups) {
      if (g == kGroupT) hipLaunchKernelGGL(k_compact_scatter<true>, dim3(nseg_used), b, 0, st, r->S, g, w.map.get(), n, tmp, w.out.get() + 1);
      else hipLaunchKernelGGL(k_compact_scatter<false>, dim3(nseg_used), b, 0, st, r->S, g, w.map.get(), n, tmp, w.out.get() + 1);
      hipLaunchKernelGGL(k_compact_copy, dim3(r->grid_surfels), b, 0, st, r->S, g, tmp, w.out.get());
    }
    SMX_LAUNCH_CHECK();
    SMX_CALL(release_staging(r, st));
  }
  hipLaunchKernelGGL(k_compact_finish, dim3(1), dim3(64), 0, st, r->st, w.out.get());
  if (r->L.dirty8)
    hipLaunchKernelGGL(k_compact_dirty, dim3(r->grid_surfels), b, 0, st, r->L.dirty8, (uint32_t)((size_t)r->nseg * kSeg), w.out.get());
  SMX_CALL(reset_derived_after_rewrite(r, st));
  if (old_to_new && n)
    SMX_HIP(hipMemcpyAsync(old_to_new, w.map.get(), (size_t)n * sizeof(uint32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  uint32_t out[2] = {0, 0};
  SMX_HIP(hipMemcpyAsync(out, w.out.get(), sizeof(out), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  if (new_size) *new_size = out[0];
  if (links_dropped) *links_dropped = out[1];
  return SMX_OK;
}

int smx_recon_deform_by_creation_frame(smx_recon r, smx_stream s, const float* frame_T, uint32_t n_frames,
                                       const uint8_t* reactivate, uint32_t frame_index, int32_t inputs_on_device) {
  SMX_CHECK_ARG(r != nullptr && (n_frames == 0 || frame_T != nullptr));
  SMX_ON_DEVICE(r->device);
  if (n_frames == 0) return SMX_OK;
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  DevTemp<float> dT(st);
  DevTemp<uint8_t> dre(st);
  const float* T = nullptr;
  const uint8_t* re = nullptr;
  SMX_CALL(stage_in(dT.buf, frame_T, (size_t)n_frames * 12, inputs_on_device != 0, st, &T));
  SMX_CALL(stage_in(dre.buf, reactivate, reactivate ? n_frames : 0, inputs_on_device != 0, st, &re));
  hipLaunchKernelGGL(k_deform_by_creation_frame, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, T, n_frames, re, frame_index,
                     r->L.dirty8, r->st);
  SMX_LAUNCH_CHECK();
  // positions and stamps changed behind the work lists, segment boxes and the flag table
  SMX_CALL(invalidate_derived(r, st));
  if (!inputs_on_device) SMX_HIP(hipStreamSynchronize(st));
  return SMX_OK;
}

}  // extern "C"
