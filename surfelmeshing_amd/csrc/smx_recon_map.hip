// smx_recon_map.hip -- map services of the surfel reconstruction object: the entry points that are called outside the
// frame loop and only read or rewrite the finished map, and their gfx950 kernels.
//
// TransferAllToCPU, ExportVertices, the viewer buffers and headless rendering, the glue of smx_recon_track /
// _triangulate / _triangulate_update, the mesher's candidate lists and triangle tests, map compaction, the
// loop-closure deformation and the debug row upload / download.  The frame loop itself (Integrate, Regularize, their
// kernels, the timing readers, and the changed-surfel delta whose marks those kernels write) is smx_recon.hip; what
// the two share is smx_recon_state.hpp.
#include <math.h>
#include <cmath>
#include <string.h>

#include <algorithm>
#include <vector>

#include "smx_recon_state.hpp"
#include "smx_track.hpp"
#include "smx_decimate.hpp"
#include "smx_mesh.hpp"
#include "smx_sort.hpp"

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

struct RenderCtx {
  double L[12];   // camera_T_global (inverted on the host in double precision)
  Mat34 Lf;       // ... rounded to float: the rotation part is exact (a transpose), used for the normal image
  double fx, fy, cx, cy, near_z, far_z;
  double half_extent;   // square mode
  double disc_factor, max_extent, f_max;   // disc mode (f_max = max(fx, fy))
  int W, H, mode;
};

// z-test: the smaller (depth bits, slot) key wins; a plain load first, so that a hidden splat costs no atomic
__device__ __forceinline__ void render_zmin(unsigned long long* p, unsigned long long key) {
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

// One thread per live slot: project, find the candidate pixel rectangle, z-test every covered pixel.  Streams the S
// and N records (32 B per slot).  (No segment culling: the segment boxes bound the raw positions, not the smooth ones.)
// The geometry is evaluated in double precision: neighbouring discs of one surface meet a pixel's ray at depths only
// 1e-6 apart, and a float evaluation would order them by its rounding errors; the key then holds the depth as a float.
__global__ void __launch_bounds__(kBlock)
k_render_splat(Surfels S, RenderCtx rc, unsigned long long* __restrict__ zbuf, const DevState* st) {
  const uint32_t N = st->surfel_count;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
    const float4 nr = *S.group(kGroupN, i);
    if (!(nr.w >= 0.0f)) continue;                       // merged
    const float4 sp = *S.group(kGroupS, i);
    const double* L = rc.L;
    const double px = sp.x, py = sp.y, pz = sp.z;
    const double cz = L[8] * px + L[9] * py + L[10] * pz + L[11];
    if (!(cz > rc.near_z && cz < rc.far_z)) continue;
    const double cx = L[0] * px + L[1] * py + L[2] * pz + L[3], cy = L[4] * px + L[5] * py + L[6] * pz + L[7];
    const double u = rc.fx * cx / cz + rc.cx, v = rc.fy * cy / cz + rc.cy;
    if (!(fabs(u) < 1e8 && fabs(v) < 1e8)) continue;   // (far outside any image; keeps the conversions below defined)
    double e = rc.half_extent, rho = 0.0;
    if (rc.mode == SMX_SPLAT_DISC) {
      rho = rc.disc_factor * sqrt((double)nr.w);
      const double dz = cz - rho;
      e = dz <= rc.near_z ? rc.max_extent : fmin(rc.max_extent, 2.0 * rc.f_max * rho / dz);
    }
    // pixels whose centre x + 1/2 lies within e of u: u - e - 1/2 <= x <= u + e - 1/2 (square mode, h = 0: floor(u))
    const bool point = rc.mode == SMX_SPLAT_SQUARE && e == 0.0;
    const double x0f = point ? floor(u) : ceil(u - e - 0.5), x1f = point ? floor(u) : floor(u + e - 0.5);
    const double y0f = point ? floor(v) : ceil(v - e - 0.5), y1f = point ? floor(v) : floor(v + e - 0.5);
    const int x0 = (int)fmax(x0f, 0.0), x1 = (int)fmin(x1f, (double)(rc.W - 1));
    const int y0 = (int)fmax(y0f, 0.0), y1 = (int)fmin(y1f, (double)(rc.H - 1));
    if (rc.mode == SMX_SPLAT_SQUARE) {
      const unsigned long long key = ((unsigned long long)__float_as_uint((float)cz) << 32) | i;
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) render_zmin(&zbuf[(size_t)y * rc.W + x], key);
    } else {
      const double nx = L[0] * nr.x + L[1] * nr.y + L[2] * nr.z, ny = L[4] * nr.x + L[5] * nr.y + L[6] * nr.z;
      const double nz = L[8] * nr.x + L[9] * nr.y + L[10] * nr.z;
      const double n_dot_c = nx * cx + ny * cy + nz * cz;
      const double rho2 = rho * rho;
      for (int y = y0; y <= y1; ++y) {
        const double dy = ((double)y + 0.5 - rc.cy) / rc.fy;
        for (int x = x0; x <= x1; ++x) {
          const double dx = ((double)x + 0.5 - rc.cx) / rc.fx;
          const double n_dot_d = nx * dx + ny * dy + nz;
          if (fabs(n_dot_d) < 1e-4) continue;
          const double t = n_dot_c / n_dot_d;
          if (!(t > rc.near_z)) continue;
          const double ex = t * dx - cx, ey = t * dy - cy, ez = t - cz;
          if (ex * ex + ey * ey + ez * ez <= rho2)
            render_zmin(&zbuf[(size_t)y * rc.W + x], ((unsigned long long)__float_as_uint((float)t) << 32) | i);
        }
      }
    }
  }
}

// One thread per pixel: decode the key, gather only the winner's records.
__global__ void __launch_bounds__(kBlock)
k_render_resolve(Surfels S, RenderCtx rc, VisColor vc, const unsigned long long* __restrict__ zbuf,
                 Img<float> depth, Img<uint32_t> index, Img<float4> normal, Img<uint32_t> color) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= rc.W || y >= rc.H) return;
  const unsigned long long key = zbuf[(size_t)y * rc.W + x];
  const bool empty = key == ~0ull;
  const uint32_t slot = empty ? kInvalid : (uint32_t)key;
  if (depth.address) depth(y, x) = empty ? 0.0f : __uint_as_float((uint32_t)(key >> 32));
  if (index.address) index(y, x) = slot;
  if (normal.address) {
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!empty) {
      const float4 nr = *S.group(kGroupN, slot);
      const Vec3 n = rotate(rc.Lf, Vec3{nr.x, nr.y, nr.z});
      o = make_float4(n.x, n.y, n.z, 0.0f);
    }
    normal(y, x) = o;
  }
  if (color.address) color(y, x) = empty ? 0u : ((vis_color(S, slot, vc) & 0x00FFFFFFu) | 0xFF000000u);
}

bool render_desc_ok(const smx_buffer_desc* d, const smx_render_params* p, size_t elem) {
  return !d || (d->address && d->width == p->width && d->height == p->height && d->pitch >= (size_t)p->width * elem &&
                d->pitch % elem == 0 && (uintptr_t)d->address % elem == 0);
}
template <typename T>
Img<T> render_img(const smx_buffer_desc* d) {
  if (d) return as_img<T>(d);
  Img<T> i; i.address = nullptr; i.height = 0; i.width = 0; i.pitch = 0;
  return i;
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

// The regulariser's accumulators and the merge marks, as a state upload leaves them.
int reset_accumulators(smx_recon r, hipStream_t st) {
  SMX_HIP(hipMemsetAsync(r->grad_acc, 0, 2 * r->S.pitch * sizeof(long long), st));
  SMX_HIP(hipMemsetAsync(r->fb.count, 0, (size_t)r->nsegB * kCountStride * sizeof(uint32_t), st));
  SMX_HIP(hipMemsetAsync(r->merge_flag, 0, r->S.pitch, st));
  return SMX_OK;
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
  hipLaunchKernelGGL(k_pack_rows, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, rl, r->staging.get(), n);
  SMX_LAUNCH_CHECK();
  struct { int row; void* dst; } rows[8] = {
      {kSmoothX, buf->surfel_x_buffer}, {kSmoothY, buf->surfel_y_buffer}, {kSmoothZ, buf->surfel_z_buffer},
      {kRadiusSq, buf->surfel_radius_squared_buffer},
      {kNormalX, buf->surfel_normal_x_buffer}, {kNormalY, buf->surfel_normal_y_buffer}, {kNormalZ, buf->surfel_normal_z_buffer},
      {kLastUpdateStamp, buf->surfel_last_update_stamp_buffer}};  // cc:348-358
  int k = 0;
  for (auto& q : rows) {
    SMX_CHECK_ARG(q.dst != nullptr);
    SMX_HIP(hipMemcpyAsync(q.dst, r->staging.get() + (size_t)k * n, bytes, hipMemcpyDeviceToHost, st));
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
  SMX_CHECK_ARG(p->width > 0 && p->height > 0 && p->width <= 16384 && p->height <= 16384);
  SMX_CHECK_ARG(std::isfinite(p->fx) && std::isfinite(p->fy) && p->fx > 0 && p->fy > 0 && std::isfinite(p->cx) && std::isfinite(p->cy));
  for (int k = 0; k < 12; ++k) SMX_CHECK_ARG(std::isfinite(p->global_T_camera[k]));
  SMX_CHECK_ARG(std::isfinite(p->near_z) && p->near_z > 0 && p->far_z > p->near_z);
  SMX_CHECK_ARG(p->splat_mode == SMX_SPLAT_SQUARE || p->splat_mode == SMX_SPLAT_DISC);
  // (a splat's pixel rectangle is bounded by these: at most (2 x 1024 + 1)^2 pixels for one thread)
  SMX_CHECK_ARG(p->splat_half_extent_in_pixels >= 0 && p->splat_half_extent_in_pixels <= 1024);
  SMX_CHECK_ARG(p->max_splat_extent_in_pixels > 0 && p->max_splat_extent_in_pixels <= 1024);
  SMX_CHECK_ARG(std::isfinite(p->disc_radius_factor) && p->disc_radius_factor > 0);
  SMX_CHECK_ARG((p->color_flags & ~15) == 0);
  SMX_CHECK_ARG(render_desc_ok(depth, p, 4) && render_desc_ok(index, p, 4) && render_desc_ok(normal, p, 16) &&
                render_desc_ok(color, p, 4));
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  const size_t px = (size_t)p->width * p->height;
  if (r->zbuf.capacity() < px) {
    if (r->zbuf.get()) SMX_HIP(hipDeviceSynchronize());   // (the previous render may still be using the old block)
    r->render_busy = false;
    SMX_CALL(r->zbuf.alloc(px, false));
  }
  if (r->render_busy) SMX_HIP(hipStreamWaitEvent(st, r->ev_render, 0));   // (the previous render's resolve, on any stream)
  RenderCtx rc;
  {
    const float* m = p->global_T_camera;
    for (int i = 0; i < 3; ++i) {   // R^T, -(R^T t)
      for (int k = 0; k < 3; ++k) rc.L[4 * i + k] = m[4 * k + i];
      rc.L[4 * i + 3] = -(rc.L[4 * i + 0] * m[3] + rc.L[4 * i + 1] * m[7] + rc.L[4 * i + 2] * m[11]);
    }
    rc.Lf = se3_inverse(m);
  }
  rc.fx = p->fx; rc.fy = p->fy; rc.cx = p->cx; rc.cy = p->cy; rc.near_z = p->near_z; rc.far_z = p->far_z;
  rc.half_extent = p->splat_half_extent_in_pixels;
  rc.disc_factor = p->disc_radius_factor; rc.max_extent = p->max_splat_extent_in_pixels; rc.f_max = std::max(p->fx, p->fy);  // (float fields widened to double)
  rc.W = p->width; rc.H = p->height; rc.mode = p->splat_mode;
  VisColor vc;
  vc.frame = p->frame_index; vc.window = p->surfel_integration_active_window_size; vc.flags = p->color_flags;
  SMX_HIP(hipMemsetAsync(r->zbuf.get(), 0xFF, px * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_render_splat, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, rc, r->zbuf.get(), r->st);
  hipLaunchKernelGGL(k_render_resolve, dim3(div_up(p->width, 64), div_up(p->height, 4)), dim3(kBlock), 0, st, r->S, rc, vc,
                     r->zbuf.get(), render_img<float>(depth), render_img<uint32_t>(index), render_img<float4>(normal),
                     render_img<uint32_t>(color));
  SMX_LAUNCH_CHECK();
  SMX_HIP(hipEventRecord(r->ev_render, st));
  r->render_busy = true;
  return SMX_OK;
}

// smx_recon_track (q, color, result_rgbd and model_photo_out null) and smx_recon_track_rgbd (p = &q->icp, result =
// &result_rgbd->icp).
static int track_call(smx_recon r, smx_stream s, float depth_scaling, const smx_buffer_desc* depth,
                      const smx_buffer_desc* normals, const float global_T_pred[12], const smx_track_params* params,
                      smx_track_result* result, int32_t result_on_device, const smx_buffer_desc* model_depth_out,
                      const smx_buffer_desc* model_normal_out, const smx_buffer_desc* color,
                      const smx_track_rgbd_params* q, smx_track_rgbd_result* result_rgbd,
                      const smx_buffer_desc* model_photo_out) {
  SMX_CHECK_ARG(r != nullptr && depth != nullptr && normals != nullptr && global_T_pred != nullptr && params != nullptr &&
                result != nullptr);
  const smx_track_params& p = *params;
  SMX_CHECK_ARG(std::isfinite(depth_scaling) && depth_scaling > 0);
  auto img_ok = [&](const smx_buffer_desc* d, size_t elem) {
    return d->address && d->width == r->W && d->height == r->H && d->pitch >= (size_t)r->W * elem && d->pitch % elem == 0 &&
           (uintptr_t)d->address % elem == 0;
  };
  SMX_CHECK_ARG(img_ok(depth, 2) && img_ok(normals, 8));
  SMX_CHECK_ARG(!model_depth_out || img_ok(model_depth_out, 4));
  SMX_CHECK_ARG(!model_normal_out || img_ok(model_normal_out, 16));
  for (int k = 0; k < 12; ++k) SMX_CHECK_ARG(std::isfinite(global_T_pred[k]));
  int levels_used = 0;
  for (int l = 0; l < kTrackLevels; ++l) {
    SMX_CHECK_ARG(p.level_iterations[l] >= 0 && p.level_iterations[l] <= kTrackMaxIterationsPerLevel);
    if (p.level_iterations[l] == 0) continue;
    ++levels_used;
    SMX_CHECK_ARG(p.level_stride[l] == 1 || p.level_stride[l] == 2 || p.level_stride[l] == 4 || p.level_stride[l] == 8);
  }
  SMX_CHECK_ARG(levels_used > 0);
  SMX_CHECK_ARG(std::isfinite(p.max_distance) && p.max_distance > 0);
  SMX_CHECK_ARG(p.max_normal_angle_deg > 0 && p.max_normal_angle_deg <= 180.0f);
  SMX_CHECK_ARG(p.convergence_rotation >= 0 && p.convergence_translation >= 0 && p.min_inliers >= 0);
  SMX_CHECK_ARG(p.min_inlier_fraction >= 0 && p.min_inlier_fraction <= 1 && p.min_pivot_ratio >= 0);
  SMX_CHECK_ARG(std::isfinite(p.near_z) && p.near_z > 0 && p.far_z > p.near_z);
  SMX_CHECK_ARG(std::isfinite(p.disc_radius_factor) && p.disc_radius_factor > 0);
  SMX_CHECK_ARG(p.max_splat_extent_in_pixels > 0 && p.max_splat_extent_in_pixels <= 1024);
  if (q) {
    // (3-byte elements: any pitch that holds a row, as smx_recon_integrate takes the image)
    SMX_CHECK_ARG(color != nullptr && color->address && color->width == r->W && color->height == r->H &&
                  color->pitch >= (size_t)r->W * 3);
    SMX_CHECK_ARG(!model_photo_out || img_ok(model_photo_out, 16));
    SMX_CHECK_ARG(std::isfinite(q->photometric_weight) && q->photometric_weight >= 0);
    SMX_CHECK_ARG(std::isfinite(q->max_intensity_difference) && q->max_intensity_difference > 0);
    SMX_CHECK_ARG(std::isfinite(q->min_gradient) && q->min_gradient >= 0);
    SMX_CHECK_ARG(std::isfinite(q->gradient_max_relative_depth_step) && q->gradient_max_relative_depth_step > 0);
  }
  const bool photo = q && q->photometric_weight != 0.0f;
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  const size_t px = (size_t)r->W * r->H;
  if (!r->trk_state.get()) {   // (all four or none: a call that fails here leaves nothing behind for the next one to trip over)
    DevBuf<float> depth_img; DevBuf<float4> normal_img; DevBuf<double> slabs; DevBuf<TrackDev> state;
    SMX_CALL(depth_img.alloc(px, false));
    SMX_CALL(normal_img.alloc(px, false));
    SMX_CALL(slabs.alloc((size_t)kTrackMaxSlabs * kTrackRgbdSlabStride, false));
    SMX_CALL(state.alloc(1, false));
    r->trk_depth = std::move(depth_img); r->trk_normal = std::move(normal_img);
    r->trk_slabs = std::move(slabs); r->trk_state = std::move(state);
  }
  if (q && !r->trk_photo.get()) {   // (both or none, likewise)
    DevBuf<uint32_t> color_img; DevBuf<float4> photo_img;
    SMX_CALL(color_img.alloc(px, false));
    SMX_CALL(photo_img.alloc(px, false));
    r->trk_color = std::move(color_img); r->trk_photo = std::move(photo_img);
  }
  if (r->track_busy) SMX_HIP(hipStreamWaitEvent(st, r->ev_track, 0));   // (the previous call's kernels, on any stream)
  // the model images: smx_recon_render itself (it orders st behind the pipelined regulariser and the previous render)
  smx_render_params rp;
  memset(&rp, 0, sizeof(rp));
  rp.width = r->W; rp.height = r->H; rp.fx = r->fx; rp.fy = r->fy; rp.cx = r->cx; rp.cy = r->cy;
  for (int k = 0; k < 12; ++k) rp.global_T_camera[k] = global_T_pred[k];
  rp.near_z = p.near_z; rp.far_z = p.far_z; rp.splat_mode = SMX_SPLAT_DISC;
  rp.disc_radius_factor = p.disc_radius_factor; rp.max_splat_extent_in_pixels = p.max_splat_extent_in_pixels;
  rp.surfel_integration_active_window_size = 2147483647;
  smx_buffer_desc dd, nd, cd;
  dd.address = r->trk_depth.get(); dd.height = r->H; dd.width = r->W; dd.pitch = (size_t)r->W * sizeof(float);
  nd.address = r->trk_normal.get(); nd.height = r->H; nd.width = r->W; nd.pitch = (size_t)r->W * sizeof(float4);
  cd.address = r->trk_color.get(); cd.height = r->H; cd.width = r->W; cd.pitch = (size_t)r->W * sizeof(uint32_t);
  SMX_CALL(smx_recon_render(r, s, &rp, &dd, nullptr, &nd, photo ? &cd : nullptr));   // (color_flags 0: the colour row)
  if (model_depth_out)
    SMX_HIP(hipMemcpy2DAsync(model_depth_out->address, model_depth_out->pitch, dd.address, dd.pitch, dd.pitch, (size_t)r->H,
                             hipMemcpyDeviceToDevice, st));
  if (model_normal_out)
    SMX_HIP(hipMemcpy2DAsync(model_normal_out->address, model_normal_out->pitch, nd.address, nd.pitch, nd.pitch, (size_t)r->H,
                             hipMemcpyDeviceToDevice, st));
  TrackBuffers tb;
  tb.model_depth = r->trk_depth.get(); tb.model_normal = r->trk_normal.get(); tb.slabs = r->trk_slabs.get(); tb.state = r->trk_state.get();
  tb.model_color = r->trk_color.get(); tb.model_photo = r->trk_photo.get();
  SMX_CALL(track_enqueue(st, tb, r->W, r->H, r->fx, r->fy, r->cx, r->cy, depth_scaling, depth, normals, global_T_pred, p,
                         result_on_device && !q ? result : nullptr, color, q, result_on_device ? result_rgbd : nullptr));
  if (photo && model_photo_out) {
    const size_t row = (size_t)r->W * sizeof(float4);
    SMX_HIP(hipMemcpy2DAsync(model_photo_out->address, model_photo_out->pitch, r->trk_photo.get(), row, row, (size_t)r->H,
                             hipMemcpyDeviceToDevice, st));
  }
  SMX_HIP(hipEventRecord(r->ev_track, st));
  r->track_busy = true;
  r->track_last_rgbd = q != nullptr;
  if (!result_on_device) {
    const smx_track_rgbd_result* res = &r->trk_state.get()->result;
    if (q) SMX_HIP(hipMemcpyAsync(result_rgbd, res, sizeof(*res), hipMemcpyDeviceToHost, st));
    else SMX_HIP(hipMemcpyAsync(result, &res->icp, sizeof(res->icp), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
  }
  return SMX_OK;
}

int smx_recon_track(smx_recon r, smx_stream s, float depth_scaling, const smx_buffer_desc* depth,
                    const smx_buffer_desc* normals, const float global_T_pred[12], const smx_track_params* params,
                    smx_track_result* result, int32_t result_on_device, const smx_buffer_desc* model_depth_out,
                    const smx_buffer_desc* model_normal_out) {
  return track_call(r, s, depth_scaling, depth, normals, global_T_pred, params, result, result_on_device, model_depth_out,
                    model_normal_out, nullptr, nullptr, nullptr, nullptr);
}

int smx_recon_track_rgbd(smx_recon r, smx_stream s, float depth_scaling, const smx_buffer_desc* depth,
                         const smx_buffer_desc* normals, const smx_buffer_desc* color, const float global_T_pred[12],
                         const smx_track_rgbd_params* params, smx_track_rgbd_result* result, int32_t result_on_device,
                         const smx_buffer_desc* model_depth_out, const smx_buffer_desc* model_normal_out,
                         const smx_buffer_desc* model_photo_out) {
  SMX_CHECK_ARG(params != nullptr);
  return track_call(r, s, depth_scaling, depth, normals, global_T_pred, &params->icp, result ? &result->icp : nullptr,
                    result_on_device, model_depth_out, model_normal_out, color, params, result, model_photo_out);
}

// The records of the last tracking call, the first *count of them (at most kTrackRing) copied into recs.
static int track_records(smx_recon r, smx_stream s, smx_track_rgbd_iteration* recs, int32_t* count) {
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  *count = 0;
  if (!r->trk_state.get() || !r->track_busy) return SMX_OK;
  SMX_HIP(hipStreamWaitEvent(st, r->ev_track, 0));
  int32_t n = 0;
  SMX_HIP(hipMemcpyAsync(&n, &r->trk_state.get()->iterations_run, sizeof(n), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  n = std::max(0, std::min(n, (int32_t)kTrackRing));
  if (n > 0) {
    SMX_HIP(hipMemcpyAsync(recs, r->trk_state.get()->ring, sizeof(smx_track_rgbd_iteration) * (size_t)n, hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
  }
  *count = n;
  return SMX_OK;
}

int smx_recon_debug_track_rgbd_iterations(smx_recon r, smx_stream s, smx_track_rgbd_iteration* records, int32_t capacity,
                                          int32_t* count) {
  SMX_CHECK_ARG(r != nullptr && count != nullptr && capacity >= 0 && (capacity == 0 || records != nullptr));
  *count = 0;
  if (!r->track_last_rgbd) return SMX_OK;
  std::vector<smx_track_rgbd_iteration> recs(kTrackRing);
  SMX_CALL(track_records(r, s, recs.data(), count));
  std::copy_n(recs.begin(), std::min(*count, capacity), records);
  return SMX_OK;
}

// (the same records without their last two sums, which a call without colour leaves 0)
int smx_recon_debug_track_iterations(smx_recon r, smx_stream s, smx_track_iteration* records, int32_t capacity,
                                     int32_t* count) {
  SMX_CHECK_ARG(r != nullptr && count != nullptr && capacity >= 0 && (capacity == 0 || records != nullptr));
  std::vector<smx_track_rgbd_iteration> recs(kTrackRing);
  SMX_CALL(track_records(r, s, recs.data(), count));
  for (int32_t i = 0; i < std::min(*count, capacity); ++i) {
    const smx_track_rgbd_iteration& f = recs[i];
    smx_track_iteration& t = records[i];
    t.level = f.level; t.stride = f.stride; t.status = f.status; t.reserved = f.reserved;
    std::copy_n(f.sums, SMX_TRACK_SUMS, t.sums);
    std::copy_n(f.x, 6, t.x);
  }
  return SMX_OK;
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
  hipLaunchKernelGGL(k_index_rows, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, r->staging.get(), n);
  SMX_LAUNCH_CHECK();
  SMX_CALL(smx_nn_build(nn, s, r->staging.get(), r->staging.get() + n, r->staging.get() + (size_t)2 * n, n, cell_size, 1));
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
  if (n_indices > r->cand_slots.capacity()) {   // (cand_slots is allocated last: its capacity stands for both)
    SMX_HIP(hipDeviceSynchronize());
    r->cand_slots.reset();
    const size_t cap = (size_t)n_indices + n_indices / 8 + 1024;
    SMX_CALL(r->cand_q.alloc(4 * cap, false));
    SMX_CALL(r->cand_slots.alloc(cap, false));
  }
  const uint8_t* dstate = state;
  const uint32_t* dslots = surfel_indices;
  if (!inputs_on_device) {
    SMX_HIP(hipMemcpyAsync(r->cand_slots.get(), surfel_indices, (size_t)n_indices * 4, hipMemcpyHostToDevice, st));
    dslots = r->cand_slots.get();
    if (state) {
      uint32_t n = 0;
      SMX_CALL(read_surfel_count(r, st, &n));
      if (n > r->cand_state.capacity()) {
        SMX_HIP(hipDeviceSynchronize());
        SMX_CALL(r->cand_state.alloc((size_t)r->S.pitch, false));
      }
      if (n > 0) SMX_HIP(hipMemcpyAsync(r->cand_state.get(), state, n, hipMemcpyHostToDevice, st));
      dstate = r->cand_state.get();
    }
  }
  float* q = r->cand_q.get();
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
  if (!on_device) {
    SMX_CALL(dtri.alloc((size_t)n_triangles * 3));
    SMX_CALL(dflags.alloc(n_triangles));
    SMX_HIP(hipMemcpyAsync(dtri.get(), triangles, (size_t)n_triangles * 12, hipMemcpyHostToDevice, st));
  }
  const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n_triangles + kBlock - 1) / kBlock, 8192);
  hipLaunchKernelGGL(k_check_triangles, dim3(blocks), dim3(kBlock), 0, st, r->S, on_device ? triangles : dtri.get(),
                     n_triangles, r->st, long_edge_total_factor_squared, on_device ? flags : dflags.get());
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
  const float4* quads = reinterpret_cast<const float4*>(r->S.base);
  const size_t s0 = r->S.quad(kGroupS, 0), n0 = r->S.quad(kGroupN, 0);
  return mesh_triangulate(r->mesh, st, nn, quads + s0, r->S.quad(kGroupS, 1) - s0, quads + n0, r->S.quad(kGroupN, 1) - n0, n,
                          *p, triangles, capacity, on_device, n_triangles, stats);
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
  const float4* quads = reinterpret_cast<const float4*>(r->S.base);
  const size_t s0 = r->S.quad(kGroupS, 0), n0 = r->S.quad(kGroupN, 0);
  return mesh_triangulate_update(r->mesh, r->device, st, nn, cell_size, quads + s0, r->S.quad(kGroupS, 1) - s0, quads + n0,
                                 r->S.quad(kGroupN, 1) - n0, n, *p, full_above_fraction, mesh_subset_lists, r, triangles,
                                 capacity, on_device, n_triangles, stats, update_stats);
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

// ---- decimation of a triangle array by vertex clustering (include/smx.h; kernels in smx_decimate.hip) ----
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
  if (!r->ev_dec[0]) for (hipEvent_t& e : r->ev_dec) SMX_HIP(hipEventCreate(&e));
  r->dec_phases = 0;
  SMX_HIP(hipEventRecord(r->ev_dec[0], st));
  int phases = 0;
  auto stamp = [&]() -> int { SMX_HIP(hipEventRecord(r->ev_dec[++phases], st)); return SMX_OK; };
  auto finish = [&](int rc) -> int {     // (the stamps are complete before they are published)
    SMX_HIP(hipStreamSynchronize(st));
    r->dec_phases = phases;
    return rc;
  };

  // ---- workspace of the first two phases; the input on the device
  const uint32_t cell_entries = dec_table_size((uint32_t)std::min<unsigned long long>(n, 3ull * n_in));
  const uint32_t dup_entries = dec_table_size(n_in);
  const int nb = div_up(n_in, kDecBlock);
  if (!r->dec_counters.get()) SMX_CALL(r->dec_counters.alloc(kDecWords, false));
  SMX_CALL(r->dec_vmap.reserve(n));
  if (n_in > 0) {
    SMX_CALL(r->dec_cells.reserve((size_t)2 * cell_entries));
    SMX_CALL(r->dec_canon.reserve((size_t)3 * n_in));
    SMX_CALL(r->dec_own.reserve(n_in));
    SMX_CALL(r->dec_dup.reserve(dup_entries));
    SMX_CALL(r->dec_blocks.reserve((size_t)nb));
  }
  const uint32_t* din = triangles_in;
  if (!on_device && n_in > 0) {
    SMX_CALL(r->dec_in.reserve((size_t)3 * n_in));
    SMX_HIP(hipMemcpyAsync(r->dec_in.get(), triangles_in, (size_t)n_in * 12, hipMemcpyHostToDevice, st));
    din = r->dec_in.get();
  }
  uint32_t* cnt = r->dec_counters.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kDecWords * sizeof(uint32_t), st));
  uint32_t h[kDecWords];
  auto read_counters = [&]() -> int {
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    return SMX_OK;
  };

  // ---- clustering: U, the cell table, the vertex map.  (An index out of range marks nothing and is read by nothing.)
  const float inv = 1.0f / cell_size;
  DecMap map;
  const float4* quads = reinterpret_cast<const float4*>(r->S.base);
  const size_t s0 = r->S.quad(kGroupS, 0), n0 = r->S.quad(kGroupN, 0);
  map.smooth = quads + s0; map.smooth_stride = r->S.quad(kGroupS, 1) - s0;
  map.normal = quads + n0; map.normal_stride = r->S.quad(kGroupN, 1) - n0;
  map.n = n;
  DecCell* cells = reinterpret_cast<DecCell*>(r->dec_cells.get());
  DecTri* canon = reinterpret_cast<DecTri*>(r->dec_canon.get());
  SMX_CALL(dec_enqueue_cluster(st, map, din, n_in, cell_size, inv, r->dec_vmap.get(), cells, cell_entries, cnt));
  SMX_CALL(stamp());
  SMX_CALL(read_counters());
  if (h[kDecError] & kDecErrIndex) {
    set_error("triangles_in holds an index >= the %u slots of the map", n);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }
  if (h[kDecError] & kDecErrRange) {
    set_error("cell_size %g is too small for the extent of the map: a cell coordinate is outside [-2^20, 2^20)", (double)cell_size);
    return finish(SMX_ERR_INVALID_ARGUMENT);
  }

  // ---- remap and duplicates; survivors counted and scanned
  SMX_CALL(dec_enqueue_remap(st, din, n_in, r->dec_vmap.get(), canon, r->dec_own.get(), r->dec_dup.get(), dup_entries, cnt));
  SMX_CALL(stamp());
  if (n_in > 0) {
    SMX_CALL(dec_enqueue_count(st, n_in, r->dec_own.get(), r->dec_dup.get(), r->dec_blocks.get()));
    enqueue_segment_scan(st, r->dec_blocks.get(), nb, cnt + kDecTotal);
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
    for (int k = 0; k < 2; ++k) { SMX_CALL(r->dec_keys[k].reserve(T)); SMX_CALL(r->dec_vals[k].reserve(T)); }
    SMX_CALL(r->dec_hist.reserve(radix_sort_workspace_elems(T)));
    SMX_CALL(dec_enqueue_write(st, n_in, r->dec_own.get(), r->dec_dup.get(), r->dec_blocks.get(), canon, bits, r->dec_keys[0].get(),
                               r->dec_vals[0].get()));
    SMX_CALL(stamp());
    int cur = radix_sort(r->dec_keys, r->dec_vals, T, 2 * bits, r->dec_hist.get(), st);
    SMX_LAUNCH_CHECK();
    SMX_CALL(dec_enqueue_keys_p(st, T, r->dec_vals[cur].get(), canon, r->dec_keys[0].get(), r->dec_vals[0].get()));
    cur = radix_sort(r->dec_keys, r->dec_vals, T, bits, r->dec_hist.get(), st);
    SMX_LAUNCH_CHECK();
    uint32_t* dst = triangles_out;
    if (!on_device) {
      SMX_CALL(r->dec_out.reserve((size_t)3 * T));
      dst = r->dec_out.get();
    }
    SMX_CALL(dec_enqueue_emit(st, T, r->dec_vals[cur].get(), canon, dst));
    if (!on_device) SMX_HIP(hipMemcpyAsync(triangles_out, dst, (size_t)T * 12, hipMemcpyDeviceToHost, st));
  } else {
    SMX_CALL(stamp());
  }
  if (vertex_map && n > 0)
    SMX_HIP(hipMemcpyAsync(vertex_map, r->dec_vmap.get(), (size_t)n * sizeof(uint32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  SMX_CALL(stamp());
  return finish(SMX_OK);
}

int smx_recon_debug_decimate_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= SMX_DECIMATE_PHASES);
  SMX_ON_DEVICE(r->device);
  for (int i = 0; i < SMX_DECIMATE_PHASES; ++i) {
    out_ms[i] = 0.0f;
    if (i < r->dec_phases) SMX_HIP(hipEventElapsedTime(&out_ms[i], r->ev_dec[i], r->ev_dec[i + 1]));
  }
  return SMX_OK;
}

int smx_recon_debug_download_surfels(smx_recon r, smx_stream s, float* rows, uint32_t count) {
  SMX_CHECK_ARG(r != nullptr && rows != nullptr && count <= r->max_surfels);
  SMX_ON_DEVICE(r->device);
  if (count == 0) return SMX_OK;
  SMX_CALL(join_regularizer(r, (hipStream_t)s));
  SMX_CALL(acquire_staging(r, (hipStream_t)s, (size_t)kRows * count));
  hipLaunchKernelGGL(k_pack_rows, dim3(r->grid_surfels), dim3(kBlock), 0, (hipStream_t)s, r->S, all_rows(), r->staging.get(), count);
  SMX_HIP(hipMemcpyAsync(rows, r->staging.get(), (size_t)kRows * count * 4, hipMemcpyDeviceToHost, (hipStream_t)s));
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
    SMX_HIP(hipMemcpyAsync(r->staging.get(), rows, (size_t)kRows * count * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_unpack_rows, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S, all_rows(), r->staging.get(), count);
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
  if (!r->cmp_out.get()) {   // (allocated last: it stands for all three)
    SMX_CALL(r->cmp_map.alloc(r->S.pitch, false));
    SMX_CALL(r->cmp_seg.alloc((size_t)r->nseg, false));
    SMX_CALL(r->cmp_out.alloc(2, false));
  }
  SMX_HIP(hipMemsetAsync(r->cmp_out.get(), 0, 2 * sizeof(uint32_t), st));
  const dim3 b(kBlock);
  if (n) {
    const int nseg_used = div_up((long long)n, kSeg);
    // (merge_flag -- one byte per slot, reset below -- holds the keep bits: a byte per four slots)
    hipLaunchKernelGGL(k_compact_count, dim3(nseg_used), b, 0, st, r->S, n, r->merge_flag, r->cmp_seg.get());
    enqueue_segment_scan(st, r->cmp_seg.get(), nseg_used, r->cmp_out.get());
    hipLaunchKernelGGL(k_compact_map, dim3(nseg_used), b, 0, st, r->merge_flag, r->cmp_seg.get(), n, r->cmp_map.get());
    SMX_LAUNCH_CHECK();
    SMX_CALL(acquire_staging(r, st, (size_t)4 * n));
    float4* tmp = reinterpret_cast<float4*>(r->staging.get());
    const int groups[5] = {kGroupP, kGroupS, kGroupN, kGroupC, kGroupT};
    for (int g : groups) {
      if (g == kGroupT) hipLaunchKernelGGL(k_compact_scatter<true>, dim3(nseg_used), b, 0, st, r->S, g, r->cmp_map.get(), n, tmp, r->cmp_out.get() + 1);
      else hipLaunchKernelGGL(k_compact_scatter<false>, dim3(nseg_used), b, 0, st, r->S, g, r->cmp_map.get(), n, tmp, r->cmp_out.get() + 1);
      hipLaunchKernelGGL(k_compact_copy, dim3(r->grid_surfels), b, 0, st, r->S, g, tmp, r->cmp_out.get());
    }
    SMX_LAUNCH_CHECK();
    SMX_CALL(release_staging(r, st));
  }
  // Derived state: everything a state upload resets (smx_recon_debug_upload_surfels), and the state an upload of the
  // same slots never had to care about, because compaction changes WHICH SLOT a byte belongs to:
  //  * both copies of the double-buffered flag table: zeroed, the current one rebuilt from the records, and copied
  //    into the other (pass A of the next call reads the current copy; the other one is relied on through seg_streak);
  //  * seg_streak = 0: a streak >= 2 means "the copy written two calls ago already holds this segment's bytes";
  //  * hot_epoch = this call's epoch: every group counts as hot for the next calls (a group that looks hot only costs
  //    gathers; the hold-off of invalidate_derived keeps pass B unfiltered for two calls in any case, after which
  //    every mark it reads has been written after the compaction);
  //  * seg_targets = all groups: a superset of the groups a segment's links point into, which is all the skip test
  //    of pass B needs (the first unfiltered pass rebuilds the bitmaps).
  // The boxes and visible lists are dropped by invalidate_derived (count 0 = no box: no segment is culled before it
  // has been read again, and reading a segment resets its streak).
  hipLaunchKernelGGL(k_compact_finish, dim3(1), dim3(64), 0, st, r->st, r->cmp_out.get());
  SMX_CALL(reset_accumulators(r, st));
  if (r->L.dirty8)
    hipLaunchKernelGGL(k_compact_dirty, dim3(r->grid_surfels), b, 0, st, r->L.dirty8, (uint32_t)((size_t)r->nseg * kSeg), r->cmp_out.get());
  SMX_HIP(hipMemsetAsync(r->flags_buf[0], 0, (size_t)r->nsegB * kSegB, st));
  SMX_HIP(hipMemsetAsync(r->flags_buf[1], 0, (size_t)r->nsegB * kSegB, st));
  SMX_HIP(hipMemsetAsync(r->L.seg_streak, 0, (size_t)r->nseg, st));
  SMX_HIP(hipMemsetAsync(r->L.hot_epoch, (int)(r->L.epoch & 255u), (size_t)r->L.n_hot_groups + 64, st));
  SMX_HIP(hipMemsetAsync(r->L.seg_targets, 0xFF, (size_t)r->nsegB * kBlockB * sizeof(uint16_t), st));
  SMX_CALL(invalidate_derived(r, st));   // (rebuilds the current flag table)
  uint8_t* other_flags = (r->L.flags8 == r->flags_buf[0]) ? r->flags_buf[1] : r->flags_buf[0];
  SMX_HIP(hipMemcpyAsync(other_flags, r->L.flags8, (size_t)r->nsegB * kSegB, hipMemcpyDeviceToDevice, st));
  if (old_to_new && n)
    SMX_HIP(hipMemcpyAsync(old_to_new, r->cmp_map.get(), (size_t)n * sizeof(uint32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  uint32_t out[2] = {0, 0};
  SMX_HIP(hipMemcpyAsync(out, r->cmp_out.get(), sizeof(out), hipMemcpyDeviceToHost, st));
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
  if (!inputs_on_device) {
    SMX_CALL(dT.alloc((size_t)n_frames * 12));
    SMX_HIP(hipMemcpyAsync(dT.get(), frame_T, (size_t)n_frames * 48, hipMemcpyHostToDevice, st));
    if (reactivate) {
      SMX_CALL(dre.alloc(n_frames));
      SMX_HIP(hipMemcpyAsync(dre.get(), reactivate, n_frames, hipMemcpyHostToDevice, st));
    }
  }
  hipLaunchKernelGGL(k_deform_by_creation_frame, dim3(r->grid_surfels), dim3(kBlock), 0, st, r->S,
                     inputs_on_device ? frame_T : dT.get(), n_frames, inputs_on_device ? reactivate : dre.get(), frame_index,
                     r->L.dirty8, r->st);
  SMX_LAUNCH_CHECK();
  // positions and stamps changed behind the work lists, segment boxes and the flag table
  SMX_CALL(invalidate_derived(r, st));
  if (!inputs_on_device) SMX_HIP(hipStreamSynchronize(st));
  return SMX_OK;
}

}  // extern "C"
