// smx_import.hip -- smx_recon_import_points: a point cloud becomes surfels behind the map's slots, and its
// gfx950 kernels.  The definition is in include/smx.h, the arithmetic in smx_import.hpp; this file holds the phases:
//   stage    k_import_stage   a lane per point: the BAD test, the three rows the index wants, one 16-byte record per point
//   build    smx_nn_build over the rows
//   query    smx_nn_query_self: every point's k nearest inside the search radius
//   fit      k_import_fit     a lane per point: its list row in 16-byte pieces, a 16-byte record per neighbour, nine double
//                             sums in list order, Jacobi in registers, the class; counts: one atomic per workgroup
//   number   k_import_count, enqueue_segment_scan, k_import_map: ranks of the imported points, one read-back
//   write    k_import_write   a lane per imported point writes the six records at old_size + rank
//   finish   the count into DevState, then the resets a merge makes (reset_derived_after_rewrite)
// The map is written by write and finish only, after the last allocation and the capacity test.  No float atomics.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "smx_recon_state.hpp"

using namespace smx;

namespace {

struct ImportStage { int32_t orient; uint32_t default_color; };

// Reads 12 B (+ 4 B colour, + 12 B origin) per point, writes 12 B of rows, a 16-byte record and the class byte.
__global__ void __launch_bounds__(kBlock)
k_import_stage(const float* __restrict__ points, const uint32_t* __restrict__ colors, const float* __restrict__ origins, uint32_t n, size_t npad,
               ImportStage sp, float* __restrict__ rows, float4* __restrict__ rec, uint8_t* __restrict__ cls, uint32_t* __restrict__ ctr) {
  uint32_t count[1] = {0};
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const ImVec p{points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    bool bad = !im_vec_finite(p);
    if (sp.orient == SMX_IMPORT_ORIENT_ORIGINS) bad = bad || !im_vec_finite(ImVec{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]});
    const float nanv = __builtin_nanf("");
    rows[i] = bad ? nanv : p.x;
    rows[npad + i] = bad ? nanv : p.y;
    rows[2 * npad + i] = bad ? nanv : p.z;
    rec[i] = make_float4(p.x, p.y, p.z, __uint_as_float(colors ? colors[i] : sp.default_color));
    cls[i] = (uint8_t)(bad ? kImportBad : kImportOk);
    count[0] += bad ? 1u : 0u;
  }
  block_counts<1>(ctr + kImBad, count);
}

// The hot path.  Per point: k x 4 B of list, up to k gathered 16-byte records (neighbours in space; in memory as near as the
// cloud's order puts them), one d2 word; 16 B of fit out.  kVec: k is a multiple of 4, so a list row is whole 16-byte pieces.
template <bool kVec>
__global__ void __launch_bounds__(kBlock)
k_import_fit(const float4* __restrict__ rec, const float* __restrict__ origins, uint32_t n, ImFitParams prm, const uint32_t* __restrict__ idx,
             const float* __restrict__ d2, const int32_t* __restrict__ cnt, uint8_t* __restrict__ cls, float4* __restrict__ fit,
             uint32_t* __restrict__ ctr) {
  uint32_t tally[4] = {0, 0, 0, 0};   // sparse, degenerate, rough, saturated
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    if (cls[i] == kImportBad) continue;
    const int k = prm.k;
    const int m = min(max(cnt[i], 0), k);
    tally[3] += m == k ? 1u : 0u;
    float radius_squared;
    uint32_t c = im_class_early(m, m > 0 ? d2[i * k + im_radius_entry(prm.radius_rank, m)] : 0.0f, prm, &radius_squared);
    float4 out = make_float4(0.0f, 0.0f, 0.0f, radius_squared);
    if (c == kImportOk) {
      const float4 self = rec[i];
      const ImVec p{self.x, self.y, self.z};
      ImSums sums = im_sums_zero();
      const uint32_t* row = idx + i * k;
      if (kVec) {
        const uint4* row4 = reinterpret_cast<const uint4*>(row);
        for (int e = 0; e < m; e += 4) {
          const uint4 piece = row4[e >> 2];
          const uint32_t j[4] = {piece.x, piece.y, piece.z, piece.w};
          float4 q[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) q[u] = rec[e + u < m && j[u] < n ? j[u] : (uint32_t)i];   // (the four fetches are in flight together)
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (e + u < m) im_sums_add(sums, p, ImVec{q[u].x, q[u].y, q[u].z});
        }
      } else {
        for (int e = 0; e < m; ++e) {
          const uint32_t j = row[e];
          const float4 q = rec[j < n ? j : (uint32_t)i];
          im_sums_add(sums, p, ImVec{q.x, q.y, q.z});
        }
      }
      ImVec o = prm.view_point;
      if (prm.orient == SMX_IMPORT_ORIENT_ORIGINS) o = ImVec{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]};
      const ImFit f = im_fit(sums, m, p, o, radius_squared, prm);
      c = f.cls;
      out = make_float4(f.n.x, f.n.y, f.n.z, radius_squared);
    }
    cls[i] = (uint8_t)c;
    fit[i] = out;
    tally[0] += c == kImportSparse ? 1u : 0u;
    tally[1] += c == kImportDegenerate ? 1u : 0u;
    tally[2] += c == kImportRough ? 1u : 0u;
  }
  block_counts<4>(ctr + kImSparse, tally);       // (kImSparse, kImDegenerate, kImRough, kImSaturated)
}

// Per kSeg points (four per lane, as k_merge_count): the imported ones.
__device__ __forceinline__ uint32_t import_class_bits(const uint8_t* cls, size_t i0, uint32_t n) {
  if (i0 >= n) return 0;
  const uchar4 c = *reinterpret_cast<const uchar4*>(&cls[i0]);   // (cls is padded to a multiple of kSeg)
  const uint32_t v[4] = {c.x, c.y, c.z, c.w};
  uint32_t a = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (i0 + j < n && v[j] == kImportOk) a |= 1u << j;
  return a;
}
__global__ void __launch_bounds__(kBlock)
k_import_count(const uint8_t* __restrict__ cls, uint32_t n, uint32_t* __restrict__ seg) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  uint32_t total;
  const uint32_t a = import_class_bits(cls, ((size_t)blockIdx.x * kBlock + threadIdx.x) * 4, n);
  (void)block_excl_scan((uint32_t)__popc(a), wave_tot, total);
  if (threadIdx.x == 0) seg[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kBlock)
k_import_map(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ seg, uint32_t n, uint32_t old_size, uint32_t* __restrict__ slot) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const size_t i0 = ((size_t)blockIdx.x * kBlock + threadIdx.x) * 4;
  uint32_t total;
  const uint32_t a = import_class_bits(cls, i0, n);
  uint32_t rank = seg[blockIdx.x] + block_excl_scan((uint32_t)__popc(a), wave_tot, total);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (i0 + j >= n) break;
    slot[i0 + j] = (a & (1u << j)) ? old_size + rank++ : kImportNone;
  }
}

// Consecutive ranks are consecutive records of the map: a wavefront's stores are as dense as its imported points are.
__global__ void __launch_bounds__(kBlock)
k_import_write(Surfels S, uint32_t n, uint32_t max_surfels, const float4* __restrict__ rec, const float4* __restrict__ fit,
               const uint8_t* __restrict__ cls, const uint32_t* __restrict__ slot, float confidence, uint32_t frame_index,
               uint8_t* __restrict__ dirty8) {
  const float stamp = __uint_as_float(frame_index);
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    if (cls[i] != kImportOk) continue;
    const uint32_t d = slot[i];
    if (d >= max_surfels) continue;   // (cannot happen behind the capacity test; a store past the map must not, either)
    const float4 p = rec[i], f = fit[i];
    *S.group(kGroupP, d) = make_float4(p.x, p.y, p.z, stamp);
    *S.group(kGroupS, d) = make_float4(p.x, p.y, p.z, 0.0f);
    *S.group(kGroupN, d) = f;
    S.set_neighbors(d, make_uint4(kImportNone, kImportNone, kImportNone, kImportNone));
    *S.group(kGroupC, d) = make_float4(confidence, stamp, p.w, 0.0f);
    *S.group(kGroupG, d) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (dirty8) dirty8[d] = 1;
  }
}

// The device state after an import: the new count, the merge count as it was, every other counter reset (as a merge leaves it).
__global__ void k_import_finish(DevState* st, uint32_t new_size) {
  if (threadIdx.x != 0) return;
  DevState h;
  memset(&h, 0, sizeof(h));
  h.surfel_count = new_size;
  h.merge_count = st->merge_count;
  *st = h;
}

}  // namespace

extern "C" {

int smx_import_params_default(smx_import_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  memset(out, 0, sizeof(*out));
  out->cell_size = 0.05f; out->search_radius = 0.1f; out->k = 16; out->min_neighbors = 6;
  out->max_surface_variation = (float)(1.0 / 3.0); out->radius_rank = 8; out->radius_scale_squared = 2.0f;
  out->confidence = 1.0f; out->default_color = 0; out->frame_index = 1; out->orient = SMX_IMPORT_ORIENT_NONE;
  return SMX_OK;
}

int smx_recon_import_points(smx_recon r, smx_stream s, smx_nn nn, const float* points, const uint32_t* colors, const float* origins,
                            uint32_t n, int32_t inputs_on_device, const smx_import_params* p, uint32_t* point_to_slot,
                            uint32_t capacity, int32_t on_device, smx_import_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && nn != nullptr && p != nullptr);
  // (the parameters first: these refusals look at no object)
  SMX_CHECK_ARG(p->cell_size > 0 && p->search_radius > 0 &&p->radius_scale_squared > 0);
  SMX_CHECK_ARG(p->k >= 4 && p->k <= 64 && p->min_neighbors >= 3 && p->min_neighbors <= p->k);
  SMX_CHECK_ARG(p->max_surface_variation >= 0 && p->max_surface_variation <= (float)(1.0 / 3.0));
  SMX_CHECK_ARG(p->radius_rank >= 1 && p->radius_rank <= 63 && p->frame_index >= 1);
  SMX_CHECK_ARG(finite_f(p->confidence) && finite_f(p->view_point[0]) && finite_f(p->view_point[1]) && finite_f(p->view_point[2]));
  SMX_CHECK_ARG(p->orient >= SMX_IMPORT_ORIENT_NONE && p->orient <= SMX_IMPORT_ORIENT_ORIGINS);
  SMX_CHECK_ARG(n == 0 || points != nullptr);
  SMX_CHECK_ARG(n == 0 || p->orient != SMX_IMPORT_ORIENT_ORIGINS || origins != nullptr);
  if (point_to_slot && capacity < n) {
    set_error("point_to_slot holds %u entries, the cloud has %u points", capacity, n);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(r, st));
  uint32_t old_size = 0;
  SMX_CALL(read_surfel_count(r, st, &old_size));
  smx_import_stats h;
  memset(&h, 0, sizeof(h));
  h.n_points = n; h.old_size = h.new_size = old_size;
  if (stats) *stats = h;
  if (n == 0) return SMX_OK;
  const int k = p->k;
  const bool use_origins = p->orient == SMX_IMPORT_ORIENT_ORIGINS;

  // ---- the workspace: every allocation of this file before the first launch
  ImportWork& w = r->import;
  const int nseg = div_up((long long)n, kSeg);
  const size_t npad = (size_t)nseg * kSeg;
  if (npad > w.cls.capacity() || !w.ctr.get()) {
    SMX_HIP(hipDeviceSynchronize());   // (an earlier call's work is done: the calls are synchronous; this orders other streams)
    w.rows.reset(); w.rec.reset(); w.fit.reset(); w.slot.reset(); w.seg.reset(); w.cls.reset(); w.ctr.reset();
    SMX_CALL(alloc_all(w.rows, 3 * npad, w.rec, npad, w.fit, npad, w.slot, npad, w.seg, (size_t)nseg, w.cls, npad, w.ctr, (size_t)kImWords));
  }
  if ((size_t)n * k > w.idx.capacity() || n > w.cnt.capacity()) {
    SMX_HIP(hipDeviceSynchronize());
    w.idx.reset(); w.d2.reset(); w.cnt.reset();
    SMX_CALL(alloc_all(w.idx, (size_t)n * k, w.d2, (size_t)n * k, w.cnt, (size_t)n));
  }
  const float* d_points = points;
  const uint32_t* d_colors = colors;
  const float* d_origins = use_origins ? origins : nullptr;
  if (!inputs_on_device) {
    // (room first, so that no copy is enqueued before the last allocation)
    SMX_CALL(w.in_points.reserve((size_t)3 * n));
    if (colors) SMX_CALL(w.in_colors.reserve(n));
    if (use_origins) SMX_CALL(w.in_origins.reserve((size_t)3 * n));
  }
  SMX_CALL(w.stamps.begin(st));
  SMX_CALL(stage_in(w.in_points, points, (size_t)3 * n, inputs_on_device != 0, st, &d_points));
  if (colors) SMX_CALL(stage_in(w.in_colors, colors, (size_t)n, inputs_on_device != 0, st, &d_colors));
  if (use_origins) SMX_CALL(stage_in(w.in_origins, origins, (size_t)3 * n, inputs_on_device != 0, st, &d_origins));

  // ---- stage
  const dim3 b(kBlock);
  const dim3 g_pts((unsigned)std::min<size_t>(blocks_for(n), 2048));
  uint32_t* ctr = w.ctr.get();
  float* rows = w.rows.get();
  SMX_HIP(hipMemsetAsync(ctr, 0, kImWords * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_import_stage, g_pts, b, 0, st, d_points, d_colors, d_origins, n, npad, ImportStage{p->orient, p->default_color}, rows,
                     w.rec.get(), w.cls.get(), ctr);
  SMX_LAUNCH_CHECK();
  SMX_CALL(w.stamps.mark(st));

  // ---- index build (synchronises st twice; its own workspace lives in nn)
  SMX_CALL(smx_nn_build(nn, s, rows, rows + npad, rows + 2 * npad, n, p->cell_size, 1));
  SMX_CALL(w.stamps.mark(st));

  // ---- self query
  SMX_CALL(smx_nn_query_self(nn, s, nullptr, p->search_radius * p->search_radius, k, nullptr, 0, w.idx.get(), w.d2.get(), w.cnt.get()));
  SMX_CALL(w.stamps.mark(st));

  // ---- fit
  ImFitParams fp;
  fp.k = k; fp.min_neighbors = p->min_neighbors; fp.radius_rank = p->radius_rank; fp.orient = p->orient;
  fp.max_surface_variation = p->max_surface_variation; fp.radius_scale_squared = p->radius_scale_squared;
  fp.view_point = ImVec{p->view_point[0], p->view_point[1], p->view_point[2]};
  const dim3 g_fit((unsigned)blocks_for(n));
  if (k % 4 == 0)
    hipLaunchKernelGGL(k_import_fit<true>, g_fit, b, 0, st, w.rec.get(), d_origins, n, fp, w.idx.get(), w.d2.get(), w.cnt.get(), w.cls.get(),
                       w.fit.get(), ctr);
  else
    hipLaunchKernelGGL(k_import_fit<false>, g_fit, b, 0, st, w.rec.get(), d_origins, n, fp, w.idx.get(), w.d2.get(), w.cnt.get(), w.cls.get(),
                       w.fit.get(), ctr);
  SMX_LAUNCH_CHECK();
  SMX_CALL(w.stamps.mark(st));

  // ---- number: ranks by the segment scan, then the one read-back the capacity test needs
  uint32_t* seg = w.seg.get();
  hipLaunchKernelGGL(k_import_count, dim3(nseg), b, 0, st, w.cls.get(), n, seg);
  enqueue_segment_scan(st, seg, nseg, ctr + kImImported);
  hipLaunchKernelGGL(k_import_map, dim3(nseg), b, 0, st, w.cls.get(), seg, n, old_size, w.slot.get());
  SMX_LAUNCH_CHECK();
  uint32_t c[kImWords];
  SMX_HIP(hipMemcpyAsync(c, ctr, sizeof(c), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  SMX_CALL(w.stamps.mark(st));
  h.n_bad = c[kImBad]; h.n_sparse = c[kImSparse]; h.n_degenerate = c[kImDegenerate]; h.n_rough = c[kImRough];
  h.n_saturated = c[kImSaturated]; h.n_imported = c[kImImported];
  if ((unsigned long long)old_size + h.n_imported > r->max_surfels) {   // (the map has not been written)
    if (stats) *stats = h;
    set_error("the import appends %u slots to %u, the map holds %u", h.n_imported, old_size, r->max_surfels);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  h.new_size = old_size + h.n_imported;

  // ---- write
  if (h.n_imported) {
    hipLaunchKernelGGL(k_import_write, g_pts, b, 0, st, r->S, n, r->max_surfels, w.rec.get(), w.fit.get(), w.cls.get(), w.slot.get(),
                       p->confidence, p->frame_index, r->L.dirty8);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- finish: the count, then the derived state as a merge resets it (the marks of the delta hand-off are per slot)
  hipLaunchKernelGGL(k_import_finish, dim3(1), dim3(64), 0, st, r->st, h.new_size);
  SMX_CALL(reset_derived_after_rewrite(r, st));
  if (point_to_slot)
    SMX_HIP(hipMemcpyAsync(point_to_slot, w.slot.get(), (size_t)n * sizeof(uint32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  SMX_CALL(w.stamps.mark(st));
  SMX_HIP(hipStreamSynchronize(st));
  w.stamps.publish();
  if (stats) *stats = h;
  return SMX_OK;
}

int smx_recon_debug_import_timings(smx_recon r, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr && capacity >= 0);
  SMX_ON_DEVICE(r->device);
  float ms[SMX_IMPORT_PHASES];
  SMX_CALL(r->import.stamps.elapsed_ms(ms, SMX_IMPORT_PHASES));
  float whole = 0.0f;
  for (float v : ms) whole += v;
  for (int k = 0; k < std::min<int>(capacity, SMX_IMPORT_PHASES + 1); ++k) out_ms[k] = k == 0 ? whole : ms[k - 1];
  return SMX_OK;
}

}  // extern "C"
