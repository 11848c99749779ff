// smx_merge.hip -- smx_recon_merge_map: a source map into a destination map under a given pose, and its
// gfx950 kernels.  The definition is in include/smx.h, the arithmetic in smx_merge.hpp; this file holds the phases:
//   move     k_merge_move     a lane per source slot: the query rows and the moved records into the workspace
//   query    smx_nn_query_batch over an index of dst as it stood, in chunks of source slots
//   select   k_merge_select   a lane per source slot walks its candidates, first compatible normal wins; counts: one atomic per workgroup
//   number   k_merge_count, enqueue_segment_scan, k_merge_map: ranks of the appended slots (and of the matched pairs)
//   append   k_merge_append   a lane per appended source slot writes the six records at old_size + rank
//   blend    radix_sort of the (d, i) pairs, k_merge_blend: a lane per run of equal d walks the run in order
//   finish   the counts into DevState, then the resets compaction makes (reset_derived_after_rewrite)
// dst is written by append, blend and finish only, after the last allocation and the capacity test.  No float atomics.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "smx_recon_state.hpp"
#include "smx_sort.hpp"

using namespace smx;

namespace {

struct MergePose { float m[12]; };

__device__ __forceinline__ MgVec mg_xyz(const float4& v) { return MgVec{v.x, v.y, v.z}; }

// Streams the source's P, S and N records (48 B per slot), writes 16 B of query rows and 48 B of moved records per slot.
__global__ void __launch_bounds__(kBlock)
k_merge_move(Surfels src, uint32_t n, MergePose T, float factor_sq, float* __restrict__ q, float4* __restrict__ moved,
             uint8_t* __restrict__ cls, uint32_t* __restrict__ ctr) {
  uint32_t count[2] = {0, 0};
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const float4 p = *src.group(kGroupP, i), s = *src.group(kGroupS, i), nr = *src.group(kGroupN, i);
    const MgMoved m = mg_move_slot(T.m, mg_xyz(p), mg_xyz(s), mg_xyz(nr), nr.w, factor_sq);
    const bool ask = m.cls == kMergeAppend;   // dead and BAD slots: an empty ball at the origin, as k_candidate_queries gives
    q[i] = ask ? m.S.x : 0.0f;
    q[(size_t)n + i] = ask ? m.S.y : 0.0f;
    q[(size_t)2 * n + i] = ask ? m.S.z : 0.0f;
    q[(size_t)3 * n + i] = m.r2;
    moved[i] = make_float4(m.P.x, m.P.y, m.P.z, 0.0f);
    moved[(size_t)n + i] = make_float4(m.S.x, m.S.y, m.S.z, 0.0f);
    moved[(size_t)2 * n + i] = make_float4(m.N.x, m.N.y, m.N.z, nr.w);
    cls[i] = (uint8_t)m.cls;
    count[0] += m.cls != kMergeDead ? 1u : 0u;
    count[1] += m.cls == kMergeBad ? 1u : 0u;
  }
  block_counts<2>(ctr + kMgLive, count);         // (kMgLive, kMgBad)
}

// The source slots [off, off + nq) against the answer of their query chunk.  The gathers of dst's N records are the cost:
// up to k per slot, 16 B each, neighbours in space and so mostly neighbours in memory of a map grown from a camera stream.
__global__ void __launch_bounds__(kBlock)
k_merge_select(Surfels dst, uint32_t n_dst, uint32_t off, uint32_t nq, uint32_t n, int k, float cos_max,
               const float4* __restrict__ moved, const uint32_t* __restrict__ idx, const int32_t* __restrict__ cnt,
               uint8_t* __restrict__ cls, uint32_t* __restrict__ match, uint32_t* __restrict__ ctr) {
  uint32_t tally[2] = {0, 0};
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < nq; j += gridDim.x * kBlock) {
    const uint32_t i = off + j;
    if (cls[i] != kMergeAppend) continue;
    const float4 nr = moved[(size_t)2 * n + i];
    const int count = min(max(cnt[j], 0), k);
    bool saturated;
    const float nanv = __builtin_nanf("");
    const uint32_t m = mg_select(mg_xyz(nr), idx + (size_t)j * k, count, k, cos_max,
                                 [&](uint32_t d) { return d < n_dst ? mg_xyz(*dst.group(kGroupN, d)) : MgVec{nanv, nanv, nanv}; }, &saturated);
    if (m != kMergeNone) { cls[i] = (uint8_t)kMergeMatched; match[i] = m; }
    tally[0] += m != kMergeNone ? 1u : 0u;
    tally[1] += saturated ? 1u : 0u;
  }
  block_counts<2>(ctr + kMgMatched, tally);      // (kMgMatched, kMgSaturated)
}

// Per kSeg source slots (four per lane, as k_compact_count): the appended and the matched slots, packed (low and high half).
__device__ __forceinline__ uint32_t merge_class_bits(const uint8_t* cls, uint32_t i0, uint32_t n, uint32_t* a, uint32_t* m) {
  *a = *m = 0;
  if (i0 >= n) return 0;
  const uchar4 c = *reinterpret_cast<const uchar4*>(&cls[i0]);   // (cls is padded to a multiple of kSeg)
  const uint32_t v[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (i0 + j >= n) break;
    if (v[j] == kMergeAppend) *a |= 1u << j;
    if (v[j] == kMergeMatched) *m |= 1u << j;
  }
  return (uint32_t)__popc(*a) | ((uint32_t)__popc(*m) << 16);
}
__global__ void __launch_bounds__(kBlock)
k_merge_count(const uint8_t* __restrict__ cls, uint32_t n, int nseg, uint32_t* __restrict__ seg) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  uint32_t a, m, total;
  const uint32_t mine = merge_class_bits(cls, (blockIdx.x * kBlock + threadIdx.x) * 4, n, &a, &m);
  (void)block_excl_scan(mine, wave_tot, total);
  if (threadIdx.x == 0) { seg[blockIdx.x] = total & 0xFFFFu; seg[nseg + blockIdx.x] = total >> 16; }
}
// match[i] becomes src_to_dst[i]; with pairs != 0 the matched slots leave (d, i) at their rank, ascending in i.
__global__ void __launch_bounds__(kBlock)
k_merge_map(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ seg, int nseg, uint32_t n, uint32_t old_size,
            uint32_t* __restrict__ match, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ uint32_t wave_tot[kBlock / 64];
  const uint32_t i0 = (blockIdx.x * kBlock + threadIdx.x) * 4;
  uint32_t a, m, total;
  const uint32_t excl = block_excl_scan(merge_class_bits(cls, i0, n, &a, &m), wave_tot, total);
  uint32_t ra = seg[blockIdx.x] + (excl & 0xFFFFu), rm = seg[nseg + blockIdx.x] + (excl >> 16);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t i = i0 + j;
    if (i >= n) break;
    if (a & (1u << j)) {
      match[i] = old_size + ra++;
    } else if (m & (1u << j)) {
      if (keys) { keys[rm] = match[i]; vals[rm] = i; }
      ++rm;
    } else {
      match[i] = kMergeNone;
    }
  }
}

// Consecutive ranks are consecutive records of dst: the stores of a wavefront are as dense as its appended slots are.  The
// link gathers go to the class bytes and the map (1 + 4 B per link, read-mostly, small).
__global__ void __launch_bounds__(kBlock)
k_merge_append(Surfels src, Surfels dst, uint32_t n, const float4* __restrict__ moved, const uint8_t* __restrict__ cls,
               const uint32_t* __restrict__ map, uint32_t frame_index, uint8_t* __restrict__ dirty8, uint32_t* __restrict__ ctr) {
  uint32_t dropped[1] = {0};
  const float stamp = __uint_as_float(frame_index);
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    if (cls[i] != kMergeAppend) continue;
    const uint32_t d = map[i];
    const float4 p = moved[i], s = moved[(size_t)n + i], nr = moved[(size_t)2 * n + i];
    const uint4 t = *reinterpret_cast<const uint4*>(src.group(kGroupT, i));
    const float4 c = *src.group(kGroupC, i);
    const uint32_t in[4] = {t.x, t.y, t.z, t.w};
    uint32_t out[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      out[e] = mg_link(in[e], n, [&](uint32_t l) { return (uint32_t)cls[l]; }, [&](uint32_t l) { return map[l]; }, &dropped[0]);
    *dst.group(kGroupP, d) = make_float4(p.x, p.y, p.z, stamp);
    *dst.group(kGroupS, d) = make_float4(s.x, s.y, s.z, 0.0f);
    *dst.group(kGroupN, d) = nr;
    dst.set_neighbors(d, make_uint4(out[0], out[1], out[2], out[3]));
    *dst.group(kGroupC, d) = make_float4(c.x, stamp, c.z, 0.0f);
    *dst.group(kGroupG, d) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (dirty8) dirty8[d] = 1;
  }
  block_counts<1>(ctr + kMgDropped, dropped);
}

// The head of a run of equal d walks it: its sources in ascending order, as the stable sort left them.  Runs are short.
__global__ void __launch_bounds__(kBlock)
k_merge_blend(Surfels src, Surfels dst, uint32_t n, const float4* __restrict__ moved, const unsigned long long* __restrict__ keys,
              const uint32_t* __restrict__ vals, uint32_t n_pairs, float cap, uint32_t frame_index, uint8_t* __restrict__ dirty8,
              uint32_t* __restrict__ ctr) {
  uint32_t heads[1] = {0};
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n_pairs; j += gridDim.x * kBlock) {
    const unsigned long long key = keys[j];
    if (j != 0 && keys[j - 1] == key) continue;
    ++heads[0];
    const uint32_t d = (uint32_t)key;
    const float4 p = *dst.group(kGroupP, d), s = *dst.group(kGroupS, d), nr = *dst.group(kGroupN, d);
    MgBlend b{mg_xyz(p), mg_xyz(s), mg_xyz(nr), dst.f(kConfidence, d), nr.w};
    for (uint32_t e = j; e < n_pairs && keys[e] == key; ++e) {
      const uint32_t i = vals[e];
      const float4 mn = moved[(size_t)2 * n + i];
      mg_blend_step(b, mg_xyz(moved[i]), mg_xyz(moved[(size_t)n + i]), mg_xyz(mn), src.f(kConfidence, i), mn.w, cap);
    }
    *dst.group(kGroupP, d) = make_float4(b.P.x, b.P.y, b.P.z, __uint_as_float(frame_index));
    *dst.group(kGroupS, d) = make_float4(b.S.x, b.S.y, b.S.z, s.w);
    *dst.group(kGroupN, d) = make_float4(b.N.x, b.N.y, b.N.z, b.r);
    dst.f(kConfidence, d) = b.c;
    if (dirty8) dirty8[d] = 1;
  }
  block_counts<1>(ctr + kMgBlended, heads);
}

// The device state after a merge: the new count, the merge count as it was, every other counter reset (as a state upload does).
__global__ void k_merge_finish(DevState* st, uint32_t new_size) {
  if (threadIdx.x != 0) return;
  DevState h;
  memset(&h, 0, sizeof(h));
  h.surfel_count = new_size;
  h.merge_count = st->merge_count;
  *st = h;
}

bool pose_finite(const float* T) {
  for (int k = 0; k < 12; ++k) if (!finite_f(T[k])) return false;
  return true;
}

}  // namespace

extern "C" {

int smx_merge_params_default(smx_merge_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  memset(out, 0, sizeof(*out));
  out->cell_size = 0.05f; out->radius_factor_squared = 1.0f; out->max_normal_angle_deg = 30.0f; out->k = 8;
  out->mode = SMX_MERGE_KEEP_DST; out->confidence_cap = 3.402823466e+38f; out->frame_index = 1;
  return SMX_OK;
}

int smx_recon_merge_map(smx_recon dst, smx_stream s, smx_nn nn, smx_recon src, const float dst_T_src[12],
                        const smx_merge_params* p, uint32_t* src_to_dst, uint32_t capacity, int32_t on_device,
                        smx_merge_stats* stats) {
  SMX_CHECK_ARG(dst != nullptr && src != nullptr && nn != nullptr && dst_T_src != nullptr && p != nullptr);
  // (the parameters first: these refusals look at neither object)
  SMX_CHECK_ARG(p->k >= 1 && p->k <= 64 && p->frame_index >= 1);
  SMX_CHECK_ARG(p->cell_size > 0 && p->radius_factor_squared > 0);
  SMX_CHECK_ARG(p->max_normal_angle_deg >= 0 && p->max_normal_angle_deg <= 180.0f);
  SMX_CHECK_ARG(p->mode == SMX_MERGE_KEEP_DST || p->mode == SMX_MERGE_BLEND);
  SMX_CHECK_ARG(p->confidence_cap == p->confidence_cap && pose_finite(dst_T_src));
  SMX_CHECK_ARG(src != dst);
  SMX_CHECK_ARG(src->device == dst->device);
  SMX_ON_DEVICE(dst->device);
  hipStream_t st = (hipStream_t)s;
  SMX_CALL(join_regularizer(dst, st));
  SMX_CALL(join_regularizer(src, st));
  uint32_t n = 0, old_size = 0;
  SMX_CALL(read_surfel_count(src, st, &n));
  SMX_CALL(read_surfel_count(dst, st, &old_size));
  if (src_to_dst && capacity < n) {   // (nothing has been changed yet)
    set_error("src_to_dst holds %u entries, the source map has %u slots", capacity, n);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  smx_merge_stats h;
  memset(&h, 0, sizeof(h));
  h.n_src_slots = n; h.old_size = h.new_size = old_size;
  if (stats) *stats = h;
  if (n == 0) return SMX_OK;
  const bool blend = p->mode == SMX_MERGE_BLEND;
  const int k = p->k;
  const float cos_max = (float)cos((double)p->max_normal_angle_deg * (M_PI / 180.0));

  // ---- the workspace: every allocation of this file before the first launch
  MergeWork& w = dst->merge;
  const int nseg = div_up((long long)n, kSeg);
  const size_t npad = (size_t)nseg * kSeg;
  const uint32_t chunk = std::min<uint32_t>(w.chunk ? w.chunk : kMergeChunkDefault, n);
  if (npad > w.cls.capacity() || !w.ctr.get()) {
    SMX_HIP(hipDeviceSynchronize());   // (an earlier call's work is done: the calls are synchronous; this orders other streams)
    w.q.reset(); w.moved.reset(); w.match.reset(); w.seg.reset(); w.cls.reset(); w.ctr.reset();
    SMX_CALL(alloc_all(w.q, 4 * npad, w.moved, 3 * npad, w.match, npad, w.seg, (size_t)2 * nseg, w.cls, npad, w.ctr, (size_t)kMgWords));
  }
  if ((size_t)chunk * k > w.idx.capacity() || chunk > w.cnt.capacity()) {
    SMX_HIP(hipDeviceSynchronize());
    w.idx.reset(); w.d2.reset(); w.cnt.reset();
    SMX_CALL(alloc_all(w.idx, (size_t)chunk * k, w.d2, (size_t)chunk * k, w.cnt, (size_t)chunk));
  }
  if (blend && (n > w.vals[0].capacity() || radix_sort_workspace_elems(n) > w.hist.capacity())) {
    SMX_HIP(hipDeviceSynchronize());
    for (int e = 0; e < 2; ++e) { w.keys[e].reset(); w.vals[e].reset(); }
    w.hist.reset();
    SMX_CALL(alloc_all(w.keys[0], (size_t)n, w.keys[1], (size_t)n, w.vals[0], (size_t)n, w.vals[1], (size_t)n, w.hist,
                       radix_sort_workspace_elems(n)));
  }
  SMX_CALL(w.stamps.begin(st));

  // ---- index of dst as it stood (orders st behind both regularisers once more, reads the count back)
  SMX_CALL(smx_recon_build_neighbor_index(dst, s, nn, p->cell_size));
  SMX_CALL(w.stamps.mark(st));

  // ---- move
  const dim3 b(kBlock);
  const dim3 g_src((unsigned)std::min<size_t>(blocks_for(n), 2048));
  MergePose T;
  memcpy(T.m, dst_T_src, sizeof(T.m));
  float* q = w.q.get();
  uint32_t* ctr = w.ctr.get();
  SMX_HIP(hipMemsetAsync(ctr, 0, kMgWords * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_merge_move, g_src, b, 0, st, src->S, n, T, p->radius_factor_squared, q, w.moved.get(), w.cls.get(), ctr);
  SMX_LAUNCH_CHECK();
  SMX_CALL(w.stamps.mark(st));

  // ---- query + select, a chunk of source slots at a time (the [chunk][k] answer is the workspace's largest block)
  for (uint32_t off = 0; off < n; off += chunk) {
    const uint32_t nq = std::min(chunk, n - off);
    SMX_CALL(smx_nn_query_batch(nn, s, nq, q + off, q + (size_t)n + off, q + (size_t)2 * n + off, q + (size_t)3 * n + off, k, nullptr, 0, 1,
                                w.idx.get(), w.d2.get(), w.cnt.get(), 1));
    hipLaunchKernelGGL(k_merge_select, dim3((unsigned)std::min<size_t>(blocks_for(nq), 2048)), b, 0, st, dst->S, old_size, off, nq, n, k,
                       cos_max, w.moved.get(), w.idx.get(), w.cnt.get(), w.cls.get(), w.match.get(), ctr);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- number: ranks by the segment scan, then the one read-back the capacity test needs
  uint32_t* seg = w.seg.get();
  hipLaunchKernelGGL(k_merge_count, dim3(nseg), b, 0, st, w.cls.get(), n, nseg, seg);
  enqueue_segment_scan(st, seg, nseg, ctr + kMgAppended);
  enqueue_segment_scan(st, seg + nseg, nseg, ctr + kMgPairs);
  hipLaunchKernelGGL(k_merge_map, dim3(nseg), b, 0, st, w.cls.get(), seg, nseg, n, old_size, w.match.get(),
                     blend ? w.keys[0].get() : nullptr, blend ? w.vals[0].get() : nullptr);
  SMX_LAUNCH_CHECK();
  uint32_t c[kMgWords];
  SMX_HIP(hipMemcpyAsync(c, ctr, sizeof(c), hipMemcpyDeviceToHost, st));
  SMX_HIP(hipStreamSynchronize(st));
  SMX_CALL(w.stamps.mark(st));
  h.n_src_live = c[kMgLive]; h.n_bad = c[kMgBad]; h.n_matched = c[kMgMatched]; h.n_saturated = c[kMgSaturated];
  h.n_appended = c[kMgAppended];
  if ((unsigned long long)old_size + h.n_appended > dst->max_surfels) {   // (dst has not been written)
    if (stats) *stats = h;
    set_error("the merge appends %u slots to %u, the destination holds %u", h.n_appended, old_size, dst->max_surfels);
    return SMX_ERR_INVALID_ARGUMENT;
  }
  h.new_size = old_size + h.n_appended;

  // ---- append
  if (h.n_appended) {
    hipLaunchKernelGGL(k_merge_append, g_src, b, 0, st, src->S, dst->S, n, w.moved.get(), w.cls.get(), w.match.get(), p->frame_index,
                       dst->L.dirty8, ctr);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- blend
  if (blend && h.n_matched) {
    int bits = 1;
    while (bits < 32 && ((old_size - 1) >> bits) != 0) ++bits;
    const int cur = radix_sort(w.keys, w.vals, h.n_matched, bits, w.hist.get(), st);
    hipLaunchKernelGGL(k_merge_blend, dim3((unsigned)std::min<size_t>(blocks_for(h.n_matched), 2048)), b, 0, st, src->S, dst->S, n,
                       w.moved.get(), w.keys[cur].get(), w.vals[cur].get(), h.n_matched, p->confidence_cap, p->frame_index, dst->L.dirty8, ctr);
    SMX_LAUNCH_CHECK();
  }
  SMX_CALL(w.stamps.mark(st));

  // ---- finish: the counts, then the derived state as compaction resets it (the marks of the delta hand-off are per slot)
  hipLaunchKernelGGL(k_merge_finish, dim3(1), dim3(64), 0, st, dst->st, h.new_size);
  SMX_CALL(reset_derived_after_rewrite(dst, st));
  if (src_to_dst)
    SMX_HIP(hipMemcpyAsync(src_to_dst, w.match.get(), (size_t)n * sizeof(uint32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  SMX_HIP(hipMemcpyAsync(c, ctr, sizeof(c), hipMemcpyDeviceToHost, st));
  SMX_CALL(w.stamps.mark(st));
  SMX_HIP(hipStreamSynchronize(st));
  w.stamps.publish();
  h.n_blended_dst = c[kMgBlended]; h.links_dropped = c[kMgDropped];
  if (stats) *stats = h;
  return SMX_OK;
}

int smx_recon_debug_merge_timings(smx_recon dst, float* out_ms, int32_t capacity) {
  SMX_CHECK_ARG(dst != nullptr && out_ms != nullptr && capacity >= 0);
  SMX_ON_DEVICE(dst->device);
  float ms[SMX_MERGE_PHASES];
  SMX_CALL(dst->merge.stamps.elapsed_ms(ms, SMX_MERGE_PHASES));
  float whole = 0.0f;
  for (float v : ms) whole += v;
  for (int k = 0; k < std::min<int>(capacity, SMX_MERGE_PHASES + 1); ++k) out_ms[k] = k == 0 ? whole : ms[k - 1];
  return SMX_OK;
}

int smx_recon_debug_set_merge_chunk(smx_recon dst, uint32_t chunk_queries) {
  SMX_CHECK_ARG(dst != nullptr);
  dst->merge.chunk = chunk_queries;
  return SMX_OK;
}

}  // extern "C"
