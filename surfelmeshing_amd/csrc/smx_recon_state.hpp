// smx_recon_state.hpp -- the surfel reconstruction object as its translation units see it (internal).
//
// smx_recon.hip holds the frame loop (Integrate / Regularize, their kernels, the changed-surfel delta),
// smx_recon_map.hip the map services that read or rewrite the finished map outside of it (row transfers, export,
// viewer buffers, the splat render, neighbour and meshing glue, compaction, deformation); tracking, decimation, the
// components, hole filling, the mesh distance, the rim, the ray cast, the mesh sampler and the mesh render live with their kernels in smx_track.hip, smx_decimate.hip,
// smx_components.hip, smx_fill.hip, smx_merge.hip, smx_import.hip, smx_distance.hip, smx_rim.hip, smx_raycast.hip, smx_sample.hip and smx_mesh_raster.hip.  This header is what
// they all need: the attribute layout, the plain structs that are members of smx_recon_s, the object itself -- the
// frame loop's state, then one workspace per service, each defined in the service's own header -- and the few host
// helpers every entry point starts with.  Kernels stay in anonymous namespaces of the .hip files.
#pragma once

#include "smx_common.hpp"
#include "smx_components.hpp"
#include "smx_decimate.hpp"
#include "smx_distance.hpp"
#include "smx_fill.hpp"
#include "smx_import.hpp"
#include "smx_merge.hpp"
#include "smx_raycast.hpp"
#include "smx_render.hpp"
#include "smx_rim.hpp"
#include "smx_sample.hpp"
#include "smx_track.hpp"

namespace smx {

struct MeshWorkspace;   // smx_mesh.hpp

// Attribute ids = the reference's SoA row numbers, APP/cuda_surfel_reconstruction_kernels.cuh:49-78 (the
// storage itself is grouped differently, see Surfels below)
enum : int {
  kX = 0, kY = 1, kZ = 2, kSmoothX = 3, kSmoothY = 4, kSmoothZ = 5, kConfidence = 6, kRadiusSq = 7,
  kNormalX = 8, kNormalY = 9, kNormalZ = 10, kGradX = 11, kGradY = 12, kGradZ = 13,
  kCreationStamp = 17, kLastUpdateStamp = 18, kNeighbor0 = 19, kGradCount = 23, kColor = 24, kRows = 25
};

struct DevState {
  uint32_t surfel_count;   // slots in use (incl. merged zombies)
  uint32_t merge_count;
  uint32_t create_base_next;  // slot count seen by k_new_flags_scan (which may run beside the previous frame's pass B)
  uint32_t recent_count;   // statistics: slots inside the regulariser window
  uint32_t create_base;
  uint32_t new_count;
  uint32_t capacity_clamped;
  uint32_t n_visible, n_merged, n_edges, n_integrated, n_replaced, n_conflict_hits;
  uint32_t n_window_edges, n_contributors;
  uint32_t n_segments_skipped;
  uint32_t reg_saturated;  // sticky: a regulariser term hit the +-16 m clamp or a sender-class counter came near its byte
  uint32_t n_pairs, n_overflow_pairs, max_tile_pairs;   // statistics of the association tiles' bins
};

// HBM layout of the surfel attributes.  The reference keeps 25 separate rows (SoA, kernels.cuh:49-78); that is
// ideal for its all-slot scans but makes every per-surfel gather touch one cache line per attribute.  Here
// the attributes are grouped into six 16-byte records per slot, chosen by which kernels use them together,
// and each group is its own array (group-major):
//   P  X, Y, Z, LastUpdateStamp      -- exactly what pass A streams (16 B/slot), and what every projection needs
//   S  SmoothX, SmoothY, SmoothZ, -   -- what the regulariser gathers per neighbour (one line instead of three)
//   N  NormalX, NormalY, NormalZ, RadiusSquared
//   T  Neighbor0..3                  -- what pass B streams (16 B/slot)
//   C  Confidence, CreationStamp, Color, -
//   G  GradientX, GradientY, GradientZ, -  (parked next smooth position)
// (Rounds 1-2 kept a copy of T in the second half of a 32-byte S record, so that the regulariser could see with one
// gather whether a neighbour lists the slot back; with the far-term bins nobody asks that question any more.)
// The reference's row order only matters at the boundary (TransferAllToCPU, ExportVertices, the debug row
// accessors); pack/unpack kernels convert there.  Rows 14-16 (Accum*, never used) and 23 (GradientCount,
// replaced by the fixed-point accumulators) have no storage.
enum : int { kGroupP = 0, kGroupS, kGroupN, kGroupT, kGroupC, kGroupG, kGroups };
__host__ __device__ constexpr int row_group(int row) {
  return row <= 2 ? kGroupP : row <= 5 ? kGroupS : row == 6 ? kGroupC : row == 7 ? kGroupN : row <= 10 ? kGroupN
       : row <= 13 ? kGroupG : row <= 16 ? -1 : row == 17 ? kGroupC : row == 18 ? kGroupP : row <= 22 ? kGroupT
       : row == 24 ? kGroupC : -1;
}
__host__ __device__ constexpr int row_sub(int row) {
  return row <= 2 ? row : row <= 5 ? row - 3 : row == 6 ? 0 : row == 7 ? 3 : row <= 10 ? row - 8
       : row <= 13 ? row - 11 : row == 17 ? 1 : row == 18 ? 3 : row <= 22 ? row - 19 : row == 24 ? 2 : -1;
}
// start of each group array in units of pitch x 16 bytes
__host__ __device__ constexpr int group_start(int g) { return g; }
constexpr int kQuadsPerSlot = 6;   // 96 bytes per slot
struct Surfels {
  float* base;
  size_t pitch;  // slots per group array (multiple of 64)
  __host__ __device__ __forceinline__ size_t quad(int g, uint32_t i) const { return (size_t)group_start(g) * pitch + (size_t)i; }
  __device__ __forceinline__ float& f(int row, uint32_t i) const { return base[quad(row_group(row), i) * 4 + row_sub(row)]; }
  __device__ __forceinline__ uint32_t& u(int row, uint32_t i) const {
    return reinterpret_cast<uint32_t*>(base)[quad(row_group(row), i) * 4 + row_sub(row)];
  }
  // whole 16-byte group of slot i
  __device__ __forceinline__ float4* group(int g, uint32_t i) const { return reinterpret_cast<float4*>(base) + quad(g, i); }
  __device__ __forceinline__ void set_neighbors(uint32_t i, const uint4& t) const { *reinterpret_cast<uint4*>(group(kGroupT, i)) = t; }
  __device__ __forceinline__ void set_neighbor(uint32_t i, int q, uint32_t v) const { u(kNeighbor0 + q, i) = v; }
  // a group for the code that does not know this layout (the mesher, decimation): slot i's record is p[i * stride]
  struct View { const float4* p; size_t stride; };
  View view(int g) const { return View{reinterpret_cast<const float4*>(base) + quad(g, 0), quad(g, 1) - quad(g, 0)}; }
};

// The association images of a frame (built per image tile by k_assoc_tiles).  `assoc` is one 16-byte record per pixel,
// {first depth (float bits), conflict key, count, supporting surfel}: what the integration and the flag pass need of a
// pixel in one request.  The supporting surfel and the count are ALSO kept as images, for the kernels that read them
// alone or next to the depth sums (the blend, the neighbour update, the creation).
struct Scratch {
  uint32_t* supporting;
  uint32_t* counts;
  long long* depth_sums;
  uint4* assoc;
};

constexpr int kBlock = 256;

// ---- what the glue of every map service asks ----
inline unsigned blocks_for(uint32_t n) { return (unsigned)div_up(n, kBlock); }
inline bool finite_f(float v) { return v - v == 0.0f; }
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
inline unsigned long long word64(const uint32_t* h, int lo) { return ((unsigned long long)h[lo + 1] << 32) | h[lo]; }   // a (lo, hi) pair

// Work lists are SEGMENTED: the slots [s*kSeg, (s+1)*kSeg) are scanned by one workgroup, which writes the
// indices it selects to list[s*kSeg ...] (ascending) and their number to seg[s].  No global counter, no
// atomics, and the list order is deterministic.
constexpr int kSeg = 1024;
// Pass B uses larger segments (kSegB slots, one 1024-thread workgroup each): the in-segment regulariser sums
// live in 128 KB of LDS, and the larger the segment the fewer edges leave it (image-row neighbours are a few
// hundred slots apart), i.e. the fewer 64-bit global atomics remain.
constexpr int kSegB = 1024;
constexpr int kBlockB = kSegB / 4;
// The non-empty 256-entry chunks of a segmented list, appended by the pass that builds the list: descriptor = chunk id
// (segment * chunks-per-segment + sub-chunk) | (entries - 1) << 24.  The list kernels walk these instead of probing every
// chunk of every segment: on the frame's binding cycle each dependent memory round trip costs microseconds, and a probe
// that finds an empty chunk is one (profiles/r04_critical_cycle_notes.md).
// The descriptors go to kSubLists INTERLEAVED sub-lists, each with a counter in a cache line of its own: walk step w is
// entry w / kSubLists of sub-list w % kSubLists.  Rounds 1-3 had ONE list behind ONE counter: a returning atomic per
// non-empty segment, 1 300 per launch of pass A at C2 and 5 400 at C3, all arriving within the same few microseconds at
// the end of their workgroups' chains -- and atomics on one address retire at ~12 ns each, so the tail of the launch was
// that queue.  Sixteen counters take a sixteenth each; the producers deal their segments round-robin, so the sub-lists
// stay equally long up to the spread of the descriptors per segment, and a walk that covers kSubLists x the longest one
// meets few empty steps.  A consumer still finds its first descriptor without waiting for any counter (its place does
// not depend on them), which is what a prefix over the sub-lists would have cost.
constexpr uint32_t kCountStride = 32;     // one counter per 128-byte line: atomics on one line serialise, whatever word they hit
constexpr uint32_t kSubLists = 16;
struct Chunks { uint32_t* desc; uint32_t* count; uint32_t stride; };   // desc[k * stride + j], count[k * kCountStride]
struct Lists {
  Chunks vis_chunks, rec_chunks;   // (vis_chunks: only the kSubLists counters = the lengths of the visible list's runs)
  Chunks acc_chunks;      // segments the edge kernel has work in (descriptor = segment); its counters share rec_chunks' lines (kAccCount)
  uint32_t* vis_list;     // slots that project into the image this frame: kSubLists dense runs, run k at k * vis_region (vis_*)
  uint32_t vis_region;    // entries per run: every kSubLists-th surviving segment's slots at most
  float* seg_box;         // per pass-A segment: min xyz, max xyz, covered slot count (u32), newest stamp (u32)
  uint32_t* vis_seg;
  uint8_t* seg_streak;      // per pass-A segment: in how many calls in a row pass A has culled it (k_scan_visible, step 2)
  uint32_t* recent_list;  // slots whose last update stamp lies inside the regulariser window
  uint32_t* recent_seg;
  uint32_t* act_list;     // per pass-B segment: the slots the edge kernel has work for (ActEntry), ascending
  uint8_t* flags8;        // per slot: bit 0 = stamp inside the regulariser window, bit 1 = detach request
  uint8_t* dirty8;        // delta tracking (null = off): 1 = a transferred attribute of the slot changed since the
                          // last smx_recon_transfer_changed_to_cpu
  // "Hot" groups (pass B's filter for its far flag gathers, see k_neighbor_scan): per group of slots the number
  // (mod 256) of the last Integrate call in which the group held a slot inside the regulariser window (pass A) or a
  // flag byte / link record of it was written.  `epoch` = this call's number.  (At C2 a group is 2048 slots, at C3 8192.)
  uint8_t* seg_act;       // per pass-A segment: 1 = pass A found visible or recently updated slots in it this frame
  uint32_t descending;    // != 0: this call's all-slot kernels walk the segments downwards (segment_of_block)
  uint32_t plain_gathers; // != 0: the neighbour update gathers without range-checked buffers (RecordGather): group arrays of
                          // 4 GB and more, or scan mode bit 10
  uint8_t* hot_epoch;
  uint16_t* seg_targets;  // per pass-B segment: bitmap of the groups its links point into (see k_neighbor_scan)
  uint32_t n_hot_groups;
  uint32_t epoch;
  int hot_shift;          // slots per group = 1 << hot_shift: the smallest power of two >= 1024 that keeps the table <= 4 KB
};

// Far-term bins of the regulariser (k_reg_accumulate -> k_reg_step): one bin per destination segment of kSegB slots.
// A gradient term whose target lies outside the sender's segment is APPENDED to the target segment's bin -- record =
// (target's position in its segment | sender class << 10, gx, gy, gz in 2^-22 fixed point) -- and the segment's
// workgroup of k_reg_step sums its bin in LDS.  The reference pushes these terms with four float atomics each
// (kernels.cu:2176-2182); rounds 1-2 used exclusive "inbox" slots for symmetric links and two packed 64-bit atomics for
// the rest (0.43 M device-scope atomics and 0.39 M random 16-byte stores per frame at C2, and 64 bytes of inbox per
// recent slot read back by the step).  Appending costs one returning atomic per (sender workgroup, destination segment)
// -- 55 k per frame -- and the records of such a pair are adjacent.
struct FarBins {
  uint4* rec;            // [segments][cap]
  uint32_t* count;       // [segments * kCountStride]: word 0 = terms appended since the bin was last consumed (may exceed cap),
                         // word 1 = "some terms for this segment went to grad_acc instead"; both zeroed by the consumer
  uint32_t cap;
  uint32_t hash_mask;    // size - 1 of the sender's LDS table of destinations (kFarHash - 1; tests shrink it)
};

// Pass A's pairs, binned by association tile (see "association tiles" in smx_recon.hip).
struct TileBins {
  uint2* pairs;          // [n_tiles][cap]: (slot, code)
  uint32_t* count;       // [n_tiles * kCountStride]: pairs appended in this call (zeroed again by the tile's workgroup); may exceed cap,
  uint4* ovf;            // in which case the rest went to this list: (tile, slot, code, -), room for 2 pairs per slot
  uint32_t* ovf_count;   // this call's overflow counter (two in alternation: the tile kernel zeroes the next call's)
  uint32_t cap;
  int tiles_x;
  uint32_t n_tiles;
};

// Exclusive prefix sum of one value per thread over a workgroup of kWaves wavefronts (wave64 shuffles + LDS).
template <int kWaves = kBlock / 64>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t mine, uint32_t* wave_tot /* LDS [kWaves] */, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(incl, off);
    if (lane >= (uint32_t)off) incl += t;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t wave_off = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if ((uint32_t)w < wave) wave_off += wave_tot[w];
    total += wave_tot[w];
  }
  return wave_off + incl - mine;
}

// ---- folds over a wavefront (wave64 shuffles) ----
// one atomic per wavefront: the number of its lanes with `pred`
__device__ __forceinline__ void wave_count(uint32_t* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m != 0 && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(counter, (uint32_t)__popcll(m));
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int32_t wave_imin(int32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int32_t o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int32_t wave_imax(int32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int32_t o = __shfl_xor(v, off); v = o > v ? o : v; }
  return v;
}

// The counts of a launch: every lane counts in registers over its grid-stride loop, the wavefronts fold their lanes by ballots'
// kin (wave_sum) and add to the workgroup's LDS words, and one lane adds each word to the device counter: one global atomic per
// workgroup and counter (the counters of a launch are consecutive words, ctr[0 .. kCounters)).  (One per wavefront and loop trip was 57 k atomics on one address for 3.6 M slots, at ~12 ns apiece
// longer than the kernel's memory traffic.)  Every lane of the workgroup calls this, once, behind its loop.
template <int kCounters>
__device__ __forceinline__ void block_counts(uint32_t* __restrict__ ctr, const uint32_t (&mine)[kCounters]) {
  __shared__ uint32_t tot[kCounters];
  if (threadIdx.x < kCounters) tot[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kCounters; ++c) {
    const uint32_t s = wave_sum(mine[c]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot[c], s);
  }
  __syncthreads();
  if (threadIdx.x < kCounters && tot[threadIdx.x]) atomicAdd(ctr + threadIdx.x, tot[threadIdx.x]);
}

// The maps of the multi-launch blend fallback (kernels.cc:165-166).
struct BlendBufs {
  uint8_t* distance_map; uint8_t* new_distance_map; float* deltas; float* new_deltas;
};

// Pass A's work lists (k_cull_segments -> k_scan_visible).
struct SegWork {
  uint32_t* surv_list;   // segments pass A has to read in this call (any order)
  uint32_t* copy_list;   // culled segments whose flag bytes have to be copied
  uint32_t* count;       // [0] survivors, [1] copies; zeroed for the next call by k_assoc_tiles
};

// ---- the colour of a slot in the viewer buffers, the splat render and the mesh render ----
struct VisColor { uint32_t frame; int window; int flags; };

// float -> u8 for the colour conversions below: the reference converts values in [0, 256) (truncation); outside that
// range its conversion is undefined, here it saturates (NaN -> 0)
__device__ __forceinline__ uint32_t vis_u8(float v) { return (uint32_t)fminf(fmaxf(v, 0.0f), 255.0f); }
__device__ __forceinline__ uint32_t vis_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// The colour word of UpdateSurfelVertexBufferCUDAKernel (kernels.cu:306-349) for one slot, flags in the reference
// template's precedence (smx.h SMX_VIS_*).  Shared by the vertex buffer and the render's colour image.
__device__ __forceinline__ uint32_t vis_color(const Surfels& S, uint32_t i, const VisColor& vc) {
  if (vc.flags & (SMX_VIS_LAST_UPDATE | SMX_VIS_CREATION)) {
    const bool creation = (vc.flags & SMX_VIS_CREATION) != 0;
    const int age = (int)(vc.frame - (creation ? S.u(kCreationStamp, i) : S.u(kLastUpdateStamp, i)));
    const int max_age = creation ? 3000 : vc.window;
    if (age < 1) return vis_rgb(255, 80, 80);
    if (age > max_age) return vis_rgb(40, 40, 255);
    float blend = (float)(age - 1) * 1.0f / (float)(max_age - 1);
    blend = fminf(1.0f, fmaxf(0.0f, blend));
    const uint32_t intensity = (255u - vis_u8(255.99f * blend)) & 255u;
    return vis_rgb(intensity, intensity, intensity);
  }
  if (vc.flags & SMX_VIS_RADII) {
    const float radius = sqrtf(S.f(kRadiusSq, i));
    float blend = (radius - 0.0005f) / (0.01f - 0.0005f);
    blend = fminf(1.0f, fmaxf(0.0f, blend));
    const uint32_t red = vis_u8(255.99f * blend);
    return vis_rgb(red, 255u - red, 80u);
  }
  if (vc.flags & SMX_VIS_NORMALS) {
    const float4 n = *S.group(kGroupN, i);
    return vis_rgb(vis_u8(255.99f / 2.0f * (n.x + 1.0f)), vis_u8(255.99f / 2.0f * (n.y + 1.0f)),
                   vis_u8(255.99f / 2.0f * (n.z + 1.0f)));
  }
  return S.u(kColor, i);
}

// ---- workspaces of the services in smx_recon_map.hip (allocated by the first call that needs them) ----
// Row-layout staging for the boundary conversions (TransferAllToCPU, the delta hand-off, debug rows, compaction).  The mark
// is recorded after the last enqueued read: TransferAllToCPU returns with its row downloads in flight, and the next user
// may come on another stream.
struct StagingWork { DevBuf<float> buf; StreamMark mark; };
// smx_recon_compact, all or none: old_to_new [pitch], per-segment counts / offsets [nseg], [0] = new count, [1] = links dropped
struct CompactWork { DevBuf<uint32_t> map, seg, out; };
// smx_recon_neighbor_candidates: queries [4][capacity] and staged slots [capacity], both or none; a host array's state bytes
struct CandidateWork { DevBuf<float> q; DevBuf<uint32_t> slots; DevBuf<uint8_t> state; };

}  // namespace smx

// Created value-initialised (everything zero / empty) and deleted as a whole: `mem` owns the blocks smx_recon_create
// allocates -- the pointers in S, L, fb, sc, tb, sw, bb and the plain pointer members below are views of them -- every
// buffer a service allocates on demand is a DevBuf, and every event a service creates belongs to a StreamMark or a
// PhaseStamps of its workspace.  The frame loop's own events and stream are created and destroyed by smx_recon_create /
// _destroy.
struct smx_recon_s {
  smx::DevBlocks mem;
  int device;               // the HIP device the object lives on (every entry point runs on it)
  uint32_t max_surfels;
  int W, H;
  float fx, fy, cx, cy;
  smx::Surfels S;
  long long* grad_acc;      // [slots][2] packed fixed point (see pack_pair), cross-segment contributions (atomics)
  float4* reg_rec;          // two dense arrays [slots + kSegAcc] of the recent slots' results, by (segment, rank in its recent list):
                            // the in-segment sums, then the own terms (each written by ONE store instruction per chunk: full sectors)
  smx::FarBins fb;               // far terms of the regulariser, per destination segment (see FarBins)
  smx::Lists L;
  int nseg;                 // number of kSeg-slot segments (= workgroups of pass A)
  int nsegB;                // number of kSegB-slot segments (= workgroups of pass B)
  uint8_t* merge_flag;
  bool table_valid;         // flag table's "recent" bits correspond to (table_frame, table_window)
  uint32_t table_frame;
  int table_window;
  int stats_enabled;
  hipEvent_t hook_consumed, hook_chain;   // smx_recon_integrate_hooks: one-shot, taken by the next Integrate call
  hipEvent_t hook_ready;                  // smx_recon_integrate_inputs_ready: likewise
  int blend_multi_launch;   // A/B switch: 1 = the reference's start + iteration launches instead of the fused kernel
  smx::Scratch sc;               // the association images (every pixel is rewritten by k_assoc_tiles in every call)
  smx::TileBins tb;              // pass A's pairs, binned by association tile
  smx::SegWork sw;               // pass A's work lists (k_cull_segments -> k_scan_visible)
  bool sw_dirty;            // a call failed between the cull step and the tile kernel: the lists' counters are not zero
  hipEvent_t pending_mark;  // != null: the caller's stream has not waited for the previous call's update + create yet (smx_recon_integrate)
  uint32_t* ovf_count_set[2];   // overflow counters, alternating by call (the tile kernel zeroes the next call's)
  unsigned long long* stamps;   // -DSMX_STAMPS builds: [3][8192 workgroups][16] shader clocks (tile kernel, blend kernel), wall clocks + counts (edge kernel)
  int no_lds_tables;        // A/B switch (scan mode bit 4)
  int blend_other_tile;     // A/B switch (scan mode bit 7)
  int cu_count;             // compute units of the object's device
  uint32_t bin_cap_full;    // the bins' allocated capacity (tb.cap is lowered by the A/B switch that forces overflows)
  uint32_t* vis_count_set[2];   // chunk counters of the visible list, alternating by call (k_update_and_create zeroes the next call's)
  uint32_t* dir_host;           // page-locked word: the direction the tile kernel last chose for the all-slot kernels
  uint32_t* dir_dev;            // (segment_of_block); its device alias
  int sc_cur;
  int hot_holdoff;          // > 0: pass B does not use the hot-group table (decremented per Integrate call)
  int hot_filter_enabled;   // A/B switch (smx_recon_set_scan_mode bit 2 clears it)
  int fuse_edges;           // pass B does the edge work of its segment itself (one launch less); scan mode bit 9 sets it
  uint16_t* blended_depth;  // [H][W] output of the fused blend (stored into the caller's depth by k_new_flags_scan)
  smx::BlendBufs bb;
  uint8_t* new_flags;
  uint32_t* new_ranks;
  uint32_t* block_sums;     // per k_new_flags_scan workgroup: flagged pixels
  uint32_t* block_offsets;  // exclusive scan of block_sums (written by k_new_create's workgroup 0)
  uint32_t* tmp_u32;  // [W*H] debug decode target
  int n_scan_blocks;
  smx::DevState* st;
  int scan_mode;
  int timing_enabled;       // bit 0: the reference's 14 stage events, bit 1: events around every kernel, bit 2: stage stamps (default)
  bool have_timings;
  unsigned long long* ts_ring;   // [kTsRing][kTsWords] stage stamps of the last kTsRing Integrate calls (StageStamps)
  unsigned long long* ts_host;   // page-locked copy target of the ring (the waiting read)
  volatile unsigned long long* ts_mapped;   // page-locked ring the tile kernel copies complete records into (the non-waiting read)
  unsigned long long* ts_mapped_dev;        // ... its device alias
  unsigned long long ts_seq;     // Integrate calls with stamps so far (a call's record: ts_ring[seq % kTsRing])
  int wall_khz;                  // rate of the device's wall clock (hipDeviceAttributeWallClockRate)
  hipEvent_t ev[14];
  // per-kernel instrumentation (timing_enabled bit 1) and single-kernel profiling over many frames
  hipEvent_t kev[2 * 16];
  bool kev_recorded[16];
  int prof_slot;
  int prof_cap, prof_n;
  hipEvent_t* prof_ev;
  smx::DevBuf<uint8_t> dirty;         // delta tracking: the block behind L.dirty8 while it is on
  smx::DevBuf<uint32_t> delta_seg;    // delta hand-off: per-segment counts / offsets, and the total
  smx::DevBuf<uint32_t> delta_total;
  int grid_surfels;  // persistent grid for the grid-stride all-slot kernels
  int grid_list;     // persistent grid of the chunked list kernels
  int grid_acc;      // ... of the edge kernel (512-lane workgroups)
  int grid_list_full; // (grid_list is lowered by the A/B switch that forces long walks)
  int debug_skip;    // smx_recon_debug_set_skip (timing only)
  // Frame pipelining: the regulariser of frame f runs on an internal stream while the caller's stream already
  // executes clear / pass A / associate / merge / blend of frame f+1 (those read only P and N records, which the
  // regulariser does not write, and a second copy of the flag table).  Every entry point first orders the
  // caller's stream after the pending regulariser, so the API keeps its one-stream semantics.
  int overlap_enabled;
  hipStream_t reg_stream;     // high priority: the frame-to-frame critical path (integrate .. regulariser)
  uint32_t* gate_count;       // blend workgroups that have released their output, all calls (k_front_gate)
  uint32_t gate_expected;     // ... the value after the last call enqueued with the device-word hand-over
  int handover_mode;          // smx_recon_set_handover_mode: 1 = device word + gate kernel for front -> integration, 0 = event
  hipEvent_t ev_front;        // caller's stream: pass A .. flags of a call are enqueued
  hipEvent_t ev_upd;          // internal stream: update + create of a call are enqueued (the inputs are consumed, the map is ready for the next pass A)
  hipEvent_t ev_reg;          // internal stream: end of the work enqueued so far (recorded on demand by join_regularizer)
  bool reg_pending;
  hipStream_t last_stream;    // the caller's stream of the last Integrate call
  uint8_t* flags_buf[2];    // the flag table is double-buffered by frame (L.flags8 = the current frame's)
  bool have_frame;          // an Integrate call has been made since creation / the last state upload
  uint32_t last_frame;      // its frame_index: the segment culling of pass A presumes that it never decreases
  // ---- the map services: one workspace each, reached by the service's own file only ----
  smx::StagingWork staging;       // smx_recon_map.hip and the delta hand-off
  smx::RenderWork render;         // smx_recon_render and smx_recon_render_mesh (and, through the first, tracking)
  smx::TrackWork track;           // smx_recon_track / _rgbd
  smx::DecimateWork decimate;     // smx_recon_decimate_mesh
  smx::ComponentsWork components; // smx_recon_mesh_components
  smx::FillWork fill;             // smx_recon_fill_holes
  smx::DistanceWork distance;     // smx_recon_mesh_distance
  smx::RimWork rim;               // smx_recon_mesh_rim
  smx::RaycastWork raycast;       // smx_recon_raycast_mesh
  smx::SampleWork sample;         // smx_recon_sample_mesh
  smx::CompareWork compare;       // smx_recon_compare_meshes
  smx::RegisterMeshWork register_mesh;   // smx_recon_register_mesh
  smx::CompactWork compact;       // smx_recon_compact
  smx::CandidateWork candidates;  // smx_recon_neighbor_candidates
  smx::MergeWork merge;           // smx_recon_merge_map (this object as the destination)
  smx::ImportWork import;         // smx_recon_import_points
  smx::MeshWorkspace* mesh;       // smx_recon_triangulate / _update (created by the first call): lists, rings, counts, output staging
};

namespace smx {

// ---- host helpers shared by the object's files (defined in smx_recon.hip) -----------------------------------------
// Orders stream st after the regulariser that may still run on the internal stream.
int join_regularizer(smx_recon r, hipStream_t st);
// The slot count (merged slots included), read back on st; returns with st synchronised.
int read_surfel_count(smx_recon r, hipStream_t st, uint32_t* n);
// Exclusive scan in place of per-segment counts, the total to *total_out (k_delta_scan: the delta hand-off and compaction).
void enqueue_segment_scan(hipStream_t st, uint32_t* seg_count, int nseg, uint32_t* total_out);
// Every user of the shared staging buffer first orders its stream after the previous user's last read (and gets room
// for `floats`), and leaves its mark after its own.
int acquire_staging(smx_recon r, hipStream_t st, size_t floats);
int release_staging(smx_recon r, hipStream_t st);
// After surfel attributes were changed from outside the frame loop (state upload, compaction, deformation).
int invalidate_derived(smx_recon r, hipStream_t st);
// The regulariser's accumulators and the merge marks, as a state upload leaves them (smx_recon_map.hip).
int reset_accumulators(smx_recon r, hipStream_t st);
// ... and what compaction and a map merge reset beyond that: both flag tables, the streaks, the hot marks, the link bitmaps
// (smx_recon_map.hip; calls reset_accumulators and invalidate_derived).
int reset_derived_after_rewrite(smx_recon r, hipStream_t st);

}  // namespace smx
