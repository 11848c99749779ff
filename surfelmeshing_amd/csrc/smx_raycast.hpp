// smx_raycast.hpp -- rays against a triangle array over the map (smx_recon_raycast_mesh).
//
// Part 1: the arithmetic of the contract and the traversal as plain inline functions (the BAD test of a ray, the candidate test
// of step 3 with its key, the inflated box of a triangle, the saturating cell function, the dominant axis and its layers, the t
// interval and the cell rectangle of one layer, the exit test, the walk of one ray).  smx_raycast.hip calls them from its
// kernels; a test compiles this part alone for the host (SMX_RAYCAST_HOST_ONLY) and walks the same passes with plain words.
// The classes of step 1, the cell key, the cell table and the packed records are those of smx_distance.hpp.
// Part 2: the workspace the object keeps for the call (kernels and glue: smx_raycast.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_RAYCAST_HOST_ONLY)
#if !defined(SMX_DISTANCE_HOST_ONLY)
#define SMX_DISTANCE_HOST_ONLY 1
#endif
#endif
#include "smx_distance.hpp"
#define SMX_RAY_FN SMX_DIST_FN

namespace smx {

constexpr float kRayMaxOrigin = 64.0f;                      // |O_k| above this: BAD (SMX_DIST_MAX_COORD)
constexpr float kRayMaxDir = 1024.0f;                       // SMX_RAY_MAX_DIR
constexpr float kRayMinDir = 0.0009765625f;                 // SMX_RAY_MIN_DIR = 2^-10
constexpr float kRayMaxT = 1048576.0f;                      // SMX_RAY_MAX_T = 2^20
constexpr float kRayBoxSlack = 0.000244140625f;             // SMX_RAY_BOX_SLACK = 2^-12 m
constexpr float kRayMinCell = 0.001953125f;                 // SMX_RAY_MIN_CELL = 2^-9 m
constexpr float kRayCellLimit = 1073741824.0f;              // the cell function of the traversal saturates at +-2^30
// how far the solved ends of a layer's t interval are moved outwards before the cell function is asked: this much along the
// dominant axis (a few ulps of 64 m), and this share of |t|.  Only the number of doublings depends on them, never an answer.
constexpr float kRayPad = 0.000030517578125f;               // 2^-15 m
constexpr float kRayPadT = 4.76837158203125e-7f;            // 2^-21
enum : uint32_t { kRayFlagBad = 1u, kRayFlagHit = 2u, kRayFlagFront = 4u };

// ---- step 2 --------------------------------------------------------------------------------------------------------------
SMX_RAY_FN float ray_abs(float v) { return v < 0.0f ? -v : v; }
SMX_RAY_FN bool ray_bad(const DistVec& O, const DistVec& D) {
  if (!(dist_point_ok(O) && dec_finite(D.x) && dec_finite(D.y) && dec_finite(D.z))) return true;
  const float ax = ray_abs(D.x), ay = ray_abs(D.y), az = ray_abs(D.z);
  if (ax > kRayMaxDir || ay > kRayMaxDir || az > kRayMaxDir) return true;
  return dist_max3(ax, ay, az) < kRayMinDir;
}

// ---- step 3 --------------------------------------------------------------------------------------------------------------
SMX_RAY_FN float ray_at(float o, float d, float t) { return o + t * d; }      // H_k: a product, then a sum
SMX_RAY_FN bool ray_in_slab(float h, float a, float b, float c) {
  return dist_min3(a, b, c) - kRayBoxSlack <= h && h <= dist_max3(a, b, c) + kRayBoxSlack;
}
struct RayHit { float t, u, v, det; };
// The key of triangle i for the ray: (float_bits(t + 0.0f) << 32) | i if it is a candidate, kDistNone otherwise.
SMX_RAY_FN unsigned long long ray_key(const DistVec& O, const DistVec& D, const DistVec& A, const DistVec& B, const DistVec& C, uint32_t i,
                                      float t_min, float t_max, int cull, RayHit* hit) {
  const DistVec e1 = dist_sub(B, A), e2 = dist_sub(C, A), p = dist_cross(D, e2);
  const float det = dist_dot(e1, p);
  if (!(det > 0.0f || det < 0.0f)) return kDistNone;
  if ((cull == 1 && !(det > 0.0f)) || (cull == 2 && !(det < 0.0f))) return kDistNone;
  const float inv = 1.0f / det;
  const DistVec s = dist_sub(O, A);
  const float u = dist_dot(s, p) * inv;
  const DistVec q = dist_cross(s, e1);
  const float v = dist_dot(D, q) * inv, w = u + v, t = dist_dot(e2, q) * inv;
  if (!(u >= 0.0f && v >= 0.0f && w <= 1.0f && t >= t_min && t <= t_max)) return kDistNone;
  if (!(ray_in_slab(ray_at(O.x, D.x, t), A.x, B.x, C.x) && ray_in_slab(ray_at(O.y, D.y, t), A.y, B.y, C.y) &&
        ray_in_slab(ray_at(O.z, D.z, t), A.z, B.z, C.z)))
    return kDistNone;
  hit->t = t + 0.0f; hit->u = u; hit->v = v; hit->det = det;
  return dec_value_word(t + 0.0f, i);
}

// ---- the grid ------------------------------------------------------------------------------------------------------------
SMX_RAY_FN float ray_cell_size(float cell_size) { return cell_size > kRayMinCell ? cell_size : kRayMinCell; }
// The box of the cells a triangle is entered in: from the cell of min3 - SLACK to the cell of max3 + SLACK, the expressions of
// step 3.  |x| <= 64 + SLACK and c >= 2^-9: |x / c| < 2^16, inside the 21 bits of dec_cell_key.
SMX_RAY_FN DistBox ray_box(const DistVec& a, const DistVec& b, const DistVec& c, float cell) {
  DistBox box;
  box.lo[0] = dist_cell(dist_min3(a.x, b.x, c.x) - kRayBoxSlack, cell); box.hi[0] = dist_cell(dist_max3(a.x, b.x, c.x) + kRayBoxSlack, cell);
  box.lo[1] = dist_cell(dist_min3(a.y, b.y, c.y) - kRayBoxSlack, cell); box.hi[1] = dist_cell(dist_max3(a.y, b.y, c.y) + kRayBoxSlack, cell);
  box.lo[2] = dist_cell(dist_min3(a.z, b.z, c.z) - kRayBoxSlack, cell); box.hi[2] = dist_cell(dist_max3(a.z, b.z, c.z) + kRayBoxSlack, cell);
  return box;
}
// dist_cell held to +-2^30, for coordinates far along a ray: monotone in x like dist_cell, and equal to it wherever a triangle
// of R can be entered.
SMX_RAY_FN int32_t ray_cell(float x, float c) {
  float q = floorf(x / c);
  q = q < -kRayCellLimit ? -kRayCellLimit : (q > kRayCellLimit ? kRayCellLimit : q);
  return (int32_t)q;
}

// ---- the traversal -------------------------------------------------------------------------------------------------------
// The ray with its components in the order (a, b, c): a = the dominant axis (largest |D_a|, the lowest axis on a tie), b and c
// the other two in ascending order; the occupied box in the same order; the layers of a the ray's [t_min, t_max] meets inside
// the occupied box, numbered 0 .. n_layers - 1 in the order the ray meets them (layer m is cell first + sgn * m of axis a).
struct RayAxes {
  float oa, ob, oc, da, db, dc;
  int32_t lo_b, hi_b, lo_c, hi_c;
  int32_t axis, sgn, first;
  uint32_t n_layers;
};
// occ = the occupied cell box: lo x, y, z, hi x, y, z (lo > hi: no cell is occupied).
SMX_RAY_FN RayAxes ray_axes(const DistVec& O, const DistVec& D, int32_t lo_x, int32_t lo_y, int32_t lo_z, int32_t hi_x, int32_t hi_y,
                            int32_t hi_z, float cell, float t_min, float t_max) {
  RayAxes r;
  const float ax = ray_abs(D.x), ay = ray_abs(D.y), az = ray_abs(D.z);
  r.axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  int32_t lo_a, hi_a;
  if (r.axis == 0) {
    r.oa = O.x; r.da = D.x; r.ob = O.y; r.db = D.y; r.oc = O.z; r.dc = D.z;
    lo_a = lo_x; hi_a = hi_x; r.lo_b = lo_y; r.hi_b = hi_y; r.lo_c = lo_z; r.hi_c = hi_z;
  } else if (r.axis == 1) {
    r.oa = O.y; r.da = D.y; r.ob = O.x; r.db = D.x; r.oc = O.z; r.dc = D.z;
    lo_a = lo_y; hi_a = hi_y; r.lo_b = lo_x; r.hi_b = hi_x; r.lo_c = lo_z; r.hi_c = hi_z;
  } else {
    r.oa = O.z; r.da = D.z; r.ob = O.x; r.db = D.x; r.oc = O.y; r.dc = D.y;
    lo_a = lo_z; hi_a = hi_z; r.lo_b = lo_x; r.hi_b = hi_x; r.lo_c = lo_y; r.hi_c = hi_y;
  }
  r.sgn = r.da > 0.0f ? 1 : -1;
  r.first = 0; r.n_layers = 0;
  if (lo_a > hi_a) return r;
  const int32_t l0 = ray_cell(ray_at(r.oa, r.da, t_min), cell), l1 = ray_cell(ray_at(r.oa, r.da, t_max), cell);
  if (r.sgn > 0) {                                   // l0 <= l1 by monotonicity
    const int32_t from = l0 > lo_a ? l0 : lo_a, to = l1 < hi_a ? l1 : hi_a;
    r.first = from;
    if (from <= to) r.n_layers = (uint32_t)(to - from) + 1u;
  } else {                                           // l0 >= l1
    const int32_t from = l0 < hi_a ? l0 : hi_a, to = l1 > lo_a ? l1 : lo_a;
    r.first = from;
    if (from >= to) r.n_layers = (uint32_t)(from - to) + 1u;
  }
  return r;
}
// The number of the layer that holds H_a(t), in the order of the walk (negative: before the first layer).
SMX_RAY_FN int32_t ray_layer_of(const RayAxes& r, float cell, float t) {
  return r.sgn * (ray_cell(ray_at(r.oa, r.da, t), cell) - r.first);     // (|cell| <= 2^30 and |first| < 2^17)
}
// One end of layer L's t interval: `solved` moved outwards (dir = -1: towards t_min, +1: towards t_max) until the cell
// function itself puts H_a there strictly outside L on that side, or the end of [t_min, t_max] is reached.
SMX_RAY_FN float ray_layer_end(const RayAxes& r, float cell, int32_t L, float solved, int dir, float limit) {
  float pad = kRayPad / ray_abs(r.da) + ray_abs(solved) * kRayPadT;
  for (;;) {
    const float t = dir < 0 ? solved - pad : solved + pad;
    if (dir < 0 ? !(t > limit) : !(t < limit)) return limit;
    const int32_t side = r.sgn * (ray_cell(ray_at(r.oa, r.da, t), cell) - L);
    if (dir < 0 ? side < 0 : side > 0) return t;
    pad += pad;
  }
}
struct RayRect { int32_t b0, b1, c0, c1; };            // cells [b0, b1] x [c0, c1] of the axes b and c; empty if b0 > b1 or c0 > c1
SMX_RAY_FN void ray_span(float o, float d, float t0, float t1, float cell, int32_t lo, int32_t hi, int32_t* x0, int32_t* x1) {
  const int32_t p = ray_cell(ray_at(o, d, t0), cell), q = ray_cell(ray_at(o, d, t1), cell);
  const int32_t mn = p < q ? p : q, mx = p < q ? q : p;
  *x0 = mn > lo ? mn : lo; *x1 = mx < hi ? mx : hi;
}
// The cells of layer m the ray can meet: every t of [t_min, t_max] with H_a(t) in the layer lies in [t0, t1], because
// t -> H_a(t) is monotone and H_a(t0), H_a(t1) lie outside the layer (or t0, t1 are the ends); H_b and H_c are monotone too, so
// their cells over [t0, t1] lie between their cells at the two ends.
SMX_RAY_FN RayRect ray_layer_rect(const RayAxes& r, float cell, float t_min, float t_max, uint32_t m) {
  const int32_t L = r.first + r.sgn * (int32_t)m;
  const float near_plane = (float)(r.sgn > 0 ? L : L + 1) * cell, far_plane = (float)(r.sgn > 0 ? L + 1 : L) * cell;
  const float t0 = ray_layer_end(r, cell, L, (near_plane - r.oa) / r.da, -1, t_min);
  const float t1 = ray_layer_end(r, cell, L, (far_plane - r.oa) / r.da, +1, t_max);
  RayRect q;
  ray_span(r.ob, r.db, t0, t1, cell, r.lo_b, r.hi_b, &q.b0, &q.b1);
  ray_span(r.oc, r.dc, t0, t1, cell, r.lo_c, r.hi_c, &q.c0, &q.c1);
  return q;
}
SMX_RAY_FN uint32_t ray_rect_cells(const RayRect& q) {
  return (q.b0 > q.b1 || q.c0 > q.c1) ? 0u : ((uint32_t)(q.b1 - q.b0) + 1u) * ((uint32_t)(q.c1 - q.c0) + 1u);
}
// cell number j (0 <= j < ray_rect_cells) of layer m's rectangle, b fastest, as the key of the cell table
SMX_RAY_FN unsigned long long ray_rect_key(const RayAxes& r, const RayRect& q, uint32_t m, uint32_t j) {
  const uint32_t nb = (uint32_t)(q.b1 - q.b0) + 1u;
  const int32_t a = r.first + r.sgn * (int32_t)m, b = q.b0 + (int32_t)(j % nb), c = q.c0 + (int32_t)(j / nb);
  return r.axis == 0 ? dec_cell_key(a, b, c) : (r.axis == 1 ? dec_cell_key(b, a, c) : dec_cell_key(b, c, a));
}
// After layer m: may the walk stop?  Yes once the layer of H_a(t_best) lies strictly before layer m + 1: every candidate not
// yet met has its H in a later layer, so by monotonicity a larger t and a larger key.
SMX_RAY_FN bool ray_done(const RayAxes& r, float cell, unsigned long long best, uint32_t next_layer) {
  if (best == kDistNone) return false;
  const int32_t at = ray_layer_of(r, cell, dist_key_dist2(best));
  return at < 0 || (uint32_t)at < next_layer;
}

// The smallest key over records [first, end), stepping by `stride` (the lanes of a wavefront share a run).
template <class Recs>
SMX_RAY_FN unsigned long long ray_walk(const Recs& recs, uint32_t first, uint32_t end, uint32_t stride, const DistVec& O, const DistVec& D,
                                       float t_min, float t_max, int cull, unsigned long long best, uint32_t* tests) {
  for (uint32_t j = first; j < end; j += stride) {
    DistVec A, B, C;
    uint32_t i;
    RayHit h;
    recs.load(j, &A, &B, &C, &i);
    const unsigned long long key = ray_key(O, D, A, B, C, i, t_min, t_max, cull, &h);
    best = key < best ? key : best;
    ++*tests;
  }
  return best;
}

// One ray's view of the cast: the wide list, then layer after layer.  k_ray_cast makes the same look-ups 64 layers at a time and
// walks the same records with its lanes sharing a run; the host walk calls this as it stands.  Seen: void operator()(cell key)
// for every cell looked up (the tests' completeness check); early_exit = false walks every layer.
struct RayWork { uint32_t layers, lookups, tests; };
template <class Tab, class Recs, class Seen>
SMX_RAY_FN unsigned long long ray_cast_one(const Tab& tab, uint32_t mask, const Recs& cell_recs, const Recs& wide_recs, uint32_t n_wide,
                                           const RayAxes& r, const DistVec& O, const DistVec& D, float cell, float t_min, float t_max, int cull,
                                           bool early_exit, Seen& seen, RayWork* work) {
  unsigned long long best = ray_walk(wide_recs, 0, n_wide, 1, O, D, t_min, t_max, cull, kDistNone, &work->tests);
  for (uint32_t m = 0; m < r.n_layers; ++m) {
    if (early_exit && ray_done(r, cell, best, m)) break;
    const RayRect q = ray_layer_rect(r, cell, t_min, t_max, m);
    const uint32_t cells = ray_rect_cells(q);
    ++work->layers;
    for (uint32_t j = 0; j < cells; ++j) {
      const unsigned long long key = ray_rect_key(r, q, m, j);
      uint32_t first, end;
      seen(key);
      ++work->lookups;
      if (dist_table_find(tab, mask, key, &first, &end)) best = ray_walk(cell_recs, first, end, 1, O, D, t_min, t_max, cull, best, &work->tests);
    }
  }
  return best;
}

#if !defined(SMX_RAYCAST_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of the device counters: [kRayCellBits] = c as its bits, [kRayOccLo .. +2] / [kRayOccHi .. +2] = the occupied cell
// box as int32, the 64-bit words as (lo, hi) pairs
enum : int { kRayNotLive = 0, kRayRepeated, kRayRange, kRayInRCount, kRayNWide, kRayEntries, kRayCells, kRayBadRays, kRayHits, kRayFrontHits,
             kRayMaxBits, kRayError, kRayCellBits, kRayOccLo = 13, kRayOccHi = 16, kRayPadWord = 19, kRayExtentLo = 20, kRayExtentHi,
             kRayEntries64Lo, kRayEntries64Hi, kRayLayersLo, kRayLayersHi, kRayLookupsLo, kRayLookupsHi, kRayTestsLo, kRayTestsHi, kRayWords = 32 };

constexpr int kRayBlock = 256;                               // triangles, entries or rays (k_ray_cast: 4 rays) per workgroup
constexpr int kRayWaves = kRayBlock / 64;

// The workspace, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so nothing
// reads a block that goes.
struct RaycastWork {
  DevBuf<uint32_t> mark;                   // [n_in] entry count of the triangle, kDistWide, or 0 (not in R)
  DevBuf<uint32_t> blocks;                 // entries per workgroup, then their offsets
  DevBuf<uint32_t> wide_t;                 // [n_wide] the wide list, in arrival order (the minimum does not depend on it)
  DevBuf<unsigned long long> keys[2];      // [n_entries] the sort's records
  DevBuf<uint32_t> vals[2];
  DevBuf<uint32_t> hist;                   // the sort's workspace
  DevBuf<float> recs, wide_recs;           // [n_entries] / [n_wide] DistRec, the first in the sorted order
  DevBuf<unsigned long long> table;        // [table entries][2] DistCell
  DevBuf<unsigned long long> best;         // [n_rays] the winning key of every ray
  DevBuf<uint32_t> work;                   // [n_rays][4] layers, look-ups, pair tests, flags of every ray
  DevBuf<uint32_t> in;                     // staging when the caller's arrays are host memory
  DevBuf<float> rays, out_t, out_uv;
  DevBuf<uint32_t> out_hit;
  DevBuf<uint32_t> counters;               // [kRayWords]
  PhaseStamps<SMX_RAY_PHASES> stamps;      // of the last call; a refused call publishes the phases it completed
};

// ---- what smx_raycast.hip and smx_rayscene.hip share: how a kernel reads the table and the records, the wave folds ----------
struct RayDeviceTable {
  DistCell* e;
  __device__ __forceinline__ unsigned long long key(uint32_t h) const { return e[h].key; }
  __device__ __forceinline__ unsigned long long value(uint32_t h) const { return e[h].value; }
  __device__ __forceinline__ unsigned long long claim(uint32_t h, unsigned long long expected, unsigned long long desired) const {
    return atomicCAS(&e[h].key, expected, desired);
  }
  __device__ __forceinline__ void bump(uint32_t h, unsigned long long inc) const { atomicAdd(&e[h].value, inc); }
};

struct RayDeviceRecs {
  const DistRec* r;
  __device__ __forceinline__ void load(uint32_t j, DistVec* A, DistVec* B, DistVec* C, uint32_t* i) const {
    const DistRec x = r[j];
    *A = DistVec{x.a.x, x.a.y, x.a.z}; *B = DistVec{x.b.x, x.b.y, x.b.z}; *C = DistVec{x.c.x, x.c.y, x.c.z};
    *i = __float_as_uint(x.a.w);
  }
};

// one atomic per wavefront: the number of its lanes with `pred`
__device__ __forceinline__ void ray_wave_count(uint32_t* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m != 0 && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(counter, (uint32_t)__popcll(m));
}
__device__ __forceinline__ unsigned long long ray_wave_min(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned long long ray_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int32_t ray_wave_imin(int32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int32_t o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int32_t ray_wave_imax(int32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int32_t o = __shfl_xor(v, off); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ void ray_load(const float* rays, uint32_t p, DistVec* O, DistVec* D) {
  const float* r = rays + 6 * (size_t)p;
  *O = DistVec{r[0], r[1], r[2]}; *D = DistVec{r[3], r[4], r[5]};
}

inline unsigned ray_blocks(uint32_t n) { return (unsigned)div_up(n, kRayBlock); }
inline bool ray_finite_f(float v) { return v - v == 0.0f; }
inline bool ray_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
inline unsigned long long ray_word64(const uint32_t* h, int lo) { return ((unsigned long long)h[lo + 1] << 32) | h[lo]; }

// The mark and the index phase of smx_recon_raycast_mesh, enqueued on st (smx_raycast.hip).  The caller has reserved w.mark,
// w.blocks ([div_up(n_in, kRayBlock)]) and w.wide_t for n_in and zeroed the kRayWords words of cnt; din is device memory.
// Between the two it reads cnt back: kRayError, the 64-bit entry count, E = [kRayEntries] and Wd = [kRayNWide].
int ray_enqueue_mark(RaycastWork& w, const DistMap& map, const uint32_t* din, uint32_t n_in, float cell_size, uint32_t* cnt, hipStream_t st);
// Reserves the sort's buffers in w, then recs, wide_recs and table (the caller's: the workspace's own, or a scene's), in the
// order the call always has; *sorted_keys = the E sorted cell keys, in w until its next use.
int ray_enqueue_index(RaycastWork& w, const DistMap& map, const uint32_t* din, uint32_t n_in, uint32_t E, uint32_t Wd, uint32_t* cnt,
                      DevBuf<float>& recs, DevBuf<float>& wide_recs, DevBuf<unsigned long long>& table, uint32_t* mask,
                      const unsigned long long** sorted_keys, hipStream_t st);
#endif

}  // namespace smx
