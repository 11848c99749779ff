// smx_raycast.hpp -- rays against a triangle array over the map: the one traversal of smx_recon_raycast_mesh and
// of a kept scene (smx_rayscene).
//
// Part 1: the arithmetic of the contract and the traversal as plain inline functions (the BAD test of a ray, the candidate test
// of step 3 with its key, the inflated box of a triangle, the saturating cell function, the dominant axis and its layers, the t
// interval and the cell rectangle of one layer, the exit test, the look-up of a cell behind an optional occupancy bit grid, the
// walk of a run of records that keeps the winner's (u, v, det), the walk of one ray).  smx_raycast.hip calls them from its
// kernels; the ray host tests compile this part alone for the host (SMX_RAYCAST_HOST_ONLY) and walk the same passes with plain words.
// The classes of step 1, the cell key, the cell table and the packed records are the triangle grid's (smx_trigrid.hpp).
// Part 2: the counter words, an index a cast can read, a cast's workspace and the host functions of a cast, and the workspace
// the object keeps for the one-shot call (kernels and glue: smx_raycast.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_RAYCAST_HOST_ONLY) && !defined(SMX_TRIGRID_HOST_ONLY)
#define SMX_TRIGRID_HOST_ONLY 1
#endif
#include "smx_trigrid.hpp"
#define SMX_RAY_FN SMX_TG_FN

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
SMX_RAY_FN bool ray_bad(const TgVec& O, const TgVec& D) {
  if (!(tg_point_ok(O) && dec_finite(D.x) && dec_finite(D.y) && dec_finite(D.z))) return true;
  const float ax = ray_abs(D.x), ay = ray_abs(D.y), az = ray_abs(D.z);
  if (ax > kRayMaxDir || ay > kRayMaxDir || az > kRayMaxDir) return true;
  return tg_max3(ax, ay, az) < kRayMinDir;
}

// ---- step 3 --------------------------------------------------------------------------------------------------------------
SMX_RAY_FN float ray_at(float o, float d, float t) { return o + t * d; }      // H_k: a product, then a sum
SMX_RAY_FN bool ray_in_slab(float h, float a, float b, float c) {
  return tg_min3(a, b, c) - kRayBoxSlack <= h && h <= tg_max3(a, b, c) + kRayBoxSlack;
}
struct RayHit { float t, u, v, det; };
// The key of triangle i for the ray: (float_bits(t + 0.0f) << 32) | i if it is a candidate, kTgNone otherwise.
SMX_RAY_FN unsigned long long ray_key(const TgVec& O, const TgVec& D, const TgVec& A, const TgVec& B, const TgVec& C, uint32_t i,
                                      float t_min, float t_max, int cull, RayHit* hit) {
  const TgVec e1 = tg_sub(B, A), e2 = tg_sub(C, A), p = tg_cross(D, e2);
  const float det = tg_dot(e1, p);
  if (!(det > 0.0f || det < 0.0f)) return kTgNone;
  if ((cull == 1 && !(det > 0.0f)) || (cull == 2 && !(det < 0.0f))) return kTgNone;
  const float inv = 1.0f / det;
  const TgVec s = tg_sub(O, A);
  const float u = tg_dot(s, p) * inv;
  const TgVec q = tg_cross(s, e1);
  const float v = tg_dot(D, q) * inv, w = u + v, t = tg_dot(e2, q) * inv;
  if (!(u >= 0.0f && v >= 0.0f && w <= 1.0f && t >= t_min && t <= t_max)) return kTgNone;
  if (!(ray_in_slab(ray_at(O.x, D.x, t), A.x, B.x, C.x) && ray_in_slab(ray_at(O.y, D.y, t), A.y, B.y, C.y) &&
        ray_in_slab(ray_at(O.z, D.z, t), A.z, B.z, C.z)))
    return kTgNone;
  hit->t = t + 0.0f; hit->u = u; hit->v = v; hit->det = det;
  return dec_value_word(t + 0.0f, i);
}

// ---- the grid ------------------------------------------------------------------------------------------------------------
SMX_RAY_FN float ray_cell_size(float cell_size) { return tg_cell_size(cell_size, kRayMinCell); }
// The box of the cells a triangle is entered in: from the cell of min3 - SLACK to the cell of max3 + SLACK, the expressions of
// step 3.  |x| <= 64 + SLACK and c >= 2^-9: |x / c| < 2^16, inside the 21 bits of dec_cell_key.
SMX_RAY_FN TgBox ray_box(const TgVec& a, const TgVec& b, const TgVec& c, float cell) { return tg_box_slack(a, b, c, cell, kRayBoxSlack); }
// tg_cell held to +-2^30, for coordinates far along a ray: monotone in x like tg_cell, and equal to it wherever a triangle
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
SMX_RAY_FN RayAxes ray_axes(const TgVec& O, const TgVec& D, int32_t lo_x, int32_t lo_y, int32_t lo_z, int32_t hi_x, int32_t hi_y,
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
// cell number j (0 <= j < ray_rect_cells) of layer m's rectangle, b fastest
SMX_RAY_FN void ray_rect_cell(const RayAxes& r, const RayRect& q, uint32_t m, uint32_t j, int32_t* x, int32_t* y, int32_t* z) {
  const uint32_t nb = (uint32_t)(q.b1 - q.b0) + 1u;
  const int32_t a = r.first + r.sgn * (int32_t)m, b = q.b0 + (int32_t)(j % nb), c = q.c0 + (int32_t)(j / nb);
  if (r.axis == 0) { *x = a; *y = b; *z = c; } else if (r.axis == 1) { *x = b; *y = a; *z = c; } else { *x = b; *y = c; *z = a; }
}
// After layer m: may the walk stop?  Yes once the layer of H_a(t_best) lies strictly before layer m + 1: every candidate not
// yet met has its H in a later layer, so by monotonicity a larger t and a larger key.
SMX_RAY_FN bool ray_done(const RayAxes& r, float cell, unsigned long long best, uint32_t next_layer) {
  if (best == kTgNone) return false;
  const int32_t at = ray_layer_of(r, cell, tg_key_float(best));
  return at < 0 || (uint32_t)at < next_layer;
}

// ---- the occupancy bit grid in front of the cell table (built by a scene, smx_rayscene.hpp) ---------------------------------
// It spans the occupied cell box from lo on; a block is 2^k cells per axis.  k < 0: no grid, and every cell goes to the table.
// nb = 0 on every axis: the box is empty, and so is the grid.
struct RayGrid { int32_t lo[3]; uint32_t nb[3]; int32_t k; };
// The bit number of the block of cell (x, y, z); false for a cell outside the box (the traversal asks about none: ray_axes and
// ray_span clamp to the occupied box).
SMX_RAY_FN bool ray_grid_bit(const RayGrid& g, int32_t x, int32_t y, int32_t z, unsigned long long* bit) {
  const uint32_t bx = (uint32_t)(x - g.lo[0]) >> g.k, by = (uint32_t)(y - g.lo[1]) >> g.k, bz = (uint32_t)(z - g.lo[2]) >> g.k;
  if (x < g.lo[0] || y < g.lo[1] || z < g.lo[2] || bx >= g.nb[0] || by >= g.nb[1] || bz >= g.nb[2]) return false;
  *bit = ((unsigned long long)bz * g.nb[1] + by) * g.nb[0] + bx;
  return true;
}
struct RayWork { uint32_t layers, bit_tests, lookups, misses, tests; };
// The look-up of one cell: with a grid a clear bit is "no run" and a set bit goes on to the table; without one the table is
// asked at once.  Bits: bool test(unsigned long long bit).
template <class Bits, class Tab>
SMX_RAY_FN bool ray_find(const RayGrid& g, const Bits& bits, const Tab& tab, uint32_t mask, int32_t x, int32_t y, int32_t z, uint32_t* first,
                         uint32_t* end, RayWork* w) {
  if (g.k >= 0) {
    unsigned long long bit;
    ++w->bit_tests;
    if (!ray_grid_bit(g, x, y, z, &bit) || !bits.test(bit)) return false;
  }
  ++w->lookups;
  const bool found = tg_table_find(tab, mask, dec_cell_key(x, y, z), first, end);
  if (!found) ++w->misses;
  return found;
}

// The smallest key over records [first, end), stepping by `stride` (the lanes of a wavefront share a run), and what the lane's
// own smallest key came with: a cast reads no map, so the winner's (u, v) and the sign of det are taken from the lane that
// computed the winning key.  Any lane with that key computed it from the same three corners by the same expressions.
struct RayKeep { unsigned long long own; float u, v, det; };
template <class Recs>
SMX_RAY_FN unsigned long long ray_walk(const Recs& recs, uint32_t first, uint32_t end, uint32_t stride, const TgVec& O, const TgVec& D,
                                       float t_min, float t_max, int cull, unsigned long long best, RayKeep* keep, uint32_t* tests) {
  for (uint32_t j = first; j < end; j += stride) {
    TgVec A, B, C;
    uint32_t i;
    RayHit h{0.0f, 0.0f, 0.0f, 0.0f};
    recs.load(j, &A, &B, &C, &i);
    const unsigned long long key = ray_key(O, D, A, B, C, i, t_min, t_max, cull, &h);
    if (key < best) { best = key; keep->own = key; keep->u = h.u; keep->v = h.v; keep->det = h.det; }
    ++*tests;
  }
  return best;
}

// One ray's view of the cast: the wide list, then layer after layer.  k_ray_cast makes the same look-ups 64 layers at a time and
// walks the same records with its lanes sharing a run; the host walk calls this as it stands.  Seen: void operator()(cell key)
// for every cell looked up in the table (the tests' completeness check); early_exit = false walks every layer.
template <class Bits, class Tab, class Recs, class Seen>
SMX_RAY_FN unsigned long long ray_cast_one(const RayGrid& g, const Bits& bits, const Tab& tab, uint32_t mask, const Recs& cell_recs,
                                           const Recs& wide_recs, uint32_t n_wide, const RayAxes& r, const TgVec& O, const TgVec& D, float cell,
                                           float t_min, float t_max, int cull, bool early_exit, Seen& seen, RayKeep* keep, RayWork* work) {
  unsigned long long best = ray_walk(wide_recs, 0, n_wide, 1, O, D, t_min, t_max, cull, kTgNone, keep, &work->tests);
  for (uint32_t m = 0; m < r.n_layers; ++m) {
    if (early_exit && ray_done(r, cell, best, m)) break;
    const RayRect q = ray_layer_rect(r, cell, t_min, t_max, m);
    const uint32_t cells = ray_rect_cells(q);
    ++work->layers;
    for (uint32_t j = 0; j < cells; ++j) {
      int32_t x, y, z;
      uint32_t first, end;
      ray_rect_cell(r, q, m, j, &x, &y, &z);
      const uint32_t before = work->lookups;
      const bool found = ray_find(g, bits, tab, mask, x, y, z, &first, &end, work);
      if (work->lookups != before) seen(dec_cell_key(x, y, z));
      if (found) best = ray_walk(cell_recs, first, end, 1, O, D, t_min, t_max, cull, best, keep, &work->tests);
    }
  }
  return best;
}

#if !defined(SMX_RAYCAST_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// the words of a cast's counters, a block of their own; the 64-bit words as (lo, hi) pairs
enum : int { kRayBadRays = 0, kRayHits, kRayFrontHits, kRayMaxBits, kRayLayersLo, kRayLayersHi, kRayBitTestsLo, kRayBitTestsHi, kRayLookupsLo,
             kRayLookupsHi, kRayMissesLo, kRayMissesHi, kRayTestsLo, kRayTestsHi, kRayWords = 16 };
enum : uint32_t { kRayWorkWords = 8 };                      // per ray: layers, bit tests, look-ups, misses, pair tests, flags, -, -

constexpr int kRayBlock = 256;                               // lanes per workgroup of the ray kernels (k_ray_cast: 4 rays)
constexpr int kRayWaves = kRayBlock / 64;

struct RayBits {
  const uint32_t* w;
  __device__ __forceinline__ bool test(unsigned long long bit) const { return (w[bit >> 5] >> (uint32_t)(bit & 31u)) & 1u; }
};
struct RayBox { int32_t lo[3], hi[3]; };                     // the occupied cell box (lo > hi: no cell is occupied)

// An index a cast can read: views, it owns nothing.  The one-shot call fills it from its workspace, a scene from what it keeps.
struct RayIndex {
  const TgCell* table; uint32_t mask;
  const TgRec* recs; const TgRec* wide_recs;
  uint32_t n_entries, n_wide;
  float cell; RayBox occ;
  RayGrid grid; const uint32_t* bits;      // grid.k < 0: none, and bits is not read
  const uint32_t* built;                   // the build's counter words on the device where the index was built for this cast alone
};
// cell and the occupied box of an index from the build's counter words as tg_read_counts brought them to the host
inline void ray_index_read(RayIndex* ix, const uint32_t* h) {
  memcpy(&ix->cell, &h[kTgCellBits], sizeof(float));
  for (int a = 0; a < 3; ++a) { ix->occ.lo[a] = (int32_t)h[kTgOccLo + a]; ix->occ.hi[a] = (int32_t)h[kTgOccHi + a]; }
}

// What a cast needs beside an index.  Each buffer grows on demand; a cast is synchronous, so nothing reads a block that goes.
struct RayCastWork {
  DevBuf<unsigned long long> best;         // [n_rays] the winning key of every ray
  DevBuf<uint32_t> work;                   // [n_rays][kRayWorkWords]
  DevBuf<float> rays, out_t, out_uv;       // staging when the caller's arrays are host memory
  DevBuf<uint32_t> out_hit;
  DevBuf<uint32_t> counters;               // [kRayWords]
  unsigned long long bytes() const;        // device memory held
};
// The device side of a cast's arrays: the caller's own, or the staging.
struct RayCastArrays { const float* rays; uint32_t* hit; float* t; float* uv; };

// A cast in four steps, which smx_recon_raycast_mesh and smx_rayscene_cast take in this order behind their argument checks, with
// what is their own between them (smx_raycast.hip).  First the overlap check, without touching any object; `fn` names the caller
// and `what` the input in the text.
int ray_cast_overlap(const char* fn, const char* what, const void* in, size_t in_bytes, uint32_t n_rays, const uint32_t* hit, const float* t,
                     const float* uv);
// Every reservation of the cast, the rays staged in, the counters zeroed: nothing is allocated after it.
int ray_cast_stage(RayCastWork& w, const float* rays, uint32_t n_rays, uint32_t* hit, float* t, float* uv, bool on_device, hipStream_t st,
                   RayCastArrays* d);
// The cast kernel: the thin one over the build's counter words where ix.built is set, the one that takes the grid, c and the
// box by value otherwise.  The caller stamps the end of its cast phase behind it.
int ray_cast_launch(RayCastWork& w, const RayIndex& ix, const smx_raycast_params* p, const RayCastArrays& d, uint32_t n_rays, hipStream_t st);
// The stats kernel, the copy-back of staged outputs, the counter read-back and the fill of *out; with built_cells the cell count
// of ix.built comes to the host in the same wait.  Returns after the stream has been waited for; the caller stamps the end of
// its stats phase.
int ray_cast_finish(RayCastWork& w, const RayIndex& ix, const RayCastArrays& d, uint32_t n_rays, uint32_t* hit, float* t, float* uv, bool on_device,
                    hipStream_t st, smx_rayscene_cast_stats* out, uint32_t* built_cells = nullptr);

// The workspace of smx_recon_raycast_mesh, a member of smx_recon_s.  smx_recon_build_rayscene builds with `grid`
// and `in` too, into a scene's records and table.
struct RaycastWork {
  TgWork grid;                             // the build's
  DevBuf<uint32_t> in;                     // staging when the caller's triangles are host memory
  DevBuf<uint32_t> counters;               // [kTgWords] the build's
  DevBuf<float> recs, wide_recs;           // [n_entries] / [n_wide] TgRec, the first in the sorted order
  DevBuf<unsigned long long> table;        // [table entries][2] TgCell
  RayCastWork cast;
  PhaseStamps<SMX_RAY_PHASES> stamps;      // of the last call; a refused call publishes the phases it completed
};

__device__ __forceinline__ void ray_load(const float* rays, uint32_t p, TgVec* O, TgVec* D) {
  const float* r = rays + 6 * (size_t)p;
  *O = TgVec{r[0], r[1], r[2]}; *D = TgVec{r[3], r[4], r[5]};
}
#endif

}  // namespace smx
