// smx_trigrid.hpp -- the triangle grid: a triangle array over the map, searched through a uniform grid of cells.
// smx_recon_mesh_distance, smx_recon_raycast_mesh, smx_recon_build_rayscene and smx_recon_build_distscene all build it, and
// build it here.
//
// Part 1: what the contracts of the three services share, as plain inline functions (the vector type, step 1's classes, the
// cell of a coordinate, the box of a triangle and its entry count, the cell table's insert and look-up templated on how an
// entry is read, claimed and bumped, the float in a key).  The kernels call them; a test compiles this part alone for the host
// (SMX_TRIGRID_HOST_ONLY, which the host-only switches of smx_distance.hpp, smx_distscene.hpp, smx_raycast.hpp and
// smx_rayscene.hpp set) and walks
// the same passes with plain words.
// Part 2: the device-side records, the counter words, the workspace of the build and its three steps (kernels and glue:
// smx_trigrid.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_TRIGRID_HOST_ONLY)
#if !defined(SMX_DECIMATE_HOST_ONLY)
#define SMX_DECIMATE_HOST_ONLY 1
#endif
#define SMX_TG_FN static inline
#else
#include "smx_common.hpp"
#define SMX_TG_FN __host__ __device__ __forceinline__
#endif
#include "smx_decimate.hpp"   // dec_live, dec_finite, dec_hash, dec_table_size, dec_cell_key, dec_value_word

namespace smx {

constexpr float kTgMaxCoord = 64.0f;                        // SMX_DIST_MAX_COORD
constexpr uint32_t kTgWideCells = 64;                       // SMX_DIST_WIDE_CELLS
constexpr unsigned long long kTgNone = ~0ull;               // the key of "no candidate"
constexpr unsigned long long kTgEmpty = 0ull;               // a table entry's key word is the cell key + 1: zeroed memory is empty
constexpr uint32_t kTgWide = 0x80000000u;                   // the mark word of a triangle on the wide list (else: its entry count)
enum : uint32_t { kTgInR = 0, kTgDropNotLive = 1, kTgDropRepeated = 2, kTgDropRange = 3 };

struct TgVec { float x, y, z; };
SMX_TG_FN TgVec tg_sub(const TgVec& a, const TgVec& b) { return TgVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
SMX_TG_FN TgVec tg_add(const TgVec& a, const TgVec& b) { return TgVec{a.x + b.x, a.y + b.y, a.z + b.z}; }
SMX_TG_FN TgVec tg_scale(float s, const TgVec& a) { return TgVec{s * a.x, s * a.y, s * a.z}; }
SMX_TG_FN float tg_dot(const TgVec& u, const TgVec& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
SMX_TG_FN TgVec tg_cross(const TgVec& u, const TgVec& v) {
  return TgVec{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

// ---- step 1 and step 2 ---------------------------------------------------------------------------------------------------
SMX_TG_FN bool tg_coord_ok(float v) { return dec_finite(v) && !(v > kTgMaxCoord) && !(v < -kTgMaxCoord); }
SMX_TG_FN bool tg_point_ok(const TgVec& p) { return tg_coord_ok(p.x) && tg_coord_ok(p.y) && tg_coord_ok(p.z); }
// The class of a triangle whose three indices are in range; live0..2 = dec_live of its corners.
SMX_TG_FN uint32_t tg_classify(uint32_t i0, uint32_t i1, uint32_t i2, bool live0, bool live1, bool live2, const TgVec& a, const TgVec& b,
                               const TgVec& c) {
  if (!(live0 && live1 && live2)) return kTgDropNotLive;
  if (i0 == i1 || i1 == i2 || i0 == i2) return kTgDropRepeated;
  if (!(tg_point_ok(a) && tg_point_ok(b) && tg_point_ok(c))) return kTgDropRange;
  return kTgInR;
}
// the float in the upper half of a key (a squared distance, a ray's t)
SMX_TG_FN float tg_key_float(unsigned long long key) {
  const uint32_t bits = (uint32_t)(key >> 32);
  float v;
  __builtin_memcpy(&v, &bits, sizeof(v));
  return v;
}

// ---- the grid ------------------------------------------------------------------------------------------------------------
// c: what was asked for (cell_size, or the mean extent over R), held to the lower bound the service sets
SMX_TG_FN float tg_cell_size(float cell_size, float least) { return cell_size > least ? cell_size : least; }
// |x| <= 64 (and a little) and c >= 1.125e-3: |x / c| < 2^16, so the cell fits the 21 bits of dec_cell_key with room for the
// +-1 of a query
SMX_TG_FN int32_t tg_cell(float x, float c) { return (int32_t)floorf(x / c); }
SMX_TG_FN float tg_min3(float a, float b, float c) { const float m = a < b ? a : b; return m < c ? m : c; }
SMX_TG_FN float tg_max3(float a, float b, float c) { const float m = a > b ? a : b; return m > c ? m : c; }
// the largest of the three extents of the triangle's box (cell_size == 0 takes their mean over R)
SMX_TG_FN float tg_extent(const TgVec& a, const TgVec& b, const TgVec& c) {
  return tg_max3(tg_max3(a.x, b.x, c.x) - tg_min3(a.x, b.x, c.x), tg_max3(a.y, b.y, c.y) - tg_min3(a.y, b.y, c.y),
                 tg_max3(a.z, b.z, c.z) - tg_min3(a.z, b.z, c.z));
}
struct TgBox { int32_t lo[3], hi[3]; };
SMX_TG_FN TgBox tg_box(const TgVec& a, const TgVec& b, const TgVec& c, float cell) {
  TgBox box;
  box.lo[0] = tg_cell(tg_min3(a.x, b.x, c.x), cell); box.hi[0] = tg_cell(tg_max3(a.x, b.x, c.x), cell);
  box.lo[1] = tg_cell(tg_min3(a.y, b.y, c.y), cell); box.hi[1] = tg_cell(tg_max3(a.y, b.y, c.y), cell);
  box.lo[2] = tg_cell(tg_min3(a.z, b.z, c.z), cell); box.hi[2] = tg_cell(tg_max3(a.z, b.z, c.z), cell);
  return box;
}
// The box inflated by `slack` on every side: from the cell of min3 - slack to the cell of max3 + slack.
SMX_TG_FN TgBox tg_box_slack(const TgVec& a, const TgVec& b, const TgVec& c, float cell, float slack) {
  TgBox box;
  box.lo[0] = tg_cell(tg_min3(a.x, b.x, c.x) - slack, cell); box.hi[0] = tg_cell(tg_max3(a.x, b.x, c.x) + slack, cell);
  box.lo[1] = tg_cell(tg_min3(a.y, b.y, c.y) - slack, cell); box.hi[1] = tg_cell(tg_max3(a.y, b.y, c.y) + slack, cell);
  box.lo[2] = tg_cell(tg_min3(a.z, b.z, c.z) - slack, cell); box.hi[2] = tg_cell(tg_max3(a.z, b.z, c.z) + slack, cell);
  return box;
}
// The mark word of a triangle of R: the number of cells of its box, or kTgWide above kTgWideCells.
SMX_TG_FN uint32_t tg_mark(const TgBox& box) {
  unsigned long long cells = 1;
  for (int k = 0; k < 3; ++k) {
    const unsigned long long d = (unsigned long long)(box.hi[k] - box.lo[k]) + 1ull;    // (at most 2^17 + 1 each)
    cells = cells * d > 0xFFFFFFFFull ? 0xFFFFFFFFull : cells * d;
  }
  return cells > kTgWideCells ? kTgWide : (uint32_t)cells;
}
// Cell number j (0 <= j < the mark word) of the box, x fastest.
SMX_TG_FN unsigned long long tg_box_key(const TgBox& box, uint32_t j) {
  const uint32_t nx = (uint32_t)(box.hi[0] - box.lo[0]) + 1u, ny = (uint32_t)(box.hi[1] - box.lo[1]) + 1u;
  return dec_cell_key(box.lo[0] + (int32_t)(j % nx), box.lo[1] + (int32_t)((j / nx) % ny), box.lo[2] + (int32_t)(j / (nx * ny)));
}

// ---- the cell table: 16-byte entries (cell key + 1, first | end << 32 of the cell's run in the sorted entries) --------------
// Tab: unsigned long long key(h), unsigned long long value(h) (plain reads), unsigned long long claim(h, expected, desired)
// (compare-and-swap on the key word, returns the old word), void bump(h, inc) (add to the value word).  The table has at least
// twice as many entries as there are cells.  The head of a run adds its position, the tail its position + 1 in the upper half.
template <class Tab>
SMX_TG_FN void tg_table_add(Tab& t, uint32_t mask, unsigned long long cell_key, unsigned long long inc) {
  uint32_t h = dec_hash(cell_key, mask);
  for (;;) {
    const unsigned long long prev = t.claim(h, kTgEmpty, cell_key + 1);
    if (prev == kTgEmpty || prev == cell_key + 1) break;
    h = (h + 1) & mask;
  }
  t.bump(h, inc);
}
// entry j of the sorted (key, t) pairs: what it adds to the table, if anything
template <class Tab>
SMX_TG_FN bool tg_table_entry(Tab& t, uint32_t mask, const unsigned long long* keys, uint32_t n_entries, uint32_t j) {
  const unsigned long long k = keys[j];
  const bool head = j == 0 || keys[j - 1] != k, tail = j + 1 == n_entries || keys[j + 1] != k;
  if (head || tail) tg_table_add(t, mask, k, (head ? (unsigned long long)j : 0ull) + (tail ? (unsigned long long)(j + 1) << 32 : 0ull));
  return head;
}
// The run [first, end) of a cell; false if the cell is empty.  (after the inserts: plain reads)
template <class Tab>
SMX_TG_FN bool tg_table_find(const Tab& t, uint32_t mask, unsigned long long cell_key, uint32_t* first, uint32_t* end) {
  for (uint32_t h = dec_hash(cell_key, mask);; h = (h + 1) & mask) {
    const unsigned long long k = t.key(h);
    if (k == cell_key + 1) {
      const unsigned long long v = t.value(h);
      *first = (uint32_t)v; *end = (uint32_t)(v >> 32);
      return true;
    }
    if (k == kTgEmpty) return false;
  }
}

#if !defined(SMX_TRIGRID_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// The words of the build's device counters, the same for every service; a service's own words follow from kTgWords on.
// [kTgCellBits] = c as its bits, [kTgOccLo .. +2] / [kTgOccHi .. +2] = the occupied cell box as int32 (folded only for rays),
// [kTgExtentLo / Hi] = the sum of the extents in 2^-20 m, [kTgEntries64Lo / Hi] = the entries as a 64-bit sum (the scan's
// 32-bit total must not have wrapped).  The 64-bit words sit at even indices.
enum : int { kTgNotLive = 0, kTgRepeated, kTgRange, kTgInRCount, kTgNWide, kTgEntries, kTgCells, kTgError, kTgCellBits, kTgOccLo,
             kTgOccHi = kTgOccLo + 3, kTgPadWord = kTgOccHi + 3, kTgExtentLo, kTgExtentHi, kTgEntries64Lo, kTgEntries64Hi, kTgWords };
static_assert(kTgExtentLo % 2 == 0 && kTgEntries64Lo % 2 == 0 && kTgWords % 2 == 0, "64-bit atomics");

struct TgRec { float4 a, b, c; };                            // corners in input order; a.w = the bits of t
struct TgCell { unsigned long long key, value; };            // one 16-byte entry of the cell table
static_assert(sizeof(TgRec) == 48 && sizeof(TgCell) == 16, "packed records");

// The map as in mesh_triangulate: smooth position (x, y, z, -) of slot i at smooth[i * smooth_stride], (normal, RadiusSquared)
// at normal[i * normal_stride].
struct TgMap {
  const float4* smooth; size_t smooth_stride;
  const float4* normal; size_t normal_stride;
  uint32_t n;
};

constexpr int kTgBlock = 256;                                // triangles or entries per workgroup of every kernel of the build

// how a kernel reads the table and the records
struct TgDeviceTable {
  TgCell* e;
  __device__ __forceinline__ unsigned long long key(uint32_t h) const { return e[h].key; }
  __device__ __forceinline__ unsigned long long value(uint32_t h) const { return e[h].value; }
  __device__ __forceinline__ unsigned long long claim(uint32_t h, unsigned long long expected, unsigned long long desired) const {
    return atomicCAS(&e[h].key, expected, desired);
  }
  __device__ __forceinline__ void bump(uint32_t h, unsigned long long inc) const { atomicAdd(&e[h].value, inc); }
};
struct TgDeviceRecs {
  const TgRec* r;
  __device__ __forceinline__ void load(uint32_t j, TgVec* A, TgVec* B, TgVec* C, uint32_t* t) const {
    const TgRec x = r[j];
    *A = TgVec{x.a.x, x.a.y, x.a.z}; *B = TgVec{x.b.x, x.b.y, x.b.z}; *C = TgVec{x.c.x, x.c.y, x.c.z};
    *t = __float_as_uint(x.a.w);
  }
};
__device__ __forceinline__ TgVec tg_pos(const TgMap& map, uint32_t i) {
  const float4 s = map.smooth[(size_t)i * map.smooth_stride];
  return TgVec{s.x, s.y, s.z};
}
__device__ __forceinline__ float tg_cell_of(const uint32_t* cnt) { return __uint_as_float(cnt[kTgCellBits]); }

// The build's workspace: DistanceWork and RaycastWork hold one each.  Each buffer grows on demand; the calls are synchronous,
// so nothing reads a block that goes.
struct TgWork {
  DevBuf<uint32_t> mark;                   // [n_in] entry count of the triangle, kTgWide, or 0 (not in R)
  DevBuf<uint32_t> blocks;                 // entries per workgroup, then their offsets
  DevBuf<uint32_t> wide_t;                 // [n_wide] the wide list, in arrival order (the minimum does not depend on it)
  DevBuf<unsigned long long> keys[2];      // the sort's records: the entries (and whatever else the service sorts in them)
  DevBuf<uint32_t> vals[2];
  DevBuf<uint32_t> hist;                   // the sort's workspace
  int reserve_mark(uint32_t n_in);         // mark, blocks and wide_t for n_in triangles, in this order
};

// The two compile-time variants of the build: the boxes as they are, or inflated by SMX_RAY_BOX_SLACK with the occupied cell
// box folded into [kTgOccLo / Hi].
enum class TgBoxes { kExact, kForRays };

// The build in three steps, enqueued on st (smx_trigrid.hip).  Before the first the caller has called w.reserve_mark(n_in) and
// zeroed its counters cnt (at least kTgWords words); din is device memory; c >= least_cell.
int tg_enqueue_mark(TgWork& w, TgBoxes boxes, const TgMap& map, const uint32_t* din, uint32_t n_in, float cell_size, float least_cell,
                    uint32_t* cnt, hipStream_t st);
// Copies n_words of cnt to h, waits for st and refuses an index out of range (the map has n_slots) or more than 2^30 entries:
// SMX_ERR_INVALID_ARGUMENT with the error text set.  *E = the entries, *Wd = the length of the wide list.
int tg_read_counts(const uint32_t* cnt, uint32_t* h, int n_words, uint32_t n_slots, hipStream_t st, uint32_t* E, uint32_t* Wd);
// Reserves the sort's buffers in w for max(E, min_sort) records, then recs, wide_recs and table (the caller's), in the order
// the call always has; *sorted_keys (may be null) = the E sorted cell keys, *sorted_vals (may be null) = the triangle of every
// sorted entry beside them, both in w until its next use.  Nothing is reserved after the sort is enqueued.
int tg_enqueue_index(TgWork& w, TgBoxes boxes, const TgMap& map, const uint32_t* din, uint32_t n_in, uint32_t E, uint32_t Wd, uint32_t min_sort,
                     uint32_t* cnt, DevBuf<float>& recs, DevBuf<float>& wide_recs, DevBuf<unsigned long long>& table, uint32_t* mask,
                     const unsigned long long** sorted_keys, hipStream_t st, const uint32_t** sorted_vals = nullptr);
#endif

}  // namespace smx
