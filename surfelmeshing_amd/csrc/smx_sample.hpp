// smx_sample.hpp -- points drawn on a triangle array over the map in proportion to area, and the two one-sided surface distances
// between two triangle arrays (smx_recon_sample_mesh, smx_recon_compare_meshes).
//
// Part 1: the arithmetic of the contract as plain inline functions (the weight of a triangle, the saturating sum, the random
// words, the stratum of a sample, the search in a prefix, the point, the normal, the fixed-point words of a distance).
// smx_sample.hip calls them from its kernels; a test compiles this part alone for the host (SMX_SAMPLE_HOST_ONLY) and walks the
// same passes with plain words.  The vector type and the classes of step 1 are the triangle grid's (smx_trigrid.hpp).
// Part 2: the counter words and the workspaces the object keeps for the two calls (kernels and glue: smx_sample.hip).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(SMX_SAMPLE_HOST_ONLY) && !defined(SMX_DISTANCE_HOST_ONLY)
#define SMX_DISTANCE_HOST_ONLY 1
#endif
#include "smx_distance.hpp"   // (and through it smx_trigrid.hpp: TgVec, tg_classify, dot and cross)
#define SMX_SMP_FN SMX_TG_FN

namespace smx {

constexpr unsigned long long kSmpSat = 1ull << 62;          // sat(x) = min(x, 2^62)
constexpr uint32_t kSmpNone = 0xFFFFFFFFu;                   // tri of a sample that is "none"
constexpr int kSmpBlock = 256;                               // triangles per workgroup of the weights: the unit of the two-level prefix

// ---- step 2: the weight of a triangle of R = twice its area in units of 2^-30 m^2 ------------------------------------------
struct SmpFace { TgVec ab, ac, N; float a; };
SMX_SMP_FN SmpFace smp_face(const TgVec& A, const TgVec& B, const TgVec& C) {
  SmpFace f;
  f.ab = tg_sub(B, A); f.ac = tg_sub(C, A);
  f.N = tg_cross(f.ab, f.ac);
  f.a = sqrtf(tg_dot(f.N, f.N));
  return f;
}
// (corners within 64 m: a < 2^16, so the product by 2^30 is exact and below 2^46)
SMX_SMP_FN unsigned long long smp_weight(float a) { return a > 0.0f ? (unsigned long long)(a * 1073741824.0f) : 0ull; }

// ---- step 3: min(2^62, a + b) on [0, 2^62] is associative, so any tree of it gives the saturated sum ------------------------
SMX_SMP_FN unsigned long long smp_sat_add(unsigned long long a, unsigned long long b) {
  const unsigned long long s = a + b;                        // (at most 2^63: no wrap)
  return s < kSmpSat ? s : kSmpSat;
}

// ---- step 4: the random words ------------------------------------------------------------------------------------------------
SMX_SMP_FN uint32_t smp_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
SMX_SMP_FN uint32_t smp_rand(uint32_t k, uint32_t j, uint32_t seed) { return smp_mix(smp_mix(3u * k + j) ^ seed); }

// ---- step 5: u_k = k S + floor(S r0 / 2^32), the high 64 bits of S * (r0 << 32) ------------------------------------------------
SMX_SMP_FN unsigned long long smp_stratum(uint32_t k, unsigned long long S, uint32_t r0) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned long long hi = __umul64hi(S, (unsigned long long)r0 << 32);
#else
  const unsigned long long hi = (S >> 32) * r0 + (((S & 0xFFFFFFFFull) * r0) >> 32);
#endif
  return (unsigned long long)k * S + hi;
}

// ---- step 6: the first of n ascending words that is > x (n if none).  Words: unsigned long long operator()(uint32_t) -------
template <class Words>
SMX_SMP_FN uint32_t smp_upper(const Words& w, uint32_t n, unsigned long long x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (w(mid) > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// The triangle of u in the two-level prefix: off[b] = the saturated sum of the blocks before block b of kSmpBlock triangles,
// incl[t] = the sum of the weights of t's block up to and including t.  0 <= u < W and W < 2^62 (nothing saturated).
template <class Off, class Incl>
SMX_SMP_FN uint32_t smp_find(const Off& off, uint32_t n_blocks, const Incl& incl, uint32_t n_in, unsigned long long u) {
  uint32_t b = smp_upper(off, n_blocks, u);                  // (off[0] = 0 <= u: b >= 1)
  b = b > 0 ? b - 1 : 0;
  const uint32_t first = b * (uint32_t)kSmpBlock, len = n_in - first < (uint32_t)kSmpBlock ? n_in - first : (uint32_t)kSmpBlock;
  const unsigned long long x = u - off(b);
  const uint32_t j = smp_upper([&](uint32_t i) { return incl(first + i); }, len, x);
  return first + (j < len ? j : len - 1);                    // (j < len whenever u < W; held to the block all the same)
}

// ---- step 7: the point and the normal ------------------------------------------------------------------------------------------
SMX_SMP_FN void smp_bary(uint32_t r1, uint32_t r2, float* v, float* w) {
  float x = (float)(r1 >> 8) * 5.9604644775390625e-8f, y = (float)(r2 >> 8) * 5.9604644775390625e-8f;      // 2^-24
  if (x + y > 1.0f) { x = 1.0f - x; y = 1.0f - y; }
  *v = x; *w = y;
}
SMX_SMP_FN TgVec smp_point(const TgVec& A, const SmpFace& f, float v, float w) {
  return tg_add(tg_add(A, tg_scale(v, f.ab)), tg_scale(w, f.ac));
}
SMX_SMP_FN TgVec smp_normal(const SmpFace& f) { return TgVec{f.N.x / f.a, f.N.y / f.a, f.N.z / f.a}; }

// ---- the words of smx_recon_compare_meshes: a matched distance in units of 2^-20 m, and its square in two halves -------------
SMX_SMP_FN uint32_t cmp_dq(float distance) { return (uint32_t)(distance * 1048576.0f); }      // (distance <= 16: at most 2^24)
SMX_SMP_FN void cmp_square(uint32_t dq, unsigned long long* lo, unsigned long long* hi) {
  const unsigned long long sq = (unsigned long long)dq * dq;
  *lo = sq & 0xFFFFFFFFull; *hi = sq >> 32;
}

#if !defined(SMX_SAMPLE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
// The words of the device counters.  The counts, which every wavefront of the weights and of the draw adds to, sit in the first
// 64-byte block; W (written once by the scan) in the second; the three 64-bit sums of the comparison, which every wavefront of
// its kernel adds to, in a block each (atomics on one block queue behind each other).
enum : int { kSmpNotLive = 0, kSmpRepeated, kSmpRange, kSmpZero, kSmpError, kSmpHit, kSmpTotalLo = 16, kSmpTotalHi, kCmpSumD = 32,
             kCmpSumSqLo = 48, kCmpSumSqHi = 64, kSmpWords = 80 };
static_assert(kSmpHit < 16 && kSmpTotalLo % 16 == 0 && kCmpSumD % 16 == 0 && kCmpSumSqLo % 16 == 0 && kCmpSumSqHi % 16 == 0,
              "counts and 64-bit sums in 64-byte blocks of their own");

// The workspace of smx_recon_sample_mesh, a member of smx_recon_s.  Each buffer grows on demand; the call is synchronous, so
// nothing reads a block that goes.
struct SampleWork {
  DevBuf<unsigned long long> incl;         // [n_in] the sum of the weights of a triangle's block up to and including it
  DevBuf<unsigned long long> blocks;       // [blocks] the weight of every block, then the saturated sum of the blocks before it
  DevBuf<uint32_t> in;                     // staging when the caller's arrays are host memory
  DevBuf<float> out_points, out_bary, out_normals;
  DevBuf<uint32_t> out_tri;
  DevBuf<uint32_t> counters;               // [kSmpWords]
  PhaseStamps<SMX_SAMPLE_PHASES> stamps;   // of the last call; a refused call publishes the phases it completed
};
// The workspace of smx_recon_compare_meshes: both triangle arrays on the device, and one side's samples and answers.
struct CompareWork {
  DevBuf<uint32_t> in_a, in_b;             // staging when the caller's arrays are host memory
  DevBuf<float> points, distance;          // [n_samples][3], [n_samples]
  DevBuf<uint32_t> tri, nearest;           // [n_samples]
  DevBuf<uint32_t> counters;               // [kSmpWords] (the three sums)
  PhaseStamps<SMX_COMPARE_PHASES> stamps;
  int32_t directions = 0;                  // of the last call: a side not asked for reads 0 ms whatever lies between its stamps
};
// The workspace of smx_recon_register_mesh: the triangle array on the device, the samples and their normals.
struct RegisterMeshWork {
  DevBuf<uint32_t> in;                     // staging when the caller's array is host memory
  DevBuf<float> points, normals;           // [n_samples][3]
  DevBuf<uint32_t> tri;                    // [n_samples]
};
#endif

}  // namespace smx
