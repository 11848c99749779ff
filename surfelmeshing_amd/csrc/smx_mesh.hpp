// smx_mesh.hpp -- localized Delaunay triangulation of the surfel map (smx_recon_triangulate).
//
// Part 1: the per-surfel arithmetic as plain inline functions (projection, angular key, in-circle test with the surfel
// at the origin, star construction, ring lookup, triangle filters).  smx_mesh.hip calls them from its kernels; a test
// compiles this part alone for the host (SMX_MESH_HOST_ONLY) and runs the same functions over the same inputs.
// Part 2: what smx_recon.hip needs of smx_mesh.hip (the workspace and the one entry point).
#pragma once

#include <stdint.h>

#if defined(SMX_MESH_HOST_ONLY)
#include <math.h>
#define SMX_MESH_FN static inline
#else
#include "smx_common.hpp"
#define SMX_MESH_FN __host__ __device__ __forceinline__
#endif

namespace smx {

constexpr int kMeshMaxStarDegree = 16;   // ring entries per slot: one 64-byte row
constexpr int kMeshMaxNeighbors = 64;    // candidates per slot = lanes of a wavefront
// meta word of a slot: bits 0-7 degree, bits 8-23 "ring[i] and ring[(i + 1) % degree] span a star triangle", bit 31 overflow
constexpr uint32_t kMeshOverflowBit = 0x80000000u;

struct MeshVec { float x, y, z; };

SMX_MESH_FN float mesh_dot(const MeshVec& a, const MeshVec& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
SMX_MESH_FN MeshVec mesh_sub(const MeshVec& a, const MeshVec& b) { return MeshVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
SMX_MESH_FN MeshVec mesh_cross3(const MeshVec& a, const MeshVec& b) {
  return MeshVec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
SMX_MESH_FN bool mesh_finite(float v) { return v - v == 0.0f; }

// Orthonormal basis (u, v) of the plane with normal n (any basis serves: the star does not depend on it): u is the
// coordinate axis along which n is smallest, made orthogonal to n; v = n x u, so that (u, v, n) is right-handed and
// "counter-clockwise in the plane" means counter-clockwise seen from the side n points to.
SMX_MESH_FN void mesh_basis(const MeshVec& n, MeshVec* u, MeshVec* v) {
  const float ax = fabsf(n.x), ay = fabsf(n.y), az = fabsf(n.z);
  MeshVec e{0.0f, 0.0f, 0.0f};
  if (ax <= ay && ax <= az) e.x = 1.0f; else if (ay <= az) e.y = 1.0f; else e.z = 1.0f;
  const float nn = mesh_dot(n, n);
  const float k = mesh_dot(e, n) / nn;
  MeshVec t{e.x - k * n.x, e.y - k * n.y, e.z - k * n.z};
  const float inv = 1.0f / sqrtf(mesh_dot(t, t));
  *u = MeshVec{t.x * inv, t.y * inv, t.z * inv};
  const float invn = 1.0f / sqrtf(nn);
  const MeshVec c = mesh_cross3(n, *u);
  *v = MeshVec{c.x * invn, c.y * invn, c.z * invn};
}

// Candidate j of slot p, already known to lie in p's ball: kept unless it is p itself, its normal is too far from
// p's, or its projection (x, y) falls onto p.
SMX_MESH_FN bool mesh_candidate_ok(uint32_t p, uint32_t j, const MeshVec& np, const MeshVec& nj, float cos_max_normal_angle,
                                   float x, float y, float radius_squared) {
  if (j == p) return false;
  if (!(mesh_dot(np, nj) > cos_max_normal_angle)) return false;
  return x * x + y * y > 1e-12f * radius_squared;
}

SMX_MESH_FN float mesh_cross2(float ax, float ay, float bx, float by) { return ax * by - ay * bx; }

// In-circle test with the surfel at the origin: the sign of the 3x3 determinant of the rows (x, y, x^2 + y^2).  For a
// counter-clockwise (origin, a, b), c lies strictly inside the circle through the three iff the value is negative.
SMX_MESH_FN float mesh_incircle(float ax, float ay, float aq, float bx, float by, float bq, float cx, float cy, float cq) {
  return ax * (by * cq - bq * cy) - ay * (bx * cq - bq * cx) + aq * (bx * cy - by * cx);
}

// Monotonic in the polar angle of (x, y), in [0, 4): orders the ring without trigonometry.
SMX_MESH_FN float mesh_pseudo_angle(float x, float y) {
  const float p = x / (fabsf(x) + fabsf(y));
  return y >= 0.0f ? 1.0f - p : 3.0f + p;
}

// Successor of candidate j in the star of the origin: the candidate b with a turn from j to b in (0, pi) such that no
// other candidate lies strictly inside the circle (origin, j, b); -1 if there is none.  x / y / q hold the projections
// and their squared lengths of m entries, q <= 0 marking an entry that is no candidate.  A tournament finds the only
// possible b (under inversion about the origin the star is the convex hull of the candidates and the tournament is a
// gift-wrapping step), a second sweep verifies it against the definition, so whatever comes back satisfies it.
template <typename A>
SMX_MESH_FN int mesh_star_successor(int j, int m, const A& x, const A& y, const A& q) {
  const float ax = x[j], ay = y[j], aq = q[j];
  int best = -1;
  float bx = 0.0f, by = 0.0f, bq = 0.0f;
  for (int c = 0; c < m; ++c) {
    const float cx = x[c], cy = y[c], cq = q[c];
    if (c == j || !(cq > 0.0f) || !(mesh_cross2(ax, ay, cx, cy) > 0.0f)) continue;
    if (best < 0 || mesh_incircle(ax, ay, aq, bx, by, bq, cx, cy, cq) < 0.0f) { best = c; bx = cx; by = cy; bq = cq; }
  }
  if (best < 0) return -1;
  for (int c = 0; c < m; ++c) {
    const float cq = q[c];
    if (c == j || c == best || !(cq > 0.0f)) continue;
    if (mesh_incircle(ax, ay, aq, bx, by, bq, x[c], y[c], cq) < 0.0f) return -1;
  }
  return best;
}

// Ring order: entry j comes before entry c iff (angle, index) is smaller.
SMX_MESH_FN bool mesh_ring_before(float ang_j, int j, float ang_c, int c) { return ang_j < ang_c || (ang_j == ang_c && j < c); }

SMX_MESH_FN uint32_t mesh_meta_degree(uint32_t meta) { return meta & 0xFFu; }

// Is (origin, a, b) -- in this order -- a star triangle of the slot whose ring row and meta word are given?
SMX_MESH_FN bool mesh_ring_has_pair(const uint32_t ring[kMeshMaxStarDegree], uint32_t meta, uint32_t a, uint32_t b) {
  const uint32_t deg = mesh_meta_degree(meta);
  bool found = false;
#if !defined(SMX_MESH_HOST_ONLY)
#pragma unroll
#endif
  for (int t = 0; t < kMeshMaxStarDegree; ++t) {
    const uint32_t next = ((uint32_t)(t + 1) < deg && t + 1 < kMeshMaxStarDegree) ? ring[(t + 1) % kMeshMaxStarDegree] : ring[0];
    found = found || ((uint32_t)t < deg && ((meta >> (8 + t)) & 1u) && ring[t] == a && next == b);
  }
  return found;
}
// ... in either sense of rotation (the three tangent planes need not agree on it)
SMX_MESH_FN bool mesh_ring_has_triangle(const uint32_t ring[kMeshMaxStarDegree], uint32_t meta, uint32_t a, uint32_t b) {
  return mesh_ring_has_pair(ring, meta, a, b) || mesh_ring_has_pair(ring, meta, b, a);
}

// Cosine of the interior angle at `at` between the edges to b and c.
SMX_MESH_FN float mesh_angle_cos(const MeshVec& at, const MeshVec& b, const MeshVec& c) {
  const MeshVec e = mesh_sub(b, at), f = mesh_sub(c, at);
  return mesh_dot(e, f) / sqrtf(mesh_dot(e, e) * mesh_dot(f, f));
}

// The triangle filters on the 3-D smooth positions.  Returns 0 if the triangle is rejected, 1 if (p, a, b) is
// counter-clockwise seen from the side its oriented normal points to, 2 if (p, b, a) is.
SMX_MESH_FN int mesh_triangle_filter(const MeshVec& P, const MeshVec& A, const MeshVec& B, const MeshVec& np,
                                     const MeshVec& na, const MeshVec& nb, float cos_min_angle, float cos_max_angle) {
  const float c0 = mesh_angle_cos(P, A, B), c1 = mesh_angle_cos(A, B, P), c2 = mesh_angle_cos(B, P, A);
  // angle in [min, max]  <=>  cos in [cos max, cos min]; a degenerate triangle gives NaN and fails
  if (!(c0 <= cos_min_angle && c0 >= cos_max_angle && c1 <= cos_min_angle && c1 >= cos_max_angle &&
        c2 <= cos_min_angle && c2 >= cos_max_angle)) return 0;
  MeshVec n = mesh_cross3(mesh_sub(A, P), mesh_sub(B, P));
  const MeshVec sum{np.x + na.x + nb.x, np.y + na.y + nb.y, np.z + na.z + nb.z};
  const float s = mesh_dot(n, sum);
  if (!(s > 0.0f) && !(s < 0.0f)) return 0;
  const bool flip = s < 0.0f;
  if (flip) n = MeshVec{-n.x, -n.y, -n.z};
  if (!(mesh_dot(n, np) > 0.0f && mesh_dot(n, na) > 0.0f && mesh_dot(n, nb) > 0.0f)) return 0;
  return flip ? 2 : 1;
}

// The changed-predicate of smx_recon_triangulate_update.  A slot's seven words, in the order smooth x, y,
// z, RadiusSquared, normal x, y, z, are compared BITWISE with the kept snapshot: a NaN equals itself, -0 differs from +0
// (conservative: a slot found changed is only recomputed).  Slots at or past the kept slot count are changed.
SMX_MESH_FN uint32_t mesh_word_bits(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, sizeof(u));
  return u;
}
SMX_MESH_FN bool mesh_slot_changed(uint32_t slot, uint32_t n_prev, const float now[7], const float kept[7]) {
  if (slot >= n_prev) return true;
  uint32_t differs = 0;
  for (int t = 0; t < 7; ++t) differs |= mesh_word_bits(now[t]) ^ mesh_word_bits(kept[t]);
  return differs != 0;
}

// The coarse filter in front of the update's reverse test: a bit table over cells of edge h, hashed.  Changed points and
// ghosts set the bit of their cell; an unchanged slot whose ball has radius <= h / 2 can only reach a point in one of the
// 27 cells around its own, so if none of those bits is set it is left out of the reverse test.  Collisions only let more
// slots through.  A coordinate whose cell index does not fit (|x / h| >= 2^20) gives false: the caller then does not filter.
constexpr int kMeshNearBitsLog2 = 27;    // 16 MiB of bits
SMX_MESH_FN bool mesh_coarse_cell(float x, float y, float z, float inv_h, int* ix, int* iy, int* iz) {
  const float cx = x * inv_h, cy = y * inv_h, cz = z * inv_h;
  if (!(fabsf(cx) < 1048576.0f && fabsf(cy) < 1048576.0f && fabsf(cz) < 1048576.0f)) return false;
  *ix = (int)floorf(cx); *iy = (int)floorf(cy); *iz = (int)floorf(cz);
  return true;
}
SMX_MESH_FN uint32_t mesh_coarse_bit(int ix, int iy, int iz) {
  uint32_t h = (uint32_t)ix * 73856093u ^ (uint32_t)iy * 19349663u ^ (uint32_t)iz * 83492791u;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
  return h & ((1u << kMeshNearBitsLog2) - 1u);
}

#if !defined(SMX_MESH_HOST_ONLY)
// ---- part 2: the interface between smx_recon.hip (owner of the map) and smx_mesh.hip (owner of the kernels) ----
struct MeshWorkspace;   // lists, rings, counts, output staging, statistics, timed events; grows on demand, reused
int mesh_workspace_create(MeshWorkspace** out);
void mesh_workspace_destroy(MeshWorkspace* w);
int mesh_check_params(const smx_mesh_params& p);
// The map as two strided arrays of 16-byte records: smooth position (x, y, z, -) and (normal x, y, z, RadiusSquared) of
// slot i at smooth[i * smooth_stride] / normal[i * normal_stride].  `nn` has been built over the n slots already, between
// mesh_stamp_begin and this call.  Synchronises st.  Arguments are validated by the caller; the capacity rule is applied here.
int mesh_triangulate(MeshWorkspace* w, hipStream_t st, smx_nn nn, const float4* smooth, size_t smooth_stride,
                     const float4* normal, size_t normal_stride, uint32_t n, const smx_mesh_params& p, uint32_t* triangles,
                     uint32_t capacity, int32_t on_device, uint32_t* n_triangles, smx_mesh_stats* stats);
// stamps of the last call: before the index build, and after each of build / list query / star / agreement+write
int mesh_stamp_begin(MeshWorkspace* w, hipStream_t st);
int mesh_phase_ms(MeshWorkspace* w, float out_ms[4]);

// smx_recon_triangulate_update.  The kept state lives in the workspace.  `lists` fills the candidate lists
// of a device list of slots from `nn` (the owner of the map does that: smx_recon_neighbor_candidates' route).  `nn` is
// (re)built over the map here, from the rows the diff kernel writes (merged slots are NaN rows, as k_index_rows makes them).
typedef int (*MeshSubsetLists)(void* ctx, hipStream_t st, smx_nn nn, const uint32_t* slots, uint32_t n_slots, float factor_squared,
                               int K, uint32_t* out_idx, float* out_d2, int32_t* out_count);
constexpr float kMeshUpdateDefaultFullAboveFraction = 0.2f;
int mesh_triangulate_update(MeshWorkspace* w, int device, hipStream_t st, smx_nn nn, float cell_size, const float4* smooth,
                            size_t smooth_stride, const float4* normal, size_t normal_stride, uint32_t n,
                            const smx_mesh_params& p, float full_above_fraction, MeshSubsetLists lists, void* lists_ctx,
                            uint32_t* triangles, uint32_t capacity, int32_t on_device, uint32_t* n_triangles,
                            smx_mesh_stats* stats, smx_mesh_update_stats* update_stats);
int mesh_update_reset(MeshWorkspace* w);
int mesh_update_phase_ms(MeshWorkspace* w, float out_ms[6]);
#endif

}  // namespace smx
