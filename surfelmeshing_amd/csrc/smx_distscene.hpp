// smx_distscene.hpp -- a distance scene: the index of smx_recon_mesh_distance kept between queries (smx_distscene).
//
// Part 1: what only a kept scene needs, as plain inline functions: the first-record rule (which of a triangle's records
// first_rec[t] names) and the read of the winner's corners through it.  The distance arithmetic, the walk and the query of one
// point are smx_distance.hpp's.  The kernels call them; a test compiles this part alone for the host (SMX_DISTSCENE_HOST_ONLY)
// and walks the same passes with plain words.
// Part 2: what the scene object holds (kernels and glue: smx_distscene.hip; the query's kernels: smx_distance.hip).
#pragma once

#include <stdint.h>

#if defined(SMX_DISTSCENE_HOST_ONLY)
#if !defined(SMX_DISTANCE_HOST_ONLY)
#define SMX_DISTANCE_HOST_ONLY 1
#endif
#endif
#include "smx_distance.hpp"

namespace smx {

// ---- the first record of a triangle ----------------------------------------------------------------------------------------
// first_rec[t] = the smallest position among the records that hold triangle t: a position in the sorted cell records (below
// 2^30), or a position in the wide list (below 2^28) with the top bit set.  A triangle of R is in cells or on the wide list,
// never both, so the two kinds never meet in one word; a triangle outside R keeps kDsceneNoRec and is never a winner.  The
// smallest position is one integer minimum per record, so the word does not depend on the order the records arrive in.
constexpr uint32_t kDsceneWideBit = 0x80000000u;
constexpr uint32_t kDsceneNoRec = 0xFFFFFFFFu;
SMX_DIST_FN uint32_t dscene_first_word(uint32_t position, bool wide) { return wide ? (position | kDsceneWideBit) : position; }
SMX_DIST_FN uint32_t dscene_first_min(uint32_t held, uint32_t word) { return word < held ? word : held; }
// The corners of triangle t as ANY of its records holds them: the float32 words the map held at the build, in input order.
// Recs: void load(j, &A, &B, &C, &t) as in dist_walk.  *t_held = the triangle the record names (t itself).
template <class Recs>
SMX_DIST_FN void dscene_winner(uint32_t first_word, const Recs& cell_recs, const Recs& wide_recs, TgVec* A, TgVec* B, TgVec* C, uint32_t* t_held) {
  if (first_word & kDsceneWideBit) wide_recs.load(first_word & ~kDsceneWideBit, A, B, C, t_held);
  else cell_recs.load(first_word, A, B, C, t_held);
}

#if !defined(SMX_DISTSCENE_HOST_ONLY)
// ---- part 2 ----------------------------------------------------------------------------------------------------------
struct RegDev;                                               // smx_register.hpp
// What smx_distscene_register keeps with the scene besides the query's workspace (glue: smx_register.hip).  The one call on a
// scene that may return before its kernels are done: `mark` lies behind them, and whoever frees or grows a block of the scene
// waits for it on the host first.
struct RegisterWork {
  DevBuf<float> pts, nrm;                  // staging when the caller's arrays are host memory
  DevBuf<float> moved;                     // [m][3] the samples of an iteration as the pose moved them: the query's points
  DevBuf<uint32_t> nearest;                // [m] the query's outputs
  DevBuf<float> distance, closest;         // [m], [m][3]
  DevBuf<double> slabs;                    // [kTrackMaxSlabs][kTrackSlabStride] the reduce kernel's per-workgroup sums
  DevBuf<uint32_t> robust_counts;          // [kTrackMaxSlabs][2] the robust reduce kernel's two counts per workgroup; its first call allocates it
  DevBuf<RegDev> state;                    // [1]
  bool last_robust = false;                // the last call ran the robust reduce kernel
  StreamMark mark;
  PhaseStamps<1> whole;                    // the last call
  PhaseStamps<4> last;                     // move, query, reduce, solve of its last iteration
};

// What smx_distscene_score_poses and smx_distscene_register_global keep with the scene (glue and kernels: smx_global.hip).  Both
// calls are synchronous, so nothing reads a block that goes; the association runs in the query's workspace.
struct GlobalWork {
  DevBuf<float> pts;                       // staging when the caller's points are host memory
  DevBuf<float> poses;                     // [P][12] every candidate pose of a call
  DevBuf<float> moved;                     // [chunk poses][m][3] a chunk's samples as its poses moved them: the query's points
  DevBuf<uint32_t> nearest;                // [chunk poses][m] the query's outputs
  DevBuf<float> distance;
  DevBuf<smx_pose_score> scores;           // [P]
  uint32_t chunk_points = 1u << 22;        // samples a chunk may hold (smx_distscene_debug_set_score_chunk)
  PhaseStamps<1> whole;                    // the score phase of the last call
  PhaseStamps<3> last;                     // move, query, score kernel of its last chunk
  float host_ms[3] = {0.0f, 0.0f, 0.0f};   // select, refine, rescore of the last smx_distscene_register_global, on the host's clock
};

constexpr int kDsceneBuildWords = 32;                        // the build's counters: the grid's words; device_bytes counts 32
static_assert(kTgWords <= kDsceneBuildWords, "the build's counters");
#endif

}  // namespace smx

#if !defined(SMX_DISTSCENE_HOST_ONLY)
// A snapshot: after a build a query reads nothing but these.
struct smx_distscene_s {
  int device = 0;
  bool built = false;
  // the build's
  smx::DevBuf<float> recs, wide_recs;              // [n_entries] / [n_wide] TgRec
  smx::DevBuf<unsigned long long> table;           // [mask + 1][2] TgCell
  smx::DevBuf<uint32_t> first_rec;                 // [n_in] dscene_first_word of every triangle of R
  smx::DevBuf<uint8_t> rim;                        // [n_in] smx_recon_mesh_rim's bytes, indexed like nearest (smx_recon_build_distscene_rim only)
  bool has_rim = false;
  smx::DevBuf<uint32_t> counters;                  // [kDsceneBuildWords] as the build left them: c
  uint32_t h[smx::kDsceneBuildWords] = {};         // ... and on the host
  uint32_t mask = 0, n_entries = 0, n_wide = 0, n_in = 0;
  float max_distance = 0.0f;                       // the bound of the build: a query asks for no more
  smx::DistQueryWork query;                        // a query's, and a registration's
  smx::RegisterWork reg;                           // a registration's own
  smx::GlobalWork glob;                            // the pose scores' own
  smx::PhaseStamps<3> build_stamps;                // mark, index, first of the last build
  smx::PhaseStamps<2> query_stamps;                // query, stats of the last query
};
#endif
