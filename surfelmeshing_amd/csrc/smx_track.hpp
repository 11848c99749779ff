// smx_track.hpp -- frame-to-model ICP (smx_recon_track): what smx_recon.hip needs of smx_track.hip.
//
// The object (smx_recon_s) owns the buffers; smx_track.hip owns the kernels and enqueues all iterations of a call.
#pragma once

#include "smx_common.hpp"

namespace smx {

constexpr int kTrackLevels = 3;
constexpr int kTrackMaxIterationsPerLevel = 32;
constexpr int kTrackRing = kTrackLevels * kTrackMaxIterationsPerLevel;   // one record per iteration of a call
constexpr int kTrackSlabStride = 32;    // doubles per workgroup slab (SMX_TRACK_SUMS of them used)
constexpr int kTrackMaxSlabs = 256;     // workgroups of the reduce kernel, at most

// Device-resident state of one call.  Written by k_track_begin and by lane 0 of k_track_solve only.
struct TrackDev {
  double T_rel[12];       // model camera <- frame camera, row-major 3x4
  double T_prev[12];      // ... before the update of the last iteration run
  float Tf[12];           // T_rel rounded to float: what the reduce kernel of the next iteration reads
  int32_t status;         // SMX_TRACK_*; a bad one is sticky
  int32_t iterations_run; // iterations that produced sums (the one that raised a bad status included)
  int32_t converged_level;// level whose remaining iterations are skipped, -1 = none
  int32_t pad;
  smx_track_result result;
  smx_track_iteration ring[kTrackRing];
};

struct TrackBuffers {
  const float* model_depth;     // [H][W] dense
  const float4* model_normal;   // [H][W] dense
  double* slabs;                // [kTrackMaxSlabs][kTrackSlabStride]
  TrackDev* state;
};

// Enqueues begin + every (reduce, solve) pair of the schedule on st; the last solve launch writes the result into
// b.state->result and, if result_dev is not null, into *result_dev as well.  Arguments are validated by the caller.
int track_enqueue(hipStream_t st, const TrackBuffers& b, int W, int H, float fx, float fy, float cx, float cy,
                  float depth_scaling, const smx_buffer_desc* depth, const smx_buffer_desc* normals,
                  const float global_T_pred[12], const smx_track_params& p, smx_track_result* result_dev);

// ---- smx_recon_track_rgbd: the same schedule with the photometric term ----
constexpr int kTrackRgbdSlabStride = 40;   // doubles per workgroup slab (SMX_TRACK_RGBD_SUMS of them used)

// What a call with colour keeps beside TrackDev (whose ring and result it fills as well, with the first 31 sums).
struct TrackRgbdDev {
  smx_track_rgbd_result result;
  smx_track_rgbd_iteration ring[kTrackRing];
};

struct TrackRgbdBuffers {
  TrackBuffers icp;             // (icp.slabs is not used: the 33 sums have a slab block of their own)
  const uint32_t* model_color;  // [H][W] dense uchar4, alpha 0 = empty
  float4* model_photo;          // [H][W] dense (L, gx, gy, valid)
  double* slabs;                // [kTrackMaxSlabs][kTrackRgbdSlabStride]
  TrackRgbdDev* state;
};

// As track_enqueue, with one k_track_photo_prepare launch in front (none if p.photometric_weight == 0, when
// model_color / model_photo are not touched either).
int track_rgbd_enqueue(hipStream_t st, const TrackRgbdBuffers& b, int W, int H, float fx, float fy, float cx, float cy,
                       float depth_scaling, const smx_buffer_desc* depth, const smx_buffer_desc* normals,
                       const smx_buffer_desc* color, const float global_T_pred[12], const smx_track_rgbd_params& p,
                       smx_track_rgbd_result* result_dev);

}  // namespace smx
