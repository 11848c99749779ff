/*
 * smx.h -- C-ABI of the MI355X-native surfel-integration library (libsmx.so).
 *
 * This is the drop-in boundary for the hot path of puzzlepaint/surfelmeshing:
 * every entry point replaces one piece of the reference's CUDA-side interface
 * (cited per declaration; paths relative to the reference checkout,
 * APP = applications/surfel_meshing/src/surfel_meshing, VIS = libvis/src/libvis).
 * Plain C types only: opaque handles, POD descriptors, pointers and sizes.
 * The C++ shim include/smx_shim.hpp re-creates the reference's class names
 * (CUDABuffer<T>, CUDASurfelReconstruction, CUDASurfelsCPU) on top of it; the
 * Python mirror is surfelmeshing_amd/api.py.  See INTEGRATION.md.
 *
 * Conventions:
 *  - every function returns 0 on success or a negative smx_status; the last
 *    error text is available from smx_last_error().  The reference aborts via
 *    LOG(FATAL) (VIS/cuda/cuda_util.h:35-49); the shims convert non-zero into
 *    an abort / exception to keep that behaviour.
 *  - all work is enqueued on the HIP stream passed in (a hipStream_t cast to
 *    void*; NULL = the default stream).  Calls return asynchronously; unlike
 *    the reference, Integrate does not block the host (the surfel count lives
 *    in device memory), so counts are read with smx_recon_counts(), which
 *    synchronises the stream.
 *  - single caller thread per object; no process-global state -- the library neither keeps any nor touches the process
 *    environment (smx_runtime_advice reports what the application should set) -- (the reference's
 *    function-local static buffer at APP/cuda_surfel_reconstruction_kernels.cc:479
 *    is per-object here), so one object per GPU / per stream works.
 *  - camera cx, cy are in the pixel-CORNER convention, as
 *    PinholeCamera4f::parameters()[2..3] in the reference.
 */
#ifndef SMX_H_
#define SMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  SMX_OK = 0,
  SMX_ERR_INVALID_ARGUMENT = -1,
  SMX_ERR_HIP = -2,          /* a HIP runtime call failed */
  SMX_ERR_NO_DEVICE = -3,    /* no usable gfx950 device */
  SMX_ERR_UNSUPPORTED = -4
} smx_status;

typedef void* smx_stream;                 /* hipStream_t */
typedef struct smx_buffer_s* smx_buffer;  /* owns pitched device memory */
typedef struct smx_recon_s* smx_recon;    /* CUDASurfelReconstruction */
typedef struct smx_nn_s* smx_nn;          /* radius-neighbor search index */

/* POD passed to kernels by value, identical in layout to the reference's
 * CUDABuffer_<T> {T* address_; int height_; int width_; size_t pitch_;}
 * (VIS/cuda/cuda_buffer.cuh:44-119). */
typedef struct {
  void* address;
  int32_t height;
  int32_t width;
  size_t pitch;   /* bytes */
} smx_buffer_desc;

const char* smx_last_error(void);
/* Runtime settings the frame loop wants and the library does not make itself (process-global: the application's to set):
 * returns the number of recommendations (0 = none) and their text.  Today: GPU_MAX_HW_QUEUES >= 8, read by the HIP runtime at
 * the process's first HIP call (INTEGRATION.md "Streams, queues, priorities").  The first smx_recon_create of a process prints
 * the text once on stderr unless SMX_QUIET=1. */
int smx_runtime_advice(char* text, size_t capacity);
/* Number of visible HIP devices / select one for the calling thread. */
int smx_device_count(int* count);
int smx_set_device(int device);
int smx_device_name(int device, char* name, size_t capacity);
int smx_stream_create(smx_stream* out);
/* priority_class: -1 = lowest, 0 = default, +1 = highest priority the device offers (cudaStreamCreateWithPriority) */
int smx_stream_create_with_priority(smx_stream* out, int32_t priority_class);
/* A stream whose kernels only run on a subset of the compute units (hipExtStreamCreateWithCUMask; no CUDA counterpart):
 * bit k of mask_words[k / 32] set = compute unit k may be used.  On this part consecutive bits fall on consecutive XCDs
 * (bit k -> XCD k % 8), so the low n bits are n / 8 compute units of every XCD.  Default priority.  Measured use:
 * a partition between the preprocessing queue and the surfel queues (profiles/r6_ab_notes.md section 10). */
int smx_stream_create_with_cu_mask(smx_stream* out, const uint32_t* mask_words, uint32_t n_words);
/* Page-locked host memory for upload staging (cudaHostAlloc(..., cudaHostAllocWriteCombined) / cudaFreeHost,
 * APP/main.cc:825-829, 917): copies from it are asynchronous to the host.  write_combined memory is fast to
 * upload from and slow for the CPU to read. */
int smx_host_alloc(void** out, size_t bytes, int32_t write_combined);
int smx_host_free(void* p);
/* *yes = 1 if [p, p + bytes) lies inside page-locked memory the device can read (smx_host_alloc / hipHostMalloc /
 * hipHostRegister), else 0.  What smx_buffer_upload_by_kernel requires of its source; a caller with a choice of routes asks
 * before it enqueues anything (smx_driver does). */
int smx_host_is_page_locked(const void* p, size_t bytes, int32_t* yes);
int smx_stream_destroy(smx_stream s);
int smx_stream_synchronize(smx_stream s);
/* Events for cross-stream ordering (hipEvent_t, timing disabled): the frame driver overlaps depth
 * preprocessing of the next frame with the integration of the current one, as APP/main.cc overlaps uploads
 * (main.cc:902, 995).  An smx_event orders the streams of ONE device: it is created with a device-scope release
 * (hipEventReleaseToDevice), so work behind it is visible to kernels and copies of that GPU; it is not meant to be
 * waited for by the host or by another GPU (use smx_stream_synchronize for the host). */
typedef void* smx_event;
int smx_event_create(smx_event* out);
int smx_event_destroy(smx_event e);
int smx_event_record(smx_event e, smx_stream s);
int smx_stream_wait_event(smx_stream s, smx_event e);
/* Events that carry a time stamp (measurement only: the driver's per-stage profile of the preprocessing stream);
 * smx_event_elapsed_ms blocks until `stop` has completed. */
int smx_event_create_timed(smx_event* out);
int smx_event_elapsed_ms(smx_event start, smx_event stop, float* ms);
/* Launches an empty kernel (k_smx_marker) that delimits regions in kernel traces. */
int smx_debug_marker(smx_stream s, int32_t id);
/* (measurement) n ping-pongs of an empty kernel between two streams, each leg handed over by an event record + a stream wait:
 * mean time per leg in microseconds.  Synchronises both streams. */
int smx_debug_handover_probe(smx_stream a, smx_stream b, int32_t n, float* us_per_handover);
/* (measurement, process-wide) the device and page-locked host blocks smx_recon, smx_nn and the mesh workspace hold at this
 * moment, and their bytes (smx_buffer and smx_host_alloc are not counted).  Either pointer may be null. */
int smx_debug_live_allocations(uint64_t* blocks, uint64_t* bytes);
/* (test hook, process-wide) makes the nth next allocation of those objects (0 = the next one) fail with the out-of-memory
 * error -- on the host, HIP is not called -- and disarms itself; nth < 0 disarms a pending one. */
int smx_debug_fail_allocation(int32_t nth);

/* ---- CUDABuffer<T>  (VIS/cuda/cuda_buffer.h:45-129, cuda_buffer_inl.h:36-172) ---- */
/* CUDABuffer(int height, int width): cudaMallocPitch */
int smx_buffer_create(int32_t height, int32_t width, int32_t elem_bytes, smx_buffer* out);
int smx_buffer_destroy(smx_buffer b);
/* ToCUDA() */
int smx_buffer_get_desc(smx_buffer b, smx_buffer_desc* out);
/* UploadAsync / UploadPitchedAsync (src_pitch = 0: dense rows of width*elem_bytes) */
int smx_buffer_upload(smx_buffer b, smx_stream s, const void* src, size_t src_pitch);
/* The same copy done by a KERNEL that reads the page-locked source over the bus (src must come from smx_host_alloc /
 * hipHostMalloc; otherwise SMX_ERR_INVALID_ARGUMENT) -- an addition for callers that stage uploads on a stream of their own:
 * a kernel's stores reach later kernels on other streams through the ordinary event ordering, whereas a copy-engine write
 * followed by a cross-stream wait that the runtime finds already satisfied is dropped together with the cache invalidation
 * the consumer needs (measured: stale reads now and then).  Few workgroups (the copy is bound by the bus, not the chip).
 * done: optional completion event of the launch (no packet of its own on the stream). */
int smx_buffer_upload_by_kernel(smx_buffer b, smx_stream s, const void* src_pagelocked, size_t src_pitch, smx_event done);
/* DownloadAsync / DownloadPitchedAsync */
int smx_buffer_download(smx_buffer b, smx_stream s, void* dst, size_t dst_pitch);
/* UploadPartAsync / DownloadPartAsync: byte range [start, start+length) of the allocation */
int smx_buffer_upload_part(smx_buffer b, smx_stream s, size_t start, size_t length, const void* src);
int smx_buffer_download_part(smx_buffer b, smx_stream s, size_t start, size_t length, void* dst);
/* Clear(T value, stream): pattern points at one element (elem_bytes bytes) */
int smx_buffer_clear(smx_buffer b, smx_stream s, const void* pattern);
/* SetTo(const CUDABuffer<T>& other, stream) */
int smx_buffer_set_to(smx_buffer dst, smx_buffer src, smx_stream s);

/* ---- depth preprocessing free functions (APP/cuda_depth_processing.cuh:43-122) ---- */
/* BilateralFilteringAndDepthCutoffCUDA, APP/cuda_depth_processing.cu:120-158.  The disc radius is
 * (int)(radius_factor * sigma_xy + 0.5f) as there; radii 0 .. 8 are implemented, a larger one is refused with
 * SMX_ERR_INVALID_ARGUMENT before anything is launched (the output is left as it was). */
int smx_bilateral_filtering_and_depth_cutoff(
    smx_stream s, float sigma_xy, float sigma_value_factor, uint16_t value_to_ignore,
    float radius_factor, uint16_t max_depth, float depth_valid_region_radius,
    const smx_buffer_desc* input_depth /*u16*/, const smx_buffer_desc* output_depth /*u16*/);
/* OutlierDepthMapFusionCUDA<count,u16>, both overloads (cu:229-285 and :399-455):
 * other_count = count-1 in {2,4,6,8}; required_count < 0 selects the
 * all-must-agree overload.  others_TR_reference: other_count row-major 3x4. */
int smx_outlier_depth_map_fusion(
    smx_stream s, int32_t other_count, int32_t required_count, float tolerance,
    const smx_buffer_desc* input_depth, float fx, float fy, float cx, float cy,
    const smx_buffer_desc* other_depths /*[other_count]*/, const float* others_TR_reference,
    const smx_buffer_desc* output_depth);
/* BilateralFilteringAndDepthCutoffCUDA (value_to_ignore = 0) followed by OutlierDepthMapFusionCUDA, as the reference's
 * caller chains them (APP/main.cc:1015-1115), in ONE launch where the shape allows it (eight other frames, filter radius 1..8):
 * the outlier test of a pixel only needs that pixel's own filtered depth.  Same output image as the two calls; scratch_depth
 * (the intermediate image of the two-call form) is only written when the shape needs the two launches. */
int smx_bilateral_outlier_fusion(
    smx_stream s, float sigma_xy, float sigma_value_factor, float radius_factor, uint16_t max_depth,
    float depth_valid_region_radius, const smx_buffer_desc* input_depth,
    int32_t other_count, int32_t required_count, float tolerance, float fx, float fy, float cx, float cy,
    const smx_buffer_desc* other_depths /*[other_count]*/, const float* others_TR_reference,
    const smx_buffer_desc* scratch_depth, const smx_buffer_desc* output_depth);
/* ErodeDepthMapCUDA (radius 1..3), cu:540-579; CopyWithoutBorderCUDA, cu:609-633 */
int smx_erode_depth_map(smx_stream s, int32_t radius, const smx_buffer_desc* input_depth,
                        const smx_buffer_desc* output_depth);
int smx_copy_without_border(smx_stream s, const smx_buffer_desc* input_depth,
                            const smx_buffer_desc* output_depth);
/* MedianFilterAndDensifyDepthMap, APP/main.cc:206-252: in the reference a CPU loop before the upload (its TODO at
 * main.cc:928 asks for the GPU), one call per `median_filter_and_densify_iterations`.  Input and output must differ. */
int smx_median_filter_and_densify_depth_map(smx_stream s, const smx_buffer_desc* input_depth,
                                            const smx_buffer_desc* output_depth);
/* Image<u16>::DownscaleUsingMedianWhileExcluding, VIS/image.h:1003-1053 -- the depth half of --pyramid_level
 * (APP/main.cc:941-962), a CPU loop in the reference.  The output size selects the source blocks. */
int smx_downscale_using_median_while_excluding(smx_stream s, uint16_t value_to_ignore, const smx_buffer_desc* input,
                                               const smx_buffer_desc* output);
/* The colour half of --pyramid_level (APP/main.cc:973-981): ImagePyramid(frame, pyramid_level) = pyramid_level times
 * Image<Vec3u8>::DownscaleToHalfSize (VIS/image_cache.h:203-243, VIS/image.h:929-948: per channel
 * a/4 + b/4 + c/4 + d/4, each term truncated), a CPU loop in the reference.  3-byte pixels; 1 <= pyramid_level <= 4;
 * the input size must be divisible by 2^pyramid_level and the output buffer must have the resulting size. */
int smx_color_image_pyramid(smx_stream s, int32_t pyramid_level, const smx_buffer_desc* input,
                            const smx_buffer_desc* output);
/* ComputeNormalsAndDropBadPixelsCUDA, cu:720-762 */
int smx_compute_normals_and_drop_bad_pixels(
    smx_stream s, float observation_angle_threshold_deg, float depth_scaling,
    float fx, float fy, float cx, float cy,
    const smx_buffer_desc* in_depth, const smx_buffer_desc* out_depth,
    const smx_buffer_desc* out_normals /*float2*/);
/* ComputePointRadiiAndRemoveIsolatedPixelsCUDA, cu:839-883 */
int smx_compute_point_radii_and_remove_isolated_pixels(
    smx_stream s, float point_radius_extension_factor, float point_radius_clamp_factor,
    float depth_scaling, float fx, float fy, float cx, float cy,
    const smx_buffer_desc* depth_buffer, const smx_buffer_desc* radius_buffer /*float*/,
    const smx_buffer_desc* out_depth);

/* The three calls above that always follow each other in the caller (APP/main.cc:1128-1191: ErodeDepthMapCUDA or, for
 * erosion_radius 0, CopyWithoutBorderCUDA; ComputeNormalsAndDropBadPixelsCUDA; ComputePointRadiiAndRemoveIsolatedPixelsCUDA)
 * as ONE launch: the two intermediate depth images stay in LDS tiles.  out_depth, out_normals and radius_buffer receive
 * exactly what the three separate calls leave in their last outputs.  in_depth and out_depth must differ. */
int smx_erode_normals_radii(smx_stream s, int32_t erosion_radius, float observation_angle_threshold_deg,
                            float point_radius_extension_factor, float point_radius_clamp_factor, float depth_scaling,
                            float fx, float fy, float cx, float cy, const smx_buffer_desc* in_depth,
                            const smx_buffer_desc* out_depth, const smx_buffer_desc* out_normals /*float2*/,
                            const smx_buffer_desc* radius_buffer /*float*/);
/* The same launch with `done` (may be null) as its own completion event: equivalent to smx_event_record(done, s) behind the
 * call, without a packet of its own on the stream (the frame loop's "preprocessed" mark: smx_driver.cpp). */
int smx_erode_normals_radii_signal(smx_stream s, int32_t erosion_radius, float observation_angle_threshold_deg,
                                   float point_radius_extension_factor, float point_radius_clamp_factor, float depth_scaling,
                                   float fx, float fy, float cx, float cy, const smx_buffer_desc* in_depth,
                                   const smx_buffer_desc* out_depth, const smx_buffer_desc* out_normals /*float2*/,
                                   const smx_buffer_desc* radius_buffer /*float*/, smx_event done);

/* ---- CUDASurfelReconstruction (APP/cuda_surfel_reconstruction.h:44-176) ---- */
/* trailing arguments of Integrate(), .h:59-77; defaults APP/main.cc:323-368 */
typedef struct {
  float sensor_noise_factor;
  float max_surfel_confidence;
  float regularizer_weight;
  int32_t regularization_frame_window_size;
  int32_t do_blending;
  int32_t measurement_blending_radius;
  int32_t regularization_iterations_per_integration_iteration;
  float radius_factor_for_regularization_neighbors;
  float normal_compatibility_threshold_deg;
  int32_t surfel_integration_active_window_size;
} smx_integrate_params;

/* CUDASurfelBuffersCPU, APP/cuda_surfels_cpu.h:40-74 */
typedef struct {
  uint32_t frame_index;
  size_t surfel_count;
  float* surfel_x_buffer;
  float* surfel_y_buffer;
  float* surfel_z_buffer;
  float* surfel_radius_squared_buffer;
  float* surfel_normal_x_buffer;
  float* surfel_normal_y_buffer;
  float* surfel_normal_z_buffer;
  uint32_t* surfel_last_update_stamp_buffer;
} smx_surfel_buffers_cpu;

/* ctor, .h:47-53 / .cc:44-91 (the three GL resources and the render window are dropped).
 * device_id: the HIP device the object lives on, -1 = the calling thread's current device.  The object remembers
 * it: every smx_recon_* call makes it current for its duration (and restores the caller's device), so one process
 * can hold one object per GPU and call them from one thread each -- or from one thread -- without smx_set_device
 * in between.  Streams and buffers passed to a call must belong to the object's device. */
int smx_recon_create(uint32_t max_surfel_count, int32_t width, int32_t height,
                     float fx, float fy, float cx, float cy, int32_t device_id, smx_recon* out);
int smx_recon_destroy(smx_recon r);
/* Integrate, .h:59-77 / .cc:112-320.  depth is MUTATED by blending as in the
 * reference; global_T_local is row-major 3x4 (SE3f::matrix3x4()).
 * frame_index normally counts up from call to call (the reference's caller does, APP/main.cc:1015; stamps are compared
 * with it in windows, kernels.cu:77-87, 2132): pass A keeps, per 1024-slot segment, the newest stamp it has seen and
 * skips segments whose stamps have left the regulariser window, which presumes that time moves forward.  A call with a
 * smaller frame_index than the previous one is accepted like in the reference: it drops that cache (the call reads
 * every segment again) and costs one stream join.
 * measurement_blending_radius is only read (and range-checked, 2..255) when do_blending != 0. */
int smx_recon_integrate(smx_recon r, smx_stream s, uint32_t frame_index, float depth_scaling,
                        const smx_buffer_desc* depth /*u16*/, const smx_buffer_desc* normals /*float2*/,
                        const smx_buffer_desc* radius /*float*/, const smx_buffer_desc* color /*uchar3*/,
                        const float global_T_local[12], const smx_integrate_params* params);
/* Regularize, .h:82-87 / .cc:322-337 */
int smx_recon_regularize(smx_recon r, smx_stream s, uint32_t frame_index, float regularizer_weight,
                         float radius_factor_for_regularization_neighbors,
                         int32_t regularization_frame_window_size);
/* TransferAllToCPU, .h:91-94 / .cc:339-359.  Fills frame_index and surfel_count,
 * enqueues the 8 row downloads; the caller synchronises the stream
 * (APP/main.cc:1266-1267).  Reads the device-side count first (one small
 * blocking copy). */
int smx_recon_transfer_all_to_cpu(smx_recon r, smx_stream s, uint32_t frame_index,
                                  smx_surfel_buffers_cpu* buffers);
/* Changed-surfel delta for the mesher (not in the reference: SURVEY.md 8f-1, the step right after this path).
 * TransferAllToCPU moves 32 B x N over PCIe every time and leaves it to the CPU to find out what changed
 * (SurfelMeshing::IntegrateCUDABuffers, APP/surfel_meshing.cc:190-300 walks all N).  With tracking on, every kernel
 * that changes one of the eight transferred attributes of a slot marks the slot; the transfer compacts the marked
 * slots on the GPU, downloads (slot index ascending, the eight attributes) for those only and clears the marks.
 * Contract: applying every delta since a full transfer to that transfer's arrays reproduces the current full arrays
 * bit for bit (a delta may contain slots whose values did not change).  Enabling marks every existing slot.
 * smx_recon_transfer_changed_to_cpu is synchronous (it returns with the arrays filled); if count > capacity it fails,
 * reports the needed count and keeps the marks. */
typedef struct {
  uint32_t capacity;      /* in: entries each array can hold */
  uint32_t count;         /* out: entries written */
  uint32_t frame_index;   /* out */
  uint32_t surfel_count;  /* out: slots in use (as smx_surfel_buffers_cpu.surfel_count) */
  uint32_t* surfel_index;
  float* x;
  float* y;
  float* z;
  float* radius_squared;
  float* normal_x;
  float* normal_y;
  float* normal_z;
  uint32_t* last_update_stamp;
} smx_surfel_delta_cpu;
int smx_recon_set_delta_tracking(smx_recon r, smx_stream s, int32_t enabled);
int smx_recon_transfer_changed_to_cpu(smx_recon r, smx_stream s, uint32_t frame_index, smx_surfel_delta_cpu* delta);
/* ExportVertices, .h:109-112 / .cc:405-410: position 1 x 3N float, colour 1 x 3N u8 */
int smx_recon_export_vertices(smx_recon r, smx_stream s, const smx_buffer_desc* position_buffer,
                              const smx_buffer_desc* color_buffer);
/* GetTimings, .h:115-122 / .cc:412-429: data association, merging, blending, integration, neighbor update, new surfel
 * creation, regularization (ms) of the LAST smx_recon_integrate call; like the reference it waits until that call is
 * through (cudaEventSynchronize(regularization_end_event_), cc:420).  On from the first call; cost 1.4 - 2.2 % of the frame rate at
 * 640 x 480 / 5 M surfels, nothing measurable at 1280 x 960 (bench.py: stage_timing_cost; smx_recon_set_timing_enabled(r, 0)
 * switches the stamps off): the stages are not bracketed by event records (each a packet between two kernels of a stream that is never idle: fourteen
 * of them cost a third of the frame rate here) but stamped by the kernels themselves -- device wall clock, first
 * workgroup in of the launch that begins a stage / of the launch that follows it on the same stream, last workgroups out
 * where nothing follows -- into a per-call record.  Stages the
 * design fuses into another stage's launch report 0 -- out_ms[1] (surfel_merging: decided in the association kernel,
 * applied by the integration kernel) and out_ms[5] (new_surfel_creation: the first workgroups of the neighbour-update
 * launch): their time is INSIDE out_ms[0] / out_ms[3] and out_ms[4], so the seven values still add up to the call; a caller
 * that accumulates the reference's seven columns (APP/main.cc:1511-1530) gets two empty ones. */
int smx_recon_get_timings(smx_recon r, float out_ms[7]);
/* The same for a frame loop that must not wait: the stage times of the NEWEST call whose record has been handed over --
 * every call copies the record of the call before the previous one (complete by stream order at that point) into
 * page-locked host memory, so the read lags the queue by two calls and touches neither the device nor any stream.
 * *call_number: that call's 1-based number, 0 (and zeros) if there is none yet. */
int smx_recon_get_timings_nowait(smx_recon r, float out_ms[7], uint64_t* call_number);
/* How the front of a pipelined smx_recon_integrate call (pass A .. blend, on the caller's stream) hands over to the
 * internal stream: 1 = the blend's workgroups count themselves in a device word and a one-wavefront gate kernel in front of the
 * integration polls it (default: no event packet on the internal stream, and no release of the XCDs' L2s behind the blend --
 * its output leaves write-through -- + 3.6 % at 640 x 480, profiles/r6_ab_notes.md section 13), 0 = an event (rounds 3 - 6).
 * Results identical.  The two measurement modes of smx_recon_set_timing_enabled that bracket kernels with event records of
 * their own (bits 0 and 1) keep the event whatever the mode. */
int smx_recon_set_handover_mode(smx_recon r, int32_t mode);
/* The mode in use.  smx_recon_create starts an object in mode 0 when the process runs under a profiler that collects hardware
 * counters (ROCPROF_COUNTER_COLLECTION set, i.e. rocprofv3 --pmc): such a tool serialises the kernel dispatches of ALL queues, the
 * gate can then reach the chip in front of the launch it waits for, and nothing else is let on.  The gate's poll is bounded
 * (0.25 s); one that gives up invalidates the map, the next smx_recon_counts / smx_recon_get_stats returns SMX_ERR_UNSUPPORTED, and
 * the object goes back to mode 0 with its next smx_recon_integrate call (the gate leaves its mark in page-locked memory). */
int smx_recon_get_handover_mode(smx_recon r, int32_t* mode);
/* Experiment: the object's internal stream re-created on a subset of the compute units (mask as for
 * smx_stream_create_with_cu_mask; n_words = 0: all of them again, at the highest priority).  Waits for the object's work. */
int smx_recon_set_internal_cu_mask(smx_recon r, const uint32_t* mask_words, uint32_t n_words);
/* Measurement: the object's internal stream (for smx_debug_handover_probe; never enqueue work on it). */
int smx_recon_debug_internal_stream(smx_recon r, smx_stream* out);
/* Measurement: the raw stage-stamp records of the last 8 smx_recon_integrate calls (8 x 16 words of device wall clock,
 * rate in *wall_clock_khz; word 0 = the call's number, then: cull begin, tiles end*, blend begin, blend end*, integrate
 * begin, integrate end*, update begin, update end*, pass B begin, step end*, pass A begin, tiles begin, edge kernel begin,
 * step begin; * = maximum over the last workgroups dispatched).  bench.py turns them into the in-frame timeline of the
 * pipelined run -- no profiler, no event packets.  Call after synchronising. */
int smx_recon_debug_stamp_ring(smx_recon r, uint64_t* out, int32_t capacity_words, int32_t* wall_clock_khz);
/* enabled: bit 2 = stage stamps (default ON: what smx_recon_get_timings reads), bit 0 = the reference's own 14 stage
 * events instead (measurement: smx_recon_get_timings then reads those), bit 1 = events around every kernel */
int smx_recon_set_timing_enabled(smx_recon r, int32_t enabled);
/* Per-kernel device times of the last Integrate call (needs timing bit 1); slot names from
 * smx_recon_kernel_slot_name(0 .. smx_recon_kernel_slot_count()-1). */
int smx_recon_kernel_slot_count(void);
const char* smx_recon_kernel_slot_name(int32_t slot);
int smx_recon_get_kernel_timings(smx_recon r, float* out_ms, int32_t capacity);
/* HIP-event timing of ONE kernel slot over many Integrate calls (2 event records per frame on the
 * launch stream): begin, run up to max_frames frames, end -> average launch duration. */
int smx_recon_profile_begin(smx_recon r, int32_t slot, int32_t max_frames);
int smx_recon_profile_end(smx_recon r, float* avg_ms, int32_t* frames);
/* surfel_count() = slots - merged, surfels_size() = slots, .h:125-128.  Synchronises s. */
int smx_recon_counts(smx_recon r, smx_stream s, uint32_t* surfel_count, uint32_t* surfels_size);

/* Value distributions of the last Integrate call: synchronises s. */
typedef struct {
  uint32_t surfels_size, merge_count;
  uint32_t n_visible;      /* slots projecting into the image with z > 0 */
  uint32_t n_new, n_merged, n_recent, n_edges;
  uint32_t n_integrated, n_replaced, n_conflict_hits;
  uint32_t capacity_clamped;  /* 1 if new-surfel creation hit max_surfel_count */
  uint32_t n_window_edges;    /* neighbour links whose target lies inside the regulariser window */
  uint32_t n_contributors;    /* slots with at least one such link */
  uint32_t n_segments_skipped;  /* 1024-slot segments pass A did not have to read (out of view, unchanged) */
  uint32_t regularizer_saturated;  /* sticky since creation / state upload: a regulariser gradient term reached the
                                    * +-16 m range of the exact fixed-point sums, or one slot collected >= 100 senders
                                    * of one neighbour-count class; smooth positions may then deviate from the
                                    * reference.  Terms are 2 * regularizer_weight / count * (n . d) * n: with
                                    * neighbour distances of centimetres any weight below ~100 is far inside. */
  uint32_t n_pairs;            /* (slot, pixel) pairs pass A appended to the association tiles' bins */
  uint32_t n_overflow_pairs;   /* ... of which went through the overflow list (a tile's bin was full) */
  uint32_t max_tile_pairs;     /* pairs of the fullest tile */
} smx_recon_stats;
int smx_recon_get_stats(smx_recon r, smx_stream s, smx_recon_stats* out);
/* The n_* counters above are single-address atomics; they are collected only while enabled
 * (default on; benchmarks switch them off for the timed region).  surfels_size / merge_count are
 * always exact. */
int smx_recon_set_stats_enabled(smx_recon r, int32_t enabled);

/* Test / benchmark hooks (not part of the reference interface): raw access to
 * the surfel SoA rows (25 rows as in APP/cuda_surfel_reconstruction_kernels.cuh:49-78,
 * dense [25][count] on the host side) and to the per-pixel association images. */
int smx_recon_debug_download_surfels(smx_recon r, smx_stream s, float* rows, uint32_t count);
int smx_recon_debug_upload_surfels(smx_recon r, smx_stream s, const float* rows, uint32_t count,
                                   uint32_t merge_count);
enum {
  SMX_SCRATCH_SUPPORTING = 0,      /* u32 [H][W] */
  SMX_SCRATCH_SUPPORT_COUNTS = 1,  /* u32 */
  SMX_SCRATCH_DEPTH_SUMS = 2,      /* i64, 2^-32 fixed point */
  SMX_SCRATCH_CONFLICTING = 3,     /* u32, decoded index or 0xFFFFFFFF */
  SMX_SCRATCH_FIRST_DEPTH = 4,     /* f32 */
  SMX_SCRATCH_NEW_FLAGS = 5,       /* u8 [W*H] */
  SMX_SCRATCH_NEW_INDICES = 6      /* u32 [W*H], exclusive ranks */
};
int smx_recon_debug_download_scratch(smx_recon r, smx_stream s, int32_t which, void* dst);
/* Number of 1024-slot segments the last regulariser link scan did not have to read (every link of theirs stays among
 * slots nothing happened to; only with the statistics counters off -- the edge counters visit every link).  Tests. */
int smx_recon_debug_count_skipped_segments(smx_recon r, smx_stream s, uint32_t* out);
/* A/B switches; results are identical in every mode.  bit 0: every surfel kernel scans all slots like
 * the reference does instead of the compacted lists; bit 1: measurement blending as the reference's
 * start + iteration launches instead of the fused LDS kernel; bit 2: the regulariser's link scan gathers the flag byte
 * of every far link (no hot-group filter); bit 3: association bins of 16 pairs per tile, so that most pairs travel
 * through the overflow list; bit 4: pass A reserves bin space pair by pair instead of per (workgroup, tile) through
 * an LDS table (the path a pair takes that finds no room in that table); bit 5: the regulariser's far-term bins hold 4 records
 * per destination segment, bit 6: a sender workgroup addresses 2 destination segments through the bins -- the other far
 * terms take the atomic accumulators (the overflow paths of those bins); bit 7: the blend's other tile size (the
 * library picks 32 x 32 or 40 x 40 pixels by the number of tiles per compute unit; this bit swaps the choice);
 * bit 8: the list kernels run on a grid of four workgroups, so that every workgroup walks many steps;
 * bit 9: the regulariser's pass B and its edge kernel as ONE launch (the workgroup of a segment does the segment's edge work
 * itself, the work list stays in LDS) instead of two (pass B writes the work lists to memory, k_reg_accumulate walks
 * them: the default -- the fused launch is shorter alone and longer in the frame);
 * bit 10: the neighbour update gathers its candidates' records with plain loads instead of range-checked buffer loads (the
 * route of capacities from 2^28 slots, whose arrays 32-bit buffer offsets do not reach). */
int smx_recon_set_scan_mode(smx_recon r, int32_t mode);
/* TIMING ONLY -- the map is WRONG afterwards: leaves launches of smx_recon_integrate out, for the upper-bound runs of
 * bench.py --ub (what would the frame rate be without this chain?).  bit 0: no regulariser (pass B, edges, step);
 * bit 1: the front of the frame only (pass A, association tiles, blend): no integration, neighbour update, creation
 * or regulariser either.  bit 2: the internal stream does not wait for the front of the frame (blend -> integrate
 * hand-over left out), bit 3: the caller's stream does not wait for update + create (-> next pass A): what the two
 * cross-stream hand-overs cost the frame -- results undefined; bit 4: another arrangement of the streams (integrate + update
 * stay on the caller's stream behind the blend and wait for the previous call's edge kernel only, the internal stream keeps
 * pass B / edges / step and waits for update + create: the step kernel off every cycle, two hand-overs on the critical one) --
 * measured 5 % slower even as an upper bound, profiles/r6_ab_notes.md; bit 5 (test only): the front gate waits for one workgroup
 * more than the blend has and gives up after its bound; bit 6: the caller's stream is released behind the integration launch
 * instead of behind update + create; bit 7: the edge kernel works on the first 256 entries of every segment only; bit 8: the blend
 * stops behind its start ring (bits 6 - 8: upper bounds, profiles/r6_ab_notes.md sections 16, 21, 24).  0 = off. */
int smx_recon_debug_set_skip(smx_recon r, int32_t mask);
/* Frame pipelining (default on): the regulariser of a frame runs on an internal stream beside the first
 * kernels of the next smx_recon_integrate call (which only read what the regulariser does not write).
 * Every entry point that takes a stream first orders that stream after the pending regulariser, so the
 * one-stream semantics of CUDASurfelReconstruction are kept; results are identical on and off. */
int smx_recon_set_overlap(smx_recon r, int32_t enabled);
/* Dependency routing for a caller that runs its own pipeline around Integrate (smx_driver does: preprocessing of
 * later frames on a second stream).  An event record or wait costs a stream 6 - 8 us on this hardware, and the
 * caller's stream carries the frame-to-frame critical chain; these two hooks move one record and one wait per frame
 * from it to the internal stream.  Both are one-shot: they apply to the NEXT smx_recon_integrate call (also when
 * that call fails); either may be null.
 *   inputs_consumed  is recorded at the point from which that call no longer reads its four input images.
 *   chain_after      must have been recorded already; the call's internal completion mark waits for it.  The next
 *                    call orders its integration kernels -- and so every call after that all of its kernels -- after
 *                    that mark: work covered by chain_after is complete before the call AFTER the next one starts to
 *                    read its inputs, without any wait on the caller's stream.
 * With pipelining off both act on the caller's stream at the same points.
 * CONTRACT CHANGE for a caller that passes inputs_consumed (pipelining on): the caller's stream no longer waits for the
 * call's second half (integration, neighbour update, creation) when the call returns -- that wait is deferred into
 * the NEXT smx_recon_integrate call.  Until then the stream is NOT ordered behind the kernels that write the blended
 * depths back into the depth image and read the colour image: a caller that touches those four images (or reuses them)
 * outside another smx_recon_* entry point must first make its stream wait for inputs_consumed itself.  smx_driver does:
 * every run ends with that wait, and its frame upload / render / work-image download entry points wait for the steps
 * in flight.  Every other smx_recon_* entry point still orders its stream behind all internal work. */
int smx_recon_integrate_hooks(smx_recon r, smx_event inputs_consumed, smx_event chain_after);
/* A third hook of the same kind (one-shot, may be null): `inputs_ready` must have been recorded already (e.g. at the end of
 * the preprocessing of the frame, on the caller's preprocessing stream); the NEXT smx_recon_integrate call waits for it
 * on the caller's stream itself, AFTER its first kernel -- the all-slot scan, which does not read the four input images --
 * instead of the caller waiting in front of the call. */
int smx_recon_integrate_inputs_ready(smx_recon r, smx_event inputs_ready);

/* ---- radius-neighbor search (replaces CompressedOctree::FindNearestSurfelsWithinRadius,
 * APP/octree.h:470-477, APP/octree.cc:313-470, for batched queries) ---- */
/* Build a uniform-grid index over n points given as three device or host rows.
 * cell_size > 0; queries with radius <= cell_size touch at most 27 cells.  Points with a non-finite coordinate
 * are not indexed (no finite ball contains them).  The grid is sparse (sorted cell keys + a hash table of the occupied
 * 4x4x4-cell bricks), so cell_size is kept at any scene extent; results do not depend on it.  Synchronises s (two
 * small read-backs); the rows may be released / overwritten when the call returns.  Workspace is kept in the handle. */
/* device_id as in smx_recon_create; the index owns its workspace and reuses it from call to call. */
int smx_nn_create(int32_t device_id, smx_nn* out);
int smx_nn_destroy(smx_nn nn);
int smx_nn_build(smx_nn nn, smx_stream s, const float* x, const float* y, const float* z,
                 uint32_t n, float cell_size, int32_t rows_on_device);
/* For each query: up to k nearest points with dist^2 <= r2[q], ascending by
 * (dist^2, index).  state (may be NULL): points whose state byte has a bit of
 * skip_mask set are skipped (octree.cc:330-335).  Outputs are device or host
 * pointers according to outputs_on_device; out_idx/out_d2 are [nq][k].
 * With device-resident queries and outputs the call only enqueues kernels on s (no allocation once the workspace
 * has grown to the batch size, no synchronisation); with host pointers it returns after the results have arrived. */
int smx_nn_query_batch(smx_nn nn, smx_stream s, uint32_t nq, const float* qx, const float* qy,
                       const float* qz, const float* r2, int32_t k, const uint8_t* state,
                       uint8_t skip_mask, int32_t queries_on_device,
                       uint32_t* out_idx, float* out_d2, int32_t* out_count,
                       int32_t outputs_on_device);

/* Index geometry and (while enabled) counters of the queries since smx_nn_set_stats_enabled: what the C5 roofline of
 * SURVEY.md 8(d) is computed from.  The counters are single-address atomics (one per tile): off by default. */
typedef struct {
  uint32_t n_points, n_indexed, n_bricks;   /* given to the last build / with finite coordinates / occupied 4x4x4-cell bricks */
  float cell_size;                          /* the caller's, unless the 2^21-cells-per-axis key range forced it up */
  int32_t dim[3];                           /* cells per axis of the (sparse) grid */
  int32_t key_bits;                         /* width of the sort keys = 8 bits per radix pass */
  uint64_t tiles;                           /* query tiles (<= 64 queries of one brick) */
  uint64_t staged_candidates;               /* points staged in LDS, summed over the tiles */
  uint64_t distance_tests;                  /* exact tests, summed over the queries */
  uint64_t results;                         /* entries returned */
} smx_nn_stats;
/* Every indexed point queries its own neighbourhood (the full-retriangulation pattern, config C5 of SURVEY.md 8d;
 * APP/surfel_meshing.cc:549, 819-823): the same results as smx_nn_query_batch with the points' own positions, with
 * r^2 = factor * radius_squared[i] (device array indexed like the build rows) or, if radius_squared is NULL, r^2 =
 * factor for all.  Rows are indexed by point; points without finite coordinates get count 0.  Nothing is keyed, sorted
 * or gathered: a tile is an occupied brick, its queries are the brick's own records.  Device pointers only; enqueues
 * kernels on s, no allocation, no synchronisation. */
int smx_nn_query_self(smx_nn nn, smx_stream s, const float* radius_squared, float factor, int32_t k,
                      const uint8_t* state, uint8_t skip_mask, uint32_t* out_idx, float* out_d2, int32_t* out_count);
/* A/B switch of the query kernel (results are identical): 2 = one LANE per query over the brick tiles staged in LDS,
 * queries it cannot hold (more than 32 matches, very large regions) answered by kernel 0 afterwards (default);
 * 0 = one wavefront per query over the same staged tiles; 1 = one wavefront per query reading the brick ranges
 * through L1 / L2. */
int smx_nn_set_query_mode(smx_nn nn, int32_t mode);
int smx_nn_set_stats_enabled(smx_nn nn, smx_stream s, int32_t enabled);
int smx_nn_get_stats(smx_nn nn, smx_stream s, smx_nn_stats* out);

/* ---- the loop-closure hook the reference describes but does not ship (README.md:152-176; its call site is the
 * "### Loop closures ###" block of main.cc:1194-1200, between preprocessing and Integrate) ----
 * Every live surfel created at frame c < n_frames moves by the rigid correction frame_T[c] (row-major 3x4,
 * new_global_T_old_global; identity rows for frames that stay): offset = T * (X,Y,Z) - (X,Y,Z) is added to the raw
 * and to the smooth position (README.md:160-165), the normal becomes R * normal (:166-168); where reactivate[c] != 0
 * (array may be NULL) LastUpdateStamp is set to frame_index, which makes the surfel active for integration again
 * (:172-174).  Merged slots and slots created at c >= n_frames are untouched.  frame_T / reactivate are device
 * pointers if inputs_on_device, host pointers (synchronous call) otherwise. */
int smx_recon_deform_by_creation_frame(smx_recon r, smx_stream s, const float* frame_T, uint32_t n_frames,
                                       const uint8_t* reactivate, uint32_t frame_index, int32_t inputs_on_device);

/* ---- map compaction (not in the reference: its map only grows) ----
 * Removes every slot whose RadiusSquared < 0 (the merge mark) from [0, surfels_size()), keeping the remaining slots
 * in ascending order.  Synchronous: returns when the map is compacted.
 *   kept slots    slot i is kept iff !(RadiusSquared[i] < 0) and moves to old_to_new[i] = its rank among the kept
 *                 slots; every attribute row except the scratch rows 11-16 and 23 moves bit for bit.
 *   removed slots old_to_new[i] = 0xFFFFFFFF.
 *   links         the neighbour links of kept slots (rows 19-22) go through the same map; a link to a removed slot
 *                 becomes 0xFFFFFFFF.
 *   counts        afterwards surfels_size() == surfel_count() (unchanged) and the merge count is 0.
 *   links_dropped the valid links held by removed slots plus the links of kept slots that pointed into removed slots.
 *                 A merged slot keeps its outgoing links in the reference's semantics, and the regulariser still takes
 *                 one last gradient term from it when its neighbour re-enters the window; compaction removes that term.
 *                 links_dropped == 0 means that the continuation is an exact relabelling of the uncompacted run.
 * old_to_new may be NULL; otherwise it holds >= surfels_size() entries (capacity), and is a device pointer if
 * on_device, a host pointer otherwise.  A capacity that is too small fails with SMX_ERR_INVALID_ARGUMENT and leaves
 * the map unchanged.  new_size and links_dropped (host pointers) may be NULL.
 * The call is ordered after everything enqueued on the object before it (the pipelined regulariser and a deferred
 * smx_recon_integrate_hooks wait included); the next smx_recon_integrate may use any frame_index, as after a state
 * upload.  With delta tracking on, the next smx_recon_transfer_changed_to_cpu delivers every slot in [0, new_size).
 * A neighbour index (smx_nn) built before the call is stale: the caller rebuilds it, and remaps every slot index it
 * holds (mesher triangles, candidate lists) through old_to_new. */
int smx_recon_compact(smx_recon r, smx_stream s, uint32_t* old_to_new, uint32_t capacity, int32_t on_device,
                      uint32_t* new_size, uint32_t* links_dropped);

/* ---- viewer buffers: UpdateVisualizationBuffers, .h:100-108 / .cc:361-403 ----
 * The reference's three fill kernels (APP/cuda_surfel_reconstruction_kernels.cu:278-351, 434-449, 498-514) over
 * slots [0, surfels_size()) -- merged slots included -- into device buffers the caller owns (a viewer maps its GL
 * buffers itself and passes the pointers; the library does no graphics interop).  A NULL buffer is skipped; each
 * buffer receives slots [0, min(surfels_size(), its capacity)) and nothing beyond its capacity is written.  The slot
 * count is read on the device: the call enqueues work on s, ordered after the pipelined regulariser, and does not
 * synchronise with the host.  It changes no map state.
 *   vertex_buffer         4 floats per slot (Point3fC3u8): smooth x, y, z, then the 32 colour bits (uchar4 r, g, b, w).
 *                         x is NaN when creation_stamp > latest_triangulated_frame_index && slot < latest_mesh_surfel_count.
 *                         Colour, by precedence of the flags below:
 *                           LAST_UPDATE or CREATION  age = int(frame_index - stamp) (u32 difference), stamp = the creation
 *                                                  stamp if CREATION is set, the last-update stamp otherwise; age < 1 ->
 *                                                  (255, 80, 80), age > max -> (40, 40, 255), else grey 255 -
 *                                                  u8(255.99 * clamp((age - 1) / (max - 1))); max = 3000 for CREATION,
 *                                                  surfel_integration_active_window_size otherwise
 *                           RADII                  red = u8(255.99 * clamp((sqrt(r^2) - 0.0005) / 0.0095)), green = 255 -
 *                                                  red, blue = 80 (a merged slot: NaN -> clamp gives 0 -> (0, 255, 80))
 *                           NORMALS                u8(127.995 * (n + 1)) per axis
 *                           none                   the colour row's 32 bits as they are
 *                         (clamp is fminf(1, fmaxf(0, .)); the byte w is 0 in the computed modes)
 *   neighbor_index_buffer 8 u32 per slot: (slot, neighbour k or slot if the link is invalid) for k = 0..3
 *   normal_vertex_buffer  6 floats per slot: smooth position, smooth position + sqrt(r^2) * normal */
enum {
  SMX_VIS_LAST_UPDATE = 1,   /* visualize_last_update_timestamp */
  SMX_VIS_CREATION = 2,      /* visualize_creation_timestamp */
  SMX_VIS_RADII = 4,         /* visualize_radii */
  SMX_VIS_NORMALS = 8        /* visualize_normals */
};
int smx_recon_update_visualization_buffers(smx_recon r, smx_stream s, uint32_t frame_index,
    uint32_t latest_triangulated_frame_index, uint32_t latest_mesh_surfel_count,
    int32_t surfel_integration_active_window_size, int32_t flags,
    float* vertex_buffer, uint32_t vertex_capacity,
    uint32_t* neighbor_index_buffer, uint32_t neighbor_capacity,
    float* normal_vertex_buffer, uint32_t normal_capacity);

/* ---- headless map rendering (not in the reference: its viewer draws the vertex buffer with OpenGL) ----
 * Rasterises the live slots (i < surfels_size(), RadiusSquared >= 0) as splats into a 64-bit z-buffer and resolves it
 * into images of any size, from any camera.  p = smooth position, n = normal, c = R^T (p - t), n_c = R^T n for
 * global_T_camera = [R | t] (row-major 3x4, inverted on the host as in smx_recon_integrate, here in double precision;
 * the splat geometry is evaluated in double precision too, the key's depth is that value rounded to float).  A slot is drawn if
 * near_z < c.z < far_z; u = fx c.x / c.z + cx, v = fy c.y / c.z + cy (pixel-corner convention: pixel (x, y) spans
 * [x, x+1) x [y, y+1)).
 *   SMX_SPLAT_SQUARE  pixel covered iff |x + 1/2 - u| <= h and |y + 1/2 - v| <= h, h = splat_half_extent_in_pixels
 *                     (h = 0: the pixel (floor u, floor v) only); depth c.z.
 *   SMX_SPLAT_DISC    a disc of radius rho = disc_radius_factor * sqrt(r^2) around p, normal n.  Candidate pixels: centre
 *                     within e of (u, v) per axis, e = max_splat_extent_in_pixels if c.z - rho <= near_z, else
 *                     min(max extent, 2 max(fx, fy) rho / (c.z - rho)).  Ray d = ((x + 1/2 - cx) / fx, (y + 1/2 - cy) / fy, 1);
 *                     skipped if |n_c . d| < 1e-4; t = (n_c . c) / (n_c . d); covered iff t > near_z and
 *                     |t d - c|^2 <= rho^2; depth t.
 * Z-test: every pixel keeps the minimum of (float_bits(depth) << 32) | slot (ties go to the lower slot): the result
 * does not depend on scheduling, two renders are bit-identical.  Outputs (each may be NULL; otherwise exactly
 * height x width with the element size given, any pitch):
 *   depth  float   the winner's depth, 0 where no splat covers the pixel
 *   index  u32     the winning slot, 0xFFFFFFFF where empty
 *   normal float4  (n_c, 0) of the winner, zeros where empty
 *   color  uchar4  the winner's vertex-buffer colour (smx_recon_update_visualization_buffers, color_flags) with alpha
 *                  255; (0, 0, 0, 0) where empty
 * Enqueued on s after the pipelined regulariser, no host synchronisation; the map is only read (no delta marks, stats
 * or stamps change), so a render is valid between any two smx_recon_integrate calls.  The z-buffer (width x height x
 * 8 bytes) belongs to the object and grows on demand (growing it waits for the device).  Invalid sizes, parameters or
 * descriptors fail with SMX_ERR_INVALID_ARGUMENT. */
enum { SMX_SPLAT_SQUARE = 0, SMX_SPLAT_DISC = 1 };
typedef struct {
  int32_t width, height;
  float fx, fy, cx, cy;                    /* pixel-corner convention */
  float global_T_camera[12];               /* row-major 3x4 */
  float near_z, far_z;                     /* 0 < near_z < far_z */
  int32_t splat_mode;                      /* SMX_SPLAT_* */
  float splat_half_extent_in_pixels;       /* square mode, >= 0 (the reference viewer's default: 3) */
  float disc_radius_factor;                /* disc mode, > 0 (default 1) */
  float max_splat_extent_in_pixels;        /* disc mode, > 0 (default 16) */
  int32_t color_flags;                     /* SMX_VIS_* */
  uint32_t frame_index;                    /* for the age colours */
  int32_t surfel_integration_active_window_size;
} smx_render_params;
int smx_recon_render(smx_recon r, smx_stream s, const smx_render_params* p, const smx_buffer_desc* depth,
                     const smx_buffer_desc* index, const smx_buffer_desc* normal, const smx_buffer_desc* color);

/* ---- camera tracking against the map: frame-to-model point-to-plane ICP (not in the reference, which is fed by an
 * external SLAM system) ----
 * Inputs: the preprocessed depth and normal images of a frame exactly as smx_recon_integrate takes them, and a predicted
 * pose global_T_pred.  The call renders the map once at the prediction with the object's own size and intrinsics (disc
 * splats, by the kernels of smx_recon_render): model depth D (0 = empty) and model normal M in the prediction's camera
 * frame; model vertex of pixel (x, y): q = D ((x + 1/2 - cx) / fx, (y + 1/2 - cy) / fy, 1).  State: T_rel (model camera
 * <- frame camera), the identity at the start; answer global_T_frame = global_T_pred T_rel.
 * One iteration at pixel stride s visits the frame pixels (x, y) = (s/2 + i s, s/2 + j s): vertex v = z ((x + 1/2 - cx) /
 * fx, (y + 1/2 - cy) / fy, 1), z = depth / depth_scaling (skipped if depth == 0), normal n = (nx, ny, -sqrt(max(0, 1 -
 * nx^2 - ny^2))); p = R_rel v + t_rel, m = R_rel n; skipped unless p.z > 0 and (u, w) = (floor(fx p.x / p.z + cx),
 * floor(fy p.y / p.z + cy)) lies in the image and D(w, u) > 0 (the pixel is then "associated"); gates |p - q|^2 <=
 * max_distance^2 and m . M >= cos(max_normal_angle); residual r = M . (p - q), Jacobian row J = (p x M, M) -- rotation
 * first, then translation: the update is a twist applied on the left, in the model camera's frame.  The per-pixel terms
 * are single precision, their sums double precision in a fixed order (per-workgroup partial sums, added in index
 * order): two calls give the same bits.  x = -(J^T J)^-1 J^T r by an LDL^T factorisation, T_rel <- exp(x) T_rel', both
 * in double precision on the device; T_rel is kept in double and handed to an iteration as 12 floats, T_rel' (the pose the
 * iteration linearised at, which the twist corrects).  Levels run in the order given (coarse to fine); strides sample, no pyramid is built.
 * Status, decided on the device per iteration, in this order:
 *   NOT_FINITE       a sum or the solution is not finite;
 *   DEGENERATE       pixels with depth but none associated (an empty render), or a pivot of the factorisation below
 *                    min_pivot_ratio x the largest diagonal entry (one plane);
 *   TOO_FEW_INLIERS  inliers < min_inliers in any iteration (nothing is solved below that floor), or -- judged on the
 *                    LAST iteration run only -- inliers < min_inlier_fraction x pixels with depth;
 *   CONVERGED        |rotation part of x| < convergence_rotation and |translation part| < convergence_translation: the
 *                    remaining iterations of that level are skipped, the next level still runs;
 *   OK               otherwise.
 * A bad status (>= SMX_TRACK_TOO_FEW_INLIERS) is sticky: T_rel keeps the value it had before the failing iteration's
 * update and the later kernels of the call return at once.  The host looks at nothing until the end: every iteration
 * of every level is enqueued back to back on s (the render, one state-reset launch, then a reduce and a solve launch per
 * iteration).  The call is ordered like smx_recon_render and changes no map state, delta mark, statistic or stamp.
 * result is a device pointer if result_on_device (the call stays asynchronous), else a host pointer (the call returns
 * with it filled).  model_depth_out / model_normal_out (may be NULL; the object's width x height, float / float4)
 * receive the model images the call used: bit for bit what smx_recon_render gives for the same parameters.
 * SMX_ERR_INVALID_ARGUMENT (nothing launched): wrong image sizes or element sizes, a stride outside {1, 2, 4, 8}, no
 * level with iterations, more than 32 iterations in a level, non-positive gates, near_z >= far_z.  An empty map is no
 * error (DEGENERATE). */
enum { SMX_TRACK_OK = 0, SMX_TRACK_CONVERGED = 1, SMX_TRACK_TOO_FEW_INLIERS = 2,
       SMX_TRACK_DEGENERATE = 3, SMX_TRACK_NOT_FINITE = 4 };
typedef struct {            /* smx_track_params_default() fills the defaults */
  int32_t level_stride[3];  int32_t level_iterations[3];   /* stride in {1,2,4,8}; 0 iterations = level unused */
  float max_distance;  float max_normal_angle_deg;
  float convergence_rotation;  float convergence_translation;
  int32_t min_inliers;  float min_inlier_fraction;  float min_pivot_ratio;
  float near_z, far_z, disc_radius_factor, max_splat_extent_in_pixels;
} smx_track_params;
typedef struct {
  float global_T_frame[12];          /* the prediction itself if nothing could be solved */
  int32_t status;  int32_t iterations_run;
  uint32_t inliers;  uint32_t pixels_with_depth;          /* of the last iteration run */
  float rms_residual;                                      /* metres, point-to-plane, last iteration */
  float last_update_rotation, last_update_translation;
  float information[36];                                   /* JtJ of the last iteration, row-major 6x6 */
} smx_track_result;
/* Defaults: levels (4, 4), (2, 5), (1, 10); gates 10 cm / 30 degrees; convergence 1e-5 rad / 1e-5 m; min_inliers 50,
 * min_inlier_fraction 0.1, min_pivot_ratio 1e-6; near_z 0.05, far_z 20, disc_radius_factor 1, splats of <= 16 pixels. */
int smx_track_params_default(smx_track_params* out);
int smx_recon_track(smx_recon r, smx_stream s, float depth_scaling,
                    const smx_buffer_desc* depth /*u16*/, const smx_buffer_desc* normals /*float2*/,
                    const float global_T_pred[12], const smx_track_params* params,
                    smx_track_result* result, int32_t result_on_device,
                    const smx_buffer_desc* model_depth_out /*float, may be NULL*/,
                    const smx_buffer_desc* model_normal_out /*float4, may be NULL*/);
/* Tests and tuning: one record per iteration of the last smx_recon_track call that produced sums (the iteration that
 * raised a bad status included).  sums: [0..20] the upper triangle of JtJ row by row, [21..26] Jtr, [27] sum r^2,
 * [28] inliers, [29] frame pixels with a depth at this stride, [30] of which associated with a model pixel.  x is zero
 * where nothing was solved.  Synchronises s; *count = records of the call (at most `capacity` are written). */
#define SMX_TRACK_SUMS 31
typedef struct {
  int32_t level, stride, status, reserved;   /* status after the iteration */
  double sums[SMX_TRACK_SUMS];
  double x[6];
} smx_track_iteration;
int smx_recon_debug_track_iterations(smx_recon r, smx_stream s, smx_track_iteration* records, int32_t capacity,
                                     int32_t* count);

/* ---- camera tracking with colour: point-to-plane ICP + a photometric term (not in the reference) ----
 * Everything of smx_recon_track stays -- the render at the prediction, the sampling, the association, the two geometric
 * gates, r, J, the status rules and their order, the LDL^T solve, the left twist, levels and convergence -- and a one-plane
 * view that smx_recon_track reports as DEGENERATE is held in place by the map's colour (row 24) and the frame's colour
 * image (uchar3, the object's size: the image smx_recon_integrate takes).  Additions:
 * Model photometric image.  The same render also resolves colour with color_flags = 0 (uchar4, bit for bit what
 * smx_recon_render gives); from it and the model depth D one kernel writes a dense float4 P[H][W] = (L, gx, gy, valid):
 *   L  = ((0.299f r + 0.587f g) + 0.114f b) (1.0f / 255.0f)       (float, left to right; 0 at an empty pixel)
 *   gx = 0.5f (L(x+1, y) - L(x-1, y)),  gy = 0.5f (L(x, y+1) - L(x, y-1))
 *   valid = 1 iff 1 <= x <= W-2 and 1 <= y <= H-2, D > 0 at the pixel and at its four neighbours, and for each neighbour
 *           |D(nb) - D(x, y)| <= gradient_max_relative_depth_step D(x, y); otherwise gx = gy = valid = 0.
 * Frame intensity I_f(x, y): the same formula on the frame's colour at the sampled pixel.
 * Photometric term of a sampled frame pixel that has depth, is associated with model pixel (u, w) and passes the distance
 * gate (the normal gate does not apply): uc = fx p.x / p.z + cx, wc = fy p.y / p.z + cy (the values whose floors are u, w),
 *   Lm = (L + gx (uc - (u + 1/2))) + gy (wc - (w + 1/2)),  e = Lm - I_f;
 * the pixel is a photometric inlier iff valid, gx^2 + gy^2 >= min_gradient^2 and |e| <= max_intensity_difference.  Then
 *   a = ((gx fx) / p.z, (gy fy) / p.z, -(((gx fx) p.x + (gy fy) p.y) / (p.z p.z))),  J_I = (p x a, a)   (rotation first),
 * and with K = photometric_weight J_I and s = photometric_weight e (each one float product) the pixel adds K_a K_b to
 * JtJ, K_a s to Jtr and e^2 to a sum of its own.  Per-pixel terms are float, the sums double in the same fixed order.
 * Sums: SMX_TRACK_RGBD_SUMS = 33; [0..30] as SMX_TRACK_SUMS with JtJ and Jtr now the combined ones ([27..30] keep their
 * geometric meanings), [31] sum e^2, [32] photometric inliers.  Status: the rules and their order are unchanged;
 * min_inliers and min_inlier_fraction judge the GEOMETRIC inliers, the pivot test runs on the combined matrix, the
 * finiteness test covers all 33 sums.  (A frame colour alone could track -- no geometric inliers -- is TOO_FEW_INLIERS.)
 * photometric_weight == 0: neither the colour resolve nor the prepare kernel is launched, no photometric term is added
 * ([31] = [32] = 0) and the pose, status, counts, information matrix and sums [0..30] of every iteration are bit-identical
 * to smx_recon_track with the embedded smx_track_params; model_photo_out is then left untouched.
 * Launches: those of smx_recon_track + 1.  Ordering, stream semantics, "changes no map state" and the argument errors are
 * those of smx_recon_track; in addition SMX_ERR_INVALID_ARGUMENT (nothing launched) for a colour image of the wrong size
 * or element size (as far as a descriptor shows the latter: a pitch below 3 x width), a negative or non-finite weight, a non-positive max_intensity_difference or depth step, a negative
 * min_gradient.  model_photo_out (may be NULL; float4, the object's size) receives P. */
typedef struct {                 /* smx_track_rgbd_params_default() fills the defaults */
  smx_track_params icp;
  float photometric_weight;                 /* metres per unit intensity (0..1 scale); >= 0; default 0.1 */
  float max_intensity_difference;           /* > 0; default 0.2 */
  float min_gradient;                       /* >= 0, intensity per pixel; default 0.02 */
  float gradient_max_relative_depth_step;   /* > 0; default 0.02 */
} smx_track_rgbd_params;
typedef struct {
  smx_track_result icp;                     /* inliers, rms_residual: the geometric ones; information: the combined JtJ */
  uint32_t photometric_inliers;             /* of the last iteration run */
  float rms_intensity_residual;             /* intensity units (0..1 scale), last iteration */
} smx_track_rgbd_result;
#define SMX_TRACK_RGBD_SUMS 33
typedef struct {
  int32_t level, stride, status, reserved;
  double sums[SMX_TRACK_RGBD_SUMS];
  double x[6];
} smx_track_rgbd_iteration;
/* Defaults: smx_track_params_default() for icp; weight 0.1 (0.02 of intensity noise then weighs like 2 mm of depth
 * noise); max_intensity_difference 0.2; min_gradient 0.02 (+-2 grey levels of noise give central differences of at most
 * 2/255 per axis, a magnitude <= 0.011: below the gate); gradient_max_relative_depth_step 0.02. */
int smx_track_rgbd_params_default(smx_track_rgbd_params* out);
int smx_recon_track_rgbd(smx_recon r, smx_stream s, float depth_scaling,
                         const smx_buffer_desc* depth /*u16*/, const smx_buffer_desc* normals /*float2*/,
                         const smx_buffer_desc* color /*uchar3*/, const float global_T_pred[12],
                         const smx_track_rgbd_params* params, smx_track_rgbd_result* result, int32_t result_on_device,
                         const smx_buffer_desc* model_depth_out /*float, may be NULL*/,
                         const smx_buffer_desc* model_normal_out /*float4, may be NULL*/,
                         const smx_buffer_desc* model_photo_out /*float4 P, may be NULL*/);
/* As smx_recon_debug_track_iterations, for the last smx_recon_track_rgbd call (*count = 0 if the last tracking call was
 * smx_recon_track). */
int smx_recon_debug_track_rgbd_iterations(smx_recon r, smx_stream s, smx_track_rgbd_iteration* records, int32_t capacity,
                                          int32_t* count);

/* ---- candidate lists for the mesher, straight from the device-resident map ----
 * Replaces, for the surfels of one batch (e.g. one changed-surfel delta), the per-surfel octree query at the top of
 * SurfelMeshing::TriangulateSurfel (APP/surfel_meshing.cc:417-425) with the widest radius that function can ask for,
 * radius_factor_squared * radius_squared (surfel_meshing.cc:359-360, --max_neighbor_search_range_increase_factor):
 * a query with a smaller radius and the same K is the prefix of this list with dist^2 <= that radius.
 *
 * build_neighbor_index: (re)builds `nn` over the smooth positions of all surfels_size() slots without a host
 * round trip; merged slots are left out (cuda_surfel_reconstruction.cc:348-358 hands the mesher the same rows and it
 * removes merged surfels from its octree).  The index is a snapshot: rebuild it after Integrate / Regularize.
 * neighbor_candidates: for q < n_indices, up to k (<= 64) nearest indexed surfels within the ball of slot
 * surfel_indices[q], ascending by (dist^2, index); an out-of-range or merged slot gets count 0.  state / skip_mask
 * as in smx_nn_query_batch, one byte per slot (surfels_size() bytes).  surfel_indices and state are device or host
 * pointers according to inputs_on_device, the three outputs according to outputs_on_device. */
int smx_recon_build_neighbor_index(smx_recon r, smx_stream s, smx_nn nn, float cell_size);
int smx_recon_neighbor_candidates(smx_recon r, smx_stream s, smx_nn nn, const uint32_t* surfel_indices,
                                  uint32_t n_indices, float radius_factor_squared, int32_t k,
                                  const uint8_t* state, uint8_t skip_mask, int32_t inputs_on_device,
                                  uint32_t* out_idx, float* out_d2, int32_t* out_count, int32_t outputs_on_device);

/* The per-triangle tests of SurfelMeshing::CheckRemeshing (APP/surfel_meshing.cc:590-650) for a batch of triangles
 * (three slot indices each, [n_triangles][3]) against the device-resident map; the mesher keeps the sequential part
 * (RemeshTrianglesAt and the visiting order).  long_edge_total_factor_squared as in surfel_meshing.cc:171-173.
 * flags[t]: bit 0 = long-edge condition (:605-617; independent of the pivot vertex); bits 1..3 = the triangle normal
 * formed from pivot index(0) / index(1) / index(2) (right = next, left = previous vertex, :576-589) is inconsistent
 * with all three surfel normals (:632-635); bit 4 = a vertex is merged (:559-570) or out of range (then no other bit
 * is set).  triangles and flags are device pointers if on_device, host pointers (synchronous call) otherwise. */
int smx_recon_check_triangles(smx_recon r, smx_stream s, const uint32_t* triangles, uint32_t n_triangles,
                              float long_edge_total_factor_squared, uint8_t* flags, int32_t on_device);

/* ---- triangulation of the map on the device: a localized Delaunay triangulation (not in the reference, whose
 * advancing-front mesher is a sequential CPU algorithm; Gopi et al. 2000, Buchart et al. 2008) ----
 * A pure function of the map as it stands, slots [0, surfels_size()): smooth position (rows 3-5), RadiusSquared (row 7),
 * normal (rows 8-10).  A slot is live iff !(RadiusSquared < 0) and its smooth position is finite.
 * Candidates of live slot p: the list smx_nn_query_self gives for p with r^2 = search_radius_factor^2 RadiusSquared[p]
 * and k = max_neighbors (ascending by (dist^2, index)), without p itself, without every j with dot(n_p, n_j) <=
 * cos(max_angle_between_normals), and without every j whose projection onto p's tangent plane has a squared length
 * <= 1e-12 RadiusSquared[p].
 * Star of p: the candidates' smooth positions are projected onto the plane through p with normal n_p (p = origin); the
 * star is the set of Delaunay triangles of {origin} + {projections} that are incident to the origin: (origin, a, b)
 * with a turn from a to b in (0, pi) and no other candidate strictly inside the circle through the three.  Fewer than
 * two candidates: empty star.  More than max_star_degree star neighbours: empty star, counted in star_overflow.
 * Agreement: {p, a, b} is accepted iff it is in the star of p, of a and of b.
 * Filters, on the 3-D smooth positions: every interior angle within [min_triangle_angle, max_triangle_angle]; the
 * triangle normal, oriented to have a positive dot with n_p + n_a + n_b, has a positive dot with each of the three.
 * Output: uint32 [T][3], each triangle once, stored (p, a, b) with p the smallest slot index, counter-clockwise seen
 * from the side the oriented normal points to, the array ascending by (p, a, b).  Two calls on the same map give the
 * same bytes (count, exclusive scan, write: no atomic cursor).  Hence: every index is live, no triangle twice, every
 * undirected edge in at most two triangles, every edge (u, v) has |uv|^2 <= factor^2 min(r^2_u, r^2_v).
 * Where the three tangent planes disagree the triangle is rejected and a hole stays: no hole filling here. */
typedef struct {              /* smx_mesh_params_default() fills the defaults (names as in the reference's main.cc) */
  float max_angle_between_normals_deg;   /* 90 */
  float min_triangle_angle_deg;          /* 10 */
  float max_triangle_angle_deg;          /* 170 */
  float search_radius_factor;            /* 1.0; allowed 1 .. 2 (max_neighbor_search_range_increase_factor) */
  int32_t max_neighbors;                 /* 64; allowed 1 .. 64 */
  int32_t max_star_degree;               /* 16: fixed at compile time, reported by the default call, not settable */
} smx_mesh_params;
typedef struct {
  uint32_t n_live;             /* live slots */
  uint32_t n_star_triangles;   /* distinct triangles that are in at least one star */
  uint32_t n_triangles;        /* accepted by agreement and filters = T */
  uint32_t star_overflow;      /* live slots whose star had more than max_star_degree neighbours */
  uint32_t truncated_lists;    /* live slots whose candidate list came back full (max_neighbors entries) */
} smx_mesh_stats;
int smx_mesh_params_default(smx_mesh_params* out);
/* Rebuilds `nn` over the map itself (smx_recon_build_neighbor_index with cell_size) and triangulates.  Ordered after
 * everything enqueued on the object; synchronous like smx_recon_compact.  triangles: device pointer if on_device, host
 * pointer otherwise, room for `capacity` triangles.  capacity < T: SMX_ERR_INVALID_ARGUMENT, *n_triangles = T, nothing
 * is written (ask with capacity 0, allocate, call again); triangles == NULL with capacity 0 is that count-only form.
 * stats may be NULL.  SMX_ERR_INVALID_ARGUMENT (nothing launched): max_neighbors outside 1 .. 64, search_radius_factor
 * outside 1 .. 2, angles outside 0 .. 180 or min > max, a max_star_degree other than the default's.  Changes no map
 * state.  Workspace (lists, rings, counts) is kept in the object and reused. */
int smx_recon_triangulate(smx_recon r, smx_stream s, smx_nn nn, float cell_size, const smx_mesh_params* p,
                          uint32_t* triangles, uint32_t capacity, int32_t on_device, uint32_t* n_triangles,
                          smx_mesh_stats* stats);
/* Tools: milliseconds the last smx_recon_triangulate call spent in the index build, the list query, the star kernel,
 * and agreement + scan + write (timed events on the call's stream).  Zeros before the first call. */
int smx_recon_debug_mesh_timings(smx_recon r, float out_ms[4]);

/* ---- the same triangulation, kept up to date ----
 * smx_recon_triangulate_update returns exactly the bytes and statistics smx_recon_triangulate returns on the same map; it
 * keeps the last triangulation in the object, finds what changed since, and recomputes only that.
 * Kept state (written by this call): the slot count n_prev; the parameters; per slot a snapshot of the seven words the
 * triangulation reads (smooth x, y, z; RadiusSquared; normal x, y, z), the ring row and meta word, the number of triangles
 * the slot owns and the number of distinct star triangles counted at it; the scan offsets; the output array on the device.
 * With n the current slot count, f2 = float32(search_radius_factor) * float32(search_radius_factor), live as above:
 * changed(i): i >= n_prev, or any of the seven words differs BITWISE from the snapshot (a NaN equals itself, -0 differs
 *   from +0: conservative).
 * D, the slots whose star is recomputed: every changed slot (one that is no longer live gets an empty ring), and every
 *   unchanged live slot q for which some changed slot c has (c live now and d2(q, position of c) <= f2 r2_q) or (c live
 *   in the snapshot and d2(q, snapshot position of c) <= f2 r2_q); d2 and the comparison as smx_nn decides them (float32
 *   differences, squares, left-to-right sum, against the float32 product).  D is conservative where a candidate list is
 *   truncated to max_neighbors: a star that is recomputed without need comes out the same.
 * A, the slots whose owned triangles and star-triangle count are recomputed: D and every member of the old and of the
 *   new ring of every slot in D.  (Acceptance, filters, orientation and the slot a triangle is counted at depend only on
 *   which of its corners' stars hold it and on the corners' attributes; for p outside D the verdict on {p, d, x} can only
 *   change if d's star held it before or holds it now, and then p and x are in d's old or new ring.)  Slots outside A
 *   keep their counts and their run of the previous array.
 * The full path runs, and update_stats->mode says why, when: no state is kept (1; also after smx_recon_triangulate, which
 *   shares and overwrites the rings, and after smx_recon_triangulate_reset); the parameters differ from the kept ones
 *   (2); n < n_prev, as after smx_recon_compact (3); |D| > full_above_fraction n (4).  smx_recon_debug_upload_surfels and
 *   smx_recon_deform_by_creation_frame need no hook: the bitwise diff sees what they did.
 * full_above_fraction: 0 .. 1, < 0 = the library's default, 0.2.  It is the largest swept |D| / n at which the update still
 *   beat the full call by at least 10 % on an MI355X at 5.6 M slots: update time / full-call time was 0.29, 0.36, 0.78,
 *   0.91, 1.34, 1.64 at |D| / n = 0.037, 0.060, 0.138, 0.200, 0.354, 0.571.  It only chooses the path: the
 *   results are the same either way.
 * Output, arguments and errors as smx_recon_triangulate (nn ends up built over the map itself), plus: full_above_fraction
 *   > 1 is SMX_ERR_INVALID_ARGUMENT with nothing launched.  Capacity rule: capacity < T fails with
 *   SMX_ERR_INVALID_ARGUMENT, *n_triangles = T and nothing written to `triangles`, but the state HAS advanced: the second
 *   call of "ask, allocate, call again" finds 0 changed slots, does the diff and copies the kept array out.
 * Memory of the state: 32 bytes of snapshot, 4 of counts and flags, 2 x 4 of offsets per slot, two arrays of 12 T. */
typedef struct {
  uint32_t mode;          /* 0 = incremental; 1 = no state, 2 = parameters differ, 3 = fewer slots than kept,
                             4 = dirty fraction above the limit (full path ran) */
  uint32_t n_changed;     /* slots with changed(i) (mode 1 .. 3: every slot) */
  uint32_t n_dirty;       /* |D| (mode 1 .. 3: every slot) */
  uint32_t n_reagreed;    /* |A| (mode 1 .. 4: every slot) */
  uint32_t n_kept_triangles; /* copied from the previous array */
} smx_mesh_update_stats;
int smx_recon_triangulate_update(smx_recon r, smx_stream s, smx_nn nn, float cell_size, const smx_mesh_params* p,
                                 float full_above_fraction /* 0 .. 1; < 0 = the library's default */,
                                 uint32_t* triangles, uint32_t capacity, int32_t on_device, uint32_t* n_triangles,
                                 smx_mesh_stats* stats, smx_mesh_update_stats* update_stats);
int smx_recon_triangulate_reset(smx_recon r);            /* drops the kept state and frees its memory */
/* Tools: milliseconds the last smx_recon_triangulate_update spent in the diff, the index builds (reverse test's and the
 * map's), the reverse test (query and work list), the subset lists, the stars, and agreement + scan + merge.  Zeros
 * before the first call. */
int smx_recon_debug_mesh_update_timings(smx_recon r, float out_ms[6]);

/* ---- a coarser level of detail of a triangle array: vertex clustering (Rossignac and Borrel 1993) ----
 * A pure function of the map as it stands (smooth position rows 3-5, RadiusSquared row 7, slots [0, n) with n =
 * surfels_size()), of triangles_in (uint32 [n_in][3], slot indices, e.g. the output of smx_recon_triangulate) and of cell_size.
 * Every quantity is an integer or a float32 expression evaluated as written, one rounding per operation, no contraction.
 * 1. Live: a slot is live iff !(RadiusSquared < 0) and its smooth position is finite.  A triangle with a corner that is not
 *    live is dropped and counted in n_not_live (an array gone stale after an integration: not an error).  An index >= n
 *    anywhere in the input: SMX_ERR_INVALID_ARGUMENT, nothing is written.  U = the slots that occur in the remaining triangles.
 * 2. Cell: inv = 1.0f / cell_size (one float32 division); c_k = (int32)floorf(x_k * inv) for k = x, y, z.  Every c_k of every
 *    slot in U must lie in [-2^20, 2^20), otherwise SMX_ERR_INVALID_ARGUMENT (the cell is too small for the extent of the
 *    map; nothing is written).  key = ((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_z + 2^20).
 * 3. Representative: centre_k = ((float)c_k + 0.5f) * cell_size, d_k = x_k - centre_k, d2 = (d_x d_x + d_y d_y) + d_z d_z.
 *    rep(cell) = the slot of U in the cell with the smallest (float_bits(d2) << 32) | slot: the one nearest to the centre, a
 *    tie going to the lower slot.  vertex_map[i] = rep(cell(i)) for i in U, 0xFFFFFFFF for every other slot.
 * 4. Triangles: each remaining triangle becomes (rep p, rep a, rep b), winding kept.  Two equal corners: dropped, counted
 *    in n_collapsed.  Among triangles with the same set of three corners, in either winding, the earliest in triangles_in
 *    stays; the others are counted in n_duplicates.
 * 5. Output: uint32 [T_out][3], each triangle rotated so that its smallest index is first (winding kept), the array
 *    ascending by (p, a, b): the format of smx_recon_triangulate, over slot indices, so colour, normals, export, old_to_new
 *    remapping and a further call with a larger cell work on it unchanged.  Two calls give the same bytes.
 * 6. Not promised: vertex clustering does not keep the surface manifold.  An edge may lie in more than two triangles, and
 *    a triangle may end up facing against its corners' normals.  No filter is applied.
 * Calling rules as smx_recon_triangulate: ordered after everything enqueued on the object, synchronous.  on_device says
 * where triangles_in, triangles_out and vertex_map live (host arrays are staged).  capacity < T_out:
 * SMX_ERR_INVALID_ARGUMENT, *n_triangles = T_out, nothing written to triangles_out or vertex_map; triangles_out == NULL with
 * capacity 0 is that count-only form.  n_in == 0 is valid (T_out = 0).  cell_size must be finite and > 0.  triangles_out
 * must not overlap triangles_in (refused).  vertex_map may be NULL, else it has surfels_size() entries.  stats may be NULL;
 * it is filled whenever T_out is known.  Changes no map state, delta mark, statistic or stamp, nor the state
 * smx_recon_triangulate_update keeps.  The workspace belongs to the object, grows on demand and is reused. */
typedef struct {
  uint32_t n_in;             /* triangles given */
  uint32_t n_not_live;       /* of those, dropped because a corner is not live */
  uint32_t n_used_vertices;  /* distinct live slots that occur in the remaining triangles */
  uint32_t n_cells;          /* occupied cells = distinct representatives */
  uint32_t n_collapsed;      /* triangles with two corners in one cell */
  uint32_t n_duplicates;     /* triangles dropped because an earlier one has the same three corners */
  uint32_t n_triangles;      /* T_out */
} smx_decimate_stats;
int smx_recon_decimate_mesh(smx_recon r, smx_stream s, float cell_size,
                            const uint32_t* triangles_in, uint32_t n_in,
                            uint32_t* triangles_out, uint32_t capacity,
                            uint32_t* vertex_map /* may be NULL; surfels_size() entries */,
                            int32_t on_device, uint32_t* n_triangles, smx_decimate_stats* stats);
/* Tools: milliseconds the last smx_recon_decimate_mesh call spent in its SMX_DECIMATE_PHASES phases -- clustering (mark,
 * insert, look up), remapping + duplicates, survivors (count, scan, write), ordering (two sorts, emit) -- by timed events
 * on the call's stream; a phase a call did not reach reads 0.  capacity >= SMX_DECIMATE_PHASES.  Zeros before the first call. */
#define SMX_DECIMATE_PHASES 4
int smx_recon_debug_decimate_timings(smx_recon r, float* out_ms, int32_t capacity);

/* ---- the connected pieces of a triangle array: label them, measure them, drop the small ones ----
 * A pure function of the map as it stands (smooth position rows 3-5, RadiusSquared row 7, slots [0, n) with n =
 * surfels_size()), of triangles_in (uint32 [n_in][3], slot indices, in ANY order: the output of smx_recon_triangulate, of
 * smx_recon_decimate_mesh, or any other array over the map) and of p.  Every quantity is an integer or a float32 expression
 * evaluated as written, one rounding per operation, no contraction.
 * 1. Live and range, as smx_recon_decimate_mesh step 1: a triangle with a corner that is not live (!(RadiusSquared < 0) and a
 *    finite smooth position) is dropped and counted in n_not_live.  An index >= n anywhere in the input:
 *    SMX_ERR_INVALID_ARGUMENT, nothing is written.  U = the slots that occur in the remaining triangles.
 * 2. Components: the graph on U with an edge for every side of every remaining triangle; a component is a connected component
 *    of that graph.  This is connectivity through shared VERTICES: two triangles that touch in one corner only are one piece
 *    (a surfel is one point of the surface; an edge-connectivity rule would split a fan at its hub).  label(i) = the smallest
 *    slot index in i's component.  vertex_labels[i] = label(i) for i in U, 0xFFFFFFFF for every other slot.  A triangle
 *    belongs to the component of its corners.
 * 3. Measures of a component: n_vertices and n_triangles (integer counts); the box of its vertices' smooth positions, per
 *    coordinate the minimum and the maximum under the total order of k(f) = bits(f) ^ ((bits(f) >> 31) ? 0xFFFFFFFF :
 *    0x80000000), so -0 < +0 and the stored bytes are those of the winning input.  d_k = hi_k - lo_k, diag2 = (d_x d_x +
 *    d_y d_y) + d_z d_z.
 * 4. Kept: a component passes iff n_triangles >= min_triangles and diag2 >= min_diagonal * min_diagonal (one float32 product).
 *    With keep_largest = K > 0 the passing components are ranked by (n_triangles descending, label ascending) and the first K
 *    are kept; with K = 0 all that pass are.
 * 5. Output: triangles_out = the subsequence of triangles_in whose component is kept, input order and each triangle's three
 *    words unchanged (so an array in smx_recon_triangulate's order stays in it).  The table holds every component, kept or
 *    not, ascending by label.  Two calls give the same bytes in all three outputs.
 * 6. Not done: no hole is filled, no edge is made manifold, non-manifold edges are not reported.
 * Calling rules as smx_recon_decimate_mesh: ordered after everything enqueued on the object, synchronous.  on_device says
 * where triangles_in, triangles_out, vertex_labels and components live (host arrays are staged).  capacity < T_out, or
 * components != NULL and component_capacity < n_components: SMX_ERR_INVALID_ARGUMENT, *n_triangles = T_out and *n_components
 * are both reported, nothing is written to any output; triangles_out == NULL with capacity 0 is that count-only form.
 * n_in == 0 is valid.  min_diagonal must be finite and >= 0.  triangles_out must not overlap triangles_in (refused).
 * vertex_labels may be NULL, else it has surfels_size() entries; components may be NULL (component_capacity is then ignored).
 * stats may be NULL; it is filled whenever the counts are known.  Changes no map state, delta mark, statistic or stamp, nor
 * the state smx_recon_triangulate_update keeps.  The workspace belongs to the object, grows on demand and is reused. */
typedef struct {
  uint32_t min_triangles;   /* keep a component only if it has at least this many triangles; 0 = no test */
  float    min_diagonal;    /* ... and its bounding-box diagonal is at least this long (map units); 0 = no test */
  uint32_t keep_largest;    /* of the components that pass, keep only this many largest; 0 = all */
} smx_components_params;
typedef struct {            /* 40 bytes, one per component, table ascending by label */
  uint32_t label;           /* smallest slot index in the component */
  uint32_t n_vertices, n_triangles;
  uint32_t kept;            /* 0 / 1 */
  float    lo[3], hi[3];    /* bounding box of the smooth positions */
} smx_mesh_component;
typedef struct {
  uint32_t n_in;                /* triangles given */
  uint32_t n_not_live;          /* of those, dropped because a corner is not live */
  uint32_t n_used_vertices;     /* |U| */
  uint32_t n_components;
  uint32_t n_kept_components;
  uint32_t n_largest_triangles; /* triangle count of the largest component, kept or not; 0 if there is none */
  uint32_t n_triangles;         /* T_out */
} smx_components_stats;
int smx_components_params_default(smx_components_params* out);   /* 0, 0.0f, 0: labels only, everything kept */
int smx_recon_mesh_components(smx_recon r, smx_stream s, const smx_components_params* p,
                              const uint32_t* triangles_in, uint32_t n_in,
                              uint32_t* triangles_out, uint32_t capacity,
                              uint32_t* vertex_labels /* may be NULL; surfels_size() entries */,
                              smx_mesh_component* components /* may be NULL */, uint32_t component_capacity,
                              int32_t on_device, uint32_t* n_triangles, uint32_t* n_components,
                              smx_components_stats* stats);
/* Tools: milliseconds the last smx_recon_mesh_components call spent in its SMX_COMPONENTS_PHASES phases -- mark + link,
 * flatten + number, measure (+ rank), write (count, scan, triangles, labels, table) -- by timed events on the call's
 * stream; a phase a call did not reach reads 0.  capacity >= SMX_COMPONENTS_PHASES.  Zeros before the first call. */
#define SMX_COMPONENTS_PHASES 4
int smx_recon_debug_components_timings(smx_recon r, float* out_ms, int32_t capacity);

/* ---- small holes of a triangle array closed by fans, and the report of its edges ----
 * A pure function of the map as it stands (smooth position rows 3-5, RadiusSquared row 7, normal rows 8-10, slots [0, n) with
 * n = surfels_size()), of triangles_in (uint32 [n_in][3], slot indices, in ANY order) and of p.  Every quantity is an integer or
 * a float32 expression evaluated as written, one rounding per operation, no contraction; division and square root are
 * correctly rounded.
 * 1. Live and range, as smx_recon_decimate_mesh and smx_recon_mesh_components step 1: a triangle with a corner that is not live
 *    (!(RadiusSquared < 0) and a finite smooth position) is dropped and counted in n_not_live.  An index >= n anywhere in the
 *    input: SMX_ERR_INVALID_ARGUMENT, nothing is written.  The surviving triangles are R.
 * 2. Half-edges: triangle (p, a, b) of R has the half-edges p->a, a->b and b->p.  For an unordered pair {u, v}, f = the number
 *    of triangles of R with the half-edge min->max, g = the number with max->min (a half-edge u->u of a triangle with a repeated
 *    corner counts in f).  The pair is INTERIOR iff f = g = 1, BOUNDARY iff f + g = 1, and NON-MANIFOLD otherwise (three or
 *    more triangles, or two in the same direction): counted in n_nonmanifold_edges and never boundary.  n_edges = the pairs with
 *    f + g > 0.  Every boundary half-edge u->v defines the GAP v->u, the half-edge a filling triangle has to supply.
 * 3. Simple vertices and loops: out(w) = the gaps that leave w, in(w) = the gaps that enter it.  w is SIMPLE iff out(w) = in(w)
 *    = 1, and then next(w) is the head of its one outgoing gap.  Every other vertex with out + in > 0 is counted in
 *    n_pinched_vertices (two holes touch there, or a non-manifold fan does).  A LOOP of length L is a cycle w_0 -> next(w_0) =
 *    w_1 -> ... -> w_{L-1} -> w_0 of simple vertices; w_0 is its smallest slot, the loop's label.  The loops with 3 <= L <=
 *    max_hole_edges are LISTED.  Longer loops (the outer rim of a sheet is one) and chains that run into a vertex that is not
 *    simple are left alone; they appear in n_boundary_edges only.
 * 4. The fill of a listed loop is a fan from the best apex.  With pos = the smooth positions, d = pos[other] - pos[w_i] and
 *    d2 = (d_x d_x + d_y d_y) + d_z d_z: cost(i) = sum over k = 2 .. L-2, in this order, accumulated from 0.0f, of d2(w_i,
 *    w_{(i+k) mod L}).  The apex is the i with the smallest (float_bits(cost(i)) << 32) | w_i (for L = 3 every cost is 0 and
 *    the apex is the label).  Fan triangles: (w_i, w_{(i+k) mod L}, w_{(i+k+1) mod L}) for k = 1 .. L-2.  A loop is filled whole
 *    or not at all; its status is the first of these that applies:
 *      SMX_HOLE_DIAGONAL  a fan diagonal {w_i, w_{(i+k) mod L}}, 2 <= k <= L-2, is a pair of R with f + g > 0 already (so an
 *                         input whose pairs are all interior or boundary stays that way);
 *      SMX_HOLE_FILTER    some fan triangle (P, A, B), in the order above, does not get the value 1 from the triangle filter of
 *                         smx_recon_triangulate (interior angles within [min_triangle_angle_deg, max_triangle_angle_deg] by
 *                         their float32 cosines, the limits' cosines formed as (float)cos((double)deg * pi / 180); the
 *                         triangle's normal (A - P) x (B - P) agreeing in sign with the sum of the three corner normals and
 *                         with each of them).  "The other winding" is a rejection: that refuses the outer boundary of an
 *                         island and the back of an isolated triangle;
 *      SMX_HOLE_FILLED    otherwise: its L - 2 fan triangles are the loop's new triangles.
 * 5. Output: triangles_out = R in input order, every word unchanged, then the new triangles, each rotated so that its smallest
 *    index is first (winding kept), ascending by (p, a, b).  *n_kept = |R| is the split point, *n_triangles = T_out = |R| +
 *    n_new_triangles.  holes (optional) gets one row per listed loop, filled or not, ascending by label; *n_holes = their
 *    number.  Two calls give the same bytes in both outputs.
 * 6. Consequences: the vertices of different loops are disjoint.  If every pair of the input is interior or boundary, so is
 *    every pair of the output.  Each filled loop removes exactly L boundary edges.  A second call on the output fills nothing
 *    and returns its input.  A hole made by deleting one interior triangle of a triangulation comes back as that triangle.
 * 7. Not done: holes that touch in a vertex; holes longer than max_hole_edges; any triangulation better than a fan; no vertex
 *    is ever made.  The array as a whole is not in (p, a, b) order: a caller who needs that passes it through
 *    smx_recon_decimate_mesh or sorts it.
 * Parameters: 3 <= max_hole_edges <= SMX_FILL_MAX_HOLE_EDGES; the angles finite with 0 <= min < max <= 180; n_in <= 2^28.
 * Anything else: SMX_ERR_INVALID_ARGUMENT with nothing launched.
 * Calling rules as smx_recon_mesh_components: ordered after everything enqueued on the object, synchronous.  on_device says where
 * triangles_in, triangles_out and holes live (host arrays are staged).  capacity < T_out, or holes != NULL and hole_capacity <
 * n_listed_loops: SMX_ERR_INVALID_ARGUMENT, *n_triangles, *n_kept and *n_holes are all reported, nothing is written to any
 * output; triangles_out == NULL with capacity 0 is that count-only form.  n_in == 0 is valid.  triangles_out must not overlap
 * triangles_in (refused).  holes may be NULL (hole_capacity is then ignored).  stats may be NULL; it is filled whenever the
 * counts are known.  Changes no map state, delta mark, statistic or stamp, nor the state smx_recon_triangulate_update keeps.
 * The workspace belongs to the object, grows on demand and is reused. */
#define SMX_FILL_MAX_HOLE_EDGES 32
enum { SMX_HOLE_FILLED = 1, SMX_HOLE_DIAGONAL = 2, SMX_HOLE_FILTER = 3 };
typedef struct {
  uint32_t max_hole_edges;          /* loops of 3 .. this many edges are listed */
  float    min_triangle_angle_deg;  /* the triangle filter's limits, as in smx_mesh_params */
  float    max_triangle_angle_deg;
} smx_fill_params;
typedef struct {            /* 12 bytes, one per listed loop, table ascending by label */
  uint32_t label;           /* smallest slot index on the loop */
  uint32_t n_edges;         /* L */
  uint32_t status;          /* SMX_HOLE_* */
} smx_mesh_hole;
typedef struct {
  uint32_t n_in;                /* triangles given */
  uint32_t n_not_live;          /* of those, dropped because a corner is not live */
  uint32_t n_edges;             /* unordered pairs with f + g > 0 */
  uint32_t n_boundary_edges;    /* of those, with f + g = 1 (before the fill) */
  uint32_t n_nonmanifold_edges; /* neither interior nor boundary */
  uint32_t n_pinched_vertices;  /* out + in > 0 and not simple */
  uint32_t n_listed_loops;
  uint32_t n_filled_loops;
  uint32_t n_rejected_diagonal;
  uint32_t n_rejected_filter;
  uint32_t n_new_triangles;
  uint32_t n_triangles;         /* T_out */
} smx_fill_stats;
int smx_fill_params_default(smx_fill_params* out);   /* 8, 10.0f, 170.0f */
int smx_recon_fill_holes(smx_recon r, smx_stream s, const smx_fill_params* p,
                         const uint32_t* triangles_in, uint32_t n_in,
                         uint32_t* triangles_out, uint32_t capacity,
                         smx_mesh_hole* holes /* may be NULL */, uint32_t hole_capacity,
                         int32_t on_device, uint32_t* n_triangles, uint32_t* n_kept, uint32_t* n_holes,
                         smx_fill_stats* stats);
/* Tools: milliseconds the last smx_recon_fill_holes call spent in its SMX_FILL_PHASES phases -- edges (mark, insert,
 * classify), loops (walk, scan, list), fill (apex, tests, the new run's order), write (R, the new run, the table) -- by timed
 * events on the call's stream; a phase a call did not reach reads 0.  capacity >= SMX_FILL_PHASES.  Zeros before the first call. */
#define SMX_FILL_PHASES 4
int smx_recon_debug_fill_timings(smx_recon r, float* out_ms, int32_t capacity);

/* ---- the distance from points to a triangle array: closest triangle, distance, closest point ----
 * A pure function of the map as it stands (smooth position rows 3-5, RadiusSquared row 7, slots [0, n) with n =
 * surfels_size()), of `triangles` (uint32 [n_in][3], slot indices, in ANY order), of `points` (float [n_points][3]) and of p.
 * Every quantity is an integer or a float32 expression evaluated as written, one rounding per operation, no contraction; division
 * and square root are correctly rounded.  Throughout dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z, and cross(u, v) = (u_y v_z -
 * u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x).  A scalar times a vector is three products, a sum of vectors three sums.
 * 1. Live, range and shape.  An index >= n anywhere in `triangles`: SMX_ERR_INVALID_ARGUMENT, nothing is written.  A triangle
 *    with a corner that is not live (!(RadiusSquared < 0) and a finite smooth position, as smx_recon_decimate_mesh step 1) is
 *    dropped and counted in n_not_live; of the rest, one with a repeated index is dropped and counted in n_repeated; of the rest,
 *    one with a corner coordinate of magnitude > SMX_DIST_MAX_COORD is dropped and counted in n_out_of_range.  The survivors are
 *    R; each keeps t, its position in the input.
 * 2. Points.  A point with a non-finite coordinate or one of magnitude > SMX_DIST_MAX_COORD is BAD, counted in n_bad_points,
 *    and its outputs are those of "none" below.
 * 3. The closest point Q of P on (A, B, C), the corners of a triangle of R in input order: Ericson's regions in this order,
 *    first match wins:
 *      ab = B-A; ac = C-A; ap = P-A;  d1 = dot(ab,ap); d2 = dot(ac,ap)
 *      if d1 <= 0 and d2 <= 0:                 Q = A
 *      bp = P-B; d3 = dot(ab,bp); d4 = dot(ac,bp)
 *      if d3 >= 0 and d4 <= d3:                Q = B
 *      vc = d1*d4 - d3*d2
 *      if vc <= 0 and d1 >= 0 and d3 <= 0:     v = d1/(d1-d3);  Q = A + v*ab
 *      cp = P-C; d5 = dot(ab,cp); d6 = dot(ac,cp)
 *      if d6 >= 0 and d5 <= d6:                Q = C
 *      vb = d5*d2 - d1*d6
 *      if vb <= 0 and d2 >= 0 and d6 <= 0:     w = d2/(d2-d6);  Q = A + w*ac
 *      va = d3*d6 - d5*d4
 *      if va <= 0 and (d4-d3) >= 0 and (d5-d6) >= 0:
 *                                              w = (d4-d3)/((d4-d3)+(d5-d6));  Q = B + w*(C-B)
 *      else: s = (va+vb)+vc; v = vb/s; w = vc/s
 *            v = v < 0 ? 0 : (v > 1 ? 1 : v);  lim = 1 - v;  w = w < 0 ? 0 : (w > lim ? lim : w)
 *            Q = (A + v*ab) + w*ac
 *      e = P-Q;  dist2 = dot(e,e)
 *    (Exact arithmetic reaches the last branch only with va, vb, vc > 0; float32 may not, so v and w are held to the triangle:
 *    Q then lies in the hull of A, B, C in every branch, which is what lets a grid find every candidate.  The comparisons keep a
 *    NaN a NaN.)
 *    The triangle is a CANDIDATE for P iff dist2 <= max_distance*max_distance (one float32 product).  A NaN dist2 (coincident
 *    or collinear corners) therefore never is.
 * 4. The answer for P: the candidate with the smallest key (float_bits(dist2) << 32) | t -- the distance decides, then the
 *    smallest input position.  nearest = t, distance = sqrt(dist2), closest = Q.  With signed_distance, distance is negated iff
 *    dot(e, cross(ab, ac)) < 0.  With no candidate, or for a BAD point: nearest = 0xFFFFFFFF, distance = +infinity, closest =
 *    (NaN, NaN, NaN).  The answer is the minimum over ALL of R: it does not depend on cell_size, on the search structure or on
 *    the schedule.  Two calls give the same bytes.
 * 5. smx_distance_stats: the counts of steps 1 and 2; n_matched = the points with a candidate; max_dist2_bits = the largest
 *    matched dist2 as its bits (0 if none); histogram: a matched point counts in bin min(31, (uint32)((|distance| * 32.0f) /
 *    max_distance)).  n_wide, n_entries, n_cells describe the search structure: a uniform grid with c = max(cell_size, 1.125f *
 *    max_distance), the cell of a coordinate x is (int32)floorf(x / c), a triangle of R is entered in every cell of the box
 *    from the cell of its per-axis minimum to the cell of its per-axis maximum unless that box has more than
 *    SMX_DIST_WIDE_CELLS cells, in which case it goes on the wide list every query tests in full.  n_entries = the (cell,
 *    triangle) entries, n_cells = the occupied cells.  With cell_size == 0 the library takes max(1.125f * max_distance, the mean
 *    over R of the largest of the three extents of a triangle's box) for c; these three and cell_size_used are defined exactly
 *    only when cell_size > 0 is given.
 * 6. Not done: no BVH; no distance to an analytic surface.  (The distance between two meshes, both ways in one call, is
 *    smx_recon_compare_meshes below, on the samples of smx_recon_sample_mesh.)
 * Parameters: max_distance finite with 1e-3f <= max_distance <= 16.0f; cell_size 0 or finite and > 0; signed_distance 0 or 1;
 * n_in <= 2^28 and n_points <= 2^28.  Anything else: SMX_ERR_INVALID_ARGUMENT with nothing launched.  A cell_size so far below
 * the triangles' size that the grid would hold more than 2^30 entries is refused after the mark phase, nothing written.
 * Calling rules as smx_recon_mesh_components: ordered after everything enqueued on the object, synchronous.  on_device says where
 * triangles, points, nearest, distance and closest live (host arrays are staged).  n_in == 0 is valid (every point is "none"),
 * and so is n_points == 0.  closest may be NULL.  The outputs must not overlap the inputs (refused).  stats may be NULL.
 * Changes no map state, delta mark, statistic or stamp, nor the state smx_recon_triangulate_update keeps.  The workspace
 * belongs to the object, grows on demand, is reused and is freed with the object. */
#define SMX_DIST_MAX_COORD 64.0f
#define SMX_DIST_WIDE_CELLS 64
#define SMX_DIST_BINS 32
typedef struct {
  float   max_distance;      /* triangles farther than this are no candidates */
  float   cell_size;         /* 0: the library chooses */
  int32_t signed_distance;   /* 0 / 1 */
} smx_distance_params;
typedef struct {
  uint32_t n_in;                      /* triangles given */
  uint32_t n_not_live;                /* of those, dropped because a corner is not live */
  uint32_t n_repeated;                /* of the rest, with a repeated index */
  uint32_t n_out_of_range;            /* of the rest, with a coordinate beyond SMX_DIST_MAX_COORD */
  uint32_t n_points;
  uint32_t n_bad_points;
  uint32_t n_matched;
  uint32_t max_dist2_bits;
  uint32_t histogram[SMX_DIST_BINS];
  uint32_t n_wide, n_entries, n_cells;
  float    cell_size_used;
} smx_distance_stats;
int smx_distance_params_default(smx_distance_params* out);   /* 0.05f, 0.0f, 0 */
int smx_recon_mesh_distance(smx_recon r, smx_stream s, const smx_distance_params* p,
                            const uint32_t* triangles, uint32_t n_in,
                            const float* points /* [n_points][3] */, uint32_t n_points,
                            uint32_t* nearest /* [n_points] */, float* distance /* [n_points] */,
                            float* closest /* [n_points][3], may be NULL */,
                            int32_t on_device, smx_distance_stats* stats /* may be NULL */);
/* Tools: milliseconds the last smx_recon_mesh_distance call spent in its SMX_DIST_PHASES phases -- mark (classes, c, boxes,
 * the wide list, scan), index (entries, sort, records, cell table), query (the points' sort, the walk), stats -- by timed events
 * on the call's stream; a phase a call did not reach reads 0.  capacity >= SMX_DIST_PHASES.  Zeros before the first call. */
#define SMX_DIST_PHASES 4
int smx_recon_debug_distance_timings(smx_recon r, float* out_ms, int32_t capacity);

/* ---- points on a triangle array in proportion to area, and the distance between two triangle arrays ----
 * smx_recon_sample_mesh is a pure function of the map as it stands (smooth position rows 3-5, RadiusSquared row 7, slots [0, n)
 * with n = surfels_size()), of `triangles` (uint32 [n_in][3], slot indices, in ANY order), of n_samples and of seed.  Every
 * quantity is an integer or a float32 expression evaluated as written, one rounding per operation, no contraction; sqrtf and
 * division are correctly rounded; dot and cross as in smx_recon_mesh_distance above.
 * 1. Triangles.  R and the counts n_not_live, n_repeated and n_out_of_range exactly as smx_recon_mesh_distance step 1; an
 *    index >= n anywhere in `triangles`: SMX_ERR_INVALID_ARGUMENT, nothing is written.  Each triangle of R keeps t, its position
 *    in the input, and its corners A, B, C in input order.
 * 2. Weight.  ab = B-A; ac = C-A; N = cross(ab, ac); a = sqrtf(dot(N, N)) (twice the area);
 *    q_t = a > 0 ? (uint64)(a * 1073741824.0f) : 0 -- the product by 2^30 is exact, the conversion truncates, the unit is
 *    2^-30 m^2, and with the corners within SMX_DIST_MAX_COORD q_t < 2^46.  A triangle outside R has q_t = 0.  n_zero_weight
 *    counts the triangles of R with q_t == 0.
 * 3. Prefix and total.  C_t = sat(sum of q_t' over t' < t) in input order, W = sat(sum over all t), sat(x) = min(x, 2^62).
 *    (min(2^62, a + b) is associative on [0, 2^62], so a parallel scan gives exactly this.)  W == 2^62:
 *    SMX_ERR_INVALID_ARGUMENT ("total area too large") after the weights phase, nothing is written.
 * 4. Random words.  mix(x) on uint32, every operation wrapping: x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B;
 *    x ^= x >> 16.  r_j(k) = mix(mix(3k + j) ^ seed) for j = 0, 1, 2.
 * 5. Strata.  S = W / n_samples (integer division).  If W < n_samples every sample is "none" (so with W == 0 or an empty R).
 *    Otherwise u_k = k*S + floor(S * r_0(k) / 2^32), all of it in integers: the high 64 bits of S * (r_0 << 32), or
 *    (S >> 32) * r_0 + (((S & 0xFFFFFFFF) * r_0) >> 32).  So k*S <= u_k < (k+1)*S <= W: sample k is drawn from stratum k of the
 *    total weight.  The last W - n_samples*S units (fewer than n_samples of 2^-30 m^2) are never drawn.
 * 6. Triangle.  t is the triangle with C_t <= u_k < C_t + q_t.  It exists, has q_t > 0 and does not decrease with k: the
 *    output is in the order of the input triangles.
 * 7. Point.  v = (float)(r_1 >> 8) * 2^-24; w = (float)(r_2 >> 8) * 2^-24; if v + w > 1.0f: v = 1.0f - v; w = 1.0f - w (both
 *    exact).  P = (A + v*ab) + w*ac, the interior expression of smx_recon_mesh_distance.  Normal: (N_x / a, N_y / a, N_z / a).
 * 8. Outputs: points [n_samples][3], tri [n_samples] = t, bary [n_samples][2] = (v, w) (may be NULL), normals [n_samples][3]
 *    (may be NULL).  A "none" sample has tri = 0xFFFFFFFF and NaN everywhere else.
 * 9. smx_sample_stats: the counts of steps 1 and 2; n_samples; n_none; total_weight = W and stride = S; n_triangles_hit = the
 *    samples that are not "none" whose tri differs from the sample's before (the first one counts).
 * Not done: no colours interpolated onto the samples; no blue-noise or Poisson-disc spacing.
 * Parameters: n_in <= 2^28 and n_samples <= 2^28, anything else SMX_ERR_INVALID_ARGUMENT with nothing launched; n_in == 0 and
 * n_samples == 0 are valid.  Calling rules as smx_recon_mesh_distance: ordered after everything enqueued on the object,
 * synchronous.  on_device says where triangles, points, tri, bary and normals live (host arrays are staged).  An output that
 * overlaps `triangles` is refused.  Every allocation of the call lies before the first write to an output.  stats may be NULL.
 * Changes no map state, delta mark, statistic or stamp, nor the state smx_recon_triangulate_update keeps.  Two calls give the
 * same bytes.  The workspace belongs to the object, grows on demand, is reused and is freed with the object. */
typedef struct {
  uint32_t n_in;                      /* triangles given */
  uint32_t n_not_live;                /* of those, dropped because a corner is not live */
  uint32_t n_repeated;                /* of the rest, with a repeated index */
  uint32_t n_out_of_range;            /* of the rest, with a coordinate beyond SMX_DIST_MAX_COORD */
  uint32_t n_zero_weight;             /* of R, with q_t == 0 */
  uint32_t n_samples;
  uint32_t n_none;
  uint32_t n_triangles_hit;
  uint64_t total_weight;              /* W, in units of 2^-30 m^2 (twice the area) */
  uint64_t stride;                    /* S */
} smx_sample_stats;
int smx_recon_sample_mesh(smx_recon r, smx_stream s, const uint32_t* triangles, uint32_t n_in, uint32_t n_samples, uint32_t seed,
                          float* points /* [n_samples][3] */, uint32_t* tri /* [n_samples] */,
                          float* bary /* [n_samples][2], may be NULL */, float* normals /* [n_samples][3], may be NULL */,
                          int32_t on_device, smx_sample_stats* stats /* may be NULL */);
/* Tools: milliseconds the last smx_recon_sample_mesh call spent in its SMX_SAMPLE_PHASES phases -- weights (classes, q_t, the
 * sums inside a block), scan (the blocks' prefix, W, the read-back), draw -- by timed events on the call's stream; a phase a call
 * did not reach reads 0 (a refused call publishes the weights only).  capacity >= SMX_SAMPLE_PHASES.  Zeros before the first call. */
#define SMX_SAMPLE_PHASES 3
int smx_recon_debug_sample_timings(smx_recon r, float* out_ms, int32_t capacity);

/* smx_recon_compare_meshes: both one-sided surface distances between two triangle arrays A and B over the map, in one call.
 * Side A->B is BY DEFINITION smx_recon_sample_mesh(A, n_samples, seed) followed by smx_recon_mesh_distance(B, those points,
 * max_distance, cell_size, unsigned); a "none" sample is a NaN point, so the distance's n_bad_points counts it.  Side B->A swaps
 * the roles of A and B and uses the same seed.  Per side `out` holds the smx_sample_stats, the smx_distance_stats and three
 * exact sums over the matched samples: with d_q = (uint32)(distance * 1048576.0f) (at most 2^24, the unit is 2^-20 m) sum_d =
 * the uint64 sum of d_q, sum_sq_lo and sum_sq_hi = the uint64 sums of (d_q*d_q) & 0xFFFFFFFF and of (d_q*d_q) >> 32; no word
 * can overflow at 2^28 samples, and the sum of the squares is sum_sq_hi * 2^32 + sum_sq_lo.  directions: 1 = A->B only, 2 =
 * B->A only, 3 = both; a side not asked for is all zeros.  The samples stay in the call's workspace: nothing per sample crosses
 * to the host.  The parameter limits are those of the two calls it is made of (and directions 1 .. 3); a refusal by either half
 * is the call's refusal, and `out` is zeroed.  The two halves run as the calls themselves do -- each side builds the grid of
 * the mesh it measures against anew -- and publish their own timings (smx_recon_debug_sample_timings, _distance_timings: those
 * of the last side).  Calling rules as smx_recon_sample_mesh; on_device says where both triangle arrays live.
 * This call keeps no index, so each side rebuilds the grid; one side against a kept index is smx_recon_compare_to_distscene
 * below.  Not done: no distance to an analytic surface. */
typedef struct {
  float    max_distance;     /* as smx_distance_params */
  float    cell_size;        /* 0: the library chooses */
  uint32_t n_samples;        /* per side */
  uint32_t seed;
  int32_t  directions;       /* 1: A->B, 2: B->A, 3: both */
} smx_compare_params;
typedef struct {
  smx_sample_stats   sample;
  smx_distance_stats distance;
  uint64_t sum_d, sum_sq_lo, sum_sq_hi;
} smx_compare_side;
typedef struct {
  smx_compare_side a_to_b, b_to_a;
} smx_compare_stats;
int smx_recon_compare_meshes(smx_recon r, smx_stream s, const smx_compare_params* p,
                             const uint32_t* triangles_a, uint32_t n_a, const uint32_t* triangles_b, uint32_t n_b,
                             int32_t on_device, smx_compare_stats* out);
/* Tools: milliseconds the last smx_recon_compare_meshes call spent in its SMX_COMPARE_PHASES phases -- sample, distance, sums
 * of side A->B, then of side B->A -- by timed events on the call's stream; a side not asked for reads 0.  capacity >=
 * SMX_COMPARE_PHASES.  Zeros before the first call. */
#define SMX_COMPARE_PHASES 6
int smx_recon_debug_compare_timings(smx_recon r, float* out_ms, int32_t capacity);

/* ---- rays against a triangle array: the first triangle hit, the ray parameter, the barycentrics ----
 * A pure function of the map as it stands (smooth position rows 3-5, RadiusSquared row 7, slots [0, n) with n =
 * surfels_size()), of `triangles` (uint32 [n_in][3], slot indices, in ANY order), of `rays` (float [n_rays][6]: the origin O,
 * then the direction D) and of p.  Every quantity is an integer or a float32 expression evaluated as written, one rounding per
 * operation, no contraction; division is correctly rounded; dot and cross as in smx_recon_mesh_distance above.
 * 1. Triangles.  R and the counts n_not_live, n_repeated and n_out_of_range exactly as smx_recon_mesh_distance step 1; an
 *    index >= n anywhere in `triangles`: SMX_ERR_INVALID_ARGUMENT, nothing is written.  Each triangle of R keeps i, its
 *    position in the input, and its corners A, B, C in input order.
 * 2. Rays.  D is not normalised: t is in units of |D|, so the segment from P to Q is O = P, D = Q - P, t_max = 1.  A ray is
 *    BAD if a coordinate of O or D is not finite, if |O_k| > SMX_DIST_MAX_COORD, if |D_k| > SMX_RAY_MAX_DIR for some k, or if
 *    max_k |D_k| < SMX_RAY_MIN_DIR.  A BAD ray is counted in n_bad_rays and its outputs are those of "none" below.
 * 3. Candidate.  For the ray (O, D) and the triangle (A, B, C) of R:
 *      e1 = B-A; e2 = C-A; p = cross(D, e2); det = dot(e1, p)
 *      not a candidate unless det > 0 or det < 0        (a NaN or zero det never is)
 *      cull == 1: only det > 0  (front: smx_recon_triangulate's winding seen from its normal side);  cull == 2: only det < 0
 *      inv = 1.0f / det; s = O-A; u = dot(s, p) * inv; q = cross(s, e1); v = dot(D, q) * inv
 *      w = u + v; t = dot(e2, q) * inv
 *      candidate iff u >= 0 and v >= 0 and w <= 1 and t >= t_min and t <= t_max and, for each axis k,
 *        H_k = O_k + t * D_k   (a product, then a sum)
 *        min3(A_k, B_k, C_k) - SMX_RAY_BOX_SLACK <= H_k <= max3(A_k, B_k, C_k) + SMX_RAY_BOX_SLACK
 *    with min3(a, b, c) = (m = a < b ? a : b; m < c ? m : c) and max3 alike.  The last condition is part of the definition on
 *    purpose, like the clamp of v and w in smx_recon_mesh_distance: float32 Moeller-Trumbore on a sliver can place a "hit"
 *    anywhere along the ray; such a hit is none, and that is what lets a grid find every candidate.
 * 4. The answer for a ray: the candidate with the smallest key (float_bits(t + 0.0f) << 32) | i -- the nearest, then the
 *    smallest input position.  hit = i, t = t + 0.0f, uv = (u, v).  With no candidate, or for a BAD ray: hit = 0xFFFFFFFF,
 *    t = +infinity, uv = (NaN, NaN).  The answer is the minimum over ALL of R: it does not depend on cell_size, on the search
 *    structure or on the schedule.  Two calls give the same bytes.
 * 5. smx_raycast_stats: the counts of steps 1 and 2; n_hit = the rays with a candidate, n_front_hits = those whose winner has
 *    det > 0; max_t_bits = the largest winning t as its bits (0 if none).  n_wide, n_entries, n_cells describe the search
 *    structure: a uniform grid with c = max(cell_size, SMX_RAY_MIN_CELL); the cell of a coordinate x is (int32)floorf(x / c); a
 *    triangle of R is entered in every cell from the cell of min3 - SMX_RAY_BOX_SLACK to the cell of max3 +
 *    SMX_RAY_BOX_SLACK per axis (the expressions of step 3; the cell function is monotone, so the cell of H of any candidate is
 *    one of them) unless that box has more than SMX_DIST_WIDE_CELLS cells, in which case it goes on the wide list every ray
 *    tests in full.  With cell_size == 0 the library takes max(SMX_RAY_MIN_CELL, the mean over R of the largest of the three
 *    extents of a triangle's box) for c; these three and cell_size_used are defined exactly only when cell_size > 0 is given.
 *    n_layers, n_lookups, n_pair_tests say what the traversal did (layers of the dominant axis walked, cell look-ups, ray-
 *    triangle tests); they are sums of per-wavefront counts, equal between two calls with the same inputs, and defined by the
 *    implementation only.
 * 6. Not done: not watertight -- a ray aimed exactly at a shared edge or vertex may slip between two triangles, or hit the
 *    later one; no index is kept between calls; no ray packets; no BVH.
 * Parameters: t_min and t_max finite with 0 <= t_min <= t_max <= SMX_RAY_MAX_T; cell_size 0 or finite and > 0; cull 0, 1 or 2;
 * n_in <= 2^28 and n_rays <= 2^28.  Anything else: SMX_ERR_INVALID_ARGUMENT with nothing launched.  A cell_size so far below
 * the triangles' size that the grid would hold more than 2^30 entries is refused after the mark phase, nothing written.
 * Calling rules as smx_recon_mesh_distance: ordered after everything enqueued on the object, synchronous.  on_device says where
 * triangles, rays, hit, t and uv live (host arrays are staged).  n_in == 0 is valid (every ray is "none"), and so is
 * n_rays == 0.  uv may be NULL.  The outputs must not overlap the inputs (refused).  stats may be NULL.  Every allocation
 * happens before the first write to an output.  Changes no map state, delta mark, statistic or stamp, nor the state
 * smx_recon_triangulate_update keeps.  The workspace belongs to the object, grows on demand, is reused and is freed with the
 * object. */
#define SMX_RAY_MAX_DIR 1024.0f
#define SMX_RAY_MIN_DIR 0.0009765625f      /* 2^-10 */
#define SMX_RAY_MAX_T 1048576.0f           /* 2^20 */
#define SMX_RAY_BOX_SLACK 0.000244140625f  /* 2^-12 m */
#define SMX_RAY_MIN_CELL 0.001953125f      /* 2^-9 m */
typedef struct {
  float   t_min, t_max;      /* candidates have t_min <= t <= t_max */
  float   cell_size;         /* 0: the library chooses */
  int32_t cull;              /* 0: both sides, 1: front faces only (det > 0), 2: back faces only */
} smx_raycast_params;
typedef struct {
  uint32_t n_in;                      /* triangles given */
  uint32_t n_not_live;                /* of those, dropped because a corner is not live */
  uint32_t n_repeated;                /* of the rest, with a repeated index */
  uint32_t n_out_of_range;            /* of the rest, with a coordinate beyond SMX_DIST_MAX_COORD */
  uint32_t n_rays;
  uint32_t n_bad_rays;
  uint32_t n_hit;
  uint32_t n_front_hits;
  uint32_t max_t_bits;
  uint32_t n_wide, n_entries, n_cells;
  float    cell_size_used;
  uint32_t reserved;
  uint64_t n_layers, n_lookups, n_pair_tests;
} smx_raycast_stats;
int smx_raycast_params_default(smx_raycast_params* out);   /* 0.0f, SMX_RAY_MAX_T, 0.0f, 0 */
int smx_recon_raycast_mesh(smx_recon r, smx_stream s, const smx_raycast_params* p,
                           const uint32_t* triangles, uint32_t n_in,
                           const float* rays /* [n_rays][6] */, uint32_t n_rays,
                           uint32_t* hit /* [n_rays] */, float* t /* [n_rays] */,
                           float* uv /* [n_rays][2], may be NULL */,
                           int32_t on_device, smx_raycast_stats* stats /* may be NULL */);
/* Tools: milliseconds the last smx_recon_raycast_mesh call spent in its SMX_RAY_PHASES phases -- mark (classes, c, boxes, the
 * wide list, the occupied box, scan), index (entries, sort, records, cell table), cast, stats -- by timed events on the call's
 * stream; a phase a call did not reach reads 0.  capacity >= SMX_RAY_PHASES.  Zeros before the first call. */
#define SMX_RAY_PHASES 4
int smx_recon_debug_raycast_timings(smx_recon r, float* out_ms, int32_t capacity);

/* ---- a ray-casting scene: the search structure of smx_recon_raycast_mesh built once, cast against many times ----
 * smx_rayscene is a SNAPSHOT of a triangle array over the map together with its search structure.  After a build a cast reads
 * neither the map nor the caller's triangle array: its answer is what smx_recon_raycast_mesh gives on the map as it stood at
 * the build, with the same triangles and cell size, and stays so through later smx_recon_integrate, smx_recon_compact and
 * smx_recon_deform_by_creation_frame calls and after smx_recon_destroy of the object it was built from.  hit stays "position
 * in the array given at the build".  There is nothing that could go stale, hence no generation counter.
 * Build (smx_recon_build_rayscene).  Steps 1 and 5 of smx_recon_raycast_mesh unchanged: the classes, R, c, the inflated boxes,
 *    the wide list, the occupied cell box, the entries, the packed corner records in the sorted order, the cell table;
 *    smx_rayscene_stats holds step 1's counts and step 5's structure words with the same meaning.  Refused like that call: an
 *    index >= n, more than 2^30 entries, cell_size not 0 or finite and > 0, n_in > 2^28, triangles == NULL with n_in > 0; also
 *    occupancy outside -1 .. 7, and a scene and an object on different devices.  Ordered after everything enqueued on r,
 *    synchronous; changes in r only what smx_recon_raycast_mesh changes (its workspace holds the sort's buffers).  Building
 *    into a scene that holds a build replaces it.  A scene never built, or whose last build was refused or failed for any
 *    reason (an allocation included), is EMPTY: it holds no records, table or grid and refuses every cast.
 *    n_in == 0 is a valid build (every ray answers "none").
 * Occupancy bit grid.  It spans the occupied cell box [lo, hi] of the structure.  With k = occupancy - 1 a block is 2^k cells
 *    per axis: the block of cell x on an axis is (x - lo) >> k, an axis has ((hi - lo) >> k) + 1 blocks, the bit number of
 *    block (bx, by, bz) is (bz * nby + by) * nbx + bx in 64 bits, and a bit is set iff some cell of its block has an entry in
 *    the cell table.  At most 2^31 bits (256 MiB).  occupancy -1: no grid.  1 + k with 0 <= k <= 6: that block size; one that
 *    does not fit is refused after the mark phase and leaves the scene empty.  0: the library chooses -- the smallest k in
 *    0 .. 6 that fits, none if none fits or nothing was entered (DESIGN.md 5m has the measurement behind it); occupancy_log2
 *    of the stats says what was taken, -1 for none.  occupancy_bytes = the grid's size, n_blocks_set = its set bits (counted from
 *    the bits), device_bytes = the device memory the scene holds after the build (records, table, grid, counters).
 * Cast (smx_rayscene_cast).  p->cell_size must be 0; t_min, t_max, cull, BAD rays, the key, the outputs and the overlap rule
 *    are exactly those of smx_recon_raycast_mesh, and hit, t and uv are byte for byte what that call writes.  The traversal
 *    and its exit rule are that call's; the grid is a filter in front of the cell table's look-up and nothing else: a clear
 *    bit means "no run", a set bit goes on to the table.  smx_rayscene_cast_stats: n_layers and n_pair_tests equal that call's
 *    at the same c; without a grid n_bit_tests == 0 and n_lookups equals that call's; with one n_bit_tests equals that call's
 *    n_lookups and n_lookups counts only the table look-ups still made; n_lookup_misses = those that found no run (0 at
 *    k == 0), so n_lookups - n_lookup_misses does not depend on the occupancy setting.  Synchronous.  on_device says where
 *    rays, hit, t and uv live.  n_rays == 0 is valid; uv and stats may be NULL; rays must not overlap an output (refused).  A
 *    cast on an empty scene: SMX_ERR_INVALID_ARGUMENT.  A refused cast writes nothing; every allocation (ray staging, the
 *    per-ray keys and work words) happens before the first write to an output.  One caller thread per scene.  A cast does
 *    not touch r.
 * All scene memory is counted by smx_debug_live_allocations and reached by smx_debug_fail_allocation.
 * (The kept index of smx_recon_mesh_distance is smx_distscene below.)  Not done: incremental updates of a scene; ray packets; a BVH; watertightness; an
 * enqueue-only cast without host synchronisation. */
typedef struct smx_rayscene_s* smx_rayscene;
typedef struct {
  float   cell_size;         /* as smx_raycast_params.cell_size; 0: the library chooses */
  int32_t occupancy;         /* -1: no bit grid, 0: the library chooses, 1 + k: a bit per block of 2^k cells per axis (k <= 6) */
} smx_rayscene_params;
typedef struct {
  uint32_t n_in, n_not_live, n_repeated, n_out_of_range;   /* as smx_raycast_stats */
  uint32_t n_wide, n_entries, n_cells;
  float    cell_size_used;
  int32_t  occupancy_log2;            /* k of the grid built, -1: none */
  uint32_t n_blocks_set;              /* set bits of the grid */
  uint64_t occupancy_bytes;           /* the grid's size */
  uint64_t device_bytes;              /* device memory the scene holds after the build */
} smx_rayscene_stats;
typedef struct {
  uint32_t n_rays, n_bad_rays, n_hit, n_front_hits, max_t_bits, reserved;
  uint64_t n_layers, n_bit_tests, n_lookups, n_lookup_misses, n_pair_tests;
} smx_rayscene_cast_stats;
int smx_rayscene_create(int32_t device_id /* -1: the current device */, smx_rayscene* out);
int smx_rayscene_destroy(smx_rayscene sc);
int smx_rayscene_params_default(smx_rayscene_params* out);   /* 0.0f, 0 */
int smx_recon_build_rayscene(smx_recon r, smx_stream s, smx_rayscene sc, const smx_rayscene_params* p,
                             const uint32_t* triangles, uint32_t n_in, int32_t on_device,
                             smx_rayscene_stats* stats /* may be NULL */);
int smx_rayscene_cast(smx_rayscene sc, smx_stream s, const smx_raycast_params* p,
                      const float* rays /* [n_rays][6] */, uint32_t n_rays,
                      uint32_t* hit /* [n_rays] */, float* t /* [n_rays] */, float* uv /* [n_rays][2], may be NULL */,
                      int32_t on_device, smx_rayscene_cast_stats* stats /* may be NULL */);
/* Tools: milliseconds of the last build's phases mark, index, occupancy (grid clear, bits, their count), then of the last
 * cast's phases cast, stats, by timed events on the calls' streams; a phase not reached reads 0.  capacity >=
 * SMX_RAYSCENE_PHASES. */
#define SMX_RAYSCENE_PHASES 5
int smx_rayscene_debug_timings(smx_rayscene sc, float* out_ms, int32_t capacity);

/* ---- a distance scene: the search structure of smx_recon_mesh_distance built once, queried many times ----
 * smx_distscene is a SNAPSHOT of a triangle array over the map together with its search structure, for one distance bound.
 * After a build a query reads neither the map nor the caller's triangle array: its answer is what smx_recon_mesh_distance
 * gives on the map as it stood at the build, with the same triangles, and stays so through later smx_recon_integrate,
 * smx_recon_compact and smx_recon_deform_by_creation_frame calls, through a smx_recon_debug_upload_surfels that moves or kills
 * slots, and after smx_recon_destroy of the object it was built from.  nearest stays "position in the array given at the
 * build".  There is nothing that could go stale, hence no generation counter.
 * Build (smx_recon_build_distscene).  Steps 1 and 5 of smx_recon_mesh_distance unchanged: the classes, R, the exact boxes, the
 *    wide list, the entries, the packed corner records in the sorted order, the cell table, with c = max(cell_size, 1.125f *
 *    max_distance), or at cell_size == 0 the library's choice of that call; smx_distscene_stats holds step 1's counts and step
 *    5's structure words with the same meaning, and max_distance = the bound.  Behind them first_rec: per input triangle t of R
 *    the smallest position among the records that hold t, a position in the cell records, or a position in the wide list with
 *    the top bit set (a triangle is in cells or on the wide list, never both); 0xFFFFFFFF outside R.  Refused like that call:
 *    an index >= n, more than 2^30 entries, max_distance outside 1e-3f .. 16.0f, cell_size not 0 or finite and > 0, n_in >
 *    2^28, triangles == NULL with n_in > 0; also a scene and an object on different devices.  Ordered after everything enqueued
 *    on r, synchronous; changes in r only what smx_recon_mesh_distance changes (its workspace holds the sort's buffers).
 *    Building into a scene that holds a build replaces it.  A scene never built, or whose last build was refused or failed for
 *    any reason (an allocation included), is EMPTY: it holds no records, table or first_rec and refuses every query.  n_in == 0
 *    is a valid build (every point answers "none").  device_bytes = the device memory the scene holds after the build (records,
 *    table, first_rec, counters, and the query workspace as it stands).
 * Query (smx_distscene_query).  p->cell_size must be 0; p->max_distance = q must lie in 1e-3f .. the scene's max_distance, a
 *    larger one is SMX_ERR_INVALID_ARGUMENT with nothing written.  A smaller one needs no new structure: the 27 cells around a
 *    point's own hold every candidate as soon as c >= 1.125f * q, and float32 multiplication is monotone.  signed_distance, BAD
 *    points, the key, the outputs and the overlap rule are exactly those of smx_recon_mesh_distance: nearest, distance, closest
 *    and every word of smx_distance_stats are byte for byte what that call writes on the map as it stood at the build with the
 *    same triangles, max_distance = q and cell_size = the scene's cell_size_used (both sides then have the same c, so n_wide,
 *    n_entries and n_cells agree too).  The winner's closest point and sign are recomputed from the corners its first record
 *    holds: the float32 words the map held.  Synchronous.  on_device says where points, nearest, distance and closest live.
 *    n_points == 0 is valid; closest and stats may be NULL; points must not overlap an output (refused).  A query on an empty
 *    scene: SMX_ERR_INVALID_ARGUMENT.  A refused query writes nothing; every allocation (point staging, the points' sort
 *    buffers, the per-point keys) happens before the first write to an output.  One caller thread per scene.  A query does not
 *    touch r.
 * smx_recon_compare_to_distscene is BY DEFINITION smx_recon_sample_mesh(triangles, n_samples, seed) on r's map as it stands,
 *    then smx_distscene_query of those points (max_distance, unsigned, closest NULL), then the three exact sums of
 *    smx_recon_compare_meshes.  While the map is unchanged since the build, `out` equals the a_to_b side of
 *    smx_recon_compare_meshes with A = triangles, B = the scene's triangles, cell_size = the scene's cell_size_used and
 *    directions 1.  The samples never leave the device.  r and sc on different devices: refused.  A refusal by either half is the
 *    call's refusal, and `out` is zeroed.  on_device says where triangles lives.
 * All scene memory is counted by smx_debug_live_allocations and reached by smx_debug_fail_allocation.
 * Not done: incremental updates of a scene; an index shared with a smx_rayscene (their boxes differ); a BVH; an enqueue-only
 * query without host synchronisation (smx_distscene_register below enqueues the query's kernels itself). */
typedef struct smx_distscene_s* smx_distscene;
typedef struct {
  float max_distance;        /* the bound: a query asks for this much or less */
  float cell_size;           /* as smx_distance_params.cell_size; 0: the library chooses */
} smx_distscene_params;
typedef struct {
  uint32_t n_in, n_not_live, n_repeated, n_out_of_range;   /* as smx_distance_stats */
  uint32_t n_wide, n_entries, n_cells;
  float    cell_size_used;
  float    max_distance;              /* the bound of the build */
  uint64_t device_bytes;              /* device memory the scene holds after the build */
} smx_distscene_stats;
int smx_distscene_create(int32_t device_id /* -1: the current device */, smx_distscene* out);
int smx_distscene_destroy(smx_distscene sc);
int smx_distscene_params_default(smx_distscene_params* out);   /* 0.05f, 0.0f */
int smx_recon_build_distscene(smx_recon r, smx_stream s, smx_distscene sc, const smx_distscene_params* p,
                              const uint32_t* triangles, uint32_t n_in, int32_t on_device,
                              smx_distscene_stats* stats /* may be NULL */);
int smx_distscene_query(smx_distscene sc, smx_stream s, const smx_distance_params* p,
                        const float* points /* [n_points][3] */, uint32_t n_points,
                        uint32_t* nearest /* [n_points] */, float* distance /* [n_points] */,
                        float* closest /* [n_points][3], may be NULL */,
                        int32_t on_device, smx_distance_stats* stats /* may be NULL */);
int smx_recon_compare_to_distscene(smx_recon r, smx_stream s, smx_distscene sc, float max_distance, uint32_t n_samples, uint32_t seed,
                                   const uint32_t* triangles, uint32_t n_in, int32_t on_device, smx_compare_side* out);
/* Tools: milliseconds of the last build's phases mark, index, first (first_rec), then of the last query's phases query (the
 * points' sort, the walk), stats, by timed events on the calls' streams; a phase not reached reads 0.  capacity >=
 * SMX_DISTSCENE_PHASES. */
#define SMX_DISTSCENE_PHASES 5
int smx_distscene_debug_timings(smx_distscene sc, float* out_ms, int32_t capacity);

/* ---- registration of a point set to a distance scene: point-to-plane ICP against the triangles (not in the reference;
 * DESIGN.md 5q) ----
 * Inputs: a built scene, points [n][3] float32 in their own frame, optionally a unit normal per point, and a start pose T_init
 * (scene <- points, row-major 3x4).  State: T, the pose scene <- points, kept on the device in double; it starts as T_init
 * exactly, and every iteration reads it as 12 floats, Tf.  Every float32 expression below is evaluated as written, one
 * rounding per operation, no contraction.
 * One iteration of a level with stride s and gate q visits the samples j < ceil(n / s), sample j being point j s:
 *   Move.       p' = ((R00 x + R01 y) + R02 z) + t0 from Tf, likewise the other two rows; with normals m = R n, summed in the
 *               same order.
 *   Associate.  The answer for p' is exactly smx_distscene_query's at max_distance = q, unsigned: nearest t, closest Q.  A
 *               BAD p' (not finite, or a coordinate beyond 64 m) is BAD by that call's rule.  The winner's corners a, b, c
 *               are the float32 words its first record holds, as the query reads them.
 *   Row.        e1 = b - a, e2 = c - a, g = e1 x e2 (g.x = e1.y e2.z - e1.z e2.y, the others cyclic), len2 = (g.x g.x + g.y
 *               g.y) + g.z g.z.  A winner with !(len2 > 0) is collinear: the sample counts as matched and is no inlier.  N = g
 *               / sqrtf(len2) per component (smx_recon_triangulate winds counter-clockwise about the surfel normals, so N
 *               needs no flip).  With normals the sample needs (m.x N.x + m.y N.y) + m.z N.z >= cos(max_normal_angle), the
 *               cosine formed on the host as smx_recon_track forms it.  d = p' - Q, r = (N.x d.x + N.y d.y) + N.z d.z, J = (p'
 *               x N, N) -- rotation first: the update is a twist applied on the left, in the scene's frame.
 *   Sums.       The layout and the order of smx_recon_track: [0..20] JtJ, [21..26] Jtr, [27] sum r^2, [28] inliers, [29]
 *               samples that are not BAD, [30] samples matched within q; products in float, sums in double, a lane of a
 *               workgroup of 256 visiting the samples i, i + 256 grid, ..., the cross-lane tree, the wavefronts in index
 *               order, the workgroups' slabs in index order.  Two calls give the same bits.
 *   Solve.      That call's, unchanged: the finiteness test, DEGENERATE where [29] > 0 and [30] == 0 or on a small pivot,
 *               TOO_FEW_INLIERS, the LDL^T factorisation, T <- exp(x) Tf.  CONVERGED skips the rest of the level, the next
 *               level still runs; a bad status is sticky and T keeps the value it had before the failing iteration; the last
 *               iteration run is also judged against min_inlier_fraction x [29].
 * Launches per iteration: the move, the query's own three steps (the points' keys, the sort, the walk), the reduce, the
 * solve; every iteration of every level is enqueued back to back on s and nothing is read back until the end.  In a skipped
 * iteration (a bad status, a converged level) the move writes NaN points, so that the query's kernels find no work, and the
 * reduce and the solve return at once.  result is a device pointer if result_on_device, else a host pointer (the call returns
 * with it filled); with on_device points (and normals) and result_on_device the call returns without waiting for the device.
 * level_max_distance[l] = 0 means the scene's bound.  n_points == 0 is valid (TOO_FEW_INLIERS, or DEGENERATE at min_inliers ==
 * 0).  The call is ordered on s, behind the scene's previous registration on whatever stream; one caller thread per scene (it
 * uses the scene's query workspace and a workspace of its own, both counted by smx_debug_live_allocations and reached by
 * smx_debug_fail_allocation; every allocation happens before the first launch).  It touches no smx_recon: a scene is a
 * snapshot, and a registration gives the same bytes after the map has changed or the object it was built from is gone.
 * SMX_ERR_INVALID_ARGUMENT, nothing launched and nothing written: a scene without a build, no level with iterations, more than
 * 32 iterations in a level, a stride outside 1 .. 65536, a level's distance that is neither 0 nor in 1e-3f .. the scene's
 * bound, a T_init that is not finite, non-positive gates, points == NULL with n_points > 0, n_points > 2^28.
 * Not done: scale or non-rigid alignment; an incremental scene.  (Robust weights, rejecting matches on the mesh boundary and
 * mesh-to-mesh in one call: smx_distscene_register_robust and smx_recon_register_mesh below) */
typedef struct {             /* smx_register_params_default() fills the defaults */
  int32_t level_stride[3];          /* sample j of a level is point j * stride, j < ceil(n / stride); 1 .. 65536 */
  int32_t level_iterations[3];      /* 0 = level unused; at most 32 */
  float   level_max_distance[3];    /* the gate q of the level; 0 = the scene's bound; else 1e-3f .. the bound */
  float   max_normal_angle_deg;     /* used only when normals != NULL */
  float   convergence_rotation, convergence_translation;
  int32_t min_inliers;  float min_inlier_fraction;  float min_pivot_ratio;
} smx_register_params;
/* Defaults: strides 4, 2, 1; iterations 4, 5, 10; distances 0, 0, 0; 30 degrees; convergence 1e-5 rad / 1e-5 m; min_inliers
 * 50, min_inlier_fraction 0.1, min_pivot_ratio 1e-6 (the tracker's). */
typedef struct {
  float scene_T_points[12];   /* T_init itself, bit for bit, if nothing could be solved */
  int32_t status, iterations_run;               /* status: the SMX_TRACK_* values, same meaning and order */
  uint32_t inliers, points_used;                /* of the last iteration run: sums [28] and [29] */
  float rms_residual, last_update_rotation, last_update_translation;
  float information[36];                        /* JtJ of the last iteration, row-major 6x6 */
} smx_register_result;
int smx_register_params_default(smx_register_params* out);
int smx_distscene_register(smx_distscene sc, smx_stream s, const smx_register_params* p,
                           const float* points /* [n_points][3] */, const float* normals /* [n_points][3], may be NULL */,
                           uint32_t n_points, int32_t on_device, const float T_init[12],
                           smx_register_result* result, int32_t result_on_device);
/* Tests and tuning: one record per iteration of the scene's last registration that produced sums (the one that raised a bad
 * status included), with the pose it linearised at.  Synchronises s; *count = records of the call (at most `capacity` are
 * written). */
#define SMX_REGISTER_SUMS 31
typedef struct {
  int32_t level, stride, status, reserved;
  float Tf[12];               /* the pose this iteration linearised at */
  double sums[SMX_REGISTER_SUMS];
  double x[6];
} smx_register_iteration;
int smx_distscene_debug_register_iterations(smx_distscene sc, smx_stream s, smx_register_iteration* recs,
                                            int32_t capacity, int32_t* count);
/* Tools: milliseconds of the last registration by timed events on its stream: [0] the whole call, [1..4] the move, the query,
 * the reduce and the solve of the LAST iteration enqueued (a refused call leaves the figures of the one before).  capacity >=
 * SMX_REGISTER_PHASES. */
#define SMX_REGISTER_PHASES 5
int smx_distscene_debug_register_timings(smx_distscene sc, float* out_ms, int32_t capacity);

/* ---- the rim of a triangle array: which corners and edges of a triangle lie on the boundary of the surface (not in the
 * reference) ----
 * A function of the map as it stands and of `triangles` (uint32 [n_in][3], slot indices, in any order), made of integers only.
 * R is the triangle set of smx_recon_mesh_distance step 1: live corners, three different ones, within SMX_DIST_MAX_COORD; the
 * counts n_not_live, n_repeated and n_out_of_range are that step's.  c(u, v) is the number of triangles of R that have the
 * undirected edge {u, v}, whatever their winding; a triangle given twice counts twice.  An edge is a RIM EDGE iff c == 1, and a
 * slot is a RIM VERTEX iff it ends a rim edge.  rim[t] for t in R has bit k set for region k of that call's step 3, in its
 * order: bit 0 corner A is a rim vertex, bit 1 corner B, bit 2 edge AB is a rim edge, bit 3 corner C, bit 4 edge AC, bit 5
 * edge BC.  So "the closest point of that call lies on the rim" is (rim[t] >> region) & 1 with region 0 .. 5 as the branches
 * of step 3 come (A, B, AB, C, AC, BC), and the interior branch never is.  rim[t] = 0 outside R.  A corner's bit may be set
 * while none of the triangle's own edges is a rim edge: the rim edge belongs to a neighbour.
 * smx_rim_stats: the four counts of step 1; n_edges = the pairs with c >= 1; n_rim_edges (c == 1; on an array none of whose
 * triangles is repeated or out of range this is smx_fill_stats.n_boundary_edges); n_nonmanifold_edges (c >= 3; not that
 * call's word, which also counts two triangles wound alike); n_rim_vertices; n_rim_triangles = the bytes that are not 0.
 * Refused like smx_recon_mesh_distance refuses the array, nothing written: an index >= n, n_in > 2^28, triangles or rim NULL
 * with n_in > 0; also rim overlapping triangles.  n_in == 0 is valid.  on_device says where triangles and rim live.  Ordered
 * after everything enqueued on the object, synchronous; two calls give the same bytes.  Changes no map state.  The workspace
 * (the edge table of smx_recon_fill_holes, one bit per slot, the bytes) belongs to the object, grows on demand, is freed with
 * the object, is counted by smx_debug_live_allocations and reached by smx_debug_fail_allocation; every allocation comes before
 * the first write to an output.
 * smx_recon_build_distscene_rim is BY DEFINITION smx_recon_build_distscene followed by smx_recon_mesh_rim of the same array; the
 * bytes are kept with the scene, n_in of them, indexed like `nearest`, a snapshot like the rest of the scene (they survive what
 * the scene survives).  If either half fails the scene is left empty.  smx_distscene_stats keeps its meaning; device_bytes
 * includes the rim bytes.  A scene built by smx_recon_build_distscene has no rim.
 * Not done: rim flags on the samples' side; an incremental rim. */
typedef struct {
  uint32_t n_in, n_not_live, n_repeated, n_out_of_range;   /* as smx_distance_stats */
  uint32_t n_edges, n_rim_edges, n_nonmanifold_edges;
  uint32_t n_rim_vertices, n_rim_triangles;
} smx_rim_stats;
int smx_recon_mesh_rim(smx_recon r, smx_stream s, const uint32_t* triangles, uint32_t n_in, int32_t on_device,
                       uint8_t* rim /* [n_in] */, smx_rim_stats* stats /* may be NULL */);
int smx_recon_build_distscene_rim(smx_recon r, smx_stream s, smx_distscene sc, const smx_distscene_params* p,
                                  const uint32_t* triangles, uint32_t n_in, int32_t on_device,
                                  smx_distscene_stats* stats /* may be NULL */, smx_rim_stats* rim_stats /* may be NULL */);

/* ---- registration of partly overlapping surfaces: rim rejection and robust weights ----
 * smx_distscene_register_robust is smx_distscene_register with two more decisions per sample.  Everything of that call holds:
 * the move, the association by the scene's own query, the sum order, the solve, the status rules, every iteration enqueued back
 * to back with no host read until the end.  Per sample the order of decisions is: BAD -> not matched -> collinear winner -> rim
 * -> normal gate -> weight -> inlier.
 *   Rim.     region = the branch of smx_recon_mesh_distance step 3 that dist_closest takes for p' on the winner's first-record
 *            corners (the computation the query's Q came from).  With reject_rim a sample with (rim[t] >> region) & 1 counts as
 *            matched, is no inlier, and adds 1 to sum [31].
 *   Weights. float32, evaluated as written; a = fabsf(r), c = level_scale of the level; c == 0 or kernel 0: no weights.
 *            Huber: a <= c leaves the row unchanged; otherwise s = sqrtf(c / a), the row is (s J[k], s r) with e = r -- so [27]
 *            stays the geometric sum of r * r -- the sample stays an inlier and adds 1 to sum [32].
 *            Tukey: !(a < c): the sample is matched, is no inlier, and adds 1 to sum [32]; otherwise u = a / c, s = 1.0f - u * u
 *            (the weight is s * s), the row is (s J[k], s r) with e = r.
 *   Sums.    The 31 sums keep their meaning and their order; [31] and [32] are the two counts, carried in the 33-sum slabs of
 *            smx_recon_track_rgbd.  smx_distscene_debug_register_iterations serves this call's records too;
 *            smx_distscene_debug_register_robust_counts returns [31] and [32] of every recorded iteration.
 * With kernel 0 and reject_rim 0 the call IS smx_distscene_register: the same kernels, the same bytes in the result and in
 * every iteration record.  Refused (SMX_ERR_INVALID_ARGUMENT, nothing launched): what that call refuses; kernel outside 0 .. 2;
 * with kernel != 0 a level_scale of a used level that is neither 0 nor finite in 1e-6f .. 16.0f; reject_rim not 0 / 1;
 * reject_rim on a scene without a rim.
 * smx_recon_register_mesh is BY DEFINITION smx_recon_sample_mesh(triangles, n_samples, seed) on r's map as it stands with its
 * normals, then smx_distscene_register_robust of those points and normals.  The samples never leave the device.  r and sc on
 * different devices: refused.  A refusal by either half is the call's refusal.  Synchronous.  on_device says where triangles
 * lives.
 * Not done: rim flags on the samples' side; scale or non-rigid alignment; an incremental scene; other kernels (Cauchy,
 * Geman-McClure).  (A registration without a start pose: smx_distscene_register_global below) */
typedef struct {             /* smx_register_robust_params_default() fills the defaults: 0, {0, 0, 0}, 0 */
  int32_t kernel;            /* 0 none, 1 Huber, 2 Tukey */
  float   level_scale[3];    /* c of the level in metres; 0 = no weights on this level; else finite, 1e-6f .. 16.0f */
  int32_t reject_rim;        /* 1: a match whose closest point lies on the rim is no inlier; needs a scene with a rim */
} smx_register_robust_params;
int smx_register_robust_params_default(smx_register_robust_params* out);
int smx_distscene_register_robust(smx_distscene sc, smx_stream s, const smx_register_params* p,
                                  const smx_register_robust_params* rp, const float* points, const float* normals,
                                  uint32_t n_points, int32_t on_device, const float T_init[12],
                                  smx_register_result* result, int32_t result_on_device);
int smx_distscene_debug_register_robust_counts(smx_distscene sc, smx_stream s, uint32_t (*counts)[2], int32_t capacity,
                                               int32_t* count);
int smx_recon_register_mesh(smx_recon r, smx_stream s, smx_distscene sc, const uint32_t* triangles, uint32_t n_in,
                            int32_t on_device, uint32_t n_samples, uint32_t seed, const smx_register_params* p,
                            const smx_register_robust_params* rp, const float T_init[12],
                            smx_register_result* result, int32_t result_on_device);

/* ---- registration without a start pose: score a lattice of poses, refine the best (not in the reference) ----
 * Three calls: the candidate poses (host only), the score of many poses in one pass over the scene, and the whole search.
 * Every word of a score is an integer, so the scores, the selection and the winner are held to equality with a model.
 *
 * smx_register_pose_lattice.  A pure function on the host, in double with + - * / only.  Rotations: the integer quaternions (w, x,
 *    y, z) in [-k, k]^4 whose largest absolute component is exactly k, of each +- pair the one whose first non-zero component is
 *    positive, in ascending lexicographic order of (w, x, y, z); no two are parallel, so no rotation repeats; (k, 0, 0, 0) is the
 *    identity; N_k = ((2k+1)^4 - (2k-1)^4) / 2 of them (40, 272, 888, 2080, ...), k in 1 .. 8.  With n = w w + x x + y y + z z an
 *    exact integer every entry of R is one exact integer numerator divided once by n: R00 = (w w + x x - y y - z z) / n, R01 = 2 (x
 *    y - w z) / n, R02 = 2 (x z + w y) / n, R10 = 2 (x y + w z) / n, R11 = (w w - x x + y y - z z) / n, R12 = 2 (y z - w x) / n, R20 =
 *    2 (x z - w y) / n, R21 = 2 (y z + w x) / n, R22 = (w w - x x - y y + z z) / n.  For anchor a: t_i = a_i - ((R_i0 c_0 + R_i1 c_1) +
 *    R_i2 c_2), c = centre: a point in the points' frame, every anchor a point in the scene's frame where it may lie.  Each of
 *    the 12 values is rounded once to float32 (row-major 3x4, scene <- points).  Pose index = rotation index * A + anchor index.
 *    *count = N_k A is written whenever k, A (1 .. 2^20 / N_k) and the pointers are valid; poses are written only if capacity >=
 *    count and centre and anchors are finite, otherwise SMX_ERR_INVALID_ARGUMENT with *count set.  The largest angle from a
 *    rotation to the nearest lattice rotation, SAMPLED over 2000 rotations (a maximum of a sample, no bound): DESIGN.md 5s.
 *
 * smx_distscene_score_poses.  Sample j of every pose is point j * stride, j < m = ceil(n_points / stride), m <= 2^16.  For pose T
 *    (12 floats) and sample j: p' by the registration's move, float32 as written there.  The association is exactly
 *    smx_distscene_query's answer for p' at max_distance = q, unsigned (q = p->max_distance, 0 = the scene's bound).  Per pose:
 *      n_ok       samples whose p' is not BAD by the registration's rule
 *      n_matched  samples matched within q (sum [30] of a registration iteration at this pose, stride and gate)
 *      n_rim      with reject_rim: matched samples whose winner has an area (len2 > 0 as in that call's row) and whose closest
 *                 point lies on the rim -- the region of smx_recon_mesh_distance step 3 for p' on the winner's first-record
 *                 corners picks the bit of rim[t] -- which is sum [31] of smx_distscene_register_robust with reject_rim; else 0
 *      cost       the sum over all m samples of (uint32)(distance * 1048576.0f), the 2^-20 m word of smx_recon_compare_meshes,
 *                 if the sample is matched and not counted in n_rim, else of that word of q.  A BAD sample pays q's word too.
 *    Integers only: the bytes do not depend on schedule, chunking or search structure; two calls give the same bytes.  Poses are
 *    processed in chunks of floor(chunk_points / m) poses, at least one (chunk_points = 2^22 unless
 *    smx_distscene_debug_set_score_chunk says otherwise, 1 .. 2^24), which bounds the workspace; the chunks are enqueued back to
 *    back -- per chunk the move, the query's three steps, the score kernel -- and the host reads nothing until all P are scored.
 *    Synchronous; waits for a registration still running on the scene.  1 <= P <= 2^20.  poses and scores are host memory;
 *    on_device says where points live.  One caller thread per scene; touches no smx_recon: a scene is a snapshot.  The workspace
 *    belongs to the scene, is counted by smx_debug_live_allocations and reached by smx_debug_fail_allocation; every allocation
 *    comes before the first launch.  SMX_ERR_INVALID_ARGUMENT, nothing launched and nothing written: an empty scene, a pose entry
 *    that is not finite, stride outside 1 .. 65536, m > 2^16, P outside 1 .. 2^20, q neither 0 nor finite in 1e-3f .. the scene's
 *    bound, reject_rim not 0 / 1 or on a scene without a rim, points == NULL with n_points > 0, n_points > 2^28, scores
 *    overlapping poses or host points.
 *
 * smx_distscene_register_global.  BY DEFINITION, in this order:
 *    1. smx_distscene_score_poses of all P poses with gp->score.
 *    2. The poses ordered by (cost, pose index) ascending; the first M = min(n_starts, P) are the starts.  One read-back.
 *    3. For rank r = 0 .. M - 1: smx_distscene_register -- or smx_distscene_register_robust iff rp != NULL and asks for a kernel or
 *       reject_rim -- with T_init = poses[index_r], p, the points and normals given: its result, byte for byte.  A start that
 *       fails keeps its T_init, as that call's contract says.
 *    4. smx_distscene_score_poses of the M result poses with gp->score: cost_after, n_matched_after.
 *    5. The winner is the start with the smallest (cost_after, rank).
 *    out->result = the winner's smx_register_result; found = 1 iff its status is OK or CONVERGED and (float)n_matched_after >=
 *    min_matched_fraction * (float)n_ok_after; winner_rank; n_starts_run = M; starts[r] for r < M, zeros behind.  all_scores
 *    (may be NULL) receives step 1's P scores.  Refused, nothing written: what either of the two calls refuses; n_starts outside
 *    1 .. 64; min_matched_fraction outside 0 .. 1; out or all_scores overlapping poses, host points or normals, or each other.
 *    Synchronous.
 *    Not built: suppressing starts that fall into one basin; feature matching; scale; a search over translations beyond the
 *    anchors given; an enqueue-only variant. */
typedef struct {
  int32_t stride;            /* sample j is point j * stride; 1 .. 65536 */
  float   max_distance;      /* the gate q; 0 = the scene's bound; else 1e-3f .. the bound */
  int32_t reject_rim;        /* 1: a match whose closest point lies on the rim pays q; needs a scene with a rim */
} smx_score_params;
typedef struct {
  uint64_t cost;
  uint32_t n_ok, n_matched, n_rim, reserved;
} smx_pose_score;
typedef struct {             /* smx_global_params_default() fills the defaults: {1, 0, 0}, 8, 0.5 */
  smx_score_params score;
  int32_t n_starts;          /* 1 .. 64 */
  float   min_matched_fraction;
} smx_global_params;
#define SMX_GLOBAL_MAX_STARTS 64
typedef struct {
  uint32_t pose_index;
  int32_t  status, iterations_run;   /* of the registration from this start */
  uint32_t n_matched_after;
  uint64_t cost_before, cost_after;
} smx_global_start;
typedef struct {
  smx_register_result result;        /* the winner's */
  int32_t found, winner_rank, n_starts_run, reserved;
  smx_global_start starts[SMX_GLOBAL_MAX_STARTS];
} smx_global_result;
int smx_register_pose_lattice(int32_t k, const double centre[3], const double* anchors /* [A][3] */, uint32_t A,
                              float* poses /* [capacity][12] */, uint32_t capacity, uint32_t* count);
int smx_global_params_default(smx_global_params* out);
int smx_distscene_score_poses(smx_distscene sc, smx_stream s, const smx_score_params* p, const float* points /* [n_points][3] */,
                              uint32_t n_points, int32_t on_device, const float* poses /* [P][12], host */, uint32_t P,
                              smx_pose_score* scores /* [P], host */);
int smx_distscene_register_global(smx_distscene sc, smx_stream s, const smx_global_params* gp, const smx_register_params* p,
                                  const smx_register_robust_params* rp /* may be NULL */, const float* points,
                                  const float* normals /* may be NULL */, uint32_t n_points, int32_t on_device,
                                  const float* poses /* [P][12], host */, uint32_t P, smx_global_result* out,
                                  smx_pose_score* all_scores /* [P], host, may be NULL */);
/* Tests: the samples a chunk of smx_distscene_score_poses may hold (1 .. 2^24), so that a small case crosses chunk edges. */
int smx_distscene_debug_set_score_chunk(smx_distscene sc, uint32_t chunk_points);
/* Tools: milliseconds of the scene's last pose scoring and search: [0] the score phase (step 1, or the last
 * smx_distscene_score_poses) by timed events on its stream, [1..3] the move, the query and the score kernel of its LAST chunk, [4..6]
 * select, refine and rescore of the last smx_distscene_register_global on the host's clock (0 after a bare score).  capacity >=
 * SMX_GLOBAL_PHASES. */
#define SMX_GLOBAL_PHASES 7
int smx_distscene_debug_global_timings(smx_distscene sc, float* out_ms, int32_t capacity);

/* ---- a triangle array drawn to images: a software rasteriser (not in the reference, whose viewer draws the mesh with
 * OpenGL) ----
 * A pure function of the map as it stands (smooth position rows 3-5, RadiusSquared row 7, normal rows 8-10, the rows the
 * colour of smx_recon_update_visualization_buffers reads; slots [0, n) with n = surfels_size()), of `triangles` (uint32
 * [n_triangles][3], slot indices: the format smx_recon_triangulate and smx_recon_decimate_mesh write) and of p.  Camera,
 * size, near_z / far_z, color_flags, frame_index and the window are those of smx_render_params (pixel-corner convention).
 * Every floating-point quantity below is a DOUBLE expression evaluated as written, one rounding per operation, no
 * contraction; division and square root are correctly rounded.  Everything that decides coverage is an integer.
 * Vertex.  L = camera_T_global, inverted on the host in double as in smx_recon_render.  For slot i with smooth position
 *    (px, py, pz): c.k = L[4k] px + L[4k+1] py + L[4k+2] pz + L[4k+3], summed left to right; u = fx c.x / c.z + cx,
 *    v = fy c.y / c.z + cy; snapped to 1/256 pixel: X = (int64)floor(u * 256.0 + 0.5), Y likewise.
 * Triangle t = (a, b, c), in this order:
 * 1. An index >= n: counted in n_out_of_range, never dereferenced, not drawn (not an error).
 * 2. A corner that is not live (!(RadiusSquared < 0) and a finite smooth position, as in smx_recon_triangulate): n_not_live.
 * 3. A corner with !(near_z < c.z && c.z < far_z) or !(fabs(u) < 1048576.0 && fabs(v) < 1048576.0): n_clipped.
 * 4. A = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) in int64 (every product stays below 2^59).  A == 0: n_degenerate.
 * 5. Front-facing iff A < 0 (x right, y down, z forward: sign(A) = sign(a_c . n) for n = (b - a) x (c - a)).  With
 *    cull_back_faces a triangle with A > 0 is dropped and counted in n_culled.
 * 6. Pixel box x0 = ceil((min X - 128) / 256), x1 = floor((max X - 128) / 256) in integer arithmetic, y likewise, both
 *    clamped to the image.  Empty: not drawn.  Otherwise n_drawn, and n_large as well iff (x1 - x0 + 1)(y1 - y0 + 1) >
 *    SMX_MESH_RENDER_LARGE_PIXELS (which only chooses the kernel that walks the box).
 * Coverage of pixel (x, y), centre P = (256 x + 128, 256 y + 128).  s = sign(A); w0 = s E(b, c, P), w1 = s E(c, a, P),
 *    w2 = s E(a, b, P) with E(p, q, P) = (Xq - Xp)(Py - Yp) - (Yq - Yp)(Px - Xp) in int64.  Covered iff for every edge
 *    w_k > 0, or w_k == 0 and, with d = s (q - p), d.y < 0 || (d.y == 0 && d.x > 0).  Two triangles of one facing that
 *    share an edge traverse it in opposite directions, so a centre exactly on the edge belongs to exactly one of them.
 * Depth, perspective-correct: l_k = (double)w_k / (double)|A|; invz = (l0 / za + l1 / zb) + l2 / zc with z = the corners'
 *    c.z; Z = 1.0 / invz; depth = (float)Z.
 * Z-test: every pixel keeps the minimum of (float_bits(depth) << 32) | t, t = the triangle's position in `triangles` (a
 *    tie goes to the earlier triangle): the result does not depend on scheduling, two calls give the same bytes.
 * Outputs (each may be NULL; otherwise exactly height x width with the element size given, any pitch):
 *   depth  float   the winner's depth, 0 where no triangle covers the pixel
 *   index  u32     the winner's t, 0xFFFFFFFF where empty
 *   normal float4  with m_k = (l_k / z_k) * Z and n_k = the corner's normal rotated by L's rotation (in double, summed left
 *                  to right): SMX_MESH_NORMAL_VERTEX takes N = (m0 n_a + m1 n_b) + m2 n_c per component, SMX_MESH_NORMAL_FACE
 *                  g = (b_c - a_c) x (c_c - a_c) on the camera-space corners (g.x = e.y f.z - e.z f.y and cyclic), negated
 *                  if (g.x a.x + g.y a.y) + g.z a.z > 0, so that it faces the camera.  len2 = (Nx Nx + Ny Ny) + Nz Nz; the
 *                  output is (float)(N / sqrt(len2)), zeros if !(len2 > 0); w = 0; zeros where empty
 *   color  uchar4  per channel min(255, floor(((m0 C_a + m1 C_b) + m2 C_c) + 0.5)) over the bytes of the corners' vertex-
 *                  buffer colours (color_flags); alpha 255; (0, 0, 0, 0) where empty
 * Not promised: there is no near-plane clipping -- a triangle with a corner outside (near_z, far_z) is dropped whole, so
 *   a surface that passes through the near plane shows a ragged hole there.  No anti-aliasing.  A vertex-clustered mesh
 *   may hold triangles that face against their corners' normals; cull_back_faces drops them.
 * Calling rules: enqueued on s behind the pipelined regulariser and behind the previous smx_recon_render / _render_mesh /
 *   tracking call (the z-buffer is the object's, shared with them, and grows on demand; growing a workspace waits for the
 *   device).  on_device says where `triangles` lives; a host array is staged first.  With on_device != 0 and stats ==
 *   NULL nothing waits on the host; a non-NULL stats makes the call synchronise s and read the counters back.
 *   n_triangles == 0 is valid and gives empty images; at most 2^31 - 1 triangles.  Invalid sizes, parameters, modes or descriptors, or triangles ==
 *   NULL with n_triangles > 0: SMX_ERR_INVALID_ARGUMENT with nothing launched.  Changes no map state, delta mark,
 *   statistic or stamp, nor the state smx_recon_triangulate_update keeps. */
enum { SMX_MESH_NORMAL_VERTEX = 0, SMX_MESH_NORMAL_FACE = 1 };
#define SMX_MESH_RENDER_LARGE_PIXELS 256
typedef struct {
  int32_t width, height;
  float fx, fy, cx, cy;                    /* pixel-corner convention */
  float global_T_camera[12];               /* row-major 3x4 */
  float near_z, far_z;                     /* 0 < near_z < far_z */
  int32_t color_flags;                     /* SMX_VIS_* */
  uint32_t frame_index;                    /* for the age colours */
  int32_t surfel_integration_active_window_size;
  int32_t cull_back_faces;                 /* 0 / 1 */
  int32_t normal_mode;                     /* SMX_MESH_NORMAL_* */
} smx_mesh_render_params;
typedef struct {
  uint32_t n_in;             /* triangles given */
  uint32_t n_out_of_range;   /* of those, with an index >= surfels_size() */
  uint32_t n_not_live;       /* with a corner that is not live */
  uint32_t n_clipped;        /* with a corner outside (near_z, far_z) or projecting beyond +-2^20 pixels */
  uint32_t n_degenerate;     /* with A == 0 */
  uint32_t n_culled;         /* back-facing, with cull_back_faces */
  uint32_t n_drawn;          /* with a non-empty pixel box (the rest: off the image, or between pixel centres) */
  uint32_t n_large;          /* of n_drawn, with a box above SMX_MESH_RENDER_LARGE_PIXELS */
  uint32_t n_covered_pixels; /* pixels of the image some triangle covers */
} smx_mesh_render_stats;
/* width = height = 0 (to be set), near_z 0.05, far_z 1000, identity pose, the colour row, no culling, vertex normals */
int smx_mesh_render_params_default(smx_mesh_render_params* out);
int smx_recon_render_mesh(smx_recon r, smx_stream s, const smx_mesh_render_params* p,
                          const uint32_t* triangles, uint32_t n_triangles, int32_t on_device,
                          const smx_buffer_desc* depth, const smx_buffer_desc* index,
                          const smx_buffer_desc* normal, const smx_buffer_desc* color,
                          smx_mesh_render_stats* stats /* may be NULL */);
/* Tools: milliseconds the last smx_recon_render_mesh call spent in k_mrast_small (with the clears before it),
 * k_mrast_large and k_mrast_resolve, by timed events on the call's stream.  Zeros before the first call. */
int smx_recon_debug_mesh_render_timings(smx_recon r, float out_ms[3]);

/* ---- merging another session's map into this one (not in the reference: its map comes from one camera stream) ----
 * smx_recon_merge_map puts the surfels of `src` into `dst` under the pose dst_T_src (row-major 3x4, as smx_distscene_register
 * and its relatives return it): a source surfel that finds a compatible surfel of dst is dropped (KEEP_DST) or blended into
 * it (BLEND), every other one is appended.  Integers and float32 expressions only, each evaluated as written (no
 * contraction); rows are those of SURVEY.md Appendix A.  "dst as it stood" = dst before the call: all matching is against
 * that, so the result does not depend on any order of writes, and two calls give the same bytes.
 * 1. Live.  Source slot i < surfels_size(src) is live iff !(RadiusSquared_i < 0) (a NaN radius is live).
 * 2. Move.  x' = ((R00 x + R01 y) + R02 z) + t0 and likewise y', z' (the move of smx_distscene_register), applied to the raw
 *    position (rows 0-2), to the smooth position (rows 3-5), and without t to the normal (rows 8-10).  A live slot with a
 *    non-finite word among the nine moved ones is BAD: neither matched nor appended, counted in n_bad.
 * 3. Candidates.  The index is smx_recon_build_neighbor_index(dst, s, nn, cell_size): dst's smooth positions, merged slots
 *    left out.  The candidates of i are smx_nn_query_batch's answer for the moved smooth position with r2 =
 *    radius_factor_squared * RadiusSquared_i and k: up to k slots of dst, ascending by (dist^2, index).
 * 4. Match.  m(i) = the first candidate d with (n'.x N_d.x + n'.y N_d.y) + n'.z N_d.z >= cos_max, N_d from dst as it stood,
 *    cos_max = (float)cos((double)max_normal_angle_deg * (pi / 180)) as smx_recon_track forms it.  Without such a candidate i
 *    is unmatched; an unmatched i whose list was full (count == k) is counted in n_saturated as well: a compatible surfel may
 *    lie behind the k nearest, raise k if that number matters.
 * 5. Append.  The unmatched live slots that are not BAD take the slots old_size + rank of dst, in ascending order of i.
 *    old_size + n_appended > max_surfel_count(dst): SMX_ERR_INVALID_ARGUMENT, dst byte for byte unchanged, stats filled (so
 *    that the caller sees the room needed).  Rows of an appended slot: 0-5 and 8-10 the moved words; 6, 7 copied; 11-16 and
 *    23 zero; 17, 18 = frame_index; 24 the 32 colour bits copied; 19-22 the source's links through the map: a link to an
 *    appended source slot becomes that slot's new index, every other one (invalid, or to a merged, BAD or matched slot)
 *    0xFFFFFFFF.  links_dropped = the links of appended slots that were not 0xFFFFFFFF in src and are now.
 * 6. SMX_MERGE_KEEP_DST.  Matched source slots leave no trace in dst.
 * 7. SMX_MERGE_BLEND.  For a slot d of dst with the matched sources i1 < i2 < ...: start from dst's raw position P, smooth
 *    position S, normal N, c = row 6, r = row 7, and take the sources in ascending order: w = Confidence_i, W = c + w;
 *    !(W > 0): this source changes nothing; else a = c / W, b = w / W, P = (a P) + (b P'), S = (a S) + (b S'), M = (a N) +
 *    (b n') per component, len2 = (M.x M.x + M.y M.y) + M.z M.z, N = M / sqrtf(len2) per component if len2 > 0 (else N stays),
 *    r = fminf(r, RadiusSquared_i), c = fminf(W, confidence_cap).  Then rows 0-10 of d are written and row 18 = frame_index;
 *    creation stamp, links and colour stay.  n_blended_dst = the number of such d.
 * 8. src_to_dst (may be NULL; capacity >= surfels_size(src) entries; device pointer if on_device, host pointer otherwise):
 *    m(i) for a matched slot, the new index for an appended one (told apart by >= old_size), 0xFFFFFFFF for dead and BAD
 *    slots.  A triangle array over src goes through it as a mesh goes through compaction's old_to_new: a triangle that
 *    loses a corner is dropped.
 * 9. State.  Afterwards surfels_size(dst) = new_size and the merge count is unchanged; the derived frame-loop state is what
 *    smx_recon_compact leaves (a superset of a state upload's resets), except that with delta tracking on exactly the
 *    appended and blended slots are marked; the next smx_recon_integrate may use any frame_index.  nn is stale after the call
 *    (it indexes dst as it stood).  Scenes are snapshots and are unaffected.  src is read only.
 * Calling rules: synchronous like smx_recon_compact; ordered behind everything enqueued on both objects (the pipelined
 *   regulariser of each included).  Refused with SMX_ERR_INVALID_ARGUMENT, nothing launched and nothing written: a NULL
 *   pointer other than src_to_dst or stats, src == dst, objects on different devices, k outside 1..64, frame_index == 0,
 *   cell_size or radius_factor_squared not > 0, an angle outside 0..180, a non-finite dst_T_src, an unknown mode, a NaN
 *   confidence_cap, a capacity below surfels_size(src).  An empty src is valid and changes nothing; an empty dst is valid
 *   and appends everything.  The workspace belongs to dst, is counted by smx_debug_live_allocations and reached by
 *   smx_debug_fail_allocation; every allocation comes before the first write to dst, so a failed one leaves dst unchanged.
 * Not built: colour blending, links between the two sessions' surfels, de-duplication inside src, a merge that keeps the
 *   source's stamps. */
enum { SMX_MERGE_KEEP_DST = 0, SMX_MERGE_BLEND = 1 };
#define SMX_MERGE_PHASES 7
typedef struct {            /* smx_merge_params_default() fills the defaults */
  float   cell_size;                 /* of the neighbour index built over dst; > 0; default 0.05 */
  float   radius_factor_squared;     /* ball of a source surfel: r2 = factor * its RadiusSquared; default 1.0f */
  float   max_normal_angle_deg;      /* default 30; cosine formed on the host as smx_recon_track forms it */
  int32_t k;                         /* candidates looked at per source surfel, 1 .. 64; default 8 */
  int32_t mode;                      /* SMX_MERGE_KEEP_DST = 0 | SMX_MERGE_BLEND = 1 */
  float   confidence_cap;            /* BLEND only; default FLT_MAX */
  uint32_t frame_index;              /* >= 1: stamp of appended and blended slots; default 1 */
} smx_merge_params;
typedef struct {
  uint32_t n_src_slots, n_src_live, n_bad, n_matched, n_appended, n_blended_dst, n_saturated, links_dropped;
  uint32_t old_size, new_size;
} smx_merge_stats;
int smx_merge_params_default(smx_merge_params* out);
int smx_recon_merge_map(smx_recon dst, smx_stream s, smx_nn nn, smx_recon src, const float dst_T_src[12],
                        const smx_merge_params* p, uint32_t* src_to_dst, uint32_t capacity, int32_t on_device,
                        smx_merge_stats* stats);
/* Tools: milliseconds of dst's last smx_recon_merge_map call by timed events on its stream: out_ms[0] the whole call, then
 * the SMX_MERGE_PHASES phases index build, move, query + select (all chunks), number, append, blend, finish; at most
 * `capacity` values are written.  The waits of the call's read-backs fall into the phase they end.  Zeros before the first
 * call and after a call that failed. */
int smx_recon_debug_merge_timings(smx_recon dst, float* out_ms, int32_t capacity);
/* Tests: the queries of a merge run in chunks of chunk_queries source slots (0 = the default, 2^22), which bounds the
 * [chunk][k] candidate workspace; results must not depend on it. */
int smx_recon_debug_set_merge_chunk(smx_recon dst, uint32_t chunk_queries);

/* ---- importing a point cloud as surfels (not in the reference: its map comes from RGB-D frames) ----
 * smx_recon_import_points turns n points -- positions, perhaps colours, perhaps the sensor origin each was seen from -- into
 * surfels behind the map's slots: the normal is the smallest eigenvector of the covariance of the point's k nearest
 * neighbours, the radius comes from a neighbour distance.  float32 and double expressions as stated, each evaluated as
 * written (no contraction); rows are those of SURVEY.md Appendix A.
 * 1. BAD.  A point with a non-finite coordinate is BAD; with orient = SMX_IMPORT_ORIENT_ORIGINS a point with a non-finite
 *    origin word is BAD too.  A BAD point is left out of the index, so it is never a neighbour.  (A finite coordinate the
 *    index does not take, |v| > 3.0e38f, is not BAD: the point gets an empty list and is SPARSE.)
 * 2. List.  nn is built by smx_nn_build over the points that are not BAD with cell_size.  The list of point i is
 *    smx_nn_query_self's answer with r^2 = search_radius * search_radius (float32) and k: m entries (j, d2), ascending by
 *    (d2, index), the point itself included.  n_saturated counts the points with m == k.
 * 3. SPARSE.  m < min_neighbors.
 * 4. Covariance.  Over the entries e = 0 .. m-1 in list order, j the entry's point: d = (x_j - x_i, y_j - y_i, z_j - z_i),
 *    each a float32 subtraction; s_a += (double)d_a and q_ab += (double)d_a * (double)d_b for the six a <= b, nine double
 *    sums.  inv = 1.0 / (double)m, mean_a = s_a * inv, C_ab = q_ab * inv - mean_a * mean_b.
 * 5. Eigenvectors.  Cyclic Jacobi in double on A = C, V = identity: SMX_IMPORT_JACOBI_SWEEPS sweeps over the pairs (p, q) =
 *    (0,1), (0,2), (1,2), r the third index.  A pair with a_pq == 0 is skipped.  Otherwise theta = (a_qq - a_pp) / (2.0 * a_pq),
 *    t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)) (an infinite theta gives t = 0),
 *    c = 1.0 / sqrt(t * t + 1.0), sn = t * c, and from the old values
 *      a_pp' = a_pp - t * a_pq,  a_qq' = a_qq + t * a_pq,  a_pq' = 0,
 *      a_rp' = c * a_rp - sn * a_rq,  a_rq' = sn * a_rp + c * a_rq,
 *      v_ip' = c * v_ip - sn * v_iq,  v_iq' = sn * v_ip + c * v_iq  for the rows i = 0, 1, 2.
 *    lam0 = the smallest diagonal entry afterwards (ties: the lowest column), the normal that column of V; lam1, lam2 = the
 *    other two diagonal entries in ascending column order.
 * 6. ROUGH.  lam0 > (double)max_surface_variation * ((lam0 + lam1) + lam2).
 * 7. Normal.  (nx, ny, nz) = the three doubles as floats; len2 = (nx nx + ny ny) + nz nz; n = n / sqrtf(len2) per component.
 *    !(len2 > 0) or a non-finite component: DEGENERATE.  Orientation (VIEW_POINT: o = view_point, ORIGINS: o = the point's
 *    origin): v = o - p per component in float32; (nx vx + ny vy) + nz vz < 0 negates the normal, a zero dot keeps it.
 *    SMX_IMPORT_ORIENT_NONE keeps the sign Jacobi left.
 * 8. Radius.  RadiusSquared = radius_scale_squared * d2[min(radius_rank, m - 1)], d2 the list's own float32 words.
 *    !(RadiusSquared > 0): DEGENERATE (a point whose list up to that rank is duplicates of itself).
 * 9. Class.  BAD, SPARSE, DEGENERATE (by the radius, then by the normal), ROUGH, else imported: the first that holds.  Each
 *    point is counted once: n_points = n_bad + n_sparse + n_degenerate + n_rough + n_imported.
 * 10. Append.  The imported points take the slots old_size + rank, in ascending point order.  old_size + n_imported >
 *    max_surfel_count(r): SMX_ERR_INVALID_ARGUMENT, the map byte for byte unchanged, stats filled, point_to_slot not written.
 *    Rows of an appended slot: 0-2 and 3-5 the point; 6 confidence; 7 RadiusSquared; 8-10 the normal; 11-16 and 23 zero;
 *    17, 18 = frame_index; 19-22 = 0xFFFFFFFF; 24 = colors[i], or default_color where colors is NULL.
 * 11. point_to_slot (may be NULL; capacity >= n entries; device pointer if on_device, host pointer otherwise): the slot of an
 *    imported point, 0xFFFFFFFF for every other.
 * 12. State.  Afterwards surfels_size(r) = new_size and the merge count is unchanged; the derived frame-loop state is what
 *    smx_recon_merge_map leaves, with delta marks on exactly the appended slots.  Nothing is matched against the surfels the
 *    map already holds (that is smx_recon_merge_map's job).  nn indexes the cloud afterwards, not the map.
 * Calling rules: synchronous; ordered behind everything enqueued on the object.  points, colors and origins are device
 *   pointers if inputs_on_device, host pointers otherwise, and are read only.  Refused with SMX_ERR_INVALID_ARGUMENT, nothing
 *   launched and nothing written: a NULL r, nn or p; NULL points with n > 0; NULL origins with ORIGINS; a field of p outside
 *   the range below; a capacity below n with a point_to_slot.  n == 0 is valid and changes nothing.  The workspace belongs to
 *   r, is counted by smx_debug_live_allocations and reached by smx_debug_fail_allocation; every allocation comes before the
 *   first write to the map, so a failed one leaves the map unchanged.
 * Not built: voxel thinning of dense clouds, projecting the smooth position onto the fitted plane, links among imported
 *   surfels (rows 19-22), orientation without origins by propagation over the neighbour graph, per-point confidences. */
enum { SMX_IMPORT_ORIENT_NONE = 0, SMX_IMPORT_ORIENT_VIEW_POINT = 1, SMX_IMPORT_ORIENT_ORIGINS = 2 };
#define SMX_IMPORT_PHASES 7
#define SMX_IMPORT_JACOBI_SWEEPS 6
typedef struct {            /* smx_import_params_default() fills the defaults */
  float   cell_size;                 /* of the neighbour index built over the cloud; > 0; default 0.05 */
  float   search_radius;             /* metres, > 0; default 0.1 */
  int32_t k;                         /* entries of a point's list, 4 .. 64; default 16 */
  int32_t min_neighbors;             /* 3 .. k; default 6 */
  float   max_surface_variation;     /* lam0 / (lam0 + lam1 + lam2) above which a point is ROUGH, 0 .. 1/3; default 1/3 */
  int32_t radius_rank;               /* the list entry whose d2 gives the radius, 1 .. 63; default 8 */
  float   radius_scale_squared;      /* > 0; default 2.0 */
  float   confidence;                /* row 6 of every imported slot; finite; default 1.0 */
  uint32_t default_color;            /* row 24 where colors is NULL; default 0 */
  uint32_t frame_index;              /* >= 1: rows 17 and 18; default 1 */
  int32_t orient;                    /* SMX_IMPORT_ORIENT_*; default NONE */
  float   view_point[3];             /* finite; default 0, 0, 0 */
} smx_import_params;
typedef struct {
  uint32_t n_points, n_bad, n_sparse, n_degenerate, n_rough, n_imported, n_saturated;
  uint32_t old_size, new_size;
} smx_import_stats;
int smx_import_params_default(smx_import_params* out);
int smx_recon_import_points(smx_recon r, smx_stream s, smx_nn nn,
                            const float* points /* [n][3] */, const uint32_t* colors /* [n] or NULL */,
                            const float* origins /* [n][3] or NULL */, uint32_t n, int32_t inputs_on_device,
                            const smx_import_params* p, uint32_t* point_to_slot, uint32_t capacity, int32_t on_device,
                            smx_import_stats* stats);
/* Tools: milliseconds of r's last smx_recon_import_points call by timed events on its stream: out_ms[0] the whole call, then
 * the SMX_IMPORT_PHASES phases stage, index build, self-query, fit, number, write, finish; at most `capacity` values are
 * written.  The waits of the call's read-backs fall into the phase they end.  Zeros before the first call and after a call
 * that failed. */
int smx_recon_debug_import_timings(smx_recon r, float* out_ms, int32_t capacity);

/* ---- benchmark input generator (not part of the reference's interface) ----
 * Renders one frame of the synthetic room stream into device buffers:
 * depth u16 = round(depth_scaling * z) with sigma = noise_sigma * z^2 noise and coherent 8x8
 * drop-outs, colour uchar3 = hash of the 10 cm world cell.  Pure function of its arguments. */
int smx_synth_render_room(smx_stream s, const smx_buffer_desc* depth_out, const smx_buffer_desc* color_out,
                          float fx, float fy, float cx, float cy, const float global_T_frame[12],
                          uint32_t seed, uint32_t frame_index, float depth_scaling, float noise_sigma,
                          float dropout);

#ifdef __cplusplus
}
#endif
#endif
