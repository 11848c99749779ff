// smx_mesh_raster.hip -- smx_recon_render_mesh: a software rasteriser for a triangle array over the surfel map (gfx950).
// The contract is in include/smx.h, its arithmetic in smx_mesh_raster.hpp, the account in DESIGN.md 5h.
//
//   k_mrast_small    a lane per triangle, grid-stride: gathers the corners' S and N records, does the set-up, counts the
//                    verdict, and walks its own pixel box with the z-test of smx_recon_render.  A triangle whose box is
//                    above SMX_MESH_RENDER_LARGE_PIXELS is not walked but appended to a list (one atomic per wavefront).
//   k_mrast_large    a wavefront per listed triangle, grid-stride over the list (its length is read on the device): the box
//                    in 8 x 8 pixel tiles, a lane per pixel; a tile outside one edge at all four corners is skipped.
//   k_mrast_resolve  a lane per pixel: decodes the key, repeats the winner's set-up and the pixel's weights, writes the
//                    requested images and counts the covered pixels.
//
// The three kernels call the same inline functions, so set-up, coverage and depth have the same bits wherever they are
// evaluated; the z-buffer keeps the minimum key per pixel, so neither the order of the lanes nor that of the list shows.
#include "smx_recon_state.hpp"

using namespace smx;

namespace {

// z-test as in smx_recon_render: a plain load first, so that a hidden fragment costs no atomic
__device__ __forceinline__ void mrast_zmin(unsigned long long* p, unsigned long long key) {
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

__device__ __forceinline__ MrVertex mrast_corner(const Surfels& S, const MrCam& cam, uint32_t i) {
  const float4 sp = *S.group(kGroupS, i);
  return mr_vertex(cam, sp.x, sp.y, sp.z);
}

// Steps 1-6 of the contract for triangle t.  (n = slots in use; an index beyond it is never dereferenced.)
__device__ __forceinline__ int mrast_setup(const Surfels& S, const MrCam& cam, const uint32_t* __restrict__ tri, uint32_t t, uint32_t n,
                                           MrTri* out) {
  const uint32_t a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
  if (a >= n || b >= n || c >= n) return kMrOutOfRange;
  const float4 sa = *S.group(kGroupS, a), sb = *S.group(kGroupS, b), sc = *S.group(kGroupS, c);
  const float ra = S.f(kRadiusSq, a), rb = S.f(kRadiusSq, b), rc = S.f(kRadiusSq, c);
  if (!(mr_live(sa.x, sa.y, sa.z, ra) && mr_live(sb.x, sb.y, sb.z, rb) && mr_live(sc.x, sc.y, sc.z, rc))) return kMrNotLive;
  return mr_setup(cam, mr_vertex(cam, sa.x, sa.y, sa.z), mr_vertex(cam, sb.x, sb.y, sb.z), mr_vertex(cam, sc.x, sc.y, sc.z), out);
}

__device__ __forceinline__ uint32_t wave_count(bool pred) { return (uint32_t)__popcll(__ballot(pred)); }

__global__ void __launch_bounds__(kBlock)
k_mrast_small(Surfels S, MrCam cam, const uint32_t* __restrict__ tri, uint32_t n_tri, unsigned long long* __restrict__ zbuf,
              uint32_t* __restrict__ list, uint32_t* __restrict__ counters, const DevState* st) {
  const uint32_t n = st->surfel_count, lane = threadIdx.x & 63;
  // (the per-wavefront sums are the same in every lane: they live in scalar registers)
  uint32_t c_range = 0, c_live = 0, c_clip = 0, c_degen = 0, c_cull = 0, c_drawn = 0, c_large = 0;
  // every lane of a wavefront makes the same number of trips, so that the ballots see all of them
  for (uint32_t base = blockIdx.x * kBlock + (threadIdx.x & ~63u); base < n_tri; base += gridDim.x * kBlock) {
    const uint32_t t = base + lane;
    MrTri T;
    const int verdict = t < n_tri ? mrast_setup(S, cam, tri, t, n, &T) : kMrEmptyBox;
    c_range += wave_count(verdict == kMrOutOfRange); c_live += wave_count(verdict == kMrNotLive);
    c_clip += wave_count(verdict == kMrClipped); c_degen += wave_count(verdict == kMrDegenerate);
    c_cull += wave_count(verdict == kMrCulled); c_drawn += wave_count(verdict == kMrDrawn || verdict == kMrLarge);
    const unsigned long long large = __ballot(verdict == kMrLarge);
    if (large != 0) {
      c_large += (uint32_t)__popcll(large);
      uint32_t first = 0;
      if (lane == (uint32_t)(__ffsll((long long)large) - 1)) first = atomicAdd(&counters[kMrListLen], (uint32_t)__popcll(large));
      first = __shfl(first, __ffsll((long long)large) - 1);
      // (at most n_tri entries in all: every triangle is listed at most once)
      if (verdict == kMrLarge) list[first + (uint32_t)__popcll(large & ((1ull << lane) - 1ull))] = t;
    }
    if (verdict == kMrDrawn) {
      for (int y = T.y0; y <= T.y1; ++y)
        for (int x = T.x0; x <= T.x1; ++x) {
          const MrW w = mr_weights(T, x, y);
          if (mr_covered(T, w)) mrast_zmin(&zbuf[(size_t)y * cam.W + x], mr_key(mr_persp(T, w).Z, t));
        }
    }
  }
  if (lane == 0) {
    if (c_range) atomicAdd(&counters[kMrOutOfRange], c_range);
    if (c_live) atomicAdd(&counters[kMrNotLive], c_live);
    if (c_clip) atomicAdd(&counters[kMrClipped], c_clip);
    if (c_degen) atomicAdd(&counters[kMrDegenerate], c_degen);
    if (c_cull) atomicAdd(&counters[kMrCulled], c_cull);
    if (c_drawn) atomicAdd(&counters[kMrDrawn], c_drawn);
    if (c_large) atomicAdd(&counters[kMrLarge], c_large);
  }
}

__global__ void __launch_bounds__(kBlock)
k_mrast_large(Surfels S, MrCam cam, const uint32_t* __restrict__ tri, uint32_t n_tri, unsigned long long* __restrict__ zbuf,
              const uint32_t* __restrict__ list, const uint32_t* __restrict__ counters, const DevState* st) {
  const uint32_t n = st->surfel_count, lane = threadIdx.x & 63;
  const uint32_t len = min(counters[kMrListLen], n_tri);
  const uint32_t waves = gridDim.x * (kBlock / 64);
  const int lx = (int)(lane & 7), ly = (int)(lane >> 3);
  for (uint32_t j = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); j < len; j += waves) {
    const uint32_t t = list[j];
    MrTri T;
    if (mrast_setup(S, cam, tri, t, n, &T) != kMrLarge) continue;   // (the verdict k_mrast_small got: the same function)
    for (int ty = T.y0 & ~7; ty <= T.y1; ty += 8)
      for (int tx = T.x0 & ~7; tx <= T.x1; tx += 8) {
        // the tile's pixels inside the box (uniform over the wavefront, as is the whole test)
        const int ax = max(tx, T.x0), bx = min(tx + 7, T.x1), ay = max(ty, T.y0), by = min(ty + 7, T.y1);
        if (mr_tile_outside(T, ax, ay, bx, by)) continue;
        const int x = tx + lx, y = ty + ly;
        if (x < ax || x > bx || y < ay || y > by) continue;
        const MrW w = mr_weights(T, x, y);
        if (mr_covered(T, w)) mrast_zmin(&zbuf[(size_t)y * cam.W + x], mr_key(mr_persp(T, w).Z, t));
      }
  }
}

__global__ void __launch_bounds__(kBlock)
k_mrast_resolve(Surfels S, MrCam cam, VisColor vc, const uint32_t* __restrict__ tri, const unsigned long long* __restrict__ zbuf,
                Img<float> depth, Img<uint32_t> index, Img<float4> normal, Img<uint32_t> color, uint32_t* __restrict__ counters) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const bool inside = x < cam.W && y < cam.H;
  const unsigned long long key = inside ? zbuf[(size_t)y * cam.W + x] : ~0ull;
  const bool empty = key == ~0ull;
  if (inside) {
    const uint32_t t = empty ? kInvalid : (uint32_t)key;
    if (depth.address) depth(y, x) = empty ? 0.0f : __uint_as_float((uint32_t)(key >> 32));
    if (index.address) index(y, x) = t;
    if (normal.address || color.address) {
      float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      uint32_t col = 0u;
      if (!empty) {
        // the winner was drawn: its indices are in range, its corners live and inside the depth range
        const uint32_t a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
        const MrVertex va = mrast_corner(S, cam, a), vb = mrast_corner(S, cam, b), vd = mrast_corner(S, cam, c);
        MrTri T;
        (void)mr_setup(cam, va, vb, vd, &T);
        const MrPersp p = mr_persp(T, mr_weights(T, x, y));
        if (normal.address) {
          float nrm[3];
          if (cam.normal_mode == SMX_MESH_NORMAL_FACE) {
            mr_normal_face(va, vb, vd, nrm);
          } else {
            const float4 na = *S.group(kGroupN, a), nb = *S.group(kGroupN, b), nc = *S.group(kGroupN, c);
            mr_normal_vertex(p, mr_rotate(cam, na.x, na.y, na.z), mr_rotate(cam, nb.x, nb.y, nb.z), mr_rotate(cam, nc.x, nc.y, nc.z), nrm);
          }
          o = make_float4(nrm[0], nrm[1], nrm[2], 0.0f);
        }
        if (color.address) col = mr_color(p, vis_color(S, a, vc), vis_color(S, b, vc), vis_color(S, c, vc));
      }
      if (normal.address) normal(y, x) = o;
      if (color.address) color(y, x) = col;
    }
  }
  const uint32_t covered = wave_count(inside && !empty);
  if ((threadIdx.x & 63) == 0 && covered) atomicAdd(&counters[kMrCovered], covered);
}

}  // namespace

int smx_mesh_render_params_default(smx_mesh_render_params* out) {
  SMX_CHECK_ARG(out != nullptr);
  memset(out, 0, sizeof(*out));
  out->global_T_camera[0] = out->global_T_camera[5] = out->global_T_camera[10] = 1.0f;
  out->near_z = 0.05f; out->far_z = 1000.0f;
  out->normal_mode = SMX_MESH_NORMAL_VERTEX;
  return SMX_OK;
}

int smx_recon_render_mesh(smx_recon r, smx_stream s, const smx_mesh_render_params* p, const uint32_t* triangles, uint32_t n_triangles,
                          int32_t on_device, const smx_buffer_desc* depth, const smx_buffer_desc* index,
                          const smx_buffer_desc* normal, const smx_buffer_desc* color, smx_mesh_render_stats* stats) {
  SMX_CHECK_ARG(r != nullptr && p != nullptr);
  SMX_CALL(check_view(*p));
  SMX_CHECK_ARG(p->cull_back_faces == 0 || p->cull_back_faces == 1);
  SMX_CHECK_ARG(p->normal_mode == SMX_MESH_NORMAL_VERTEX || p->normal_mode == SMX_MESH_NORMAL_FACE);
  SMX_CHECK_ARG(triangles != nullptr || n_triangles == 0);
  SMX_CHECK_ARG(n_triangles <= 0x7FFFFFFFu);   // (the grid-stride loops count in 32 bits)
  const int W = p->width, H = p->height;
  SMX_CHECK_ARG(image_desc_ok_or_null(depth, W, H, 4) && image_desc_ok_or_null(index, W, H, 4) &&
                image_desc_ok_or_null(normal, W, H, 16) && image_desc_ok_or_null(color, W, H, 4));
  SMX_ON_DEVICE(r->device);
  hipStream_t st = (hipStream_t)s;
  const size_t px = (size_t)W * H;
  RenderWork& w = r->render;
  const size_t staged = on_device ? 0 : (size_t)3 * n_triangles;
  SMX_CALL(render_begin(r, st, px, w.list.capacity() < n_triangles || w.in.capacity() < staged || !w.counters.get()));
  SMX_CALL(w.list.reserve(n_triangles));   // (no-ops unless render_begin was told of them: behind its synchronisation)
  SMX_CALL(w.in.reserve(staged));
  if (!w.counters.get()) SMX_CALL(w.counters.alloc(kMrWords, false));
  MrCam cam;
  mr_invert_pose(p->global_T_camera, cam.L);
  cam.fx = p->fx; cam.fy = p->fy; cam.cx = p->cx; cam.cy = p->cy; cam.near_z = p->near_z; cam.far_z = p->far_z;   // (floats widened)
  cam.W = W; cam.H = H; cam.cull_back_faces = p->cull_back_faces; cam.normal_mode = p->normal_mode;
  VisColor vc;
  vc.frame = p->frame_index; vc.window = p->surfel_integration_active_window_size; vc.flags = p->color_flags;
  const uint32_t* tri = nullptr;
  SMX_CALL(w.stamps.begin(st));
  SMX_CALL(stage_in(w.in, triangles, (size_t)3 * n_triangles, on_device != 0, st, &tri));   // (there is room: no allocation)
  uint32_t* cnt = w.counters.get();
  unsigned long long* zbuf = w.zbuf.get();
  SMX_HIP(hipMemsetAsync(cnt, 0, kMrWords * sizeof(uint32_t), st));
  SMX_HIP(hipMemsetAsync(zbuf, 0xFF, px * sizeof(unsigned long long), st));
  if (n_triangles > 0) {
    const int blocks = std::min(div_up(n_triangles, kBlock), 8 * r->cu_count);
    hipLaunchKernelGGL(k_mrast_small, dim3(blocks), dim3(kBlock), 0, st, r->S, cam, tri, n_triangles, zbuf, w.list.get(), cnt, r->st);
  }
  SMX_CALL(w.stamps.mark(st));
  if (n_triangles > 0) {
    // (a wavefront per listed triangle; the list's length is only known on the device)
    const int blocks = std::min(div_up(n_triangles, kBlock / 64), 8 * r->cu_count);
    hipLaunchKernelGGL(k_mrast_large, dim3(blocks), dim3(kBlock), 0, st, r->S, cam, tri, n_triangles, zbuf, w.list.get(), cnt, r->st);
  }
  SMX_CALL(w.stamps.mark(st));
  hipLaunchKernelGGL(k_mrast_resolve, dim3(div_up(W, 64), div_up(H, 4)), dim3(kBlock), 0, st, r->S, cam, vc, tri,
                     zbuf, img_or_null<float>(depth), img_or_null<uint32_t>(index), img_or_null<float4>(normal),
                     img_or_null<uint32_t>(color), cnt);
  SMX_LAUNCH_CHECK();
  SMX_CALL(w.stamps.mark(st));
  SMX_CALL(render_end(r, st));
  w.stamps.publish();
  if (stats) {
    uint32_t h[kMrWords];
    SMX_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SMX_HIP(hipStreamSynchronize(st));
    stats->n_in = n_triangles; stats->n_out_of_range = h[kMrOutOfRange]; stats->n_not_live = h[kMrNotLive];
    stats->n_clipped = h[kMrClipped]; stats->n_degenerate = h[kMrDegenerate]; stats->n_culled = h[kMrCulled];
    stats->n_drawn = h[kMrDrawn]; stats->n_large = h[kMrLarge]; stats->n_covered_pixels = h[kMrCovered];
  }
  return SMX_OK;
}

int smx_recon_debug_mesh_render_timings(smx_recon r, float out_ms[3]) {
  SMX_CHECK_ARG(r != nullptr && out_ms != nullptr);
  SMX_ON_DEVICE(r->device);
  return r->render.stamps.elapsed_ms(out_ms, 3);
}
