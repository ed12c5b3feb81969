// K22 TSDF intensity (include/mi355x_match.h, "TSDF intensity"): a second volume of (gray, gweight) records beside K19's,
// fused from gray frames in the same pass as the depth, and gathered at raycast vertices (the model's intensity map for
// K21) or at mesh vertices (K20's per-vertex gray).  The arithmetic is tsdf_gray_math.h's on top of tsdf_math.h's; K19's
// kernels and bits are untouched.
//
// K22z  tsdf_gray_reset_kernel      (0, 0) into every record, two records (16 bytes) per thread.
// K22i  tsdf_integrate_gray_kernel  K19i's form: grid (ceil(nz ny / 4), batch), 256 threads, a wave per x-row, lane l the voxels
//       l, l + 64, ...; the (tsdf, weight) record lives in two registers across the loop over the frames.  The intensity
//       record is loaded LAZILY, on the first frame whose gate passes, and stored only if it was loaded: only voxels inside
//       the truncation band ever touch it, so the common voxel still costs K19's 16 bytes.  The gray read is a gather at the
//       depth sample's own pixel.  Four instances: depth float / uint16 x gray float / uint8.
// K22s  tsdf_sample_gray_kernel     grid (ceil(n / 256), batch), one thread per point on a linear index (neighbouring points of
//       a raycast row or of a mesh are neighbours in the volume); a point is four 16-byte loads (two x-adjacent corners each).
// This file's own: the kernels above and the entry points.  K19's, through tsdf_shared.h: the grid and camera structs and
// every host check of a volume, a grid, a depth range and an integration.
// No atomics, no memset, nothing allocated; every output element is written.  Built with -ffp-contract=off.
#include "common.h"
#include "tsdf_gray_math.h"
#include "tsdf_shared.h"

#include <math.h>

namespace {

// ---- K22z ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_gray_reset_kernel(float *__restrict__ ivol, long long voxels) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, pairs = voxels >> 1;
  if (i < pairs) reinterpret_cast<float4 *>(ivol)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i == pairs && (voxels & 1)) reinterpret_cast<float2 *>(ivol)[voxels - 1] = make_float2(0.0f, 0.0f);
}

// ---- K22i ------------------------------------------------------------------------------------------------------------------
template <typename D, typename G>
__global__ __launch_bounds__(256) void tsdf_integrate_gray_kernel(float2 *__restrict__ vol, float2 *__restrict__ ivol, TsdfGrid g,
                                                                  float max_weight, const D *__restrict__ depth,
                                                                  const G *__restrict__ gray, int frames, int h, int w,
                                                                  TsdfCam cam, const float *__restrict__ r,
                                                                  const float *__restrict__ t,
                                                                  const uint8_t *__restrict__ active) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);       // over nz * ny, wave-uniform
  if (row >= g.nz * g.ny) return;
  const int k = row / g.ny, j = row - k * g.ny;
  const float py = tsdf_centre(j, g.voxel_size, g.origin[1]), pz = tsdf_centre(k, g.voxel_size, g.origin[2]);
  const size_t first = ((size_t)b * (size_t)(g.nz * g.ny) + (size_t)row) * (size_t)g.nx;
  float2 *line = vol + first, *iline = ivol + first;
  const size_t hw = (size_t)h * (size_t)w;
  for (int i = lane; i < g.nx; i += 64) {
    float2 rec = line[i], irec = make_float2(0.0f, 0.0f);
    bool loaded = false;
    const float p[3] = {tsdf_centre(i, g.voxel_size, g.origin[0]), py, pz};
    for (int f = 0; f < frames; ++f) {
      const size_t bf = (size_t)b * (size_t)frames + (size_t)f;
      if (active && active[bf] == 0) continue;               // uniform over the workgroup
      const float *R = r + bf * 9, *T = t + bf * 3;
      float Rr[9], q[3], px, py2;
#pragma unroll
      for (int e = 0; e < 9; ++e) Rr[e] = R[e];
      icp_rotate(Rr, p, q);
      q[0] += T[0]; q[1] += T[1]; q[2] += T[2];
      if (!icp_project(q, cam.fx, cam.fy, cam.cx, cam.cy, w, h, &px, &py2)) continue;
      const size_t pixel = bf * hw + (size_t)(int)py2 * (size_t)w + (size_t)(int)px;             // inside the frame
      const float d = (float)depth[pixel];
      const bool fused = tsdf_fuse(d, cam.z_scale, cam.min_depth, cam.max_depth, q[2], g.truncation, max_weight, &rec.x, &rec.y);
      if (!tsdf_gray_band(fused, d, cam.z_scale, q[2], g.truncation)) continue;
      const float gv = (float)gray[pixel];
      if (!(fabsf(gv) < INFINITY)) continue;
      if (!loaded) {
        irec = iline[i];
        loaded = true;
      }
      tsdf_gray_fuse(gv, max_weight, &irec.x, &irec.y);
    }
    line[i] = rec;
    if (loaded) iline[i] = irec;
  }
}

// ---- K22s ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_sample_gray_kernel(const float *__restrict__ ivol, TsdfGrid g,
                                                               const float4 *__restrict__ points, int n,
                                                               const float *__restrict__ r, const float *__restrict__ t,
                                                               float4 *__restrict__ out) {
  const int b = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t o = (size_t)b * (size_t)n + (size_t)i;
  const float4 pt = points[o];
  float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (pt.w != 0.0f && fabsf(pt.x) < INFINITY && fabsf(pt.y) < INFINITY && fabsf(pt.z) < INFINITY) {
    float xw[3] = {pt.x, pt.y, pt.z};
    if (r) {                                                 // uniform over the launch
      float R[9], T[3];
#pragma unroll
      for (int e = 0; e < 9; ++e) R[e] = r[(size_t)b * 9 + e];
#pragma unroll
      for (int e = 0; e < 3; ++e) T[e] = t[(size_t)b * 3 + e];
      const float p[3] = {pt.x, pt.y, pt.z};
      tsdf_gray_world(p, R, T, xw);
    }
    const float *volume = ivol + (size_t)b * (size_t)g.nz * (size_t)g.ny * (size_t)g.nx * 2;
    float I;
    if (tsdf_gray_sample(volume, g.nx, g.ny, g.nz, xw, g.origin, g.voxel_size, &I)) res = make_float4(I, 0.0f, 0.0f, 1.0f);
  }
  out[o] = res;
}

// ---- host (the checks are K19's own: tsdf_shared.h) ---------------------------------------------------------------------------
template <typename D>
void launch_integrate_gray(dim3 grid, hipStream_t stream, float2 *vol, float2 *ivol, const TsdfGrid &g, float max_weight,
                           const D *depth, const void *gray, int gray_is_u8, int frames, int h, int w, const TsdfCam &cam,
                           const float *r, const float *t, const uint8_t *active) {
  if (gray_is_u8)
    hipLaunchKernelGGL((tsdf_integrate_gray_kernel<D, uint8_t>), grid, dim3(256), 0, stream, vol, ivol, g, max_weight, depth,
                       static_cast<const uint8_t *>(gray), frames, h, w, cam, r, t, active);
  else
    hipLaunchKernelGGL((tsdf_integrate_gray_kernel<D, float>), grid, dim3(256), 0, stream, vol, ivol, g, max_weight, depth,
                       static_cast<const float *>(gray), frames, h, w, cam, r, t, active);
}

}  // namespace

extern "C" int mi_tsdf_gray_reset(float *intensity_volume, int batch, int nz, int ny, int nx, mi_stream_t stream) {
  MI_ENTER();
  if (!intensity_volume) return MI_E_NULL;
  if (const int s = tsdf_volume_status(batch, nz, ny, nx)) return s;
  if (!mi_aligned16({intensity_volume})) return MI_E_ALIGN;
  const long long voxels = (long long)batch * nz * ny * nx, threads = (voxels >> 1) + 1;
  hipLaunchKernelGGL(tsdf_gray_reset_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     intensity_volume, voxels);
  return mi_launch_status();
}

extern "C" int mi_tsdf_integrate_gray(float *volume, float *intensity_volume, int batch, int nz, int ny, int nx, float origin_x,
                                      float origin_y, float origin_z, float voxel_size, float truncation, float max_weight,
                                      const void *depth, int depth_is_u16, const void *gray, int gray_is_u8, int frames, int h,
                                      int w, float fx, float fy, float cx, float cy, float z_scale, float min_depth,
                                      float max_depth, const float *r, const float *t, const uint8_t *active,
                                      mi_stream_t stream) {
  MI_ENTER();
  if (!volume || !intensity_volume || !depth || !gray || !r || !t) return MI_E_NULL;
  if (const int s = tsdf_volume_status(batch, nz, ny, nx)) return s;
  if (const int s = tsdf_frames_status(batch, frames, h, w)) return s;
  if (const int s = tsdf_grid_status(origin_x, origin_y, origin_z, voxel_size, truncation)) return s;
  const TsdfCam cam{fx, fy, cx, cy, z_scale, min_depth, max_depth};
  if (const int s = tsdf_fusion_status(max_weight, cam)) return s;
  if (!mi_aligned16({volume, intensity_volume})) return MI_E_ALIGN;
  const TsdfGrid g{nx, ny, nz, {origin_x, origin_y, origin_z}, voxel_size, truncation};
  const dim3 grid((unsigned)ceil_div(nz * ny, 4), (unsigned)batch);
  float2 *vol = reinterpret_cast<float2 *>(volume), *ivol = reinterpret_cast<float2 *>(intensity_volume);
  if (depth_is_u16)
    launch_integrate_gray(grid, (hipStream_t)stream, vol, ivol, g, max_weight, static_cast<const uint16_t *>(depth), gray, gray_is_u8,
                          frames, h, w, cam, r, t, active);
  else
    launch_integrate_gray(grid, (hipStream_t)stream, vol, ivol, g, max_weight, static_cast<const float *>(depth), gray, gray_is_u8,
                          frames, h, w, cam, r, t, active);
  return mi_launch_status();
}

extern "C" int mi_tsdf_sample_gray(const float *intensity_volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y,
                                   float origin_z, float voxel_size, const float *points, int n, const float *r, const float *t,
                                   float *intensity_out, mi_stream_t stream) {
  MI_ENTER();
  if (!intensity_volume || !points || !intensity_out || (r == nullptr) != (t == nullptr)) return MI_E_NULL;
  if (const int s = tsdf_volume_status(batch, nz, ny, nx)) return s;
  if (n < 1 || (double)batch * (double)n >= 2147483648.0) return MI_E_SHAPE;
  if (const int s = tsdf_origin_status(origin_x, origin_y, origin_z, voxel_size)) return s;
  if (!mi_aligned16({intensity_volume, points, intensity_out})) return MI_E_ALIGN;
  const TsdfGrid g{nx, ny, nz, {origin_x, origin_y, origin_z}, voxel_size, 0.0f};
  const dim3 grid((unsigned)(((long long)n + 255) / 256), (unsigned)batch);
  hipLaunchKernelGGL(tsdf_sample_gray_kernel, grid, dim3(256), 0, (hipStream_t)stream, intensity_volume, g,
                     reinterpret_cast<const float4 *>(points), n, r, t, reinterpret_cast<float4 *>(intensity_out));
  return mi_launch_status();
}
