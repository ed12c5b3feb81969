// K19 TSDF fusion (include/mi355x_match.h, "TSDF fusion"): depth frames integrated into a truncated signed distance volume,
// the volume raycast into surfel maps of mi_surfel_maps' layout, and the composition of two poses, batched over volumes under
// K18's contract.  The arithmetic is tsdf_math.h's.
//
// K19z  tsdf_reset_kernel      (1, 0) into every voxel, two voxels (16 bytes) per thread.
// K19i  tsdf_integrate_kernel  grid (ceil(nz ny / 4), batch), 256 threads: a wave owns one x-row of the volume and lane l its
//       voxels l, l + 64, ...  A voxel's record is loaded once (8 bytes), lives in two registers across the loop over the
//       frames, and is stored once: 16 bytes of volume traffic per voxel however many frames.  The poses and the active
//       bytes are indexed by (blockIdx.y, frame) only, so they are wave-uniform loads; the depth read is a gather at the
//       voxel's nearest pixel (neighbouring voxels project to neighbouring pixels: cached).
// K19r  tsdf_raycast_kernel    grid (ceil(w / 16), ceil(h / 16), batch), 256 threads: a wave owns an 8 x 8 pixel tile, so
//       that the rays of a wave stay neighbours in the volume and their gathers share cache lines.  A lane marches its ray
//       over the fixed grid of depths, restricted to the range of k whose samples can lie inside the volume's box (the
//       slab test, widened by two samples); a sample is four 16-byte loads (two x-adjacent corners each).
// K19c  tsdf_compose_kernel    one thread per pose pair.
// This file's own: the kernels above and the entry points.  Shared with K22 and K20 through tsdf_shared.h: the grid and camera
// structs and every host check of a volume, a grid, a depth range and an integration.
// No atomics, no memset, nothing allocated; every output element is written.  Built with -ffp-contract=off.
#include "common.h"
#include "tsdf_math.h"
#include "tsdf_shared.h"

#include <math.h>

namespace {

// ---- K19z ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_reset_kernel(float *__restrict__ vol, long long voxels) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, pairs = voxels >> 1;
  if (i < pairs) reinterpret_cast<float4 *>(vol)[i] = make_float4(1.0f, 0.0f, 1.0f, 0.0f);
  if (i == pairs && (voxels & 1)) reinterpret_cast<float2 *>(vol)[voxels - 1] = make_float2(1.0f, 0.0f);
}

// ---- K19i ------------------------------------------------------------------------------------------------------------------
template <typename D>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(float2 *__restrict__ vol, TsdfGrid g, float max_weight,
                                                             const D *__restrict__ depth, int frames, int h, int w, TsdfCam cam,
                                                             const float *__restrict__ r, const float *__restrict__ t,
                                                             const uint8_t *__restrict__ active) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);       // over nz * ny, wave-uniform
  if (row >= g.nz * g.ny) return;
  const int k = row / g.ny, j = row - k * g.ny;
  const float py = tsdf_centre(j, g.voxel_size, g.origin[1]), pz = tsdf_centre(k, g.voxel_size, g.origin[2]);
  float2 *line = vol + ((size_t)b * (size_t)(g.nz * g.ny) + (size_t)row) * (size_t)g.nx;
  const size_t hw = (size_t)h * (size_t)w;
  for (int i = lane; i < g.nx; i += 64) {
    float2 rec = line[i];
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
      const float d = (float)depth[bf * hw + (size_t)(int)py2 * (size_t)w + (size_t)(int)px];   // inside the frame
      tsdf_fuse(d, cam.z_scale, cam.min_depth, cam.max_depth, q[2], g.truncation, max_weight, &rec.x, &rec.y);
    }
    line[i] = rec;
  }
}

// ---- K19r ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const float *__restrict__ vol, TsdfGrid g, float step, int last_k,
                                                           float min_depth, const float *__restrict__ r,
                                                           const float *__restrict__ t, int h, int w,
                                                           const float *__restrict__ k_inv, float4 *__restrict__ vertex,
                                                           float4 *__restrict__ normal) {
  const int b = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= w || y >= h) return;
  float R[9], T[3];
#pragma unroll
  for (int e = 0; e < 9; ++e) R[e] = r[(size_t)b * 9 + e];
#pragma unroll
  for (int e = 0; e < 3; ++e) T[e] = t[(size_t)b * 3 + e];
  const float xn = ((float)x * k_inv[0] + (float)y * k_inv[1]) + k_inv[2];
  const float yn = ((float)x * k_inv[3] + (float)y * k_inv[4]) + k_inv[5];
  const float *volume = vol + (size_t)b * (size_t)g.nz * (size_t)g.ny * (size_t)g.nx * 2;

  // the range of k whose samples can lie inside the box: X_w(s) = s dw + ow per axis against [origin, origin + n voxel_size],
  // widened by two samples.  Samples outside that range have no eight corners, so leaving them out changes nothing.
  float s_in = -INFINITY, s_out = INFINITY;
  const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float dw = (R[a] * xn + R[3 + a] * yn) + R[6 + a];
    const float ow = -((R[a] * T[0] + R[3 + a] * T[1]) + R[6 + a] * T[2]);
    const float lo = g.origin[a], hi = g.origin[a] + (float)n[a] * g.voxel_size;
    const float s1 = (lo - ow) / dw, s2 = (hi - ow) / dw;     // +-inf for a ray along the slab; NaN drops out of fmin / fmax
    if (dw == 0.0f && !(ow >= lo && ow <= hi)) s_out = -INFINITY;
    s_in = fmaxf(s_in, fminf(s1, s2));
    s_out = fminf(s_out, fmaxf(s1, s2));
  }
  const float kf0 = fmaxf(0.0f, floorf((s_in - min_depth) / step) - 2.0f);
  const float kf1 = fminf((float)last_k, ceilf((s_out - min_depth) / step) + 2.0f);

  float4 vo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), no = vo;
  if (kf0 <= kf1) {                                          // false for an empty range and for NaN
    const int k0 = (int)kf0, k1 = (int)kf1;
    bool prev_ok = false;
    float f_prev = 0.0f, s_prev = 0.0f;
    for (int k = k0; k <= k1; ++k) {
      const float s = ((float)k * step) + min_depth;
      float gp[3], f;
      tsdf_grid_point(xn, yn, s, R, T, g.origin, g.voxel_size, gp);
      const bool ok = tsdf_sample(volume, g.nx, g.ny, g.nz, gp, &f);
      if (ok && f <= 0.0f) {
        if (prev_ok && f_prev > 0.0f) {
          const float sh = tsdf_hit(s_prev, step, f_prev, f);
          const float v[3] = {xn * sh, yn * sh, sh};
          float nn[3];
          tsdf_grid_point(xn, yn, sh, R, T, g.origin, g.voxel_size, gp);
          const bool nok = tsdf_normal(volume, g.nx, g.ny, g.nz, gp, R, v, nn);
          vo = make_float4(v[0], v[1], v[2], 1.0f);
          if (nok) no = make_float4(nn[0], nn[1], nn[2], 1.0f);
        }
        break;
      }
      prev_ok = ok;
      f_prev = f;
      s_prev = s;
    }
  }
  const size_t o = ((size_t)b * (size_t)h + (size_t)y) * (size_t)w + (size_t)x;
  vertex[o] = vo;
  normal[o] = no;
}

// ---- K19c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tsdf_compose_kernel(const float *__restrict__ ra, const float *__restrict__ ta,
                                                          const float *__restrict__ rb, const float *__restrict__ tb, int batch,
                                                          float *__restrict__ r, float *__restrict__ t) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  float A[9], a[3], B[9], c[3], Ro[9], to[3];
#pragma unroll
  for (int e = 0; e < 9; ++e) { A[e] = ra[(size_t)b * 9 + e]; B[e] = rb[(size_t)b * 9 + e]; }
#pragma unroll
  for (int e = 0; e < 3; ++e) { a[e] = ta[(size_t)b * 3 + e]; c[e] = tb[(size_t)b * 3 + e]; }
  tsdf_compose(A, a, B, c, Ro, to);
#pragma unroll
  for (int e = 0; e < 9; ++e) r[(size_t)b * 9 + e] = Ro[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) t[(size_t)b * 3 + e] = to[e];
}

}  // namespace

// ---- host (the checks are tsdf_shared.h's) -----------------------------------------------------------------------------------

extern "C" int mi_tsdf_reset(float *volume, int batch, int nz, int ny, int nx, mi_stream_t stream) {
  MI_ENTER();
  if (!volume) return MI_E_NULL;
  if (const int s = tsdf_volume_status(batch, nz, ny, nx)) return s;
  if (!mi_aligned16({volume})) return MI_E_ALIGN;
  const long long voxels = (long long)batch * nz * ny * nx, threads = (voxels >> 1) + 1;
  hipLaunchKernelGGL(tsdf_reset_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, volume, voxels);
  return mi_launch_status();
}

extern "C" int mi_tsdf_integrate(float *volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y,
                                 float origin_z, float voxel_size, float truncation, float max_weight, const void *depth,
                                 int depth_is_u16, int frames, int h, int w, float fx, float fy, float cx, float cy, float z_scale,
                                 float min_depth, float max_depth, const float *r, const float *t, const uint8_t *active,
                                 mi_stream_t stream) {
  MI_ENTER();
  if (!volume || !depth || !r || !t) return MI_E_NULL;
  if (const int s = tsdf_volume_status(batch, nz, ny, nx)) return s;
  if (const int s = tsdf_frames_status(batch, frames, h, w)) return s;
  if (const int s = tsdf_grid_status(origin_x, origin_y, origin_z, voxel_size, truncation)) return s;
  const TsdfCam cam{fx, fy, cx, cy, z_scale, min_depth, max_depth};
  if (const int s = tsdf_fusion_status(max_weight, cam)) return s;
  if (!mi_aligned16({volume})) return MI_E_ALIGN;
  const TsdfGrid g{nx, ny, nz, {origin_x, origin_y, origin_z}, voxel_size, truncation};
  const dim3 grid((unsigned)ceil_div(nz * ny, 4), (unsigned)batch);
  float2 *vol = reinterpret_cast<float2 *>(volume);
  if (depth_is_u16)
    hipLaunchKernelGGL(tsdf_integrate_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, vol, g, max_weight,
                       static_cast<const uint16_t *>(depth), frames, h, w, cam, r, t, active);
  else
    hipLaunchKernelGGL(tsdf_integrate_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, vol, g, max_weight,
                       static_cast<const float *>(depth), frames, h, w, cam, r, t, active);
  return mi_launch_status();
}

extern "C" int mi_tsdf_raycast(const float *volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y,
                               float origin_z, float voxel_size, float truncation, float step_fraction, const float *r,
                               const float *t, int h, int w, const float *k_inv, float min_depth, float max_depth,
                               float *vertex_out, float *normal_out, mi_stream_t stream) {
  MI_ENTER();
  if (!volume || !r || !t || !k_inv || !vertex_out || !normal_out) return MI_E_NULL;
  if (const int s = tsdf_volume_status(batch, nz, ny, nx)) return s;
  if (h < 3 || w < 3) return MI_E_SHAPE;
  if ((double)batch * (double)h * (double)w >= 2147483648.0) return MI_E_SHAPE;
  if (const int s = tsdf_grid_status(origin_x, origin_y, origin_z, voxel_size, truncation)) return s;
  if (!tsdf_positive(step_fraction) || step_fraction > 1.0f || !tsdf_depth_range_ok(min_depth, max_depth)) return MI_E_PARAM;
  const float step = step_fraction * truncation;
  const float count = ceilf((max_depth - min_depth) / step);
  if (!tsdf_positive(step) || !(count < 16777216.0f)) return MI_E_PARAM;   // k must stay exact in float32
  if (!mi_aligned16({volume, vertex_out, normal_out})) return MI_E_ALIGN;
  const TsdfGrid g{nx, ny, nz, {origin_x, origin_y, origin_z}, voxel_size, truncation};
  const dim3 grid((unsigned)ceil_div(w, 16), (unsigned)ceil_div(h, 16), (unsigned)batch);
  hipLaunchKernelGGL(tsdf_raycast_kernel, grid, dim3(256), 0, (hipStream_t)stream, volume, g, step, (int)count, min_depth, r, t, h,
                     w, k_inv, reinterpret_cast<float4 *>(vertex_out), reinterpret_cast<float4 *>(normal_out));
  return mi_launch_status();
}

extern "C" int mi_pose_compose(const float *ra, const float *ta, const float *rb, const float *tb, int batch, float *r, float *t,
                               mi_stream_t stream) {
  MI_ENTER();
  if (!ra || !ta || !rb || !tb || !r || !t) return MI_E_NULL;
  if (batch < 1) return MI_E_SHAPE;
  hipLaunchKernelGGL(tsdf_compose_kernel, dim3((unsigned)ceil_div(batch, 64)), dim3(64), 0, (hipStream_t)stream, ra, ta, rb, tb,
                     batch, r, t);
  return mi_launch_status();
}
