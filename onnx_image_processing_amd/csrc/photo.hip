// K21 direct RGB-D refinement (include/mi355x_match.h, "direct RGB-D refinement"): a photometric term joined to K18's
// point-to-plane system, batched over pairs under K18's contract.  The arithmetic is photo_math.h's and icp_math.h's; the
// geometric half is K18's own kernels (icp.hip), launched through icp_shared.h into a slab array of their own.
//
// K21m  photo_intensity_kernel  one thread per pixel: the gray value and its central differences from the four axis
//       neighbours (5 reads, cached); one 16-byte record per pixel: (I, gx, gy, valid).
// K21r  photo_reduce_kernel     the slab reduction of icp_shared.h (K18r's slabs, lanes and record) around the photometric
//       row, which is this file's.  Streamed per sample: frame 1's vertex and intensity records; gathered at clamped
//       addresses: the four intensity records of the bilinear footprint in frame 2 and frame 2's vertex at the nearest
//       pixel.  A rejected sample adds zeros.
// K21s  rgbd_solve_kernel       one wave per pair: lane c < 29 adds column c of the pair's geometric and photometric slab
//       records in slab order (float64); lane 0 forms the joint sums, then solves and updates the pose (mode STEP), or
//       writes the outputs (mode FINAL); mode SUMS writes the 29 photometric sums.  The column sum, the step and the pose
//       write are icp_shared.h's.
// A frozen pair is K18's: its state word is set, and K18r / K21r / K21s return at once for it in later iterations.
// This file's own: K21m, the row of K21r, the joint sums and the statistics of K21s, and the entry points.  Shared with
// K18 through icp_shared.h: the sample index and the tail of the reduction, the solve step, the workspace (with a second
// slab array), the checks and the refine driver.
// Built with -ffp-contract=off; every sum has a fixed order: bitwise reproducible, alone or in a batch.
#include "common.h"
#include "icp_shared.h"
#include "photo_math.h"

#include <math.h>

namespace {

// ---- K21m ------------------------------------------------------------------------------------------------------------------
template <typename G>
__global__ __launch_bounds__(256) void photo_intensity_kernel(const G *__restrict__ gray, int h, int w, long long total,
                                                              float4 *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int hw = h * w;
  const int p = (int)(i % hw), y = p / w, x = p - y * w;
  const bool interior = x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2;
  const float c = (float)gray[i];
  float l = 0.0f, r = 0.0f, u = 0.0f, d = 0.0f;
  if (interior) {
    l = (float)gray[i - 1];
    r = (float)gray[i + 1];
    u = (float)gray[i - w];
    d = (float)gray[i + w];
  }
  float rec[4];
  photo_record(c, l, r, u, d, interior, rec);
  out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

// ---- K21r ------------------------------------------------------------------------------------------------------------------
// icp_shared.h's sequence around the photometric row (its loads: the file header)
__global__ __launch_bounds__(ICP_THREADS) void photo_reduce_kernel(const float4 *__restrict__ vertex1, const float4 *__restrict__ inten1,
                                                                   const float4 *__restrict__ vertex2, const float4 *__restrict__ inten2,
                                                                   const float *__restrict__ r, const float *__restrict__ t,
                                                                   const double *__restrict__ pose64, const int *__restrict__ state,
                                                                   int h, int w, int stride, int ws, int samples, int max_slabs,
                                                                   IcpCam cam, float dist_thr, float int_thr,
                                                                   double *__restrict__ slabs) {
  __shared__ double part[4][ICP_REC];
  const int b = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  if (state && state[b] != 0) return;                        // frozen pair (uniform over the workgroup)
  float R[9], T[3];
  if (pose64) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (float)pose64[(size_t)b * 12 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) T[k] = (float)pose64[(size_t)b * 12 + 9 + k];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = r[(size_t)b * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) T[k] = t[(size_t)b * 3 + k];
  }
  const size_t frame = (size_t)b * (size_t)h * (size_t)w;
  float acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0f;
  int count = 0;
#pragma unroll
  for (int it = 0; it < ICP_PER_LANE; ++it) {
    bool in;
    const size_t i1 = frame + icp_sample_pixel(slab, it, tid, samples, ws, stride, w, &in);
    const float4 v1 = vertex1[i1], g1 = inten1[i1];
    const float p1[3] = {v1.x, v1.y, v1.z};
    float q[3], x0, y0, a, bb, px, py;
    icp_rotate(R, p1, q);
    q[0] += T[0]; q[1] += T[1]; q[2] += T[2];
    bool ok = in && v1.w != 0.0f && g1.w != 0.0f;
    ok = photo_footprint(q, cam.fx, cam.fy, cam.cx, cam.cy, w, h, &x0, &y0, &a, &bb, &px, &py) && ok;
    // when ok: 0 <= x0 <= w - 2, 0 <= y0 <= h - 2 and (px, py) is one of the footprint's pixels; else pixel 0, whose
    // footprint is inside the frame as well (h, w >= 3)
    const int ix = ok ? (int)x0 : 0, iy = ok ? (int)y0 : 0, nx = ok ? (int)px : 0, ny = ok ? (int)py : 0;
    const size_t i00 = frame + (size_t)iy * (size_t)w + (size_t)ix;
    const float4 c00 = inten2[i00], c01 = inten2[i00 + 1], c10 = inten2[i00 + (size_t)w], c11 = inten2[i00 + (size_t)w + 1];
    const float4 v2 = vertex2[frame + (size_t)ny * (size_t)w + (size_t)nx];
    const float f00[4] = {c00.x, c00.y, c00.z, c00.w}, f01[4] = {c01.x, c01.y, c01.z, c01.w};
    const float f10[4] = {c10.x, c10.y, c10.z, c10.w}, f11[4] = {c11.x, c11.y, c11.z, c11.w};
    const float p2[4] = {v2.x, v2.y, v2.z, v2.w};
    float J[6], res;
    ok = photo_row(q, g1.x, f00, f01, f10, f11, a, bb, p2, cam.fx, cam.fy, dist_thr, int_thr, J, &res) && ok;
    if (!ok) {
#pragma unroll
      for (int k = 0; k < 6; ++k) J[k] = 0.0f;
      res = 0.0f;
    }
    icp_accumulate(J, res, acc);
    count += ok ? 1 : 0;
  }
  icp_store_slab(acc, count, part, slabs + ((size_t)b * max_slabs + slab) * ICP_REC);
}

// ---- K21s ------------------------------------------------------------------------------------------------------------------
struct RgbdOut {
  float *r, *t, *information, *rmse, *rmse_photo;
  int *count, *count_photo, *steps;
  uint8_t *ok;
  double *sums;
};

// slabs_g / slabs_p: either may be null (mode SUMS has no geometric half, photo_weight 0 no photometric one): its sums
// are then zeros and take no part in the joint system.
__global__ __launch_bounds__(64) void rgbd_solve_kernel(const double *__restrict__ slabs_g, const double *__restrict__ slabs_p,
                                                        int nslabs, int max_slabs, int mode, int min_count, double w2,
                                                        double *__restrict__ pose, int *__restrict__ state,
                                                        int *__restrict__ steps, RgbdOut out) {
  __shared__ double sg[ICP_REC], sp[ICP_REC];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (mode == ICP_MODE_STEP && state[b] != 0) return;        // frozen pair
  if (lane < ICP_SUMS) {
    const double g = slabs_g ? icp_column_sum(slabs_g, b, nslabs, max_slabs, lane) : 0.0;
    const double p = slabs_p ? icp_column_sum(slabs_p, b, nslabs, max_slabs, lane) : 0.0;
    sg[lane] = g;
    sp[lane] = p;
    if (mode == ICP_MODE_SUMS) out.sums[(size_t)b * ICP_SUMS + lane] = p;
  }
  __syncthreads();
  if (mode == ICP_MODE_SUMS || lane != 0) return;
  double s[ICP_SUMS];
  photo_joint(sg, slabs_p ? sp : nullptr, w2, s);
  if (mode == ICP_MODE_STEP) {
    icp_step(s, min_count, b, pose, state, steps);
    return;
  }
  // FINAL: the statistics of the returned pose
  const int cnt_g = (int)sg[28], cnt_p = (int)sp[28];
  bool finite = true;
  for (int k = 0; k < ICP_SUMS; ++k) finite = finite && fabs(s[k]) < INFINITY && fabs(sg[k]) < INFINITY && fabs(sp[k]) < INFINITY;
  const bool good = finite && state[b] == 0 && cnt_g + cnt_p >= min_count;
  icp_write_pose(s, finite, b, pose, out.r, out.t, out.information);
  out.rmse[b] = (finite && cnt_g > 0) ? (float)sqrt(sg[27] / (double)cnt_g) : 0.0f;
  out.count[b] = finite ? cnt_g : 0;
  out.rmse_photo[b] = (finite && cnt_p > 0) ? (float)sqrt(sp[27] / (double)cnt_p) : 0.0f;
  out.count_photo[b] = finite ? cnt_p : 0;
  out.steps[b] = steps[b];
  out.ok[b] = good ? 1 : 0;
}

// ---- host: the workspace is K18's with two slab arrays, slabs[0] the geometric records, slabs[1] the photometric ones ------------
// K21r's maps and gates
struct PhotoMaps {
  const float4 *vertex1, *inten1, *vertex2, *inten2;
  float dist_thr, int_thr;
};
PhotoMaps photo_maps(const float *vertex1, const float *intensity1, const float *vertex2, const float *intensity2,
                     float distance_threshold, float intensity_threshold) {
  return PhotoMaps{reinterpret_cast<const float4 *>(vertex1), reinterpret_cast<const float4 *>(intensity1),
                   reinterpret_cast<const float4 *>(vertex2), reinterpret_cast<const float4 *>(intensity2), distance_threshold,
                   intensity_threshold};
}

int photo_reduce_launch(const PhotoMaps &m, const IcpReduceJob &job, int batch, hipStream_t s) {
  hipLaunchKernelGGL(photo_reduce_kernel, dim3((unsigned)job.nslabs, (unsigned)batch), dim3(ICP_THREADS), 0, s, m.vertex1,
                     m.inten1, m.vertex2, m.inten2, job.r, job.t, job.pose64, job.state, job.h, job.w, job.stride, job.ws,
                     job.samples, job.max_slabs, job.cam, m.dist_thr, m.int_thr, job.slabs);
  return mi_launch_status();
}

int rgbd_solve_launch(const double *slabs_g, const double *slabs_p, const IcpReduceJob &job, int batch, int mode, int min_count,
                      double w2, const IcpWork &k, RgbdOut out, hipStream_t s) {
  hipLaunchKernelGGL(rgbd_solve_kernel, dim3((unsigned)batch), dim3(64), 0, s, slabs_g, slabs_p, job.nslabs, job.max_slabs, mode,
                     min_count, w2, k.pose, k.state, k.steps, out);
  return mi_launch_status();
}

}  // namespace

extern "C" int mi_intensity_maps(const void *gray, int gray_is_u8, int batch, int h, int w, float *intensity_out,
                                 mi_stream_t stream) {
  MI_ENTER();
  if (!gray || !intensity_out) return MI_E_NULL;
  if (const int s = icp_shape_status(batch, h, w)) return s;
  if (!mi_aligned16({intensity_out})) return MI_E_ALIGN;
  const long long total = (long long)batch * h * w;
  const dim3 grid((unsigned)((total + 255) / 256));
  float4 *o = reinterpret_cast<float4 *>(intensity_out);
  if (gray_is_u8)
    hipLaunchKernelGGL(photo_intensity_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t *>(gray),
                       h, w, total, o);
  else
    hipLaunchKernelGGL(photo_intensity_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const float *>(gray), h,
                       w, total, o);
  return mi_launch_status();
}

extern "C" size_t mi_rgbd_workspace_bytes(int batch, int h, int w) {
  if (icp_shape_status(batch, h, w) != MI_OK) return 0;
  return icp_carve(nullptr, batch, h, w, 2).total;
}

extern "C" int mi_photo_linearise(const float *vertex1, const float *intensity1, const float *vertex2, const float *intensity2,
                                  const float *r, const float *t, int batch, int h, int w, float fx, float fy, float cx, float cy,
                                  int stride, float distance_threshold, float intensity_threshold, double *sums, void *workspace,
                                  size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!vertex1 || !intensity1 || !vertex2 || !intensity2 || !r || !t || !sums || !workspace) return MI_E_NULL;
  if (const int s = icp_shape_status(batch, h, w)) return s;
  if (!icp_stride_ok(stride)) return MI_E_PARAM;
  if (const int s = icp_gate_status(fx, fy, cx, cy, distance_threshold, 1.0f)) return s;   // no angle gate here
  if (!icp_positive(intensity_threshold)) return MI_E_PARAM;
  if (!mi_aligned16({workspace, vertex1, intensity1, vertex2, intensity2})) return MI_E_ALIGN;
  if (workspace_bytes < mi_rgbd_workspace_bytes(batch, h, w)) return MI_E_CAPACITY;
  const IcpWork k = icp_carve(workspace, batch, h, w, 2);
  hipStream_t s = (hipStream_t)stream;
  const IcpReduceJob job = icp_reduce_job(r, t, nullptr, nullptr, h, w, stride, IcpCam{fx, fy, cx, cy}, k.max_slabs, k.slabs[1]);
  if (const int e = photo_reduce_launch(photo_maps(vertex1, intensity1, vertex2, intensity2, distance_threshold, intensity_threshold),
                                        job, batch, s))
    return e;
  RgbdOut out = {};
  out.sums = sums;
  return rgbd_solve_launch(nullptr, k.slabs[1], job, batch, ICP_MODE_SUMS, 0, 0.0, k, out, s);
}

extern "C" int mi_rgbd_refine(const float *vertex1, const float *normal1, const float *intensity1, const float *vertex2,
                              const float *normal2, const float *intensity2, const float *r0, const float *t0, int batch, int h,
                              int w, float fx, float fy, float cx, float cy, const int32_t *strides, const int32_t *iterations,
                              int stages, float distance_threshold, float angle_threshold, float photo_weight,
                              float intensity_threshold, int min_correspondences, float *r, float *t, float *information,
                              float *rmse, int32_t *count, float *rmse_photo, int32_t *count_photo, int32_t *steps, uint8_t *ok,
                              void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!vertex1 || !normal1 || !intensity1 || !vertex2 || !normal2 || !intensity2 || !r0 || !t0 || !strides || !iterations || !r ||
      !t || !information || !rmse || !count || !rmse_photo || !count_photo || !steps || !ok || !workspace)
    return MI_E_NULL;
  if (const int s = icp_shape_status(batch, h, w)) return s;
  if (const int s = icp_schedule_status(strides, iterations, stages, min_correspondences)) return s;
  if (const int s = icp_gate_status(fx, fy, cx, cy, distance_threshold, angle_threshold)) return s;
  if (!(photo_weight >= 0.0f) || !(photo_weight < INFINITY) || !icp_positive(intensity_threshold)) return MI_E_PARAM;
  if (!mi_aligned16({workspace, vertex1, normal1, intensity1, vertex2, normal2, intensity2})) return MI_E_ALIGN;
  if (workspace_bytes < mi_rgbd_workspace_bytes(batch, h, w)) return MI_E_CAPACITY;
  const IcpWork k = icp_carve(workspace, batch, h, w, 2);
  hipStream_t s = (hipStream_t)stream;
  const IcpMaps geo = icp_maps(vertex1, normal1, vertex2, normal2, distance_threshold, angle_threshold);
  const PhotoMaps pho = photo_maps(vertex1, intensity1, vertex2, intensity2, distance_threshold, intensity_threshold);
  const bool photo = photo_weight != 0.0f;
  const double w2 = photo_weight2(photo_weight);
  if (const int e = icp_init_launch(r0, t0, batch, k.pose, k.state, k.steps, s)) return e;
  const RgbdOut out{r, t, information, rmse, rmse_photo, count, count_photo, steps, ok, nullptr};
  // one joint linearisation from the workspace's pose: K18r, K21r (when `photo`), then K21s in `mode`
  return icp_refine_drive(strides, iterations, stages, [&](int stride, int mode) {
    IcpReduceJob job = icp_reduce_job(nullptr, nullptr, k.pose, mode == ICP_MODE_STEP ? k.state : nullptr, h, w, stride,
                                      IcpCam{fx, fy, cx, cy}, k.max_slabs, k.slabs[0]);
    if (const int e = icp_reduce_launch(geo, job, batch, s)) return e;
    job.slabs = k.slabs[1];
    if (photo)
      if (const int e = photo_reduce_launch(pho, job, batch, s)) return e;
    return rgbd_solve_launch(k.slabs[0], photo ? k.slabs[1] : nullptr, job, batch, mode, min_correspondences, w2, k,
                             mode == ICP_MODE_FINAL ? out : RgbdOut{}, s);
  });
}
