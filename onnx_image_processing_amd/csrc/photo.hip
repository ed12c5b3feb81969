// K21 direct RGB-D refinement (include/mi355x_match.h, "direct RGB-D refinement"): a photometric term joined to K18's
// point-to-plane system, batched over pairs under K18's contract.  The arithmetic is photo_math.h's and icp_math.h's; the
// geometric half is K18's own kernels (icp.hip), launched through icp_shared.h into a slab array of their own.
//
// K21m  photo_intensity_kernel  one thread per pixel: the gray value and its central differences from the four axis
//       neighbours (5 reads, cached); one 16-byte record per pixel: (I, gx, gy, valid).
// K21r  photo_reduce_kernel     K18r's skeleton: grid (slabs, pairs), 256 threads, the same slabs of 2048 sampled pixels, lane
//       l takes the samples l, l + 256, ... (8 of them) into 28 float32 accumulators and an integer count.  Streamed per
//       sample: frame 1's vertex and intensity records; gathered at clamped addresses: the four intensity records of the
//       bilinear footprint in frame 2 and frame 2's vertex at the nearest pixel.  A rejected sample adds zeros, so the 8
//       iterations carry no branch.  Then wave_sum_dpp per accumulator, the 4 waves through LDS in wave order in float64
//       and 29 float64 partials stored with plain stores into the slab's 256-byte record.  No atomics.
// K21s  rgbd_solve_kernel       one wave per pair: lane c < 29 adds column c of the pair's geometric and photometric slab
//       records in slab order (float64); lane 0 forms the joint sums, then solves and updates the pose (mode STEP), or
//       writes the outputs (mode FINAL); mode SUMS writes the 29 photometric sums.
// A frozen pair is K18's: its state word is set, and K18r / K21r / K21s return at once for it in later iterations.
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
// The pose comes from r / t (float32, mi_photo_linearise) or, when pose64 is given, from the workspace's float64 pose
// rounded to float32 (mi_rgbd_refine): K18r's convention.
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
    const int s = slab * ICP_SLAB + it * ICP_THREADS + tid;
    const bool in = s < samples;
    const int sc = in ? s : 0;                               // a clamped, always valid address
    const int ys = sc / ws, xs = sc - ys * ws;
    const size_t i1 = frame + (size_t)(ys * stride) * (size_t)w + (size_t)(xs * stride);
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
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 28; ++k) {
    const float sum = wave_sum_dpp(acc[k]);
    if (lane == 0) part[wave][k] = (double)sum;
  }
  int c = count;                                             // integers: exact in any order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) part[wave][28] = (double)c;
  __syncthreads();
  if (tid < ICP_SUMS)
    slabs[((size_t)b * max_slabs + slab) * ICP_REC + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// ---- K21s ------------------------------------------------------------------------------------------------------------------
enum { RGBD_MODE_STEP = 0, RGBD_MODE_SUMS = 1, RGBD_MODE_FINAL = 2 };

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
  if (mode == RGBD_MODE_STEP && state[b] != 0) return;       // frozen pair
  if (lane < ICP_SUMS) {
    double g = 0.0, p = 0.0;
    if (slabs_g)
      for (int k = 0; k < nslabs; ++k) g += slabs_g[((size_t)b * max_slabs + k) * ICP_REC + lane];
    if (slabs_p)
      for (int k = 0; k < nslabs; ++k) p += slabs_p[((size_t)b * max_slabs + k) * ICP_REC + lane];
    sg[lane] = g;
    sp[lane] = p;
    if (mode == RGBD_MODE_SUMS) out.sums[(size_t)b * ICP_SUMS + lane] = p;
  }
  __syncthreads();
  if (mode == RGBD_MODE_SUMS || lane != 0) return;
  double s[ICP_SUMS];
  photo_joint(sg, slabs_p ? sp : nullptr, w2, s);
  if (mode == RGBD_MODE_STEP) {
    double x[6], ratio;
    if (icp_solve(s, min_count, x, &ratio)) {
      double p[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) p[k] = pose[(size_t)b * 12 + k];
      icp_update_pose(p, x);
      bool finite = true;
#pragma unroll
      for (int k = 0; k < 12; ++k) finite = finite && fabs(p[k]) < INFINITY;
      if (finite) {
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[(size_t)b * 12 + k] = p[k];
        steps[b] += 1;
        return;
      }
    }
    state[b] = 1;
    return;
  }
  // FINAL: the statistics of the returned pose
  const int cnt_g = (int)sg[28], cnt_p = (int)sp[28];
  bool finite = true;
  for (int k = 0; k < ICP_SUMS; ++k) finite = finite && fabs(s[k]) < INFINITY && fabs(sg[k]) < INFINITY && fabs(sp[k]) < INFINITY;
  const bool good = finite && state[b] == 0 && cnt_g + cnt_p >= min_count;
  for (int k = 0; k < 9; ++k) out.r[(size_t)b * 9 + k] = (float)pose[(size_t)b * 12 + k];
  for (int k = 0; k < 3; ++k) out.t[(size_t)b * 3 + k] = (float)pose[(size_t)b * 12 + 9 + k];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      const float v = finite ? (float)s[k] : 0.0f;
      out.information[(size_t)b * 36 + i * 6 + j] = v;
      out.information[(size_t)b * 36 + j * 6 + i] = v;
      ++k;
    }
  out.rmse[b] = (finite && cnt_g > 0) ? (float)sqrt(sg[27] / (double)cnt_g) : 0.0f;
  out.count[b] = finite ? cnt_g : 0;
  out.rmse_photo[b] = (finite && cnt_p > 0) ? (float)sqrt(sp[27] / (double)cnt_p) : 0.0f;
  out.count_photo[b] = finite ? cnt_p : 0;
  out.steps[b] = steps[b];
  out.ok[b] = good ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct RgbdWork {
  double *pose, *slabs_g, *slabs_p;
  int *state, *steps;
  int max_slabs;
  size_t total;
};
RgbdWork rgbd_carve(void *ws, int batch, int h, int w) {
  char *base = static_cast<char *>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
  RgbdWork k;
  k.max_slabs = ceil_div(h * w, ICP_SLAB);                   // stride 1
  k.pose = reinterpret_cast<double *>(take((size_t)batch * 12 * sizeof(double)));
  k.slabs_g = reinterpret_cast<double *>(take((size_t)batch * k.max_slabs * ICP_REC * sizeof(double)));
  k.slabs_p = reinterpret_cast<double *>(take((size_t)batch * k.max_slabs * ICP_REC * sizeof(double)));
  k.state = reinterpret_cast<int *>(take((size_t)batch * sizeof(int)));
  k.steps = reinterpret_cast<int *>(take((size_t)batch * sizeof(int)));
  k.total = off;
  return k;
}

struct RgbdMaps {
  const float4 *v1, *n1, *g1, *v2, *n2, *g2;
};

int photo_reduce_launch(const RgbdMaps &m, const float *r, const float *t, const double *pose64, const int *state, int batch,
                        int h, int w, int stride, int max_slabs, IcpCam cam, float dist_thr, float int_thr, double *slabs,
                        hipStream_t s) {
  int ws;
  const int samples = icp_samples(h, w, stride, &ws), nslabs = ceil_div(samples, ICP_SLAB);
  hipLaunchKernelGGL(photo_reduce_kernel, dim3((unsigned)nslabs, (unsigned)batch), dim3(ICP_THREADS), 0, s, m.v1, m.g1, m.v2, m.g2,
                     r, t, pose64, state, h, w, stride, ws, samples, max_slabs, cam, dist_thr, int_thr, slabs);
  return mi_launch_status();
}

// one joint linearisation from the workspace's pose: K18r, K21r (when `photo`), then K21s in `mode`
int rgbd_linearise_launch(const RgbdMaps &m, int batch, int h, int w, int stride, IcpCam cam, float dist_thr, float cos_thr,
                          float int_thr, bool photo, double w2, int mode, int min_count, const RgbdWork &k, RgbdOut out,
                          hipStream_t s) {
  int ws;
  const int nslabs = ceil_div(icp_samples(h, w, stride, &ws), ICP_SLAB);
  const int *state = mode == RGBD_MODE_STEP ? k.state : nullptr;
  if (const int e = icp_reduce_launch(m.v1, m.n1, m.v2, m.n2, nullptr, nullptr, k.pose, state, batch, h, w, stride, k.max_slabs,
                                      cam, dist_thr * dist_thr, cos_thr, k.slabs_g, s))
    return e;
  if (photo)
    if (const int e = photo_reduce_launch(m, nullptr, nullptr, k.pose, state, batch, h, w, stride, k.max_slabs, cam, dist_thr,
                                          int_thr, k.slabs_p, s))
      return e;
  hipLaunchKernelGGL(rgbd_solve_kernel, dim3((unsigned)batch), dim3(64), 0, s, k.slabs_g, photo ? k.slabs_p : nullptr, nslabs,
                     k.max_slabs, mode, min_count, w2, k.pose, k.state, k.steps, out);
  return mi_launch_status();
}

bool aligned16(const void *p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int mi_intensity_maps(const void *gray, int gray_is_u8, int batch, int h, int w, float *intensity_out,
                                 mi_stream_t stream) {
  MI_ENTER();
  if (!gray || !intensity_out) return MI_E_NULL;
  if (const int s = icp_shape_status(batch, h, w)) return s;
  if (!aligned16(intensity_out)) return MI_E_ALIGN;
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
  return rgbd_carve(nullptr, batch, h, w).total;
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
  if (!aligned16(workspace) || !aligned16(vertex1) || !aligned16(intensity1) || !aligned16(vertex2) || !aligned16(intensity2))
    return MI_E_ALIGN;
  if (workspace_bytes < mi_rgbd_workspace_bytes(batch, h, w)) return MI_E_CAPACITY;
  const RgbdWork k = rgbd_carve(workspace, batch, h, w);
  hipStream_t s = (hipStream_t)stream;
  RgbdMaps m = {};
  m.v1 = reinterpret_cast<const float4 *>(vertex1); m.g1 = reinterpret_cast<const float4 *>(intensity1);
  m.v2 = reinterpret_cast<const float4 *>(vertex2); m.g2 = reinterpret_cast<const float4 *>(intensity2);
  if (const int e = photo_reduce_launch(m, r, t, nullptr, nullptr, batch, h, w, stride, k.max_slabs, IcpCam{fx, fy, cx, cy},
                                        distance_threshold, intensity_threshold, k.slabs_p, s))
    return e;
  int ws;
  const int nslabs = ceil_div(icp_samples(h, w, stride, &ws), ICP_SLAB);
  RgbdOut out = {};
  out.sums = sums;
  hipLaunchKernelGGL(rgbd_solve_kernel, dim3((unsigned)batch), dim3(64), 0, s, nullptr, k.slabs_p, nslabs, k.max_slabs,
                     RGBD_MODE_SUMS, 0, 0.0, k.pose, k.state, k.steps, out);
  return mi_launch_status();
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
  if (stages < 1 || stages > MI_ICP_MAX_STAGES || min_correspondences < 1) return MI_E_PARAM;
  int all = 0;
  for (int i = 0; i < stages; ++i) {
    if (!icp_stride_ok(strides[i]) || iterations[i] < 0 || iterations[i] > MI_ICP_MAX_ITERATIONS) return MI_E_PARAM;
    all += iterations[i];
  }
  if (all > MI_ICP_MAX_ITERATIONS) return MI_E_PARAM;
  if (const int s = icp_gate_status(fx, fy, cx, cy, distance_threshold, angle_threshold)) return s;
  if (!(photo_weight >= 0.0f) || !(photo_weight < INFINITY) || !icp_positive(intensity_threshold)) return MI_E_PARAM;
  if (!aligned16(workspace) || !aligned16(vertex1) || !aligned16(normal1) || !aligned16(intensity1) || !aligned16(vertex2) ||
      !aligned16(normal2) || !aligned16(intensity2))
    return MI_E_ALIGN;
  if (workspace_bytes < mi_rgbd_workspace_bytes(batch, h, w)) return MI_E_CAPACITY;
  const RgbdWork k = rgbd_carve(workspace, batch, h, w);
  hipStream_t s = (hipStream_t)stream;
  RgbdMaps m;
  m.v1 = reinterpret_cast<const float4 *>(vertex1); m.n1 = reinterpret_cast<const float4 *>(normal1);
  m.g1 = reinterpret_cast<const float4 *>(intensity1); m.v2 = reinterpret_cast<const float4 *>(vertex2);
  m.n2 = reinterpret_cast<const float4 *>(normal2); m.g2 = reinterpret_cast<const float4 *>(intensity2);
  const IcpCam cam{fx, fy, cx, cy};
  const float cos_thr = (float)cos((double)angle_threshold);
  const bool photo = photo_weight != 0.0f;
  const double w2 = photo_weight2(photo_weight);
  if (const int e = icp_init_launch(r0, t0, batch, k.pose, k.state, k.steps, s)) return e;
  RgbdOut out = {};
  for (int st = 0; st < stages; ++st)
    for (int it = 0; it < iterations[st]; ++it)
      if (const int e = rgbd_linearise_launch(m, batch, h, w, strides[st], cam, distance_threshold, cos_thr, intensity_threshold,
                                              photo, w2, RGBD_MODE_STEP, min_correspondences, k, out, s))
        return e;
  out.r = r; out.t = t; out.information = information; out.rmse = rmse; out.count = count; out.rmse_photo = rmse_photo;
  out.count_photo = count_photo; out.steps = steps; out.ok = ok;
  return rgbd_linearise_launch(m, batch, h, w, strides[stages - 1], cam, distance_threshold, cos_thr, intensity_threshold, photo,
                               w2, RGBD_MODE_FINAL, min_correspondences, k, out, s);
}
