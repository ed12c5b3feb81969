// K18 dense RGB-D refinement (include/mi355x_match.h, "dense RGB-D refinement"): projective point-to-plane ICP between two
// depth frames, batched over pairs under K17's contract.  The arithmetic is icp_math.h's.
//
// K18m  icp_surfel_kernel   one thread per pixel: the vertex (the ray of mi_lift_keypoints times depth) and the normal from
//       the four axis neighbours, whose vertices the thread forms itself from their depths (5 depth reads, cached);
//       two 16-byte records per pixel: (vx, vy, vz, vertex valid) and (nx, ny, nz, normal valid).
// K18r  icp_reduce_kernel   the slab reduction of icp_shared.h (grid (slabs, pairs), 256 threads, 8 samples per lane, 29
//       float64 partials per slab record) around the geometric row, which is this file's: the streamed records of frame 1 are
//       read unconditionally, frame 2's surfel at a clamped address, and a rejected pixel adds zeros.
// K18s  icp_solve_kernel    one wave per pair: lane c < 29 adds column c of the pair's slab records in slab order
//       (float64); lane 0 then solves (LDL^T) and updates the pose in the workspace (mode STEP), or writes the 29 sums
//       (mode SUMS) or the outputs (mode FINAL).  The column sum, the step and the pose write are icp_shared.h's.
// K18i  icp_init_kernel     r0 / t0 -> the float64 pose, state and step words of the workspace.
// A pair whose solve failed is frozen: its state word is set, and K18r / K18s return at once for it in later iterations.
// This file's own: K18m, K18i, the row of K18r, the statistics of K18s and the entry points.  Shared with K21 through
// icp_shared.h: the sample index and the tail of the reduction, the solve step, the workspace, the checks, the refine driver.
// Built with -ffp-contract=off; every sum has a fixed order: bitwise reproducible, alone or in a batch.
#include "common.h"
#include "icp_math.h"
#include "icp_shared.h"

#include <math.h>

namespace {

// ---- K18m ------------------------------------------------------------------------------------------------------------------
template <typename D>
__global__ __launch_bounds__(256) void icp_surfel_kernel(const D *__restrict__ depth, int h, int w, long long total,
                                                         const float *__restrict__ k_inv, float z_scale, float min_depth,
                                                         float max_depth, float max_jump, float4 *__restrict__ vertex,
                                                         float4 *__restrict__ normal) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int hw = h * w;
  const int p = (int)(i % hw), y = p / w, x = p - y * w;
  float ki[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) ki[k] = k_inv[k];
  float c[3], n[3] = {0.0f, 0.0f, 0.0f};
  const bool vok = icp_vertex((float)depth[i], (float)x, (float)y, ki, z_scale, min_depth, max_depth, c);
  bool nok = vok && x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2;
  if (nok) {                                                 // the four neighbours are inside the frame
    float l[3], r[3], u[3], d[3];
    nok = icp_vertex((float)depth[i - 1], (float)(x - 1), (float)y, ki, z_scale, min_depth, max_depth, l);
    nok = icp_vertex((float)depth[i + 1], (float)(x + 1), (float)y, ki, z_scale, min_depth, max_depth, r) && nok;
    nok = icp_vertex((float)depth[i - w], (float)x, (float)(y - 1), ki, z_scale, min_depth, max_depth, u) && nok;
    nok = icp_vertex((float)depth[i + w], (float)x, (float)(y + 1), ki, z_scale, min_depth, max_depth, d) && nok;
    nok = nok && icp_normal(c, l, r, u, d, max_jump, n);
  }
  vertex[i] = make_float4(c[0], c[1], c[2], vok ? 1.0f : 0.0f);
  normal[i] = nok ? make_float4(n[0], n[1], n[2], 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- K18i ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void icp_init_kernel(const float *__restrict__ r0, const float *__restrict__ t0, int batch,
                                                      double *__restrict__ pose, int *__restrict__ state, int *__restrict__ steps) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) pose[(size_t)b * 12 + k] = (double)r0[(size_t)b * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pose[(size_t)b * 12 + 9 + k] = (double)t0[(size_t)b * 3 + k];
  state[b] = 0;
  steps[b] = 0;
}

// ---- K18r ------------------------------------------------------------------------------------------------------------------
// icp_shared.h's sequence around the geometric row (its loads: the file header)
__global__ __launch_bounds__(ICP_THREADS) void icp_reduce_kernel(const float4 *__restrict__ vertex1, const float4 *__restrict__ normal1,
                                                                 const float4 *__restrict__ vertex2, const float4 *__restrict__ normal2,
                                                                 const float *__restrict__ r, const float *__restrict__ t,
                                                                 const double *__restrict__ pose64, const int *__restrict__ state,
                                                                 int h, int w, int stride, int ws, int samples, int max_slabs,
                                                                 IcpCam cam, float thr2, float cos_thr, double *__restrict__ slabs) {
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
    const float4 n1 = normal1[i1], v1 = vertex1[i1];
    const float p1[3] = {v1.x, v1.y, v1.z}, m1[3] = {n1.x, n1.y, n1.z};
    float q[3], rn[3], px, py;
    icp_rotate(R, p1, q);
    q[0] += T[0]; q[1] += T[1]; q[2] += T[2];
    icp_rotate(R, m1, rn);
    bool ok = in && n1.w != 0.0f;
    ok = icp_project(q, cam.fx, cam.fy, cam.cx, cam.cy, w, h, &px, &py) && ok;
    const int ix = ok ? (int)px : 0, iy = ok ? (int)py : 0;   // inside the frame when ok
    const size_t i2 = frame + (size_t)iy * (size_t)w + (size_t)ix;
    const float4 n2 = normal2[i2], v2 = vertex2[i2];
    const float p2[3] = {v2.x, v2.y, v2.z}, m2[3] = {n2.x, n2.y, n2.z};
    float J[6], res;
    ok = icp_row(q, rn, p2, m2, thr2, cos_thr, J, &res) && ok && n2.w != 0.0f;
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

// ---- K18s ------------------------------------------------------------------------------------------------------------------
struct IcpOut {
  float *r, *t, *information, *rmse;
  int *count, *steps;
  uint8_t *ok;
  double *sums;
};

__global__ __launch_bounds__(64) void icp_solve_kernel(const double *__restrict__ slabs, int nslabs, int max_slabs, int mode,
                                                       int min_count, double *__restrict__ pose, int *__restrict__ state,
                                                       int *__restrict__ steps, IcpOut out) {
  __shared__ double s[ICP_REC];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (mode == ICP_MODE_STEP && state[b] != 0) return;        // frozen pair
  if (lane < ICP_SUMS) {
    const double a = icp_column_sum(slabs, b, nslabs, max_slabs, lane);
    s[lane] = a;
    if (mode == ICP_MODE_SUMS) out.sums[(size_t)b * ICP_SUMS + lane] = a;
  }
  __syncthreads();
  if (mode == ICP_MODE_SUMS || lane != 0) return;
  if (mode == ICP_MODE_STEP) {
    icp_step(s, min_count, b, pose, state, steps);
    return;
  }
  // FINAL: the statistics of the returned pose
  const int cnt = (int)s[28];
  bool finite = true;
  for (int k = 0; k < ICP_SUMS; ++k) finite = finite && fabs(s[k]) < INFINITY;
  const bool good = finite && state[b] == 0 && cnt >= min_count;
  icp_write_pose(s, finite, b, pose, out.r, out.t, out.information);
  out.rmse[b] = (finite && cnt > 0) ? (float)sqrt(s[27] / (double)cnt) : 0.0f;
  out.count[b] = finite ? cnt : 0;
  out.steps[b] = steps[b];
  out.ok[b] = good ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// one linearisation: K18r over the job's slabs, then K18s in `mode`
int icp_linearise_launch(const IcpMaps &m, const IcpReduceJob &job, int batch, int mode, int min_count, const IcpWork &k, IcpOut out,
                         hipStream_t s) {
  if (const int e = icp_reduce_launch(m, job, batch, s)) return e;
  hipLaunchKernelGGL(icp_solve_kernel, dim3((unsigned)batch), dim3(64), 0, s, job.slabs, job.nslabs, job.max_slabs, mode, min_count,
                     k.pose, k.state, k.steps, out);
  return mi_launch_status();
}

}  // namespace

// ---- shared with K21 (photo.hip; declared in icp_shared.h) -------------------------------------------------------------------
int icp_init_launch(const float *r0, const float *t0, int batch, double *pose, int *state, int *steps, hipStream_t s) {
  hipLaunchKernelGGL(icp_init_kernel, dim3((unsigned)ceil_div(batch, 64)), dim3(64), 0, s, r0, t0, batch, pose, state, steps);
  return mi_launch_status();
}

int icp_reduce_launch(const IcpMaps &m, const IcpReduceJob &job, int batch, hipStream_t s) {
  hipLaunchKernelGGL(icp_reduce_kernel, dim3((unsigned)job.nslabs, (unsigned)batch), dim3(ICP_THREADS), 0, s, m.vertex1, m.normal1,
                     m.vertex2, m.normal2, job.r, job.t, job.pose64, job.state, job.h, job.w, job.stride, job.ws, job.samples,
                     job.max_slabs, job.cam, m.thr2, m.cos_thr, job.slabs);
  return mi_launch_status();
}

extern "C" int mi_surfel_maps(const void *depth, int depth_is_u16, int batch, int h, int w, const float *k_inv, float z_scale,
                              float min_depth, float max_depth, float normal_max_jump, float *vertex_out, float *normal_out,
                              mi_stream_t stream) {
  MI_ENTER();
  if (!depth || !k_inv || !vertex_out || !normal_out) return MI_E_NULL;
  if (const int s = icp_shape_status(batch, h, w)) return s;
  if (!(min_depth > 0.0f) || !(max_depth >= min_depth) || !(max_depth < INFINITY) || !icp_positive(z_scale) ||
      !icp_positive(normal_max_jump))
    return MI_E_PARAM;
  if (!mi_aligned16({vertex_out, normal_out})) return MI_E_ALIGN;
  const long long total = (long long)batch * h * w;
  const dim3 grid((unsigned)((total + 255) / 256));
  float4 *v = reinterpret_cast<float4 *>(vertex_out), *n = reinterpret_cast<float4 *>(normal_out);
  if (depth_is_u16)
    hipLaunchKernelGGL(icp_surfel_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const uint16_t *>(depth),
                       h, w, total, k_inv, z_scale, min_depth, max_depth, normal_max_jump, v, n);
  else
    hipLaunchKernelGGL(icp_surfel_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const float *>(depth), h, w,
                       total, k_inv, z_scale, min_depth, max_depth, normal_max_jump, v, n);
  return mi_launch_status();
}

extern "C" size_t mi_icp_workspace_bytes(int batch, int h, int w) {
  if (icp_shape_status(batch, h, w) != MI_OK) return 0;
  return icp_carve(nullptr, batch, h, w, 1).total;
}

extern "C" int mi_icp_linearise(const float *vertex1, const float *normal1, const float *vertex2, const float *normal2,
                                const float *r, const float *t, int batch, int h, int w, float fx, float fy, float cx, float cy,
                                int stride, float distance_threshold, float angle_threshold, double *sums, void *workspace,
                                size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!vertex1 || !normal1 || !vertex2 || !normal2 || !r || !t || !sums || !workspace) return MI_E_NULL;
  if (const int s = icp_shape_status(batch, h, w)) return s;
  if (!icp_stride_ok(stride)) return MI_E_PARAM;
  if (const int s = icp_gate_status(fx, fy, cx, cy, distance_threshold, angle_threshold)) return s;
  if (!mi_aligned16({workspace, vertex1, normal1, vertex2, normal2})) return MI_E_ALIGN;
  if (workspace_bytes < mi_icp_workspace_bytes(batch, h, w)) return MI_E_CAPACITY;
  const IcpWork k = icp_carve(workspace, batch, h, w, 1);
  IcpOut out = {};
  out.sums = sums;
  return icp_linearise_launch(icp_maps(vertex1, normal1, vertex2, normal2, distance_threshold, angle_threshold),
                              icp_reduce_job(r, t, nullptr, nullptr, h, w, stride, IcpCam{fx, fy, cx, cy}, k.max_slabs, k.slabs[0]),
                              batch, ICP_MODE_SUMS, 0, k, out, (hipStream_t)stream);
}

extern "C" int mi_icp_refine(const float *vertex1, const float *normal1, const float *vertex2, const float *normal2,
                             const float *r0, const float *t0, int batch, int h, int w, float fx, float fy, float cx, float cy,
                             const int32_t *strides, const int32_t *iterations, int stages, float distance_threshold,
                             float angle_threshold, int min_correspondences, float *r, float *t, float *information, float *rmse,
                             int32_t *count, int32_t *steps, uint8_t *ok, void *workspace, size_t workspace_bytes,
                             mi_stream_t stream) {
  MI_ENTER();
  if (!vertex1 || !normal1 || !vertex2 || !normal2 || !r0 || !t0 || !strides || !iterations || !r || !t || !information ||
      !rmse || !count || !steps || !ok || !workspace)
    return MI_E_NULL;
  if (const int s = icp_shape_status(batch, h, w)) return s;
  if (const int s = icp_schedule_status(strides, iterations, stages, min_correspondences)) return s;
  if (const int s = icp_gate_status(fx, fy, cx, cy, distance_threshold, angle_threshold)) return s;
  if (!mi_aligned16({workspace, vertex1, normal1, vertex2, normal2})) return MI_E_ALIGN;
  if (workspace_bytes < mi_icp_workspace_bytes(batch, h, w)) return MI_E_CAPACITY;
  const IcpWork k = icp_carve(workspace, batch, h, w, 1);
  hipStream_t s = (hipStream_t)stream;
  const IcpMaps m = icp_maps(vertex1, normal1, vertex2, normal2, distance_threshold, angle_threshold);
  if (const int e = icp_init_launch(r0, t0, batch, k.pose, k.state, k.steps, s)) return e;
  const IcpOut out{r, t, information, rmse, count, steps, ok, nullptr};
  return icp_refine_drive(strides, iterations, stages, [&](int stride, int mode) {
    // the freeze words stop a pair's steps only: FINAL reduces every pair at its last pose
    const IcpReduceJob job = icp_reduce_job(nullptr, nullptr, k.pose, mode == ICP_MODE_STEP ? k.state : nullptr, h, w, stride,
                                            IcpCam{fx, fy, cx, cy}, k.max_slabs, k.slabs[0]);
    return icp_linearise_launch(m, job, batch, mode, min_correspondences, k, mode == ICP_MODE_FINAL ? out : IcpOut{}, s);
  });
}
