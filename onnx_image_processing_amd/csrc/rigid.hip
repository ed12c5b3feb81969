// K17 metric RGB-D pose (include/mi355x_match.h, "metric RGB-D pose"): matched keypoints lifted through aligned depth to
// 3-D, then the rigid motion X2 = R X1 + t by 3-point RANSAC -- Horn's closed-form alignment, MSAC selection, local
// optimisation -- batched over pairs under K15's contract (pose.hip).  The RANSAC skeleton -- staging, the hypothesis kernel,
// the first minimum, the float64 MSAC cost and acceptance, the mask write-back, the host checks -- is
// ransac_wave.h's; RgModel below is what K17 supplies to it.
//
// K17l  rg_lift_kernel     one thread per keypoint: the ray of mi_normalise_keypoints, depth at the nearest pixel, the point.
// K17a  rw_hyp_kernel<RgModel>: 24 bytes per staged row, 48 KB of rows + 4 KB of indices at MI_RIGID_MAX_N,
//       three workgroups per CU (K17b adds 4 KB of flags and holds two).  Each lane solves its 3-sample in registers
//       (rigid_math.h: 3x3 centred products -> Horn's 4x4 matrix -> cyclic Jacobi, fully unrolled -> quaternion -> R, t).
// K17b  rg_ransac_kernel   one wave per pair: the best hypothesis, then refine_rounds x {inliers -> refit: two passes of
//       lanes-strided sums (centroids, then the 9 + 6 + 6 centred products, wave_sum_dpp) -> the same Horn solve, every lane
//       redundantly -> rw_accept_lower}; inlier bytes, count and RMSE of the best motion at `threshold`.
// K17c  rg_refit_kernel    the refit alone on a caller's mask.
// fp32 but for the 32 float64 products of the eigenvector correction (rigid_math.h); built with -ffp-contract=off; no
// atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "ransac_wave.h"
#include "rigid_math.h"

#include <math.h>

namespace {

constexpr int RG_MAXN = MI_RIGID_MAX_N;

// ---- K17l ------------------------------------------------------------------------------------------------------------------
template <typename D>
__global__ __launch_bounds__(256) void rg_lift_kernel(const float *__restrict__ kpts, const D *__restrict__ depth, int n, int h,
                                                      int w, long long total, const float *__restrict__ k_inv, float z_scale,
                                                      float min_depth, float max_depth, const uint8_t *__restrict__ valid_in,
                                                      float *__restrict__ points, uint8_t *__restrict__ valid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float y = kpts[2 * i + 0], x = kpts[2 * i + 1];
  const float xn = (x * k_inv[0] + y * k_inv[1]) + k_inv[2];          // the arithmetic of em_normalise_kernel (essential.hip)
  const float yn = (x * k_inv[3] + y * k_inv[4]) + k_inv[5];
  const float px = floorf(x + 0.5f), py = floorf(y + 0.5f);
  // NaN fails every comparison; +-inf fails the frame test
  bool ok = (valid_in ? valid_in[i] != 0 : true) && px >= 0.0f && px < (float)w && py >= 0.0f && py < (float)h;
  float z = 0.0f;
  if (ok) {
    const size_t b = (size_t)(i / n);
    const float d = (float)depth[(b * (size_t)h + (size_t)(int)py) * (size_t)w + (size_t)(int)px];
    z = d * z_scale;
    ok = fabsf(d) < INFINITY && z >= min_depth && z <= max_depth;
  }
  points[3 * i + 0] = ok ? xn * z : 0.0f;
  points[3 * i + 1] = ok ? yn * z : 0.0f;
  points[3 * i + 2] = ok ? z : 0.0f;
  valid[i] = ok ? 1 : 0;
}

// ---- K17's model (ransac_wave.h) ----------------------------------------------------------------------------------------------
struct RgModel {
  using Row = RgRow;
  static constexpr int MAX_N = RG_MAXN, SAMPLE = 3, MIN_ROWS = 3, FLOATS = 12, STRIDE1 = 3, STRIDE2 = 3;
  struct HypScratch {};
  static __device__ __forceinline__ Row load(const float *__restrict__ p1, const float *__restrict__ p2, int i) {
    RgRow q;
    q.a[0] = p1[3 * i]; q.a[1] = p1[3 * i + 1]; q.a[2] = p1[3 * i + 2];
    q.b[0] = p2[3 * i]; q.b[1] = p2[3 * i + 1]; q.b[2] = p2[3 * i + 2];
    return q;
  }
  static __device__ __forceinline__ void *lane_scratch(HypScratch &) { return nullptr; }
  static __device__ __forceinline__ bool solve_minimal(const Row *q, void *, float *rt) { return rg_solve_minimal(q, rt); }
  static __host__ __device__ __forceinline__ float dist2(const float *rt, const Row &q) { return rg_dist2(rt, q); }
};
using RgStage = RwStage<RgModel>;

// ---- wave-wide pieces of K17b / K17c ----------------------------------------------------------------------------------------
// (R, t) from the staged rows with sel[i] != 0 (sel == nullptr: all of them).  Every lane returns the same result; false:
// fewer than 3 rows, a collinear set in either frame or no finite result.
__device__ bool rg_refit_wave(const RgStage &S, int nv, const uint8_t *sel, float *rt) {
  const int lane = threadIdx.x & 63;
  int m = 0;
  float c[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const bool on = i < nv && (sel ? sel[i] != 0 : true);
    m += wave_count(on);
    if (on) {
      const RgRow q = S.p[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) { c[j] += q.a[j]; c[3 + j] += q.b[j]; }
    }
  }
  if (m < 3) return false;
  float ca[3], cb[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    ca[j] = wave_sum_dpp(c[j]) / (float)m;
    cb[j] = wave_sum_dpp(c[3 + j]) / (float)m;
  }
  // centred products: s[i][j] = sum a_i b_j, then the upper triangles of sum a a^T and sum b b^T
  float acc[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) acc[k] = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv && (sel ? sel[i] != 0 : true)) {
      const RgRow q = S.p[i];
      const float a[3] = {q.a[0] - ca[0], q.a[1] - ca[1], q.a[2] - ca[2]}, bb[3] = {q.b[0] - cb[0], q.b[1] - cb[1], q.b[2] - cb[2]};
      int k = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) acc[k++] += a[r] * bb[cc];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = r; cc < 3; ++cc) { acc[k] += a[r] * a[cc]; acc[k + 6] += bb[r] * bb[cc]; ++k; }
    }
  }
#pragma unroll
  for (int k = 0; k < 21; ++k) acc[k] = wave_sum_dpp(acc[k]);
  if (rg_scatter_degenerate(acc + 9) || rg_scatter_degenerate(acc + 15)) return false;
  const float s[3][3] = {{acc[0], acc[1], acc[2]}, {acc[3], acc[4], acc[5]}, {acc[6], acc[7], acc[8]}};
  return rg_finish(s, ca, cb, rt);
}

// ---- K17b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rg_ransac_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                       const uint8_t *__restrict__ valid, int n, int num_hyp, float thr,
                                                       int rounds, const float *__restrict__ rt_h,
                                                       const float *__restrict__ cost_h, float *__restrict__ r_out,
                                                       float *__restrict__ t_out, uint8_t *__restrict__ inlier,
                                                       int *__restrict__ best_h_out, int *__restrict__ count_out,
                                                       float *__restrict__ rmse_out, uint8_t *__restrict__ ok_out) {
  __shared__ RwPairShared<RgModel> S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S.st, pts1 + (size_t)b * n * 3, pts2 + (size_t)b * n * 3, valid ? valid + (size_t)b * n : nullptr, n);
  float rt[12];
  int bh;
  const bool usable = rw_best_hypothesis<RgModel>(rt_h, cost_h, b, num_hyp, rt, bh);
  float sum_in = 0.0f;
  int cnt = 0;
  const float thr2 = thr * thr;
  if (usable) rw_score_wave(rt, S.st, nv, thr2, cnt, sum_in);          // the hypothesis' cost in THIS kernel's terms
  if (usable && rounds > 0) {
    double cur = rw_cost(nv, cnt, sum_in, thr2);
    for (int r = 0; r < rounds; ++r) {
      const float kr = 1.0f + 0.5f * (float)(rounds - 1 - r);
      rw_flag_inliers(S, nv, rt, (kr * thr) * (kr * thr), true);
      float rt2[12];
      const bool ok2 = rg_refit_wave(S.st, nv, S.sel, rt2);
      __syncthreads();
      if (ok2) rw_accept_lower(rt2, S.st, nv, thr2, rt, cnt, sum_in, cur);
    }
  }
  const bool ok = usable && cnt >= 3;                                 // wave-uniform
  rw_flag_inliers(S, nv, rt, thr2, ok);
  rw_write_mask(S, nv, n, inlier + (size_t)b * n);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r_out[(size_t)b * 9 + r * 3 + c] = ok ? rt[r * 3 + c] : (r == c ? 1.0f : 0.0f);
      t_out[(size_t)b * 3 + r] = ok ? rt[9 + r] : 0.0f;
    }
    best_h_out[b] = bh;
    count_out[b] = ok ? cnt : 0;
    rmse_out[b] = ok ? sqrtf(sum_in / (float)cnt) : 0.0f;
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K17c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rg_refit_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                      const uint8_t *__restrict__ mask, int n, float *__restrict__ r_out,
                                                      float *__restrict__ t_out, uint8_t *__restrict__ ok_out) {
  __shared__ RgStage S;
  const int b = blockIdx.x;
  const int nv = rw_stage(S, pts1 + (size_t)b * n * 3, pts2 + (size_t)b * n * 3, mask + (size_t)b * n, n);
  float rt[12];
  const bool ok = rg_refit_wave(S, nv, nullptr, rt);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r_out[(size_t)b * 9 + r * 3 + c] = ok ? rt[r * 3 + c] : (r == c ? 1.0f : 0.0f);
      t_out[(size_t)b * 3 + r] = ok ? rt[9 + r] : 0.0f;
    }
    ok_out[b] = ok ? 1 : 0;
  }
}

}  // namespace

extern "C" int mi_lift_keypoints(const float *keypoints, const void *depth, int depth_is_u16, int batch, int n, int h, int w,
                                 const float *k_inv, float z_scale, float min_depth, float max_depth, const uint8_t *valid_in,
                                 float *points, uint8_t *valid, mi_stream_t stream) {
  MI_ENTER();
  if (!keypoints || !depth || !k_inv || !points || !valid) return MI_E_NULL;
  if (batch < 1 || n < 1 || h < 1 || w < 1) return MI_E_SHAPE;
  const long long total = (long long)batch * n;
  if (total > 0x7fffffffLL * 256LL) return MI_E_SHAPE;
  if (!(min_depth > 0.0f) || !(max_depth >= min_depth) || !(max_depth < INFINITY) || !(z_scale > 0.0f) || !(z_scale < INFINITY))
    return MI_E_PARAM;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (depth_is_u16)
    hipLaunchKernelGGL(rg_lift_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, keypoints,
                       static_cast<const uint16_t *>(depth), n, h, w, total, k_inv, z_scale, min_depth, max_depth, valid_in, points,
                       valid);
  else
    hipLaunchKernelGGL(rg_lift_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, keypoints,
                       static_cast<const float *>(depth), n, h, w, total, k_inv, z_scale, min_depth, max_depth, valid_in, points,
                       valid);
  return mi_launch_status();
}

extern "C" int mi_rigid_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                   int num_hypotheses, float threshold, uint32_t seed, float *rt_h, float *cost, int32_t *count,
                                   mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !rt_h || !cost || !count) return MI_E_NULL;
  if (const int s = rw_hyp_params(batch, n, RG_MAXN, num_hypotheses, threshold)) return s;
  return rw_launch_hyp<RgModel>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, rt_h, cost, count,
                                (hipStream_t)stream);
}

extern "C" int mi_rigid_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *r, float *t,
                              uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !mask || !r || !t || !ok) return MI_E_NULL;
  if (const int s = rw_shape_status(batch, n, RG_MAXN)) return s;
  hipLaunchKernelGGL(rg_refit_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, pts1, pts2, mask, n, r, t, ok);
  return mi_launch_status();
}

extern "C" size_t mi_rigid_ransac_workspace_bytes(int batch, int n, int num_hypotheses) {
  return rw_workspace_bytes(batch, n, RG_MAXN, num_hypotheses, 12);
}

extern "C" int mi_rigid_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                               float threshold, int refine_rounds, uint32_t seed, float *r, float *t, uint8_t *inlier,
                               int32_t *best_h, int32_t *count, float *rmse, uint8_t *ok, void *workspace,
                               size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !r || !t || !inlier || !best_h || !count || !rmse || !ok || !workspace) return MI_E_NULL;
  if (const int s = rw_ransac_params(batch, n, RG_MAXN, num_hypotheses, threshold, refine_rounds, 12, workspace, workspace_bytes))
    return s;
  const RwWork wk = rw_carve(workspace, batch, num_hypotheses, 12);
  hipStream_t s = (hipStream_t)stream;
  if (const int st = rw_launch_hyp<RgModel>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, wk.model_h,
                                            wk.cost, wk.count, s))
    return st;
  hipLaunchKernelGGL(rg_ransac_kernel, dim3((unsigned)batch), dim3(64), 0, s, pts1, pts2, valid, n, num_hypotheses, threshold,
                     refine_rounds, wk.model_h, wk.cost, r, t, inlier, best_h, count, rmse, ok);
  return mi_launch_status();
}
