// K30 similarity alignment (include/mi355x_match_sim3.h): 3-D to 3-D landmark correspondences -> X2 = s R X1 + t by 3-point
// RANSAC -- K17's Horn rotation (rigid_math.h) with Umeyama's scale (sim3_math.h), MSAC selection, local optimisation --
// batched over pairs under K15's contract.  The RANSAC skeleton is ransac_wave.h's; Sim3Model below is what K30 supplies to
// it, once per metric (point distance in frame 2's units / symmetric reprojection error of camera-frame points).
//
// K30a  rw_hyp_kernel<Sim3Model<METRIC>>: K17a's footprint (24 bytes per staged row, 48 KB of rows + 4 KB of indices at
//       MI_SIM3_MAX_N); each lane solves its 3-sample in registers and scores it on every staged row.
// K30b  s3_ransac_kernel<METRIC>   one wave per pair: the best hypothesis, then refine_rounds x {inliers -> refit: K17b's two
//       passes of lanes-strided sums, the Horn solve, a third pass for the scale's numerator -> rw_accept_lower}.
// K30c  s3_refit_kernel            the refit alone on a caller's mask.
// K30d  s3_apply_kernel            one thread per frame pose or landmark of map 1, float64, rounded once.
// fp32 but for the eigenvector correction (rigid_math.h) and K30d; built with -ffp-contract=off; no atomics; every reduction
// has a fixed order: bitwise reproducible.
#include "common.h"
#include "ransac_wave.h"
#include "sim3_math.h"

#include <math.h>

namespace {

constexpr int S3_MAXN = MI_SIM3_MAX_N;

// ---- K30's model (ransac_wave.h) ------------------------------------------------------------------------------------------------
template <int METRIC>
struct Sim3Model {
  using Row = RgRow;
  static constexpr int MAX_N = S3_MAXN, SAMPLE = 3, MIN_ROWS = 3, FLOATS = S3_FLOATS, STORED = S3_STORED, STRIDE1 = 3, STRIDE2 = 3;
  struct HypScratch {};
  static __device__ __forceinline__ Row load(const float *__restrict__ p1, const float *__restrict__ p2, int i) {
    RgRow q;
    q.a[0] = p1[3 * i]; q.a[1] = p1[3 * i + 1]; q.a[2] = p1[3 * i + 2];
    q.b[0] = p2[3 * i]; q.b[1] = p2[3 * i + 1]; q.b[2] = p2[3 * i + 2];
    return q;
  }
  static __device__ __forceinline__ void *lane_scratch(HypScratch &) { return nullptr; }
  static __device__ __forceinline__ bool solve_minimal(const Row *q, void *, float *m) { return s3_solve_minimal(q, m); }
  static __device__ __forceinline__ void restore(float *m) { m[13] = 1.0f / m[12]; }
  static __host__ __device__ __forceinline__ float dist2(const float *m, const Row &q) { return s3_dist2<METRIC>(m, q); }
};

// ---- wave-wide pieces of K30b / K30c ------------------------------------------------------------------------------------------
// The model from the staged rows with sel[i] != 0 (sel == nullptr: all of them): rg_refit_wave's sums (rigid.hip) in its
// order, then the scale.  Every lane returns the same result; false: fewer than 3 rows, a collinear set in either frame, no
// finite result or the scale outside its range.
template <class Stage>
__device__ bool s3_refit_wave(const Stage &S, int nv, const uint8_t *sel, float *m) {
  const int lane = threadIdx.x & 63;
  int cnt = 0;
  float c[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const bool on = i < nv && (sel ? sel[i] != 0 : true);
    cnt += wave_count(on);
    if (on) {
      const RgRow q = S.p[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) { c[j] += q.a[j]; c[3 + j] += q.b[j]; }
    }
  }
  if (cnt < 3) return false;
  float ca[3], cb[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    ca[j] = wave_sum_dpp(c[j]) / (float)cnt;
    cb[j] = wave_sum_dpp(c[3 + j]) / (float)cnt;
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
  rg_rotation_from_scatter(s, m);
  float num = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv && (sel ? sel[i] != 0 : true)) {
      const RgRow q = S.p[i];
      const float a[3] = {q.a[0] - ca[0], q.a[1] - ca[1], q.a[2] - ca[2]}, bb[3] = {q.b[0] - cb[0], q.b[1] - cb[1], q.b[2] - cb[2]};
      num += s3_num_term(m, a, bb);
    }
  }
  num = wave_sum_dpp(num);
  const float den = (acc[9] + acc[12]) + acc[14];                      // trace Ca: xx, yy, zz of the upper triangle
  return s3_finish(num, den, ca, cb, m);
}

// (s, R, t) of pair b, or the neutral model
__device__ __forceinline__ void s3_write_model(bool ok, const float *m, int b, float *__restrict__ s_out, float *__restrict__ r_out,
                                               float *__restrict__ t_out) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) r_out[(size_t)b * 9 + r * 3 + c] = ok ? m[r * 3 + c] : (r == c ? 1.0f : 0.0f);
    t_out[(size_t)b * 3 + r] = ok ? m[9 + r] : 0.0f;
  }
  s_out[b] = ok ? m[12] : 1.0f;
}

// ---- K30b ------------------------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(64) void s3_ransac_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                       const uint8_t *__restrict__ valid, int n, int num_hyp, float thr,
                                                       int rounds, const float *__restrict__ m_h,
                                                       const float *__restrict__ cost_h, float *__restrict__ s_out,
                                                       float *__restrict__ r_out, float *__restrict__ t_out,
                                                       uint8_t *__restrict__ inlier, int *__restrict__ best_h_out,
                                                       int *__restrict__ count_out, float *__restrict__ rmse_out,
                                                       uint8_t *__restrict__ ok_out) {
  using M = Sim3Model<METRIC>;
  __shared__ RwPairShared<M> S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S.st, pts1 + (size_t)b * n * 3, pts2 + (size_t)b * n * 3, valid ? valid + (size_t)b * n : nullptr, n);
  float m[S3_FLOATS];
  int bh;
  const bool usable = rw_best_hypothesis<M>(m_h, cost_h, b, num_hyp, m, bh);
  float sum_in = 0.0f;
  int cnt = 0;
  const float thr2 = thr * thr;
  if (usable) rw_score_wave(m, S.st, nv, thr2, cnt, sum_in);           // the hypothesis' cost in THIS kernel's terms
  if (usable && rounds > 0) {
    double cur = rw_cost(nv, cnt, sum_in, thr2);
    for (int r = 0; r < rounds; ++r) {
      const float kr = 1.0f + 0.5f * (float)(rounds - 1 - r);
      rw_flag_inliers(S, nv, m, (kr * thr) * (kr * thr), true);
      float m2[S3_FLOATS];
      const bool ok2 = s3_refit_wave(S.st, nv, S.sel, m2);
      __syncthreads();
      if (ok2) rw_accept_lower(m2, S.st, nv, thr2, m, cnt, sum_in, cur);
    }
  }
  const bool ok = usable && cnt >= 3;                                  // wave-uniform
  rw_flag_inliers(S, nv, m, thr2, ok);
  rw_write_mask(S, nv, n, inlier + (size_t)b * n);
  if (lane == 0) {
    s3_write_model(ok, m, b, s_out, r_out, t_out);
    best_h_out[b] = bh;
    count_out[b] = ok ? cnt : 0;
    rmse_out[b] = ok ? sqrtf(sum_in / (float)cnt) : 0.0f;
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K30c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void s3_refit_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                      const uint8_t *__restrict__ mask, int n, float *__restrict__ s_out,
                                                      float *__restrict__ r_out, float *__restrict__ t_out,
                                                      uint8_t *__restrict__ ok_out) {
  __shared__ RwStage<Sim3Model<MI_SIM3_POINT>> S;
  const int b = blockIdx.x;
  const int nv = rw_stage(S, pts1 + (size_t)b * n * 3, pts2 + (size_t)b * n * 3, mask + (size_t)b * n, n);
  float m[S3_FLOATS];
  const bool ok = s3_refit_wave(S, nv, nullptr, m);
  if (threadIdx.x == 0) {
    s3_write_model(ok, m, b, s_out, r_out, t_out);
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K30d ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void s3_apply_kernel(const float *__restrict__ s_in, const float *__restrict__ r_in,
                                                       const float *__restrict__ t_in, int frames, int landmarks,
                                                       const float *__restrict__ r_k, const float *__restrict__ t_k,
                                                       const float *__restrict__ points, float *__restrict__ r_out,
                                                       float *__restrict__ t_out, float *__restrict__ points_out) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= frames + landmarks) return;
  const double s = (double)s_in[b];
  double r[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = (double)r_in[(size_t)b * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = (double)t_in[(size_t)b * 3 + k];
  if (i < frames) {
    const size_t f = (size_t)b * frames + i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double k0 = (double)r_k[f * 9 + 3 * a], k1 = (double)r_k[f * 9 + 3 * a + 1], k2 = (double)r_k[f * 9 + 3 * a + 2];
      double rp[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        rp[j] = (k0 * r[3 * j] + k1 * r[3 * j + 1]) + k2 * r[3 * j + 2];
        r_out[f * 9 + 3 * a + j] = (float)rp[j];
      }
      t_out[f * 3 + a] = (float)(s * (double)t_k[f * 3 + a] - ((rp[0] * t[0] + rp[1] * t[1]) + rp[2] * t[2]));
    }
  } else {
    const size_t l = (size_t)b * landmarks + (i - frames);
    const double x0 = (double)points[l * 3], x1 = (double)points[l * 3 + 1], x2 = (double)points[l * 3 + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) points_out[l * 3 + j] = (float)(s * ((r[3 * j] * x0 + r[3 * j + 1] * x1) + r[3 * j + 2] * x2) + t[j]);
  }
}

inline bool s3_metric_ok(int metric) { return metric == MI_SIM3_POINT || metric == MI_SIM3_REPROJ; }

}  // namespace

extern "C" int mi_sim3_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                  int num_hypotheses, float threshold, int metric, uint32_t seed, float *srt_h, float *cost,
                                  int32_t *count, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !srt_h || !cost || !count) return MI_E_NULL;
  if (const int s = rw_hyp_params(batch, n, S3_MAXN, num_hypotheses, threshold)) return s;
  if (!s3_metric_ok(metric)) return MI_E_PARAM;
  if (metric == MI_SIM3_REPROJ)
    return rw_launch_hyp<Sim3Model<MI_SIM3_REPROJ>>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, srt_h, cost, count,
                                                    (hipStream_t)stream);
  return rw_launch_hyp<Sim3Model<MI_SIM3_POINT>>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, srt_h, cost, count,
                                                 (hipStream_t)stream);
}

extern "C" int mi_sim3_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *s, float *r,
                             float *t, uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !mask || !s || !r || !t || !ok) return MI_E_NULL;
  if (const int st = rw_shape_status(batch, n, S3_MAXN)) return st;
  hipLaunchKernelGGL(s3_refit_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, pts1, pts2, mask, n, s, r, t, ok);
  return mi_launch_status();
}

extern "C" size_t mi_sim3_ransac_workspace_bytes(int batch, int n, int num_hypotheses) {
  return rw_workspace_bytes(batch, n, S3_MAXN, num_hypotheses, S3_STORED);
}

extern "C" int mi_sim3_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                              float threshold, int metric, int refine_rounds, uint32_t seed, float *s, float *r, float *t,
                              uint8_t *inlier, int32_t *best_h, int32_t *count, float *rmse, uint8_t *ok, void *workspace,
                              size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !s || !r || !t || !inlier || !best_h || !count || !rmse || !ok || !workspace) return MI_E_NULL;
  if (const int st = rw_hyp_params(batch, n, S3_MAXN, num_hypotheses, threshold)) return st;
  if (!s3_metric_ok(metric)) return MI_E_PARAM;                        // a parameter: before the alignment and the capacity
  if (const int st = rw_ransac_params(batch, n, S3_MAXN, num_hypotheses, threshold, refine_rounds, S3_STORED, workspace,
                                      workspace_bytes))
    return st;
  const RwWork wk = rw_carve(workspace, batch, num_hypotheses, S3_STORED);
  hipStream_t hs = (hipStream_t)stream;
  if (metric == MI_SIM3_REPROJ) {
    if (const int st = rw_launch_hyp<Sim3Model<MI_SIM3_REPROJ>>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed,
                                                                wk.model_h, wk.cost, wk.count, hs))
      return st;
    hipLaunchKernelGGL(s3_ransac_kernel<MI_SIM3_REPROJ>, dim3((unsigned)batch), dim3(64), 0, hs, pts1, pts2, valid, n,
                       num_hypotheses, threshold, refine_rounds, wk.model_h, wk.cost, s, r, t, inlier, best_h, count, rmse, ok);
  } else {
    if (const int st = rw_launch_hyp<Sim3Model<MI_SIM3_POINT>>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed,
                                                               wk.model_h, wk.cost, wk.count, hs))
      return st;
    hipLaunchKernelGGL(s3_ransac_kernel<MI_SIM3_POINT>, dim3((unsigned)batch), dim3(64), 0, hs, pts1, pts2, valid, n,
                       num_hypotheses, threshold, refine_rounds, wk.model_h, wk.cost, s, r, t, inlier, best_h, count, rmse, ok);
  }
  return mi_launch_status();
}

extern "C" int mi_sim3_apply(const float *s, const float *r, const float *t, int batch, int frames, int landmarks,
                             const float *r_k, const float *t_k, const float *points, float *r_out, float *t_out,
                             float *points_out, mi_stream_t stream) {
  MI_ENTER();
  if (!s || !r || !t) return MI_E_NULL;
  if (frames > 0 && (!r_k || !t_k || !r_out || !t_out)) return MI_E_NULL;
  if (landmarks > 0 && (!points || !points_out)) return MI_E_NULL;
  if (batch < 1 || frames < 0 || landmarks < 0 || (frames == 0 && landmarks == 0)) return MI_E_SHAPE;
  if (batch > 65535 || (long long)frames + landmarks > MI_SIM3_MAX_ROWS) return MI_E_PARAM;
  hipLaunchKernelGGL(s3_apply_kernel, dim3((unsigned)ceil_div(frames + landmarks, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, s, r, t, frames, landmarks, r_k, t_k, points, r_out, t_out, points_out);
  return mi_launch_status();
}
