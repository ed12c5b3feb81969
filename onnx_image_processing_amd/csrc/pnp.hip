// K23 absolute pose (include/mi355x_match.h, "absolute pose"): the camera pose X_c = R X + t from 3-D to 2-D matches by
// P3P RANSAC -- a minimal solve from three rows, the candidate picked by a fourth, MSAC selection, local optimisation by
// reprojection Gauss-Newton -- batched over pairs under K15's contract, with K15's sampler (pose_sampler.h, 4 slots), K17's
// Horn solve (rigid_math.h) and K18's float64 LDL^T solve and pose update (icp_math.h).  The new arithmetic is pnp_math.h's.
// The RANSAC skeleton -- staging, the hypothesis kernel, the first minimum, the float64 MSAC cost and acceptance, the
// mask write-back, the host checks -- is ransac_wave.h's; PnpModel below is what K23 supplies to it.
//
// K23a  rw_hyp_kernel<PnpModel>: 20 bytes per staged row, 40 KB of rows + 4 KB of indices at MI_PNP_MAX_N.
//       Each lane solves its 4-sample in registers (the candidates one after the other, the best kept).
// K23b  pnp_ransac_kernel  one wave per pair: the best hypothesis, then refine_rounds x {inliers -> refit: PNP_GN_ITERS
//       Gauss-Newton iterations from the current pose: 29 lanes-strided sums, wave_sum_dpp, the 6x6 solve in float64 on every
//       lane redundantly -> rw_accept_lower}; inlier bytes, count, RMSE and the information matrix of the best pose at
//       `threshold`.
// K23c  pnp_refit_kernel   the refit alone on a caller's mask and starting pose.
// Built with -ffp-contract=off; no atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "icp_math.h"
#include "pnp_math.h"
#include "ransac_wave.h"

#include <math.h>

namespace {

constexpr int PNP_MAXN = MI_PNP_MAX_N;
constexpr int PNP_MIN_ROWS = 4;

// ---- K23's model (ransac_wave.h) ----------------------------------------------------------------------------------------------
struct PnpModel {
  using Row = PnpRow;
  static constexpr int MAX_N = PNP_MAXN, SAMPLE = 4, MIN_ROWS = PNP_MIN_ROWS, FLOATS = 12, STRIDE1 = 3, STRIDE2 = 2;
  struct HypScratch {};
  static __device__ __forceinline__ Row load(const float *__restrict__ p3, const float *__restrict__ p2, int i) {
    PnpRow q;
    q.X[0] = p3[3 * i]; q.X[1] = p3[3 * i + 1]; q.X[2] = p3[3 * i + 2];
    q.u = p2[2 * i]; q.v = p2[2 * i + 1];
    return q;
  }
  static __device__ __forceinline__ void *lane_scratch(HypScratch &) { return nullptr; }
  static __device__ __forceinline__ bool solve_minimal(const Row *q, void *, float *rt) { return pnp_solve_minimal(q, rt); }
  static __host__ __device__ __forceinline__ float dist2(const float *rt, const Row &q) { return pnp_dist2(rt, q); }
};
using PnpStage = RwStage<PnpModel>;

// ---- wave-wide pieces of K23b / K23c ----------------------------------------------------------------------------------------
// the 29 sums (K18's layout; [28] counts ROWS, each of which gives two lines) of the reprojection system at rt over the
// staged rows with sel[i] != 0 (sel == nullptr: all of them), as doubles, the same in every lane
__device__ __forceinline__ void pnp_linearise_wave(const PnpStage &S, int nv, const uint8_t *sel, const float *rt, double *s) {
  const int lane = threadIdx.x & 63;
  float acc[ICP_SUMS];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) acc[k] = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv && (sel ? sel[i] != 0 : true)) {
      float ju[6], jv[6], ru, rv;
      if (pnp_lines(rt, S.p[i], ju, jv, &ru, &rv)) {
        icp_accumulate(ju, ru, acc);
        icp_accumulate(jv, rv, acc);
        acc[28] += 1.0f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) s[k] = (double)wave_sum_dpp(acc[k]);
}

// PNP_GN_ITERS Gauss-Newton iterations from rt0 (header: "Refit").  Every lane returns the same result; false: a
// linearisation (the PNP_GN_ITERS of the steps, or the one at the result, whose A goes to a21) was unusable.
__device__ bool pnp_refit_wave(const PnpStage &S, int nv, const uint8_t *sel, const float *rt0, float *rt, float *a21) {
  double pose[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) { pose[c] = (double)rt0[c]; rt[c] = rt0[c]; }
#pragma unroll 1
  for (int it = 0; it <= PNP_GN_ITERS; ++it) {
    double s[ICP_SUMS], x[6], ratio;
    pnp_linearise_wave(S, nv, sel, rt, s);
    if (!icp_solve(s, PNP_MIN_ROWS, x, &ratio)) return false;
    if (it == PNP_GN_ITERS) {
#pragma unroll
      for (int k = 0; k < 21; ++k) a21[k] = (float)s[k];
      break;
    }
    icp_update_pose(pose, x);
#pragma unroll
    for (int c = 0; c < 12; ++c) rt[c] = (float)pose[c];
  }
  return true;
}

// A's upper triangle (21, row-major) -> the full symmetric 6x6 (zeros when !ok), by lane 0
__device__ __forceinline__ void pnp_write_info(const float *a21, bool ok, float *__restrict__ info) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      const float v = ok ? a21[k] : 0.0f;
      info[i * 6 + j] = v;
      info[j * 6 + i] = v;
      ++k;
    }
}

// ---- K23b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pnp_ransac_kernel(const float *__restrict__ pts3, const float *__restrict__ pts2,
                                                        const uint8_t *__restrict__ valid, int n, int num_hyp, float thr,
                                                        int rounds, const float *__restrict__ rt_h,
                                                        const float *__restrict__ cost_h, float *__restrict__ r_out,
                                                        float *__restrict__ t_out, uint8_t *__restrict__ inlier,
                                                        int *__restrict__ best_h_out, int *__restrict__ count_out,
                                                        float *__restrict__ rmse_out, float *__restrict__ info_out,
                                                        uint8_t *__restrict__ ok_out) {
  __shared__ RwPairShared<PnpModel> S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S.st, pts3 + (size_t)b * n * 3, pts2 + (size_t)b * n * 2, valid ? valid + (size_t)b * n : nullptr, n);
  float rt[12];
  int bh;
  const bool usable = rw_best_hypothesis<PnpModel>(rt_h, cost_h, b, num_hyp, rt, bh);
  float sum_in = 0.0f;
  int cnt = 0;
  const float thr2 = thr * thr;
  if (usable) rw_score_wave(rt, S.st, nv, thr2, cnt, sum_in);          // the hypothesis' cost in THIS kernel's terms
  if (usable && rounds > 0) {
    double cur = rw_cost(nv, cnt, sum_in, thr2);
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
      const float kr = 1.0f + 0.5f * (float)(rounds - 1 - r);
      rw_flag_inliers(S, nv, rt, (kr * thr) * (kr * thr), true);
      float rt2[12], a21[21];                                           // a round's information matrix is not kept
      const bool ok2 = pnp_refit_wave(S.st, nv, S.sel, rt, rt2, a21);
      __syncthreads();
      if (ok2) rw_accept_lower(rt2, S.st, nv, thr2, rt, cnt, sum_in, cur);
    }
  }
  const bool ok = usable && cnt >= PNP_MIN_ROWS;                      // wave-uniform
  rw_flag_inliers(S, nv, rt, thr2, ok);
  double s[ICP_SUMS];
  pnp_linearise_wave(S.st, nv, S.sel, rt, s);                         // the information matrix: the inliers at the result
  rw_write_mask(S, nv, n, inlier + (size_t)b * n);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r_out[(size_t)b * 9 + r * 3 + c] = ok ? rt[r * 3 + c] : (r == c ? 1.0f : 0.0f);
      t_out[(size_t)b * 3 + r] = ok ? rt[9 + r] : 0.0f;
    }
    float a21[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) a21[k] = (float)s[k];
    pnp_write_info(a21, ok, info_out + (size_t)b * 36);
    best_h_out[b] = bh;
    count_out[b] = ok ? cnt : 0;
    rmse_out[b] = ok ? sqrtf(sum_in / (float)cnt) : 0.0f;
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K23c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pnp_refit_kernel(const float *__restrict__ pts3, const float *__restrict__ pts2,
                                                       const uint8_t *__restrict__ mask, const float *__restrict__ r0,
                                                       const float *__restrict__ t0, int n, float *__restrict__ r_out,
                                                       float *__restrict__ t_out, float *__restrict__ info_out,
                                                       uint8_t *__restrict__ ok_out) {
  __shared__ PnpStage S;
  const int b = blockIdx.x;
  const int nv = rw_stage(S, pts3 + (size_t)b * n * 3, pts2 + (size_t)b * n * 2, mask + (size_t)b * n, n);
  float start[12], rt[12], a21[21];
#pragma unroll
  for (int c = 0; c < 9; ++c) start[c] = r0[(size_t)b * 9 + c];
#pragma unroll
  for (int c = 0; c < 3; ++c) start[9 + c] = t0[(size_t)b * 3 + c];
#pragma unroll
  for (int k = 0; k < 21; ++k) a21[k] = 0.0f;
  const bool ok = pnp_refit_wave(S, nv, nullptr, start, rt, a21);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 9; ++c) r_out[(size_t)b * 9 + c] = ok ? rt[c] : start[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t_out[(size_t)b * 3 + c] = ok ? rt[9 + c] : start[9 + c];
    pnp_write_info(a21, ok, info_out + (size_t)b * 36);
    ok_out[b] = ok ? 1 : 0;
  }
}

}  // namespace

extern "C" int mi_pnp_hypotheses(const float *pts3, const float *pts2, const uint8_t *valid, int batch, int n,
                                 int num_hypotheses, float threshold, uint32_t seed, float *rt_h, float *cost, int32_t *count,
                                 mi_stream_t stream) {
  MI_ENTER();
  if (!pts3 || !pts2 || !rt_h || !cost || !count) return MI_E_NULL;
  if (const int s = rw_hyp_params(batch, n, PNP_MAXN, num_hypotheses, threshold)) return s;
  return rw_launch_hyp<PnpModel>(pts3, pts2, valid, batch, n, num_hypotheses, threshold, seed, rt_h, cost, count,
                                 (hipStream_t)stream);
}

extern "C" int mi_pnp_refit(const float *pts3, const float *pts2, const uint8_t *mask, const float *r0, const float *t0,
                            int batch, int n, float *r, float *t, float *info, uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts3 || !pts2 || !mask || !r0 || !t0 || !r || !t || !info || !ok) return MI_E_NULL;
  if (const int s = rw_shape_status(batch, n, PNP_MAXN)) return s;
  hipLaunchKernelGGL(pnp_refit_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, pts3, pts2, mask, r0, t0, n, r, t,
                     info, ok);
  return mi_launch_status();
}

extern "C" size_t mi_pnp_ransac_workspace_bytes(int batch, int n, int num_hypotheses) {
  return rw_workspace_bytes(batch, n, PNP_MAXN, num_hypotheses, 12);
}

extern "C" int mi_pnp_ransac(const float *pts3, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                             float threshold, int refine_rounds, uint32_t seed, float *r, float *t, uint8_t *inlier,
                             int32_t *best_h, int32_t *count, float *rmse, float *info, uint8_t *ok, void *workspace,
                             size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pts3 || !pts2 || !r || !t || !inlier || !best_h || !count || !rmse || !info || !ok || !workspace) return MI_E_NULL;
  if (const int s = rw_ransac_params(batch, n, PNP_MAXN, num_hypotheses, threshold, refine_rounds, 12, workspace, workspace_bytes))
    return s;
  const RwWork wk = rw_carve(workspace, batch, num_hypotheses, 12);
  hipStream_t s = (hipStream_t)stream;
  if (const int st = rw_launch_hyp<PnpModel>(pts3, pts2, valid, batch, n, num_hypotheses, threshold, seed, wk.model_h,
                                             wk.cost, wk.count, s))
    return st;
  hipLaunchKernelGGL(pnp_ransac_kernel, dim3((unsigned)batch), dim3(64), 0, s, pts3, pts2, valid, n, num_hypotheses, threshold,
                     refine_rounds, wk.model_h, wk.cost, r, t, inlier, best_h, count, rmse, info, ok);
  return mi_launch_status();
}
