// K24 planar two-view pose (include/mi355x_match.h, "planar two-view pose"): the homography x2 ~ H x1 between two views of a
// plane (or under a pure rotation) by 4-point RANSAC -- MSAC selection, local optimisation -- batched over pairs under K15's
// contract (pose.hip), its decomposition into rotation, translation and plane normal, and the choice between the essential
// matrix and the homography of one pair.  K15's 8-point solve is degenerate exactly here: on a plane and without a
// baseline.  The RANSAC skeleton -- staging, the hypothesis kernel, the first minimum, the float64 MSAC cost and
// acceptance, the mask write-back, the host checks -- is ransac_wave.h's; HgModel below is what K24 supplies to it.
//
// K24a  rw_hyp_kernel<HgModel>: 16 bytes per staged row (K15's float4), 32 KB of rows + 4 KB of indices at
//       MI_POSE_MAX_N.  Each lane solves its 4-sample in registers (homography_math.h: Hartley normalisation, the two
//       projective bases by cofactors, H = B2 adj(B1), the sign-matched adjugate G) and scores the 18-float model on every
//       staged row with two 3x3 products and two divisions per row.  No LDS beside the stage.
// K24b  hg_ransac_kernel   one wave per pair: the best hypothesis, then refine_rounds x {inliers -> refit: three passes of
//       lanes-strided sums (centroids, spreads, the 24 sums the 9x9 normal equations consist of; wave_sum_dpp) -> K15's
//       inverse iteration (essential_math.h), every lane redundantly -> rw_accept_lower}; inlier bytes, count and cost.
// K24c  hg_refit_kernel    the refit alone on a caller's mask.
// K24d  hg_pose_kernel     one wave per pair: the sign of H by ballot, H^T H by cyclic Jacobi, the four candidates, the
//       two depth signs per row and candidate by ballot, the candidates sorted.
// K24e  hg_select_kernel   one wave per pair: the two models' scores, lanes striding, and the choice.
// fp32 throughout (the round loop's cost comparison is float64, as K17's); built with -ffp-contract=off; no atomics; every
// reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "homography_math.h"
#include "ransac_wave.h"

#include <math.h>

namespace {

constexpr int HG_MAXN = MI_POSE_MAX_N;

// ---- K24's model (ransac_wave.h) ----------------------------------------------------------------------------------------------
struct HgModel {
  using Row = float4;                         // x1, y1, x2, y2
  static constexpr int MAX_N = HG_MAXN, SAMPLE = 4, MIN_ROWS = 4, FLOATS = 18, STRIDE1 = 2, STRIDE2 = 2;
  static constexpr int STORED = 9;            // H goes to memory; G = hg_adjugate(H), the same bits, when it is read back
  static __device__ __forceinline__ void restore(float *m) {
    if (!hg_adjugate(m, m + 9)) {
#pragma unroll
      for (int c = 9; c < 18; ++c) m[c] = 0.0f;
    }
  }
  struct HypScratch {};
  static __device__ __forceinline__ Row load(const float *__restrict__ p1, const float *__restrict__ p2, int i) {
    return make_float4(p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
  }
  static __device__ __forceinline__ void *lane_scratch(HypScratch &) { return nullptr; }
  static __device__ __forceinline__ bool solve_minimal(const Row *q, void *, float *m) { return hg_solve_minimal(q, m); }
  static __host__ __device__ __forceinline__ float dist2(const float *m, Row q) { return hg_dist2(m, q); }
};
using HgStage = RwStage<HgModel>;
using HgPairShared = RwPairShared<HgModel>;

// ---- wave-wide pieces of K24b / K24c ----------------------------------------------------------------------------------------
// The model from the staged rows with sel[i] != 0 (sel == nullptr: all of them): Hartley normalisation over those rows, the
// normal equations of the two DLT lines per row, their minimum eigenvector, denormalisation, completion.  Every lane
// returns the same model; false: fewer than 4 rows, a point set without spread or no finite, invertible result.
__device__ bool hg_refit_wave(const HgStage &S, int nv, const uint8_t *sel, float *m_out) {
  const int lane = threadIdx.x & 63;
  int m = 0;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const bool on = i < nv && (sel ? sel[i] != 0 : true);
    m += wave_count(on);
    if (on) { const float4 q = S.p[i]; s[0] += q.x; s[1] += q.y; s[2] += q.z; s[3] += q.w; }
  }
  if (m < 4) return false;
  wave_sum4(s);
  float h1[3], h2[3];
  h1[0] = s[0] / (float)m; h1[1] = s[1] / (float)m; h2[0] = s[2] / (float)m; h2[1] = s[3] / (float)m;
  float d1 = 0.0f, d2 = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv && (sel ? sel[i] != 0 : true)) {
      const float4 q = S.p[i];
      const float ax = q.x - h1[0], ay = q.y - h1[1], bx = q.z - h2[0], by = q.w - h2[1];
      d1 += ax * ax + ay * ay;
      d2 += bx * bx + by * by;
    }
  }
  d1 = wave_sum_dpp(d1);
  d2 = wave_sum_dpp(d2);
  if (!(d1 > 0.0f && d2 > 0.0f)) return false;
  h1[2] = sqrtf(2.0f) / sqrtf(d1 / (float)m);
  h2[2] = sqrtf(2.0f) / sqrtf(d2 / (float)m);
  // With u = (x1, y1, 1) a row's two lines are [u, 0, -x2 u] and [0, u, -y2 u], so M = A^T A consists of four 3x3 blocks:
  // S0 = sum u u^T, Sx = sum x2 u u^T, Sy = sum y2 u u^T, Sr = sum (x2^2 + y2^2) u u^T, upper triangles xx xy x yy y 1
  float acc[24];
#pragma unroll
  for (int k = 0; k < 24; ++k) acc[k] = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv && (sel ? sel[i] != 0 : true)) {
      const float4 q = S.p[i];
      const float x1 = (q.x - h1[0]) * h1[2], y1 = (q.y - h1[1]) * h1[2], x2 = (q.z - h2[0]) * h2[2], y2 = (q.w - h2[1]) * h2[2];
      const float p[6] = {x1 * x1, x1 * y1, x1, y1 * y1, y1, 1.0f};
      const float rr = x2 * x2 + y2 * y2;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        acc[k] += p[k];
        acc[6 + k] += x2 * p[k];
        acc[12 + k] += y2 * p[k];
        acc[18 + k] += rr * p[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 24; ++k) acc[k] = wave_sum_dpp(acc[k]);
  float mm[9][9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int lo = r < c ? r : c, hi = r < c ? c : r;
      const int k = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);               // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -> 0 .. 5
      mm[r][c] = acc[k];
      mm[3 + r][3 + c] = acc[k];
      mm[r][3 + c] = 0.0f;
      mm[3 + r][c] = 0.0f;
      mm[r][6 + c] = -acc[6 + k];
      mm[6 + c][r] = -acc[6 + k];
      mm[3 + r][6 + c] = -acc[12 + k];
      mm[6 + c][3 + r] = -acc[12 + k];
      mm[6 + r][6 + c] = acc[18 + k];
    }
  float v[9], h[9];
  em_min_eigenvector9(mm, v);
  hg_denormalise(v, h1, h2, h);
  // sign: (H X1)_2 > 0 at the centroid of the first image's rows
  const float sg = hg_w(h, h1[0], h1[1]) < 0.0f ? -1.0f : 1.0f;
  return hg_complete(h, sg, m_out);
}

// ---- K24b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hg_ransac_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                       const uint8_t *__restrict__ valid, int n, int num_hyp, float thr,
                                                       int rounds, const float *__restrict__ m_h,
                                                       const float *__restrict__ cost_h, float *__restrict__ h_out,
                                                       uint8_t *__restrict__ inlier, int *__restrict__ best_h_out,
                                                       int *__restrict__ count_out, float *__restrict__ cost_out) {
  __shared__ HgPairShared S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S.st, pts1 + (size_t)b * n * 2, pts2 + (size_t)b * n * 2, valid ? valid + (size_t)b * n : nullptr, n);
  float m[18];
  int bh;
  const bool usable = rw_best_hypothesis<HgModel>(m_h, cost_h, b, num_hyp, m, bh);
  float sum_in = 0.0f;
  int cnt = 0;
  const float thr2 = thr * thr;
  if (usable) rw_score_wave(m, S.st, nv, thr2, cnt, sum_in);           // the hypothesis' cost in THIS kernel's terms
  double cur = rw_cost(nv, cnt, sum_in, thr2);
  if (usable && rounds > 0) {
    for (int r = 0; r < rounds; ++r) {
      const float kr = 1.0f + 0.5f * (float)(rounds - 1 - r);
      rw_flag_inliers(S, nv, m, (kr * thr) * (kr * thr), true);
      float m2[18];
      const bool ok2 = hg_refit_wave(S.st, nv, S.sel, m2);
      __syncthreads();
      if (ok2) rw_accept_lower(m2, S.st, nv, thr2, m, cnt, sum_in, cur);
    }
  }
  rw_flag_inliers(S, nv, m, thr2, usable);
  rw_write_mask(S, nv, n, inlier + (size_t)b * n);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 9; ++c) h_out[(size_t)b * 9 + c] = usable ? m[c] : 0.0f;
    best_h_out[b] = bh;
    count_out[b] = usable ? cnt : 0;
    cost_out[b] = usable ? (float)cur : INFINITY;
  }
}

// ---- K24c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hg_refit_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                      const uint8_t *__restrict__ mask, int n, float *__restrict__ h_out,
                                                      uint8_t *__restrict__ ok_out) {
  __shared__ HgStage S;
  const int b = blockIdx.x;
  const int nv = rw_stage(S, pts1 + (size_t)b * n * 2, pts2 + (size_t)b * n * 2, mask + (size_t)b * n, n);
  float m[18];
  const bool ok = hg_refit_wave(S, nv, nullptr, m);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 9; ++c) h_out[(size_t)b * 9 + c] = ok ? m[c] : 0.0f;
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K24d ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hg_pose_kernel(const float *__restrict__ h_in, const float *__restrict__ pts1,
                                                     const float *__restrict__ pts2, const uint8_t *__restrict__ mask, int n,
                                                     float *__restrict__ r_out, float *__restrict__ t_out,
                                                     float *__restrict__ n_out, int *__restrict__ count_out,
                                                     uint8_t *__restrict__ pose_mask, uint8_t *__restrict__ rot_only_out,
                                                     uint8_t *__restrict__ ok_out) {
  __shared__ HgPairShared S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S.st, pts1 + (size_t)b * n * 2, pts2 + (size_t)b * n * 2, mask ? mask + (size_t)b * n : nullptr, n);
  // H at unit Frobenius norm, positive on the majority of the rows
  float h[9], fro = 0.0f;
#pragma unroll
  for (int c = 0; c < 9; ++c) { h[c] = h_in[(size_t)b * 9 + c]; fro += h[c] * h[c]; }
  bool usable = fro > 0.0f && fro < INFINITY;                         // false for NaN; wave-uniform
  const float sc = 1.0f / sqrtf(fro);
#pragma unroll
  for (int c = 0; c < 9; ++c) h[c] = usable ? h[c] * sc : 0.0f;
  int pos = 0;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    pos += wave_count(i < nv && hg_bilinear(h, S.st.p[min(i, HG_MAXN - 1)]) > 0.0f);
  }
  if (2 * pos < nv) {
#pragma unroll
    for (int c = 0; c < 9; ++c) h[c] = -h[c];
  }
  HgPose p = {};                                                      // zeros where the decomposition is not reached
  usable = usable && hg_decompose(h, p);
  int cnt[4];
  float trace[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int c = 0;
    for (int i0 = 0; i0 < nv; i0 += 64) {
      const int i = i0 + lane;
      const bool in = usable && i < nv && (p.rotation_only || hg_in_front(p.r[k], p.t[k], p.n[k], S.st.p[min(i, HG_MAXN - 1)]));
      c += wave_count(in);
    }
    cnt[k] = c;
    trace[k] = (p.r[k][0] + p.r[k][4]) + p.r[k][8];
  }
  int order[4];
  hg_order(cnt, trace, order);
  // the candidates by slot, selected without run-time indexing
  float rs[4][9], ts[4][3], ns[4][3];
  int cs[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    cs[s] = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) rs[s][c] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) ts[s][c] = ns[s][c] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (order[s] == k) {
        cs[s] = cnt[k];
#pragma unroll
        for (int c = 0; c < 9; ++c) rs[s][c] = p.r[k][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) { ts[s][c] = p.t[k][c]; ns[s][c] = p.n[k][c]; }
      }
  }
  const bool ok = usable && cs[0] >= HG_MIN_POSE_ROWS;                // wave-uniform
  for (int i = lane; i < nv; i += 64)
    S.sel[i] = (ok && (p.rotation_only || hg_in_front(rs[0], ts[0], ns[0], S.st.p[i]))) ? 1 : 0;
  __syncthreads();
  rw_write_mask(S, nv, n, pose_mask + (size_t)b * n);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int c = 0; c < 9; ++c) r_out[((size_t)b * 4 + s) * 9 + c] = ok ? rs[s][c] : (c % 4 == 0 ? 1.0f : 0.0f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        t_out[((size_t)b * 4 + s) * 3 + c] = ok ? ts[s][c] : 0.0f;
        n_out[((size_t)b * 4 + s) * 3 + c] = ok ? ns[s][c] : 0.0f;
      }
      count_out[(size_t)b * 4 + s] = ok ? cs[s] : 0;
    }
    rot_only_out[b] = (ok && p.rotation_only) ? 1 : 0;
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K24e ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hg_select_kernel(const float *__restrict__ e_in, const float *__restrict__ h_in,
                                                       const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                       const uint8_t *__restrict__ valid, int n, float thr_e, float thr_h,
                                                       float cut, float *__restrict__ score_e_out,
                                                       float *__restrict__ score_h_out, uint8_t *__restrict__ choice_out) {
  __shared__ HgStage S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S, pts1 + (size_t)b * n * 2, pts2 + (size_t)b * n * 2, valid ? valid + (size_t)b * n : nullptr, n);
  float e[9], m[18];
#pragma unroll
  for (int c = 0; c < 9; ++c) { e[c] = e_in[(size_t)b * 9 + c]; m[c] = h_in[(size_t)b * 9 + c]; }
  const bool h_ok = hg_adjugate(m, m + 9);                            // false: zero, singular or non-finite H scores 0
  const float te2 = thr_e * thr_e, th2 = thr_h * thr_h;
  float se = 0.0f, sh = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv) {
      const float4 q = S.p[i];
      se += fmaxf(0.0f, 1.0f - po_sampson(e, q) / te2);
      sh += h_ok ? fmaxf(0.0f, 1.0f - hg_dist2(m, q) / th2) : 0.0f;
    }
  }
  se = wave_sum_dpp(se);
  sh = wave_sum_dpp(sh);
  if (lane == 0) {
    score_e_out[b] = se;
    score_h_out[b] = sh;
    choice_out[b] = sh > cut * (se + sh) ? 1 : 0;
  }
}

int hg_shape_status(int batch, int n) { return rw_shape_status(batch, n, HG_MAXN); }

}  // namespace

extern "C" int mi_homography_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                        int num_hypotheses, float threshold, uint32_t seed, float *h_h, float *cost,
                                        int32_t *count, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !h_h || !cost || !count) return MI_E_NULL;
  if (const int s = rw_hyp_params(batch, n, HG_MAXN, num_hypotheses, threshold)) return s;
  return rw_launch_hyp<HgModel>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, h_h, cost, count,
                                (hipStream_t)stream);
}

extern "C" int mi_homography_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *h,
                                   uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !mask || !h || !ok) return MI_E_NULL;
  if (const int s = hg_shape_status(batch, n)) return s;
  hipLaunchKernelGGL(hg_refit_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, pts1, pts2, mask, n, h, ok);
  return mi_launch_status();
}

extern "C" size_t mi_homography_ransac_workspace_bytes(int batch, int n, int num_hypotheses) {
  return rw_workspace_bytes(batch, n, HG_MAXN, num_hypotheses, HgModel::STORED);
}

extern "C" int mi_homography_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                    int num_hypotheses, float threshold, int refine_rounds, uint32_t seed, float *h,
                                    uint8_t *inlier, int32_t *best_h, int32_t *count, float *cost, void *workspace,
                                    size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !h || !inlier || !best_h || !count || !cost || !workspace) return MI_E_NULL;
  if (const int s = rw_ransac_params(batch, n, HG_MAXN, num_hypotheses, threshold, refine_rounds, HgModel::STORED, workspace,
                                     workspace_bytes))
    return s;
  const RwWork w = rw_carve(workspace, batch, num_hypotheses, HgModel::STORED);
  hipStream_t s = (hipStream_t)stream;
  if (const int st = rw_launch_hyp<HgModel>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, w.model_h,
                                            w.cost, w.count, s))
    return st;
  hipLaunchKernelGGL(hg_ransac_kernel, dim3((unsigned)batch), dim3(64), 0, s, pts1, pts2, valid, n, num_hypotheses, threshold,
                     refine_rounds, w.model_h, w.cost, h, inlier, best_h, count, cost);
  return mi_launch_status();
}

extern "C" int mi_homography_pose(const float *h, const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n,
                                  float *r, float *t, float *normal, int32_t *count, uint8_t *pose_mask,
                                  uint8_t *rotation_only, uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!h || !pts1 || !pts2 || !r || !t || !normal || !count || !pose_mask || !rotation_only || !ok) return MI_E_NULL;
  if (const int s = hg_shape_status(batch, n)) return s;
  hipLaunchKernelGGL(hg_pose_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, h, pts1, pts2, mask, n, r, t,
                     normal, count, pose_mask, rotation_only, ok);
  return mi_launch_status();
}

extern "C" int mi_two_view_select(const float *e, const float *h, const float *pts1, const float *pts2, const uint8_t *valid,
                                  int batch, int n, float thr_e, float thr_h, float cut, float *score_e, float *score_h,
                                  uint8_t *choice, mi_stream_t stream) {
  MI_ENTER();
  if (!e || !h || !pts1 || !pts2 || !score_e || !score_h || !choice) return MI_E_NULL;
  if (const int s = hg_shape_status(batch, n)) return s;
  if (!(thr_e > 0.0f) || !(thr_e < INFINITY) || !(thr_h > 0.0f) || !(thr_h < INFINITY) || !(cut >= 0.0f) || !(cut <= 1.0f))
    return MI_E_PARAM;
  hipLaunchKernelGGL(hg_select_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, e, h, pts1, pts2, valid, n,
                     thr_e, thr_h, cut, score_e, score_h, choice);
  return mi_launch_status();
}
