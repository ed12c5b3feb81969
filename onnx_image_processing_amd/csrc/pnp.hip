// K23 absolute pose (include/mi355x_match.h, "absolute pose"): the camera pose X_c = R X + t from 3-D to 2-D matches by
// P3P RANSAC -- a minimal solve from three rows, the candidate picked by a fourth, MSAC selection, local optimisation by
// reprojection Gauss-Newton -- batched over pairs under K15's contract, with K17's kernel shapes (rigid.hip), K15's
// sampler (pose_sampler.h, 4 slots), K17's Horn solve (rigid_math.h) and K18's float64 LDL^T solve and pose update
// (icp_math.h).  The new arithmetic is pnp_math.h's.
//
// K23a  pnp_hyp_kernel     grid (ceil(H / 64), pairs), ONE WAVE per workgroup, lane = hypothesis.  The wave compacts the
//       pair's valid rows into LDS once (20 bytes per row, ballot prefix: index order kept; 40 KB of rows + 4 KB of indices
//       at MI_PNP_MAX_N).  Each lane draws its 4-sample, solves it in registers (the candidates one after the other, the
//       best kept) and scores it on every staged row: LDS broadcast reads, a serial sum in index order.
// K23b  pnp_ransac_kernel  one wave per pair: first minimum of the costs, then refine_rounds x {inliers of the best pose
//       at k_r * threshold -> PNP_GN_ITERS Gauss-Newton iterations (29 lanes-strided sums, wave_sum_dpp, the 6x6 solve
//       in float64 on every lane redundantly) -> rescore, the cost compared in float64}; inlier bytes, count, RMSE and
//       the information matrix of the best pose at `threshold`.
// K23c  pnp_refit_kernel   the refit alone on a caller's mask and starting pose.
// Built with -ffp-contract=off; no atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "icp_math.h"
#include "pnp_math.h"
#include "pose_sampler.h"

#include <math.h>

namespace {

constexpr int PNP_MAXN = MI_PNP_MAX_N;
constexpr int PNP_MAXH = MI_POSE_MAX_HYPOTHESES;
constexpr int PNP_MAXR = MI_POSE_MAX_REFINE_ROUNDS;
constexpr int PNP_MIN_ROWS = 4;

// ---- staging: the pair's selected rows, compacted in index order (one wave) ---------------------------------------------------
struct PnpStage {
  PnpRow p[PNP_MAXN];
  unsigned short idx[PNP_MAXN];   // the row's index in the caller's arrays
};
__device__ __forceinline__ int pnp_stage(PnpStage &S, const float *__restrict__ p3, const float *__restrict__ p2,
                                         const uint8_t *__restrict__ sel, int n) {
  const int lane = threadIdx.x & 63;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool v = i < n && (sel ? sel[i] != 0 : true);
    const unsigned long long mk = __ballot(v);
    if (v) {
      const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
      PnpRow q;
      q.X[0] = p3[3 * i]; q.X[1] = p3[3 * i + 1]; q.X[2] = p3[3 * i + 2];
      q.u = p2[2 * i]; q.v = p2[2 * i + 1];
      S.p[slot] = q;
      S.idx[slot] = (unsigned short)i;
    }
    base += (int)__popcll(mk);
  }
  __syncthreads();
  return base;
}

// ---- K23a ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pnp_hyp_kernel(const float *__restrict__ pts3, const float *__restrict__ pts2,
                                                     const uint8_t *__restrict__ valid, int n, int num_hyp, float thr2,
                                                     uint32_t seed, float *__restrict__ rt_h, float *__restrict__ cost_out,
                                                     int *__restrict__ count_out) {
  __shared__ PnpStage S;
  const int lane = threadIdx.x, b = blockIdx.y, h = blockIdx.x * 64 + lane;
  const int nv = pnp_stage(S, pts3 + (size_t)b * n * 3, pts2 + (size_t)b * n * 2, valid ? valid + (size_t)b * n : nullptr, n);
  if (h >= num_hyp) return;                   // no barrier below
  float rt[12];
  bool ok = nv >= PNP_MIN_ROWS;
  if (ok) {
    int pick[4];
    po_sample_ranks<4>(seed, (uint32_t)b, (uint32_t)h, nv, pick);
    PnpRow q[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) q[s] = S.p[pick[s]];
    ok = pnp_solve_minimal(q, rt);
  }
  float cost = INFINITY;
  int count = 0;
  if (ok) {
    cost = 0.0f;
    for (int i = 0; i < nv; ++i) {
      const float d2 = pnp_dist2(rt, S.p[i]);                          // the same address in every lane: a broadcast
      count += d2 <= thr2 ? 1 : 0;
      cost += fminf(d2, thr2);
    }
    if (!(cost < INFINITY)) { ok = false; cost = INFINITY; count = 0; }
  }
  const size_t o = (size_t)b * num_hyp + h;
#pragma unroll
  for (int c = 0; c < 12; ++c) rt_h[o * 12 + c] = ok ? rt[c] : 0.0f;
  cost_out[o] = cost;
  count_out[o] = count;
}

// ---- wave-wide pieces of K23b / K23c ----------------------------------------------------------------------------------------
__device__ __forceinline__ int pnp_wave_count(bool p) { return (int)__popcll(__ballot(p)); }

// inlier count and the inliers' sum of d^2 under (R, t) over the staged rows, lanes striding, fixed order (rg_score_wave)
__device__ __forceinline__ void pnp_score_wave(const float *rt, const PnpStage &S, int nv, float thr2, int &count, float &sum_in) {
  const int lane = threadIdx.x & 63;
  float s = 0.0f;
  int k = 0;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const float d2 = i < nv ? pnp_dist2(rt, S.p[i]) : INFINITY;
    const bool in = i < nv && d2 <= thr2;
    k += pnp_wave_count(in);
    s += in ? d2 : 0.0f;
  }
  sum_in = wave_sum_dpp(s);
  count = k;
}
__device__ __forceinline__ double pnp_cost(int nv, int count, float sum_in, float thr2) {
  return (double)(nv - count) * (double)thr2 + (double)sum_in;
}

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

struct PnpPairShared {
  PnpStage st;
  uint8_t sel[PNP_MAXN], by_index[PNP_MAXN];
};

// flags by staged rank -> bytes by the caller's index, every one of the n bytes written (one wave)
__device__ __forceinline__ void pnp_write_mask(PnpPairShared &S, int nv, int n, uint8_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < n; i += 64) S.by_index[i] = 0;
  __syncthreads();
  for (int i = lane; i < nv; i += 64) S.by_index[S.st.idx[i]] = S.sel[i];
  __syncthreads();
  for (int i = lane; i < n; i += 64) out[i] = S.by_index[i];
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
  __shared__ PnpPairShared S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = pnp_stage(S.st, pts3 + (size_t)b * n * 3, pts2 + (size_t)b * n * 2, valid ? valid + (size_t)b * n : nullptr, n);
  // the first minimum of the costs
  float best = INFINITY;
  int bh = 0x7fffffff;
  for (int h = lane; h < num_hyp; h += 64) {
    const float c = cost_h[(size_t)b * num_hyp + h];
    if (c < best || (c == best && h < bh)) { best = c; bh = h; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oc = __shfl_xor(best, o, 64);
    const int oh = __shfl_xor(bh, o, 64);
    if (oc < best || (oc == best && oh < bh)) { best = oc; bh = oh; }
  }
  if (bh >= num_hyp) { bh = 0; best = INFINITY; }                    // NaN costs only (mi_pnp_hypotheses writes none)
  float rt[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) rt[c] = rt_h[((size_t)b * num_hyp + bh) * 12 + c];
  const float thr2 = thr * thr;
  const bool usable = best < INFINITY;                                // wave-uniform
  float sum_in = 0.0f;
  int cnt = 0;
  if (usable) pnp_score_wave(rt, S.st, nv, thr2, cnt, sum_in);         // the hypothesis' cost in THIS kernel's terms
  if (usable && rounds > 0) {
    double cur = pnp_cost(nv, cnt, sum_in, thr2);
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
      const float kr = 1.0f + 0.5f * (float)(rounds - 1 - r);
      const float t2 = (kr * thr) * (kr * thr);
      for (int i = lane; i < nv; i += 64) S.sel[i] = pnp_dist2(rt, S.st.p[i]) <= t2 ? 1 : 0;
      __syncthreads();
      float rt2[12], a21[21], s2;
      int k2;
      const bool ok2 = pnp_refit_wave(S.st, nv, S.sel, rt, rt2, a21);
      __syncthreads();
      if (!ok2) continue;
      pnp_score_wave(rt2, S.st, nv, thr2, k2, s2);
      const double c2 = pnp_cost(nv, k2, s2, thr2);
      if (c2 < cur) {
        cur = c2;
        cnt = k2;
        sum_in = s2;
#pragma unroll
        for (int c = 0; c < 12; ++c) rt[c] = rt2[c];
      }
    }
  }
  const bool ok = usable && cnt >= PNP_MIN_ROWS;                      // wave-uniform
  for (int i = lane; i < nv; i += 64) S.sel[i] = (ok && pnp_dist2(rt, S.st.p[i]) <= thr2) ? 1 : 0;
  __syncthreads();
  double s[ICP_SUMS];
  pnp_linearise_wave(S.st, nv, S.sel, rt, s);                         // the information matrix: the inliers at the result
  pnp_write_mask(S, nv, n, inlier + (size_t)b * n);
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
  const int nv = pnp_stage(S, pts3 + (size_t)b * n * 3, pts2 + (size_t)b * n * 2, mask + (size_t)b * n, n);
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

int pnp_shape_status(int batch, int n) {
  if (batch < 1 || n < 1) return MI_E_SHAPE;
  if (n > PNP_MAXN || batch > 65535) return MI_E_PARAM;
  return MI_OK;
}

struct PnpWork {
  float *rt_h, *cost;
  int *count;
  size_t total;
};
PnpWork pnp_carve(void *ws, int batch, int num_hyp) {
  char *base = static_cast<char *>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
  PnpWork w;
  w.rt_h = reinterpret_cast<float *>(take((size_t)batch * num_hyp * 12 * sizeof(float)));
  w.cost = reinterpret_cast<float *>(take((size_t)batch * num_hyp * sizeof(float)));
  w.count = reinterpret_cast<int *>(take((size_t)batch * num_hyp * sizeof(int)));
  w.total = off;
  return w;
}

int pnp_hyp_params(int batch, int n, int num_hypotheses, float threshold) {
  if (const int s = pnp_shape_status(batch, n)) return s;
  if (num_hypotheses < 1) return MI_E_SHAPE;
  if (num_hypotheses > PNP_MAXH || !(threshold > 0.0f) || !(threshold < INFINITY)) return MI_E_PARAM;
  return MI_OK;
}

}  // namespace

extern "C" int mi_pnp_hypotheses(const float *pts3, const float *pts2, const uint8_t *valid, int batch, int n,
                                 int num_hypotheses, float threshold, uint32_t seed, float *rt_h, float *cost, int32_t *count,
                                 mi_stream_t stream) {
  MI_ENTER();
  if (!pts3 || !pts2 || !rt_h || !cost || !count) return MI_E_NULL;
  if (const int s = pnp_hyp_params(batch, n, num_hypotheses, threshold)) return s;
  hipLaunchKernelGGL(pnp_hyp_kernel, dim3((unsigned)ceil_div(num_hypotheses, 64), (unsigned)batch), dim3(64), 0,
                     (hipStream_t)stream, pts3, pts2, valid, n, num_hypotheses, threshold * threshold, seed, rt_h, cost, count);
  return mi_launch_status();
}

extern "C" int mi_pnp_refit(const float *pts3, const float *pts2, const uint8_t *mask, const float *r0, const float *t0,
                            int batch, int n, float *r, float *t, float *info, uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts3 || !pts2 || !mask || !r0 || !t0 || !r || !t || !info || !ok) return MI_E_NULL;
  if (const int s = pnp_shape_status(batch, n)) return s;
  hipLaunchKernelGGL(pnp_refit_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, pts3, pts2, mask, r0, t0, n, r, t,
                     info, ok);
  return mi_launch_status();
}

extern "C" size_t mi_pnp_ransac_workspace_bytes(int batch, int n, int num_hypotheses) {
  if (pnp_shape_status(batch, n) != MI_OK || num_hypotheses < 1 || num_hypotheses > PNP_MAXH) return 0;
  return pnp_carve(nullptr, batch, num_hypotheses).total;
}

extern "C" int mi_pnp_ransac(const float *pts3, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                             float threshold, int refine_rounds, uint32_t seed, float *r, float *t, uint8_t *inlier,
                             int32_t *best_h, int32_t *count, float *rmse, float *info, uint8_t *ok, void *workspace,
                             size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pts3 || !pts2 || !r || !t || !inlier || !best_h || !count || !rmse || !info || !ok || !workspace) return MI_E_NULL;
  if (const int s = pnp_hyp_params(batch, n, num_hypotheses, threshold)) return s;
  if (refine_rounds < 0 || refine_rounds > PNP_MAXR) return MI_E_PARAM;
  if (((uintptr_t)workspace % 16) != 0) return MI_E_ALIGN;
  if (workspace_bytes < mi_pnp_ransac_workspace_bytes(batch, n, num_hypotheses)) return MI_E_CAPACITY;
  const PnpWork wk = pnp_carve(workspace, batch, num_hypotheses);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pnp_hyp_kernel, dim3((unsigned)ceil_div(num_hypotheses, 64), (unsigned)batch), dim3(64), 0, s, pts3, pts2,
                     valid, n, num_hypotheses, threshold * threshold, seed, wk.rt_h, wk.cost, wk.count);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(pnp_ransac_kernel, dim3((unsigned)batch), dim3(64), 0, s, pts3, pts2, valid, n, num_hypotheses, threshold,
                     refine_rounds, wk.rt_h, wk.cost, r, t, inlier, best_h, count, rmse, info, ok);
  return mi_launch_status();
}
