// K17 metric RGB-D pose (include/mi355x_match.h, "metric RGB-D pose"): matched keypoints lifted through aligned depth to
// 3-D, then the rigid motion X2 = R X1 + t by 3-point RANSAC -- Horn's closed-form alignment, MSAC selection, local
// optimisation -- batched over pairs under K15's contract (pose.hip), whose sampler and kernel shapes it shares.
//
// K17l  rg_lift_kernel     one thread per keypoint: the ray of mi_normalise_keypoints, depth at the nearest pixel, the point.
// K17a  rg_hyp_kernel      grid (ceil(H / 64), pairs), ONE WAVE per workgroup, lane = hypothesis.  The wave compacts the
//       pair's valid rows into LDS once (24 bytes per row, ballot prefix: index order kept; 48 KB of rows + 4 KB of indices
//       at MI_RIGID_MAX_N, three workgroups per CU; K17b adds 4 KB of flags and holds two).  Each lane draws its 3-sample
//       (pose_sampler.h), solves it in registers (rigid_math.h: 3x3 centred products -> Horn's 4x4 matrix -> cyclic Jacobi, fully unrolled -> quaternion -> R, t) and
//       scores it on every staged row: LDS broadcast reads, a serial sum in index order -- no cross-lane reduction.
// K17b  rg_ransac_kernel   one wave per pair: first minimum of the costs (lanes stride over h, then a (cost, h) butterfly),
//       then refine_rounds x {inliers of the best motion at k_r * threshold -> two passes of lanes-strided sums (centroids,
//       then the 9 + 6 + 6 centred products, wave_sum_dpp) -> the same Horn solve, every lane redundantly -> rescore, the
//       cost compared in float64 as (rows beyond the threshold) thr^2 + (the inliers' sum of d^2)};
//       inlier bytes, count and RMSE of the best motion at `threshold`.
// K17c  rg_refit_kernel    the refit alone on a caller's mask.
// fp32 but for the 32 float64 products of the eigenvector correction (rigid_math.h); built with -ffp-contract=off; no
// atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "pose_sampler.h"
#include "rigid_math.h"

#include <math.h>

namespace {

constexpr int RG_MAXN = MI_RIGID_MAX_N;
constexpr int RG_MAXH = MI_POSE_MAX_HYPOTHESES;
constexpr int RG_MAXR = MI_POSE_MAX_REFINE_ROUNDS;

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

// ---- staging: the pair's selected rows, compacted in index order (one wave) ---------------------------------------------------
struct RgStage {
  RgRow p[RG_MAXN];
  unsigned short idx[RG_MAXN];    // the row's index in the caller's arrays
};
__device__ __forceinline__ int rg_stage(RgStage &S, const float *__restrict__ p1, const float *__restrict__ p2,
                                        const uint8_t *__restrict__ sel, int n) {
  const int lane = threadIdx.x & 63;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool v = i < n && (sel ? sel[i] != 0 : true);
    const unsigned long long mk = __ballot(v);
    if (v) {
      const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
      RgRow q;
      q.a[0] = p1[3 * i]; q.a[1] = p1[3 * i + 1]; q.a[2] = p1[3 * i + 2];
      q.b[0] = p2[3 * i]; q.b[1] = p2[3 * i + 1]; q.b[2] = p2[3 * i + 2];
      S.p[slot] = q;
      S.idx[slot] = (unsigned short)i;
    }
    base += (int)__popcll(mk);
  }
  __syncthreads();
  return base;
}

// ---- K17a ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rg_hyp_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                    const uint8_t *__restrict__ valid, int n, int num_hyp, float thr2,
                                                    uint32_t seed, float *__restrict__ rt_h, float *__restrict__ cost_out,
                                                    int *__restrict__ count_out) {
  __shared__ RgStage S;
  const int lane = threadIdx.x, b = blockIdx.y, h = blockIdx.x * 64 + lane;
  const int nv = rg_stage(S, pts1 + (size_t)b * n * 3, pts2 + (size_t)b * n * 3, valid ? valid + (size_t)b * n : nullptr, n);
  if (h >= num_hyp) return;                   // no barrier below
  float rt[12];
  bool ok = nv >= 3;
  if (ok) {
    int pick[3];
    po_sample_ranks<3>(seed, (uint32_t)b, (uint32_t)h, nv, pick);
    RgRow q[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) q[s] = S.p[pick[s]];
    ok = rg_solve_minimal(q, rt);
  }
  float cost = INFINITY;
  int count = 0;
  if (ok) {
    cost = 0.0f;
    for (int i = 0; i < nv; ++i) {
      const float d2 = rg_dist2(rt, S.p[i]);                          // the same address in every lane: a broadcast
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

// ---- wave-wide pieces of K17b / K17c ----------------------------------------------------------------------------------------
__device__ __forceinline__ int rg_wave_count(bool p) { return (int)__popcll(__ballot(p)); }

// Inlier count and the inliers' sum of d^2 under (R, t) over the staged rows, lanes striding, fixed order.  The MSAC cost
// is (nv - count) thr^2 + sum_in; rg_cost forms it in float64, where a handful of truncated rows (thr^2 each) cannot absorb
// an improvement of the inliers' residual the way a float32 sum does (0.0325 + 1e-11 == 0.0325).
__device__ __forceinline__ void rg_score_wave(const float *rt, const RgStage &S, int nv, float thr2, int &count, float &sum_in) {
  const int lane = threadIdx.x & 63;
  float s = 0.0f;
  int k = 0;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const float d2 = i < nv ? rg_dist2(rt, S.p[i]) : INFINITY;
    const bool in = i < nv && d2 <= thr2;
    k += rg_wave_count(in);
    s += in ? d2 : 0.0f;
  }
  sum_in = wave_sum_dpp(s);
  count = k;
}
__device__ __forceinline__ double rg_cost(int nv, int count, float sum_in, float thr2) {
  return (double)(nv - count) * (double)thr2 + (double)sum_in;
}

// (R, t) from the staged rows with sel[i] != 0 (sel == nullptr: all of them).  Every lane returns the same result; false:
// fewer than 3 rows, a collinear set in either frame or no finite result.
__device__ bool rg_refit_wave(const RgStage &S, int nv, const uint8_t *sel, float *rt) {
  const int lane = threadIdx.x & 63;
  int m = 0;
  float c[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const bool on = i < nv && (sel ? sel[i] != 0 : true);
    m += rg_wave_count(on);
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

// flags by staged rank -> bytes by the caller's index, every one of the n bytes written (one wave)
__device__ __forceinline__ void rg_write_mask(const RgStage &S, int nv, const uint8_t *flag, uint8_t *by_index, int n,
                                              uint8_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < n; i += 64) by_index[i] = 0;
  __syncthreads();
  for (int i = lane; i < nv; i += 64) by_index[S.idx[i]] = flag[i];
  __syncthreads();
  for (int i = lane; i < n; i += 64) out[i] = by_index[i];
}

struct RgPairShared {
  RgStage st;
  uint8_t sel[RG_MAXN], by_index[RG_MAXN];
};

// ---- K17b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rg_ransac_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                       const uint8_t *__restrict__ valid, int n, int num_hyp, float thr,
                                                       int rounds, const float *__restrict__ rt_h,
                                                       const float *__restrict__ cost_h, float *__restrict__ r_out,
                                                       float *__restrict__ t_out, uint8_t *__restrict__ inlier,
                                                       int *__restrict__ best_h_out, int *__restrict__ count_out,
                                                       float *__restrict__ rmse_out, uint8_t *__restrict__ ok_out) {
  __shared__ RgPairShared S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rg_stage(S.st, pts1 + (size_t)b * n * 3, pts2 + (size_t)b * n * 3, valid ? valid + (size_t)b * n : nullptr, n);
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
  if (bh >= num_hyp) { bh = 0; best = INFINITY; }                    // NaN costs only (mi_rigid_hypotheses writes none)
  float rt[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) rt[c] = rt_h[((size_t)b * num_hyp + bh) * 12 + c];
  const float thr2 = thr * thr;
  const bool usable = best < INFINITY;                                // wave-uniform
  float sum_in = 0.0f;
  int cnt = 0;
  if (usable) rg_score_wave(rt, S.st, nv, thr2, cnt, sum_in);          // the hypothesis' cost in THIS kernel's terms
  if (usable && rounds > 0) {
    double cur = rg_cost(nv, cnt, sum_in, thr2);
    for (int r = 0; r < rounds; ++r) {
      const float kr = 1.0f + 0.5f * (float)(rounds - 1 - r);
      const float t2 = (kr * thr) * (kr * thr);
      for (int i = lane; i < nv; i += 64) S.sel[i] = rg_dist2(rt, S.st.p[i]) <= t2 ? 1 : 0;
      __syncthreads();
      float rt2[12], s2;
      int k2;
      const bool ok2 = rg_refit_wave(S.st, nv, S.sel, rt2);
      __syncthreads();
      if (!ok2) continue;
      rg_score_wave(rt2, S.st, nv, thr2, k2, s2);
      const double c2 = rg_cost(nv, k2, s2, thr2);
      if (c2 < cur) {
        cur = c2;
        cnt = k2;
        sum_in = s2;
#pragma unroll
        for (int c = 0; c < 12; ++c) rt[c] = rt2[c];
      }
    }
  }
  const bool ok = usable && cnt >= 3;                                 // wave-uniform
  for (int i = lane; i < nv; i += 64) S.sel[i] = (ok && rg_dist2(rt, S.st.p[i]) <= thr2) ? 1 : 0;
  __syncthreads();
  rg_write_mask(S.st, nv, S.sel, S.by_index, n, inlier + (size_t)b * n);
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
  const int nv = rg_stage(S, pts1 + (size_t)b * n * 3, pts2 + (size_t)b * n * 3, mask + (size_t)b * n, n);
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

int rg_shape_status(int batch, int n) {
  if (batch < 1 || n < 1) return MI_E_SHAPE;
  if (n > RG_MAXN || batch > 65535) return MI_E_PARAM;
  return MI_OK;
}

struct RgWork {
  float *rt_h, *cost;
  int *count;
  size_t total;
};
RgWork rg_carve(void *ws, int batch, int num_hyp) {
  char *base = static_cast<char *>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
  RgWork w;
  w.rt_h = reinterpret_cast<float *>(take((size_t)batch * num_hyp * 12 * sizeof(float)));
  w.cost = reinterpret_cast<float *>(take((size_t)batch * num_hyp * sizeof(float)));
  w.count = reinterpret_cast<int *>(take((size_t)batch * num_hyp * sizeof(int)));
  w.total = off;
  return w;
}

int rg_hyp_params(int batch, int n, int num_hypotheses, float threshold) {
  if (const int s = rg_shape_status(batch, n)) return s;
  if (num_hypotheses < 1) return MI_E_SHAPE;
  if (num_hypotheses > RG_MAXH || !(threshold > 0.0f) || !(threshold < INFINITY)) return MI_E_PARAM;
  return MI_OK;
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
  if (const int s = rg_hyp_params(batch, n, num_hypotheses, threshold)) return s;
  hipLaunchKernelGGL(rg_hyp_kernel, dim3((unsigned)ceil_div(num_hypotheses, 64), (unsigned)batch), dim3(64), 0,
                     (hipStream_t)stream, pts1, pts2, valid, n, num_hypotheses, threshold * threshold, seed, rt_h, cost, count);
  return mi_launch_status();
}

extern "C" int mi_rigid_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *r, float *t,
                              uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !mask || !r || !t || !ok) return MI_E_NULL;
  if (const int s = rg_shape_status(batch, n)) return s;
  hipLaunchKernelGGL(rg_refit_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, pts1, pts2, mask, n, r, t, ok);
  return mi_launch_status();
}

extern "C" size_t mi_rigid_ransac_workspace_bytes(int batch, int n, int num_hypotheses) {
  if (rg_shape_status(batch, n) != MI_OK || num_hypotheses < 1 || num_hypotheses > RG_MAXH) return 0;
  return rg_carve(nullptr, batch, num_hypotheses).total;
}

extern "C" int mi_rigid_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                               float threshold, int refine_rounds, uint32_t seed, float *r, float *t, uint8_t *inlier,
                               int32_t *best_h, int32_t *count, float *rmse, uint8_t *ok, void *workspace,
                               size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !r || !t || !inlier || !best_h || !count || !rmse || !ok || !workspace) return MI_E_NULL;
  if (const int s = rg_hyp_params(batch, n, num_hypotheses, threshold)) return s;
  if (refine_rounds < 0 || refine_rounds > RG_MAXR) return MI_E_PARAM;
  if (((uintptr_t)workspace % 16) != 0) return MI_E_ALIGN;
  if (workspace_bytes < mi_rigid_ransac_workspace_bytes(batch, n, num_hypotheses)) return MI_E_CAPACITY;
  const RgWork wk = rg_carve(workspace, batch, num_hypotheses);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rg_hyp_kernel, dim3((unsigned)ceil_div(num_hypotheses, 64), (unsigned)batch), dim3(64), 0, s, pts1, pts2,
                     valid, n, num_hypotheses, threshold * threshold, seed, wk.rt_h, wk.cost, wk.count);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(rg_ransac_kernel, dim3((unsigned)batch), dim3(64), 0, s, pts1, pts2, valid, n, num_hypotheses, threshold,
                     refine_rounds, wk.rt_h, wk.cost, r, t, inlier, best_h, count, rmse, ok);
  return mi_launch_status();
}
