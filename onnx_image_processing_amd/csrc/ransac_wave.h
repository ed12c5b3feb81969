// The skeleton of the batched RANSAC solvers (include/mi355x_match.h, "relative pose": the contract the four share), once:
// K15 (pose.hip), K17 (rigid.hip), K23 (pnp.hip) and K24 (homography.hip) supply a model type and their own refit.
//
// A model M names
//   Row                      one staged row, and  load(p1, p2, i): row i of the caller's two arrays
//   STRIDE1, STRIDE2         floats per row of the caller's first / second array
//   MAX_N, SAMPLE, MIN_ROWS  the stage's capacity, the sample size, the fewest rows a pair can be solved from
//   FLOATS                   floats per model (9: E; 12: R row-major then t; 18: H then its adjugate G)
//   STORED, restore(m)       optional: only the first STORED floats of a model go to memory, and restore(m) completes a
//                            model read back from them (K24: G from H); without them all FLOATS are stored
//   HypScratch               LDS the minimal solve needs beside the stage (an empty struct: no bytes), and
//                            lane_scratch(x): the lane's part of it, handed on to
//   solve_minimal(q, lane's scratch, m), dist2(m, row)
// The refits are the solvers' own mathematics and stay with them, and so does the round loop that calls one: schedule
// k_r = 1 + 0.5 (R - 1 - r), rw_flag_inliers at k_r * thr, refit, then rw_accept_lower (K17, K23) or K15's float32 rule.
//
// Hypothesis kernel (rw_hyp_kernel<M>): grid (ceil(H / 64), pairs), ONE WAVE per workgroup, lane = hypothesis.  The wave
// compacts the pair's selected rows into LDS once (ballot prefix: index order kept); each lane draws its sample
// (pose_sampler.h), solves it and scores it on every staged row: LDS broadcast reads, a serial sum in index order -- no
// cross-lane reduction.  Selection kernel, one wave per pair: the first minimum of the costs (lanes stride over h, then a
// (cost, h) butterfly), local optimisation rounds, flags by staged rank written back as bytes by the caller's index.
// No atomics; every reduction has a fixed order.
#pragma once
#include "common.h"
#include "pose_sampler.h"

#include <math.h>
#include <type_traits>

namespace {

constexpr int RW_MAXH = MI_POSE_MAX_HYPOTHESES;
constexpr int RW_MAXR = MI_POSE_MAX_REFINE_ROUNDS;

__device__ __forceinline__ int wave_count(bool p) { return (int)__popcll(__ballot(p)); }

// ---- staging: the pair's selected rows, compacted in index order (one wave) ---------------------------------------------------
template <class M>
struct RwStage {
  typename M::Row p[M::MAX_N];
  unsigned short idx[M::MAX_N];   // the row's index in the caller's arrays
};
template <class M>
__device__ __forceinline__ int rw_stage(RwStage<M> &S, const float *__restrict__ p1, const float *__restrict__ p2,
                                        const uint8_t *__restrict__ sel, int n) {
  const int lane = threadIdx.x & 63;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool v = i < n && (sel ? sel[i] != 0 : true);
    const unsigned long long mk = __ballot(v);
    if (v) {
      const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
      S.p[slot] = M::load(p1, p2, i);
      S.idx[slot] = (unsigned short)i;
    }
    base += (int)__popcll(mk);
  }
  __syncthreads();
  return base;
}

// floats of a model that go to memory: M::STORED where a model names it, else all M::FLOATS
template <class M, class = void>
struct RwStored { static constexpr int value = M::FLOATS; };
template <class M>
struct RwStored<M, std::void_t<decltype(M::STORED)>> { static constexpr int value = M::STORED; };

// ---- the hypothesis kernel (K15a, K17a, K23a: rw_hyp_kernel<PoModel>, <RgModel>, <PnpModel>) ------------------------------------
template <class M>
struct RwHypShared : RwStage<M>, M::HypScratch {};

template <class M>
__global__ __launch_bounds__(64) void rw_hyp_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                    const uint8_t *__restrict__ valid, int n, int num_hyp, float thr2,
                                                    uint32_t seed, float *__restrict__ m_h, float *__restrict__ cost_out,
                                                    int *__restrict__ count_out) {
  __shared__ RwHypShared<M> S;
  static_assert(sizeof(S) == sizeof(RwStage<M>) + (std::is_empty<typename M::HypScratch>::value ? 0 : sizeof(typename M::HypScratch)),
                "an empty HypScratch must take no LDS");
  const int lane = threadIdx.x, b = blockIdx.y, h = blockIdx.x * 64 + lane;
  const int nv = rw_stage<M>(S, pts1 + (size_t)b * n * M::STRIDE1, pts2 + (size_t)b * n * M::STRIDE2,
                             valid ? valid + (size_t)b * n : nullptr, n);
  if (h >= num_hyp) return;                   // no barrier below
  float m[M::FLOATS];
  bool ok = nv >= M::MIN_ROWS;
  if (ok) {
    int pick[M::SAMPLE];
    po_sample_ranks<M::SAMPLE>(seed, (uint32_t)b, (uint32_t)h, nv, pick);
    typename M::Row q[M::SAMPLE];
#pragma unroll
    for (int s = 0; s < M::SAMPLE; ++s) q[s] = S.p[pick[s]];
    ok = M::solve_minimal(q, M::lane_scratch(S), m);
  }
  float cost = INFINITY;
  int count = 0;
  if (ok) {
    cost = 0.0f;
    for (int i = 0; i < nv; ++i) {
      const float d2 = M::dist2(m, S.p[i]);                          // the same address in every lane: a broadcast
      count += d2 <= thr2 ? 1 : 0;
      cost += fminf(d2, thr2);
    }
    if (!(cost < INFINITY)) { ok = false; cost = INFINITY; count = 0; }
  }
  const size_t o = (size_t)b * num_hyp + h;
#pragma unroll
  for (int c = 0; c < RwStored<M>::value; ++c) m_h[o * RwStored<M>::value + c] = ok ? m[c] : 0.0f;
  cost_out[o] = cost;
  count_out[o] = count;
}

// ---- wave-wide pieces of the selection kernels ------------------------------------------------------------------------------
// The first minimum of pair b's costs and its model; false: no finite cost (then bh = 0 and m holds hypothesis 0).
template <class M>
__device__ __forceinline__ bool rw_best_hypothesis(const float *__restrict__ m_h, const float *__restrict__ cost_h, int b,
                                                   int num_hyp, float *m, int &bh_out) {
  float best = INFINITY;
  int bh = 0x7fffffff;
  for (int h = threadIdx.x; h < num_hyp; h += 64) {
    const float c = cost_h[(size_t)b * num_hyp + h];
    if (c < best || (c == best && h < bh)) { best = c; bh = h; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oc = __shfl_xor(best, o, 64);
    const int oh = __shfl_xor(bh, o, 64);
    if (oc < best || (oc == best && oh < bh)) { best = oc; bh = oh; }
  }
  if (bh >= num_hyp) { bh = 0; best = INFINITY; }                    // NaN costs only (the hypothesis kernel writes none)
#pragma unroll
  for (int c = 0; c < RwStored<M>::value; ++c) m[c] = m_h[((size_t)b * num_hyp + bh) * RwStored<M>::value + c];
  if constexpr (RwStored<M>::value != M::FLOATS) M::restore(m);
  bh_out = bh;
  return best < INFINITY;                                             // wave-uniform
}

template <class M>
struct RwPairShared {
  RwStage<M> st;
  uint8_t sel[M::MAX_N], by_index[M::MAX_N];
};

// sel[i] = on and row i lies within t2 of m, by staged rank
template <class M>
__device__ __forceinline__ void rw_flag_inliers(RwPairShared<M> &S, int nv, const float *m, float t2, bool on) {
  for (int i = threadIdx.x; i < nv; i += 64) S.sel[i] = (on && M::dist2(m, S.st.p[i]) <= t2) ? 1 : 0;
  __syncthreads();
}

// flags by staged rank -> bytes by the caller's index, every one of the n bytes written (one wave)
template <class M>
__device__ __forceinline__ void rw_write_mask(RwPairShared<M> &S, int nv, int n, uint8_t *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < n; i += 64) S.by_index[i] = 0;
  __syncthreads();
  for (int i = lane; i < nv; i += 64) S.by_index[S.st.idx[i]] = S.sel[i];
  __syncthreads();
  for (int i = lane; i < n; i += 64) out[i] = S.by_index[i];
}

// Inlier count and the inliers' sum of d^2 under m over the staged rows, lanes striding, fixed order.  The MSAC cost is
// (nv - count) thr^2 + sum_in; rw_cost forms it in float64, where a handful of truncated rows (thr^2 each) cannot absorb
// an improvement of the inliers' residual the way a float32 sum does (0.0325 + 1e-11 == 0.0325).
template <class M>
__device__ __forceinline__ void rw_score_wave(const float *m, const RwStage<M> &S, int nv, float thr2, int &count, float &sum_in) {
  const int lane = threadIdx.x & 63;
  float s = 0.0f;
  int k = 0;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const float d2 = i < nv ? M::dist2(m, S.p[i]) : INFINITY;
    const bool in = i < nv && d2 <= thr2;
    k += wave_count(in);
    s += in ? d2 : 0.0f;
  }
  sum_in = wave_sum_dpp(s);
  count = k;
}
__device__ __forceinline__ double rw_cost(int nv, int count, float sum_in, float thr2) {
  return (double)(nv - count) * (double)thr2 + (double)sum_in;
}

// One round's end: m2 rescored at thr, accepted on a strictly lower float64 cost
template <class M>
__device__ __forceinline__ void rw_accept_lower(const float *m2, const RwStage<M> &S, int nv, float thr2, float *m, int &cnt,
                                                float &sum_in, double &cur) {
  float s2;
  int k2;
  rw_score_wave(m2, S, nv, thr2, k2, s2);
  const double c2 = rw_cost(nv, k2, s2, thr2);
  if (c2 < cur) {
    cur = c2;
    cnt = k2;
    sum_in = s2;
#pragma unroll
    for (int c = 0; c < M::FLOATS; ++c) m[c] = m2[c];
  }
}

// ---- host side: argument checks in the header's order of precedence, the workspace, the hypothesis launch -----------------------
inline int rw_shape_status(int batch, int n, int max_n) {
  if (batch < 1 || n < 1) return MI_E_SHAPE;
  if (n > max_n || batch > 65535) return MI_E_PARAM;
  return MI_OK;
}
inline int rw_hyp_params(int batch, int n, int max_n, int num_hypotheses, float threshold) {
  if (const int s = rw_shape_status(batch, n, max_n)) return s;
  if (num_hypotheses < 1) return MI_E_SHAPE;
  if (num_hypotheses > RW_MAXH || !(threshold > 0.0f) || !(threshold < INFINITY)) return MI_E_PARAM;
  return MI_OK;
}

struct RwWork {
  float *model_h, *cost;
  int *count;
  size_t total;
};
inline RwWork rw_carve(void *ws, int batch, int num_hyp, int floats) {
  char *base = static_cast<char *>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
  RwWork w;
  w.model_h = reinterpret_cast<float *>(take((size_t)batch * num_hyp * floats * sizeof(float)));
  w.cost = reinterpret_cast<float *>(take((size_t)batch * num_hyp * sizeof(float)));
  w.count = reinterpret_cast<int *>(take((size_t)batch * num_hyp * sizeof(int)));
  w.total = off;
  return w;
}
inline size_t rw_workspace_bytes(int batch, int n, int max_n, int num_hypotheses, int floats) {
  if (rw_shape_status(batch, n, max_n) != MI_OK || num_hypotheses < 1 || num_hypotheses > RW_MAXH) return 0;
  return rw_carve(nullptr, batch, num_hypotheses, floats).total;
}
// everything a *_ransac entry checks after its pointers
inline int rw_ransac_params(int batch, int n, int max_n, int num_hypotheses, float threshold, int refine_rounds, int floats,
                            const void *workspace, size_t workspace_bytes) {
  if (const int s = rw_hyp_params(batch, n, max_n, num_hypotheses, threshold)) return s;
  if (refine_rounds < 0 || refine_rounds > RW_MAXR) return MI_E_PARAM;
  if (((uintptr_t)workspace % 16) != 0) return MI_E_ALIGN;
  if (workspace_bytes < rw_workspace_bytes(batch, n, max_n, num_hypotheses, floats)) return MI_E_CAPACITY;
  return MI_OK;
}

template <class M>
inline int rw_launch_hyp(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                         float threshold, uint32_t seed, float *m_h, float *cost, int *count, hipStream_t stream) {
  hipLaunchKernelGGL(rw_hyp_kernel<M>, dim3((unsigned)ceil_div(num_hypotheses, 64), (unsigned)batch), dim3(64), 0, stream, pts1, pts2,
                     valid, n, num_hypotheses, threshold * threshold, seed, m_h, cost, count);
  return mi_launch_status();
}

}  // namespace
