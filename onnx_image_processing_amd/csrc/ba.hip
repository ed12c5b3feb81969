// K25 windowed bundle adjustment (include/mi355x_match.h, "windowed bundle adjustment"): the joint refinement of the poses
// of a window of frames and the landmarks they share, by Levenberg-Marquardt on the reprojection error with the landmarks
// eliminated (Schur complement), batched over independent windows under K15's contract.  The per-observation arithmetic,
// the 3x3 inverse and the LDL^T solve are ba_math.h's (on K23's pnp_lines and K18's icp_update_pose).
//
// One workgroup of 256 threads per window.  A thread owns the landmarks l = tid + 256 k and walks the frames in index
// order, so whatever belongs to one landmark (V, h, its inverse, its step, its candidate) is summed sequentially by one
// thread and lives in the workspace rows of that thread; only sums over landmarks cross threads: lanes-strided partial
// sums, wave_sum_dpp, then the four waves in wave order in float64 (ba_block_sum).
//   pass A   per landmark: V, h over its visible frames, Vi = (V + lambda diag V)^-1 -> workspace
//   pass B   per free frame f: U_f, g_f and the diagonal block of the reduced system; per pair f < f': the off-diagonal
//            block.  The observation lines are recomputed (W_fl is never stored).  S is a float64 packed upper
//            triangle in LDS (37 KB at 16 free frames).
//   solve    ba_ldlt_solve by the whole workgroup
//   pass C   the candidate poses (LDS) and points (workspace)
//   cost     the candidate's cost; accepted -> the candidate becomes the state
// K25a ba_cost_kernel, K25b ba_linearise_kernel (A, B at lambda = 0), K25c ba_refine_kernel (the loop, then A, B at
// lambda = 0 for `info`).  Built with -ffp-contract=off; no atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "ba_math.h"

#include <math.h>

namespace {

constexpr int BA_THREADS = 256, BA_WAVES = BA_THREADS / 64, BA_MAXF = MI_BA_MAX_FRAMES, BA_MAXN = 6 * BA_MAXF;
constexpr int BA_ROWS = 13;        // workspace floats per landmark: Vi (6), h (3), active (1), candidate (3); one array of Lp each
constexpr int BA_VI = 0, BA_H = 6, BA_ACT = 9, BA_CAND = 10;
constexpr int BA_SUMS = 54;        // the diagonal pass: U (21), Q (21), g (6), Y h (6)

struct BaShared {
  double s[BA_MAXN * (BA_MAXN + 1) / 2];   // the reduced system, packed upper triangle
  double x[BA_MAXN];                       // b, then the pose step
  double red[BA_SUMS];
  double pose[BA_MAXF][12], cand[BA_MAXF][12];
  float rt[BA_MAXF][12], crt[BA_MAXF][12]; // the float32 poses the lines are formed at: state and candidate
  float dp[BA_MAXN];
  float part[BA_WAVES][BA_SUMS];
};

// what the cost kernel needs of it (2 KB instead of 44 KB: its occupancy is then set by its 46 registers)
struct BaCostShared {
  double red[BA_SUMS];
  float rt[BA_MAXF][12];
  float part[BA_WAVES][BA_SUMS];
};

struct BaWin {
  const float *obs;       // (F, L, 2)
  const uint8_t *vis;     // (F, L)
  float *ws;              // BA_ROWS arrays of Lp floats
  int F, L, Lp, nf;
  float huber;
};
// points as (L, 3) rows (ps = 3, as = 1) or as three workspace arrays (ps = 1, as = Lp)
struct BaPts {
  const float *p;
  int ps, as;
};

__device__ __forceinline__ int ba_lp(int L) { return (L + 3) & ~3; }

// red[k] = the sum of acc[k] over the workgroup: wave_sum_dpp, then the waves in order in float64
template <int NS, class Shared>
__device__ __forceinline__ void ba_block_sum(Shared &S, const float *acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const float v = wave_sum_dpp(acc[k]);
    if (lane == 0) S.part[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < BA_WAVES; ++w) t += (double)S.part[w][threadIdx.x];
    S.red[threadIdx.x] = t;
  }
  __syncthreads();
}

__device__ __forceinline__ bool ba_active(const BaWin &w, int l) {
  int c = 0;
  for (int f = 0; f < w.F; ++f) c += w.vis[(size_t)f * w.L + l] != 0 ? 1 : 0;
  return c >= 2;
}

__device__ __forceinline__ void ba_load_point(const BaPts &P, int l, float *X) {
#pragma unroll
  for (int a = 0; a < 3; ++a) X[a] = P.p[(size_t)l * P.ps + (size_t)a * P.as];
}

// the cost at (rt, P) (header: "Cost"), the same in every thread; *nactive = the number of active landmarks
template <bool WRITE, class Shared>
__device__ double ba_cost_pass(Shared &S, const BaWin &w, const float (*rt)[12], const BaPts &P, float *e2_out,
                               uint8_t *active_out, int *nactive) {
  float acc[2] = {0.0f, 0.0f};
  for (int l = threadIdx.x; l < w.L; l += BA_THREADS) {
    const bool act = ba_active(w, l);
    if (WRITE) active_out[l] = act ? 1 : 0;
    acc[1] += act ? 1.0f : 0.0f;
    float X[3];
    ba_load_point(P, l, X);
    for (int f = 0; f < w.F; ++f) {
      const size_t o = (size_t)f * w.L + l;
      float e2 = 0.0f;
      if (act && w.vis[o] != 0) acc[0] += ba_rho(rt[f], X, w.obs[2 * o], w.obs[2 * o + 1], w.huber, &e2);
      if (WRITE) e2_out[o] = e2;
    }
  }
  ba_block_sum<2>(S, acc);
  *nactive = (int)S.red[1];
  return S.red[0];
}

// pass A
__device__ void ba_pass_a(const BaWin &w, const float (*rt)[12], const BaPts &P, float lambda) {
  for (int l = threadIdx.x; l < w.L; l += BA_THREADS) {
    const bool act = ba_active(w, l);
    float V[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, h[3] = {0.0f, 0.0f, 0.0f}, vi[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (act) {
      float X[3];
      ba_load_point(P, l, X);
      for (int f = 0; f < w.F; ++f) {
        const size_t o = (size_t)f * w.L + l;
        if (w.vis[o] == 0) continue;
        BaLine q;
        if (ba_line(rt[f], X, w.obs[2 * o], w.obs[2 * o + 1], w.huber, q)) ba_add_point(q, V, h);
      }
      ba_inv3(V, lambda, vi);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) w.ws[(size_t)(BA_VI + k) * w.Lp + l] = vi[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) w.ws[(size_t)(BA_H + k) * w.Lp + l] = h[k];
    w.ws[(size_t)BA_ACT * w.Lp + l] = act ? 1.0f : 0.0f;
  }
}

// the line of the (active) landmark l in frame f, if it is seen there and lies in front of the camera
__device__ __forceinline__ bool ba_obs_line(const BaWin &w, const float (*rt)[12], const float *X, int f, int l, BaLine &q) {
  const size_t o = (size_t)f * w.L + l;
  if (w.vis[o] == 0) return false;
  return ba_line(rt[f], X, w.obs[2 * o], w.obs[2 * o + 1], w.huber, q);
}

// pass B: S.s = the reduced system at damping lambda, S.x = b
__device__ void ba_pass_b(BaShared &S, const BaWin &w, const float (*rt)[12], const BaPts &P, double lambda) {
  const int nfree = w.F - w.nf, n = 6 * nfree, t = threadIdx.x;
#pragma unroll 1
  for (int p = 0; p < nfree; ++p) {
    const int f = w.nf + p;
    {
      float acc[BA_SUMS];
#pragma unroll
      for (int k = 0; k < BA_SUMS; ++k) acc[k] = 0.0f;
      for (int l = t; l < w.L; l += BA_THREADS) {
        if (w.ws[(size_t)BA_ACT * w.Lp + l] == 0.0f) continue;
        float X[3];
        ba_load_point(P, l, X);
        BaLine q;
        if (!ba_obs_line(w, rt, X, f, l, q)) continue;
        float vi[6], h[3], W[18], Y[18];
#pragma unroll
        for (int k = 0; k < 6; ++k) vi[k] = w.ws[(size_t)(BA_VI + k) * w.Lp + l];
#pragma unroll
        for (int k = 0; k < 3; ++k) h[k] = w.ws[(size_t)(BA_H + k) * w.Lp + l];
        ba_cross(q, W);
        ba_times_sym(W, vi, Y);
        ba_add_pose(q, acc, acc + 42);
        int k = 21;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = i; j < 6; ++j) acc[k++] += (Y[i * 3] * W[j * 3] + Y[i * 3 + 1] * W[j * 3 + 1]) + Y[i * 3 + 2] * W[j * 3 + 2];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[48 + i] += (Y[i * 3] * h[0] + Y[i * 3 + 1] * h[1]) + Y[i * 3 + 2] * h[2];
      }
      ba_block_sum<BA_SUMS>(S, acc);
      if (t < 21) {
        int i = 0, rem = t;
        while (rem >= 6 - i) { rem -= 6 - i; ++i; }
        const int j = i + rem;
        const double u = S.red[t];
        S.s[ba_tri(n, 6 * p + i, 6 * p + j)] = (i == j ? u + lambda * u : u) - S.red[21 + t];
      } else if (t >= 42 && t < 48) {
        S.x[6 * p + (t - 42)] = S.red[t] - S.red[t + 6];
      }
    }
#pragma unroll 1
    for (int p2 = p + 1; p2 < nfree; ++p2) {
      const int f2 = w.nf + p2;
      float acc[36];
#pragma unroll
      for (int k = 0; k < 36; ++k) acc[k] = 0.0f;
      for (int l = t; l < w.L; l += BA_THREADS) {
        if (w.ws[(size_t)BA_ACT * w.Lp + l] == 0.0f) continue;
        float X[3];
        ba_load_point(P, l, X);
        BaLine q, q2;
        if (!ba_obs_line(w, rt, X, f, l, q) || !ba_obs_line(w, rt, X, f2, l, q2)) continue;
        float vi[6], W[18], Y[18], W2[18];
#pragma unroll
        for (int k = 0; k < 6; ++k) vi[k] = w.ws[(size_t)(BA_VI + k) * w.Lp + l];
        ba_cross(q, W);
        ba_times_sym(W, vi, Y);
        ba_cross(q2, W2);
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) acc[i * 6 + j] += (Y[i * 3] * W2[j * 3] + Y[i * 3 + 1] * W2[j * 3 + 1]) + Y[i * 3 + 2] * W2[j * 3 + 2];
      }
      ba_block_sum<36>(S, acc);
      if (t < 36) S.s[ba_tri(n, 6 * p + t / 6, 6 * p2 + t % 6)] = -S.red[t];
    }
  }
  __syncthreads();
}

// pass C: the candidate poses and points from the pose step S.x
__device__ void ba_pass_c(BaShared &S, const BaWin &w, const BaPts &P) {
  const int nfree = w.F - w.nf, n = 6 * nfree, t = threadIdx.x;
  if (t < n) S.dp[t] = (float)S.x[t];
  if (t < nfree) {
    const int f = w.nf + t;
    double pose[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) pose[c] = S.pose[f][c];
    icp_update_pose(pose, &S.x[6 * t]);
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      S.cand[f][c] = pose[c];
      S.crt[f][c] = (float)pose[c];
    }
  }
  __syncthreads();
  for (int l = t; l < w.L; l += BA_THREADS) {
    float X[3], c[3];
    ba_load_point(P, l, X);
    c[0] = X[0]; c[1] = X[1]; c[2] = X[2];
    if (w.ws[(size_t)BA_ACT * w.Lp + l] != 0.0f) {
      float vi[6], s[3];
#pragma unroll
      for (int k = 0; k < 6; ++k) vi[k] = w.ws[(size_t)(BA_VI + k) * w.Lp + l];
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = w.ws[(size_t)(BA_H + k) * w.Lp + l];
      for (int f = w.nf; f < w.F; ++f) {
        BaLine q;
        if (!ba_obs_line(w, S.rt, X, f, l, q)) continue;
        const float *d = &S.dp[6 * (f - w.nf)];
        float su = q.ju[0] * d[0], sv = q.jv[0] * d[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) { su = su + q.ju[i] * d[i]; sv = sv + q.jv[i] * d[i]; }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          s[a] += (q.w * q.xu[a]) * su;
          s[a] += (q.w * q.xv[a]) * sv;
        }
      }
      c[0] = X[0] + -((vi[0] * s[0] + vi[1] * s[1]) + vi[2] * s[2]);
      c[1] = X[1] + -((vi[1] * s[0] + vi[3] * s[1]) + vi[4] * s[2]);
      c[2] = X[2] + -((vi[2] * s[0] + vi[4] * s[1]) + vi[5] * s[2]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) w.ws[(size_t)(BA_CAND + a) * w.Lp + l] = c[a];
  }
}

__device__ __forceinline__ void ba_stage_poses(BaShared &S, const float *r, const float *t, int F) {
  for (int e = threadIdx.x; e < F * 12; e += BA_THREADS) {
    const int f = e / 12, c = e % 12;
    const float v = c < 9 ? r[(size_t)f * 9 + c] : t[(size_t)f * 3 + (c - 9)];
    S.rt[f][c] = v;
    S.crt[f][c] = v;
    S.pose[f][c] = (double)v;
    S.cand[f][c] = (double)v;
  }
  __syncthreads();
}

// the reduced system as the full symmetric (6F, 6F) float32 matrix, zero in the fixed frames' rows and columns (and
// everywhere when !fill)
__device__ __forceinline__ void ba_write_system(const BaShared &S, const BaWin &w, bool fill, float *__restrict__ out) {
  const int m = 6 * w.F, off = 6 * w.nf, n = m - off;
  for (int e = threadIdx.x; e < m * m; e += BA_THREADS) {
    const int i = e / m - off, j = e % m - off;
    float v = 0.0f;
    if (fill && i >= 0 && j >= 0) v = (float)S.s[i <= j ? ba_tri(n, i, j) : ba_tri(n, j, i)];
    out[e] = v;
  }
}

__device__ __forceinline__ BaWin ba_window(const float *obs, const uint8_t *vis, float *ws, int F, int L, int nf, float huber) {
  const size_t b = blockIdx.x;
  BaWin w;
  w.F = F; w.L = L; w.Lp = ba_lp(L); w.nf = nf; w.huber = huber;
  w.obs = obs + b * F * L * 2;
  w.vis = vis + b * F * L;
  w.ws = ws ? ws + b * BA_ROWS * w.Lp : nullptr;
  return w;
}

// ---- K25a ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BA_THREADS) void ba_cost_kernel(const float *__restrict__ r, const float *__restrict__ t,
                                                             const float *__restrict__ pts, const float *__restrict__ obs,
                                                             const uint8_t *__restrict__ vis, int F, int L, float huber,
                                                             float *__restrict__ e2, float *__restrict__ cost,
                                                             uint8_t *__restrict__ active) {
  __shared__ BaCostShared S;
  const size_t b = blockIdx.x;
  const BaWin w = ba_window(obs, vis, nullptr, F, L, F, huber);
  for (int e = threadIdx.x; e < F * 12; e += BA_THREADS) {
    const int f = e / 12, c = e % 12;
    S.rt[f][c] = c < 9 ? r[(b * F + f) * 9 + c] : t[(b * F + f) * 3 + (c - 9)];
  }
  __syncthreads();
  const BaPts P{pts + b * L * 3, 3, 1};
  int nact;
  const double c = ba_cost_pass<true>(S, w, S.rt, P, e2 + b * F * L, active + b * L, &nact);
  if (threadIdx.x == 0) cost[b] = (float)c;
}

// ---- K25b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BA_THREADS) void ba_linearise_kernel(const float *__restrict__ r, const float *__restrict__ t,
                                                                  const float *__restrict__ pts, const float *__restrict__ obs,
                                                                  const uint8_t *__restrict__ vis, int F, int L, int nf, float huber,
                                                                  float *__restrict__ s_out, float *__restrict__ b_out,
                                                                  float *__restrict__ cost, float *__restrict__ ws) {
  __shared__ BaShared S;
  const size_t b = blockIdx.x;
  const BaWin w = ba_window(obs, vis, ws, F, L, nf, huber);
  ba_stage_poses(S, r + b * F * 9, t + b * F * 3, F);
  const BaPts P{pts + b * L * 3, 3, 1};
  int nact;
  const double c = ba_cost_pass<false>(S, w, S.rt, P, nullptr, nullptr, &nact);
  ba_pass_a(w, S.rt, P, 0.0f);
  ba_pass_b(S, w, S.rt, P, 0.0);
  ba_write_system(S, w, true, s_out + b * 36 * F * F);
  for (int e = threadIdx.x; e < 6 * F; e += BA_THREADS) b_out[b * 6 * F + e] = e >= 6 * nf ? (float)S.x[e - 6 * nf] : 0.0f;
  if (threadIdx.x == 0) cost[b] = (float)c;
}

// ---- K25c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BA_THREADS) void ba_refine_kernel(const float *__restrict__ r0, const float *__restrict__ t0,
                                                               const float *__restrict__ pts0, const float *__restrict__ obs,
                                                               const uint8_t *__restrict__ vis, int F, int L, int nf, int iterations,
                                                               float huber, float *__restrict__ r_out, float *__restrict__ t_out,
                                                               float *__restrict__ pts_out, uint8_t *__restrict__ point_ok,
                                                               float *__restrict__ cost0_out, float *__restrict__ cost_out,
                                                               int *__restrict__ accepted_out, float *__restrict__ info_out,
                                                               uint8_t *__restrict__ ok_out, float *__restrict__ ws) {
  __shared__ BaShared S;
  const size_t b = blockIdx.x;
  const int t = threadIdx.x, n = 6 * (F - nf);
  const BaWin w = ba_window(obs, vis, ws, F, L, nf, huber);
  ba_stage_poses(S, r0 + b * F * 9, t0 + b * F * 3, F);
  float *pts = pts_out + b * L * 3;                       // the state's points: every row is read and written by its owner alone
  for (int l = t; l < L; l += BA_THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) pts[(size_t)l * 3 + a] = pts0[(b * L + l) * 3 + a];
  }
  const BaPts P{pts, 3, 1}, C{w.ws + (size_t)BA_CAND * w.Lp, 1, w.Lp};
  int nact, accepted = 0;
  const double cost0 = ba_cost_pass<false>(S, w, S.rt, P, nullptr, nullptr, &nact);
  double cost = cost0;
  const bool refused = !(cost0 < INFINITY) || nact == 0;  // the same in every thread
  if (!refused) {
    double lambda = BA_LAMBDA0;
#pragma unroll 1
    for (int it = 0; it < iterations; ++it) {
      ba_pass_a(w, S.rt, P, (float)lambda);
      ba_pass_b(S, w, S.rt, P, lambda);
      const bool usable = ba_ldlt_solve(S.s, S.x, n, t, BA_THREADS, [] { __syncthreads(); });
      __syncthreads();
      double c = INFINITY;
      if (usable) {
        ba_pass_c(S, w, P);
        int na;
        c = ba_cost_pass<false>(S, w, S.crt, C, nullptr, nullptr, &na);
      }
      if (usable && c < INFINITY && c < cost) {
        for (int e = t; e < F * 12; e += BA_THREADS) {
          S.pose[e / 12][e % 12] = S.cand[e / 12][e % 12];
          S.rt[e / 12][e % 12] = S.crt[e / 12][e % 12];
        }
        for (int l = t; l < L; l += BA_THREADS) {
#pragma unroll
          for (int a = 0; a < 3; ++a) pts[(size_t)l * 3 + a] = w.ws[(size_t)(BA_CAND + a) * w.Lp + l];
        }
        cost = c;
        ++accepted;
        lambda = lambda / BA_LAMBDA_STEP > BA_LAMBDA_MIN ? lambda / BA_LAMBDA_STEP : BA_LAMBDA_MIN;
      } else {
        lambda = lambda * BA_LAMBDA_STEP < BA_LAMBDA_MAX ? lambda * BA_LAMBDA_STEP : BA_LAMBDA_MAX;
      }
      __syncthreads();
    }
    ba_pass_a(w, S.rt, P, 0.0f);
    ba_pass_b(S, w, S.rt, P, 0.0);
  }
  ba_write_system(S, w, !refused, info_out + b * 36 * F * F);
  for (int e = t; e < F * 12; e += BA_THREADS) {
    const int f = e / 12, c = e % 12;
    if (c < 9) r_out[(b * F + f) * 9 + c] = S.rt[f][c];
    else t_out[(b * F + f) * 3 + (c - 9)] = S.rt[f][c];
  }
  for (int l = t; l < L; l += BA_THREADS) point_ok[b * L + l] = (!refused && w.ws[(size_t)BA_ACT * w.Lp + l] != 0.0f) ? 1 : 0;
  if (t == 0) {
    cost0_out[b] = (float)cost0;
    cost_out[b] = (float)cost;
    accepted_out[b] = accepted;
    ok_out[b] = refused ? 0 : 1;
  }
}

int ba_shape_status(int batch, int frames, int landmarks) {
  if (batch < 1 || frames < 2 || landmarks < 1) return MI_E_SHAPE;
  if (batch > 65535 || frames > MI_BA_MAX_FRAMES || landmarks > MI_BA_MAX_LANDMARKS) return MI_E_PARAM;
  return MI_OK;
}
bool ba_huber_ok(float huber) { return huber >= 0.0f && huber < INFINITY; }
int ba_workspace_status(const void *workspace, size_t bytes, int batch, int frames, int landmarks) {
  if (((uintptr_t)workspace % 16) != 0) return MI_E_ALIGN;
  if (bytes < mi_ba_workspace_bytes(batch, frames, landmarks)) return MI_E_CAPACITY;
  return MI_OK;
}

}  // namespace

extern "C" int mi_ba_cost(const float *r, const float *t, const float *points, const float *obs, const uint8_t *vis, int batch,
                          int frames, int landmarks, float huber, float *e2, float *cost, uint8_t *active, mi_stream_t stream) {
  MI_ENTER();
  if (!r || !t || !points || !obs || !vis || !e2 || !cost || !active) return MI_E_NULL;
  if (const int s = ba_shape_status(batch, frames, landmarks)) return s;
  if (!ba_huber_ok(huber)) return MI_E_PARAM;
  hipLaunchKernelGGL(ba_cost_kernel, dim3((unsigned)batch), dim3(BA_THREADS), 0, (hipStream_t)stream, r, t, points, obs, vis, frames,
                     landmarks, huber, e2, cost, active);
  return mi_launch_status();
}

extern "C" size_t mi_ba_workspace_bytes(int batch, int frames, int landmarks) {
  if (ba_shape_status(batch, frames, landmarks) != MI_OK) return 0;
  return (size_t)batch * BA_ROWS * (size_t)((landmarks + 3) & ~3) * sizeof(float);
}

extern "C" int mi_ba_linearise(const float *r, const float *t, const float *points, const float *obs, const uint8_t *vis, int batch,
                               int frames, int landmarks, int num_fixed, float huber, float *s, float *b, float *cost,
                               void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!r || !t || !points || !obs || !vis || !s || !b || !cost || !workspace) return MI_E_NULL;
  if (const int st = ba_shape_status(batch, frames, landmarks)) return st;
  if (num_fixed < 1 || num_fixed > frames || !ba_huber_ok(huber)) return MI_E_PARAM;
  if (const int st = ba_workspace_status(workspace, workspace_bytes, batch, frames, landmarks)) return st;
  hipLaunchKernelGGL(ba_linearise_kernel, dim3((unsigned)batch), dim3(BA_THREADS), 0, (hipStream_t)stream, r, t, points, obs, vis,
                     frames, landmarks, num_fixed, huber, s, b, cost, (float *)workspace);
  return mi_launch_status();
}

extern "C" int mi_ba_refine(const float *r0, const float *t0, const float *points0, const float *obs, const uint8_t *vis, int batch,
                            int frames, int landmarks, int num_fixed, int iterations, float huber, float *r, float *t, float *points,
                            uint8_t *point_ok, float *cost0, float *cost, int32_t *accepted, float *info, uint8_t *ok,
                            void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!r0 || !t0 || !points0 || !obs || !vis || !r || !t || !points || !point_ok || !cost0 || !cost || !accepted || !info || !ok ||
      !workspace)
    return MI_E_NULL;
  if (const int st = ba_shape_status(batch, frames, landmarks)) return st;
  if (num_fixed < 1 || num_fixed > frames || iterations < 1 || iterations > MI_BA_MAX_ITERATIONS || !ba_huber_ok(huber))
    return MI_E_PARAM;
  if (const int st = ba_workspace_status(workspace, workspace_bytes, batch, frames, landmarks)) return st;
  hipLaunchKernelGGL(ba_refine_kernel, dim3((unsigned)batch), dim3(BA_THREADS), 0, (hipStream_t)stream, r0, t0, points0, obs, vis,
                     frames, landmarks, num_fixed, iterations, huber, r, t, points, point_ok, cost0, cost, accepted, info, ok,
                     (float *)workspace);
  return mi_launch_status();
}
