// The arithmetic of K25 (ba.hip; include/mi355x_match.h, "windowed bundle adjustment"): one observation's lines -- K23's
// pnp_lines with the point block J_x, the Huber weight and rho --, the sums a landmark and a frame collect from them, the
// closed-form inverse of a landmark's damped 3x3 block and the LDL^T solve of the reduced system on a packed upper
// triangle.  Per-observation work is float32, the solve float64; only + - * / and sqrt.  tests/native/ba_host.cpp runs it
// without a GPU and compares bits with tests/ba_oracle.py.
#pragma once
#include "pnp_math.h"     // first: rigid_math.h brings the HIP markers icp_math.h uses under hipcc
#include "icp_math.h"

#include <math.h>

namespace {

constexpr double BA_LAMBDA0 = 1e-4, BA_LAMBDA_MIN = 1e-9, BA_LAMBDA_MAX = 1e6, BA_LAMBDA_STEP = 10.0;

// one visible observation of an active landmark
struct BaLine {
  float ju[6], jv[6];      // K23's pose lines
  float xu[3], xv[3];      // the point lines: rows of [[iz, 0, -xn iz], [0, iz, -yn iz]] R
  float ru, rv, e2, w, rho;
};

// rt: (R row-major, t) of the frame, X the landmark, (u, v) the normalised observation.  false (nothing to add, rho = +inf):
// z <= 0 or e2 not finite.
__host__ __device__ __forceinline__ bool ba_line(const float *rt, const float *X, float u, float v, float huber, BaLine &o) {
  PnpRow q;
  q.X[0] = X[0]; q.X[1] = X[1]; q.X[2] = X[2];
  q.u = u; q.v = v;
  const bool front = pnp_lines(rt, q, o.ju, o.jv, &o.ru, &o.rv);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o.xu[j] = o.ju[3] * rt[j] + o.ju[5] * rt[6 + j];
    o.xv[j] = o.jv[4] * rt[3 + j] + o.jv[5] * rt[6 + j];
  }
  o.e2 = o.ru * o.ru + o.rv * o.rv;
  const bool ok = front && o.e2 < INFINITY;
  o.w = 1.0f;
  o.rho = o.e2;
  if (huber > 0.0f) {
    const float e = sqrtf(o.e2);
    if (e > huber) {
      o.w = huber / e;
      o.rho = (2.0f * huber) * e - huber * huber;
    }
  }
  if (!ok) o.rho = INFINITY;
  return ok;
}

// the cost's term alone (K23's Score arithmetic: the same x / z - u as ba_line): e2 = +inf for z <= 0 or a non-finite value
__host__ __device__ __forceinline__ float ba_rho(const float *rt, const float *X, float u, float v, float huber, float *e2) {
  PnpRow q;
  q.X[0] = X[0]; q.X[1] = X[1]; q.X[2] = X[2];
  q.u = u; q.v = v;
  *e2 = pnp_dist2(rt, q);
  if (!(*e2 < INFINITY)) return INFINITY;
  if (huber > 0.0f) {
    const float e = sqrtf(*e2);
    if (e > huber) return (2.0f * huber) * e - huber * huber;
  }
  return *e2;
}

// V (00 01 02 11 12 22) and h of a landmark: the u line, then the v line
__host__ __device__ __forceinline__ void ba_add_point(const BaLine &o, float *V, float *h) {
  float wu[3], wv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { wu[i] = o.w * o.xu[i]; wv[i] = o.w * o.xv[i]; }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      V[k] += wu[i] * o.xu[j];
      V[k] += wv[i] * o.xv[j];
      ++k;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    h[i] += wu[i] * o.ru;
    h[i] += wv[i] * o.rv;
  }
}

// W = w J_p^T J_x (6 x 3, row-major)
__host__ __device__ __forceinline__ void ba_cross(const BaLine &o, float *W) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const float a = o.w * o.ju[i], b = o.w * o.jv[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) W[i * 3 + c] = a * o.xu[c] + b * o.xv[c];
  }
}

// U's upper triangle (21, row-major) and g (6) of a frame: the u line, then the v line
__host__ __device__ __forceinline__ void ba_add_pose(const BaLine &o, float *U, float *g) {
  float wu[6], wv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) { wu[i] = o.w * o.ju[i]; wv[i] = o.w * o.jv[i]; }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      U[k] += wu[i] * o.ju[j];
      U[k] += wv[i] * o.jv[j];
      ++k;
    }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    g[i] += wu[i] * o.ru;
    g[i] += wv[i] * o.rv;
  }
}

// Y = W Vi (6 x 3) for the symmetric Vi (00 01 02 11 12 22)
__host__ __device__ __forceinline__ void ba_times_sym(const float *W, const float *vi, float *Y) {
  const float m[3][3] = {{vi[0], vi[1], vi[2]}, {vi[1], vi[3], vi[4]}, {vi[2], vi[4], vi[5]}};
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) Y[i * 3 + c] = (W[i * 3] * m[0][c] + W[i * 3 + 1] * m[1][c]) + W[i * 3 + 2] * m[2][c];
}

// Vi = (V + lambda diag V)^-1 by the adjugate, float32.  The pivots of the damped block's LDL^T are p0 = m00,
// p1 = (m00 m11 - m01^2) / m00, p2 = det / (m00 m11 - m01^2).  false (Vi = 0: the landmark is frozen for this step): the
// largest diagonal element is not positive, the smallest pivot is not above ICP_PIVOT_RATIO times it, or an element of
// the inverse is not finite.
__host__ __device__ __forceinline__ bool ba_inv3(const float *V, float lambda, float *vi) {
  const float m[6] = {V[0] + lambda * V[0], V[1], V[2], V[3] + lambda * V[3], V[4], V[5] + lambda * V[5]};
  float c[6];
  pnp_cof(m, c);
  const float det = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2];
  const float p1 = c[5] / m[0], p2 = det / c[5];
  float dmax = m[0] > m[3] ? m[0] : m[3];
  dmax = m[5] > dmax ? m[5] : dmax;
  float pmin = m[0] < p1 ? m[0] : p1;
  pmin = p2 < pmin ? p2 : pmin;
  bool ok = dmax > 0.0f && pmin > (float)ICP_PIVOT_RATIO * dmax;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    vi[k] = c[k] / det;
    ok = ok && fabsf(vi[k]) < INFINITY;
  }
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 6; ++k) vi[k] = 0.0f;
  }
  return ok;
}

// index of (r, c), r <= c, in the packed upper triangle of an n x n matrix, row-major
__host__ __device__ __forceinline__ int ba_tri(int n, int r, int c) { return r * n - (r * (r - 1)) / 2 + (c - r); }

// S x = -b for the symmetric S held as a packed upper triangle `a` (overwritten: d_j on the diagonal, l_ij at (j, i)) by
// LDL^T without pivoting, float64; x holds b on entry.  icp_solve's rule for n unknowns: false when max diag S is not
// positive, a pivot is not above ICP_PIVOT_RATIO * max diag S, or an element of x is not finite.  Every element sees its
// updates in the order of the sequential algorithm (column j = 0, 1, ...), so `nt` cooperating threads -- thread `tid`
// takes every nt-th element, sync() separates the phases -- return the bits of one thread.  n == 0: true.
template <class Sync>
__host__ __device__ inline bool ba_ldlt_solve(double *a, double *x, int n, int tid, int nt, Sync sync) {
  double dmax = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d = a[ba_tri(n, i, i)];
    dmax = (i == 0 || d > dmax) ? d : dmax;
  }
  if (n > 0 && !(dmax > 0.0)) return false;
  sync();
  for (int j = 0; j < n; ++j) {
    const double d = a[ba_tri(n, j, j)];
    if (!(d > ICP_PIVOT_RATIO * dmax) || !(d < INFINITY)) return false;      // the same in every thread
    const int row = ba_tri(n, j, j);
    for (int i = j + 1 + tid; i < n; i += nt) a[row + (i - j)] = a[row + (i - j)] / d;       // l_ij
    sync();
    const int m = n - 1 - j;                                                 // trailing block: rows / columns j + 1 .. n - 1
    for (int e = tid; e < m * m; e += nt) {
      const int r = j + 1 + e / m, c = j + 1 + e % m;
      if (r <= c) a[ba_tri(n, r, c)] -= (a[row + (r - j)] * a[row + (c - j)]) * d;
    }
    sync();
  }
  for (int i = 0; i < n; ++i) {                                              // L y = -b, column by column
    if (tid == 0) x[i] = i == 0 ? -x[0] : x[i];
    sync();
    const double yi = x[i];
    for (int k = i + 1 + tid; k < n; k += nt) x[k] = (i == 0 ? -x[k] : x[k]) - a[ba_tri(n, i, k)] * yi;
    sync();
  }
  for (int i = n - 1; i >= 0; --i) {                                         // L^T x = D^-1 y, column by column
    if (tid == 0) x[i] = i == n - 1 ? x[i] / a[ba_tri(n, i, i)] : x[i];
    sync();
    const double xi = x[i];
    for (int k = tid; k < i; k += nt) x[k] = (i == n - 1 ? x[k] / a[ba_tri(n, k, k)] : x[k]) - a[ba_tri(n, k, i)] * xi;
    sync();
  }
  bool finite = true;
  for (int i = 0; i < n; ++i) finite = finite && fabs(x[i]) < INFINITY;
  return finite;
}

}  // namespace
