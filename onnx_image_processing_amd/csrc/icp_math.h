// The arithmetic of K18 (icp.hip; include/mi355x_match.h, "dense RGB-D refinement"): the surfel maps' vertex and normal, one
// pixel's row of the point-to-plane system, the 6x6 LDL^T solve and the Rodrigues update of the pose.  Per-pixel work is
// float32, the solve and the pose float64.  No HIP header is needed: a plain C++ compiler builds it for the host as well
// (tests/native/icp_host.cpp runs it without a GPU).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ICP_HD __host__ __device__ __forceinline__
#else
#define ICP_HD inline
#endif

namespace {

constexpr int ICP_SUMS = 29;                 // 21 of A's upper triangle (row-major), 6 of b, sum r^2, count
constexpr double ICP_PIVOT_RATIO = 1e-6;     // smallest LDL^T pivot at or below this times max diag(A): degenerate
constexpr double ICP_SMALL_ANGLE = 1e-8;     // |omega| below this: Exp(omega) = I + [omega]x

// vertex of pixel (x, y) with depth d: the ray of mi_lift_keypoints, Z = d * z_scale; false (and zeros) when d is not
// finite or Z is outside [min_depth, max_depth]
ICP_HD bool icp_vertex(float d, float x, float y, const float *k_inv, float z_scale, float min_depth, float max_depth, float *v) {
  const float xn = (x * k_inv[0] + y * k_inv[1]) + k_inv[2];
  const float yn = (x * k_inv[3] + y * k_inv[4]) + k_inv[5];
  const float z = d * z_scale;
  const bool ok = fabsf(d) < INFINITY && z >= min_depth && z <= max_depth;
  v[0] = ok ? xn * z : 0.0f;
  v[1] = ok ? yn * z : 0.0f;
  v[2] = ok ? z : 0.0f;
  return ok;
}

// the normal at a valid centre c from its four VALID neighbours: left / right (x -+ 1), up / down (y -+ 1).  false (and
// zeros) when a neighbour's Z is further than max_jump from the centre's or the cross product is zero or not finite.
ICP_HD bool icp_normal(const float *c, const float *l, const float *r, const float *u, const float *d, float max_jump, float *n) {
  n[0] = n[1] = n[2] = 0.0f;
  if (!(fabsf(l[2] - c[2]) <= max_jump) || !(fabsf(r[2] - c[2]) <= max_jump) || !(fabsf(u[2] - c[2]) <= max_jump) ||
      !(fabsf(d[2] - c[2]) <= max_jump))
    return false;
  const float a[3] = {r[0] - l[0], r[1] - l[1], r[2] - l[2]}, b[3] = {d[0] - u[0], d[1] - u[1], d[2] - u[2]};
  const float m[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const float len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  if (!(len2 > 0.0f) || !(len2 < INFINITY)) return false;
  const float len = sqrtf(len2);
  float e[3] = {m[0] / len, m[1] / len, m[2] / len};
  const float facing = (e[0] * c[0] + e[1] * c[1]) + e[2] * c[2];
  const float s = facing > 0.0f ? -1.0f : 1.0f;                   // towards the camera
  n[0] = s * e[0];
  n[1] = s * e[1];
  n[2] = s * e[2];
  return true;
}

// R p (+ t): each component ((R_j0 x + R_j1 y) + R_j2 z) (+ t_j), K17's order
ICP_HD void icp_rotate(const float *R, const float *p, float *o) {
  o[0] = (R[0] * p[0] + R[1] * p[1]) + R[2] * p[2];
  o[1] = (R[3] * p[0] + R[4] * p[1]) + R[5] * p[2];
  o[2] = (R[6] * p[0] + R[7] * p[1]) + R[8] * p[2];
}

// the nearest pixel of q under the camera (fx, fy, cx, cy) as floats; false when q_z <= 0 or the pixel is outside the
// w x h frame (NaN fails every comparison)
ICP_HD bool icp_project(const float *q, float fx, float fy, float cx, float cy, int w, int h, float *px, float *py) {
  const float u = fx * (q[0] / q[2]) + cx, v = fy * (q[1] / q[2]) + cy;
  *px = floorf(u + 0.5f);
  *py = floorf(v + 0.5f);
  return q[2] > 0.0f && *px >= 0.0f && *px < (float)w && *py >= 0.0f && *py < (float)h;
}

// the distance and angle gates and, for a survivor, the row J = [q x n2, n2] and the residual r = n2 . (q - v2).
// rn1 is R n1.  false leaves J and r zero.
ICP_HD bool icp_row(const float *q, const float *rn1, const float *v2, const float *n2, float thr2, float cos_thr, float *J,
                    float *r) {
  const float d[3] = {q[0] - v2[0], q[1] - v2[1], q[2] - v2[2]};
  const float dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  const float dot = (rn1[0] * n2[0] + rn1[1] * n2[1]) + rn1[2] * n2[2];
  const bool ok = dist2 <= thr2 && dot >= cos_thr;
  J[0] = ok ? q[1] * n2[2] - q[2] * n2[1] : 0.0f;
  J[1] = ok ? q[2] * n2[0] - q[0] * n2[2] : 0.0f;
  J[2] = ok ? q[0] * n2[1] - q[1] * n2[0] : 0.0f;
  J[3] = ok ? n2[0] : 0.0f;
  J[4] = ok ? n2[1] : 0.0f;
  J[5] = ok ? n2[2] : 0.0f;
  *r = ok ? (n2[0] * d[0] + n2[1] * d[1]) + n2[2] * d[2] : 0.0f;
  return ok;
}

// acc[0..27] += the row's products (acc[28], the count, is kept by the caller): A's upper triangle row-major, then J r, r r
ICP_HD void icp_accumulate(const float *J, float r, float *acc) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) acc[k++] += J[i] * J[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r;
  acc[27] += r * r;
}

// A x = -b from the 29 sums by LDL^T without pivoting, float64.  false: count < min_count, the smallest pivot is not
// above ICP_PIVOT_RATIO * max diag(A), or anything is not finite.  *ratio = smallest pivot / max diag(A) (0 when unusable).
ICP_HD bool icp_solve(const double *s, int min_count, double *x, double *ratio) {
  double a[6][6], l[6][6], dg[6], y[6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { a[i][j] = s[k]; a[j][i] = s[k]; ++k; }
  *ratio = 0.0;
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  bool finite = true;
  for (int i = 0; i < ICP_SUMS; ++i) finite = finite && fabs(s[i]) < INFINITY;
  if (!finite || s[28] < (double)min_count) return false;
  double dmax = a[0][0];
  for (int i = 1; i < 6; ++i) dmax = a[i][i] > dmax ? a[i][i] : dmax;
  if (!(dmax > 0.0)) return false;
  double pmin = INFINITY;
  for (int j = 0; j < 6; ++j) {
    double d = a[j][j];
    for (int m = 0; m < j; ++m) d -= l[j][m] * l[j][m] * dg[m];
    dg[j] = d;
    pmin = d < pmin ? d : pmin;
    if (!(d > ICP_PIVOT_RATIO * dmax)) { *ratio = fabs(d) < INFINITY ? (d > 0.0 ? d / dmax : 0.0) : 0.0; return false; }
    for (int i = j + 1; i < 6; ++i) {
      double v = a[i][j];
      for (int m = 0; m < j; ++m) v -= l[i][m] * l[j][m] * dg[m];
      l[i][j] = v / d;
    }
  }
  *ratio = pmin / dmax;
  for (int i = 0; i < 6; ++i) {                    // L y = -b
    double v = -s[21 + i];
    for (int m = 0; m < i; ++m) v -= l[i][m] * y[m];
    y[i] = v;
  }
  for (int i = 5; i >= 0; --i) {                   // L^T x = D^-1 y
    double v = y[i] / dg[i];
    for (int m = i + 1; m < 6; ++m) v -= l[m][i] * x[m];
    x[i] = v;
  }
  for (int i = 0; i < 6; ++i) finite = finite && fabs(x[i]) < INFINITY;
  return finite;
}

// Exp(omega) by Rodrigues, row-major, float64; first order below ICP_SMALL_ANGLE
ICP_HD void icp_exp(const double *w, double *e) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
  double a = 1.0, b = 0.0;
  if (th >= ICP_SMALL_ANGLE) { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
  const double kx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double k2 = 0.0;
      for (int m = 0; m < 3; ++m) k2 += kx[i * 3 + m] * kx[m * 3 + j];
      e[i * 3 + j] = (i == j ? 1.0 : 0.0) + a * kx[i * 3 + j] + b * k2;
    }
}

// pose = (R row-major, t), 12 doubles: R <- Exp(omega) R, t <- Exp(omega) t + tau for x = (omega, tau)
ICP_HD void icp_update_pose(double *pose, const double *x) {
  double e[9], o[12];
  icp_exp(x, e);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = (e[i * 3] * pose[j] + e[i * 3 + 1] * pose[3 + j]) + e[i * 3 + 2] * pose[6 + j];
    o[9 + i] = ((e[i * 3] * pose[9] + e[i * 3 + 1] * pose[10]) + e[i * 3 + 2] * pose[11]) + x[3 + i];
  }
  for (int i = 0; i < 12; ++i) pose[i] = o[i];
}

}  // namespace
