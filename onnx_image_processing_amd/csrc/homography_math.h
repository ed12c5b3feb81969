// The arithmetic of K24 (homography.hip; include/mi355x_match.h, "planar two-view pose"): the 4-point homography through
// the projective bases of the two quadruples, the symmetric transfer error, the completion of a 3x3 matrix to the 18-float
// model (H, then its sign-matched adjugate G, both of unit Frobenius norm) and the decomposition of a homography into its
// four (R, T, N) candidates (Ma, Soatto, Kosecka, Sastry, "An Invitation to 3-D Vision", section 5.3.3).  float32 arithmetic,
// callable on the host as well (tests/native/homography_host.cpp runs it without a GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "essential_math.h"    // cross3, matvec3, det3
#include "rigid_math.h"        // rg_jacobi, RG_DEGENERATE: K17's collinearity constant

namespace {

// HG_ROTATION_TOL: a homography scaled to middle singular value 1 with w1 - w3 at or below this is a pure rotation
// (w1 >= w2 >= w3 the eigenvalues of H^T H / w2).  Measured by tests/test_homography_host.py
// (test_rotation_tolerance_is_its_measurement) on the noise-free rotation-only scenes of tests/test_gpu_homography.py
// (synth_planar_two_view seeds 0 .. 5, baseline 0, 97 rows, 25 % outliers; the oracle's whole RANSAC at 256 hypotheses):
// w1 - w3 is at most 1.60e-7 in float64 and at most 1.61e-6 in the oracle's float32 run, the largest deviation between the
// two 1.473e-6; 4 x that is 5.9e-6.  The smallest w1 - w3 of the translating scenes (seeds 1, 2, 3, 5, 6, 7, baseline 0.4)
// is 1.58e-1: 27000 times the constant.
constexpr float HG_ROTATION_TOL = 5.9e-6f;
constexpr int HG_MIN_POSE_ROWS = 4;       // mi_homography_pose: slot 0 must pass at least this many rows

// twice the signed area of the triangle (a, b, c) = det [a b c] for homogeneous (x, y, 1)
__host__ __device__ __forceinline__ float hg_tri(float ax, float ay, float bx, float by, float cx, float cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// K17's rule on three image points: with e1 = b - a, e2 = c - a, degenerate when |e1 x e2|^2 <= 1e-6 |e1|^2 |e2|^2
// (collinear or repeated points; not finite: degenerate)
__host__ __device__ __forceinline__ bool hg_collinear(float ax, float ay, float bx, float by, float cx, float cy) {
  const float e1x = bx - ax, e1y = by - ay, e2x = cx - ax, e2y = cy - ay;
  const float cz = e1x * e2y - e1y * e2x;
  const float n1 = e1x * e1x + e1y * e1y, n2 = e2x * e2x + e2y * e2y;
  return !(cz * cz > RG_DEGENERATE * n1 * n2);
}

// g = adj(h) (G H = det(H) I), negated when det H < 0 and scaled to unit Frobenius norm: a POSITIVE multiple of H^-1.
// Returns false when det H is 0 or anything is not finite (g is then unspecified).
__host__ __device__ __forceinline__ bool hg_adjugate(const float *h, float *g) {
  // row i of adj(H) is (column i+1 of H) x (column i+2 of H), transposed: adj[r][c] = cofactor[c][r]
  g[0] = h[4] * h[8] - h[5] * h[7];
  g[1] = h[2] * h[7] - h[1] * h[8];
  g[2] = h[1] * h[5] - h[2] * h[4];
  g[3] = h[5] * h[6] - h[3] * h[8];
  g[4] = h[0] * h[8] - h[2] * h[6];
  g[5] = h[2] * h[3] - h[0] * h[5];
  g[6] = h[3] * h[7] - h[4] * h[6];
  g[7] = h[1] * h[6] - h[0] * h[7];
  g[8] = h[0] * h[4] - h[1] * h[3];
  const float det = (h[0] * g[0] + h[1] * g[3]) + h[2] * g[6];
  float nn = 0.0f;
#pragma unroll
  for (int c = 0; c < 9; ++c) nn += g[c] * g[c];
  const float sc = (det < 0.0f ? -1.0f : 1.0f) / sqrtf(nn);
#pragma unroll
  for (int c = 0; c < 9; ++c) g[c] = g[c] * sc;
  return det != 0.0f && fabsf(det) < INFINITY && nn > 0.0f && nn < INFINITY;
}

// m = (H scaled to unit Frobenius norm and multiplied by sg, then G = hg_adjugate(H)).  False: H is zero, singular or not
// finite.
__host__ __device__ __forceinline__ bool hg_complete(const float *h, float sg, float *m) {
  float nn = 0.0f;
#pragma unroll
  for (int c = 0; c < 9; ++c) nn += h[c] * h[c];
  const float sc = sg / sqrtf(nn);
#pragma unroll
  for (int c = 0; c < 9; ++c) m[c] = h[c] * sc;
  const bool ok = hg_adjugate(m, m + 9);
  float chk = 0.0f;
#pragma unroll
  for (int c = 0; c < 18; ++c) chk += fabsf(m[c]);
  return ok && nn > 0.0f && chk < INFINITY;    // false for NaN and infinities
}

// H = T2^-1 H_hat T1 for the Hartley parameters h1 / h2 = (cx, cy, s) of image 1 / 2: T = [s 0 -s cx; 0 s -s cy; 0 0 1]
__host__ __device__ __forceinline__ void hg_denormalise(const float *hh, const float *h1, const float *h2, float *h) {
  float a[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {                                       // A = H_hat T1
    a[3 * r + 0] = hh[3 * r + 0] * h1[2];
    a[3 * r + 1] = hh[3 * r + 1] * h1[2];
    a[3 * r + 2] = hh[3 * r + 2] - ((hh[3 * r + 0] * h1[2]) * h1[0] + (hh[3 * r + 1] * h1[2]) * h1[1]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {                                       // H = T2^-1 A, T2^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1]
    h[c] = a[c] / h2[2] + h2[0] * a[6 + c];
    h[3 + c] = a[3 + c] / h2[2] + h2[1] * a[6 + c];
    h[6 + c] = a[6 + c];
  }
}

// the third coordinate of H X1 for X1 = (x, y, 1)
__host__ __device__ __forceinline__ float hg_w(const float *h, float x, float y) { return (h[6] * x + h[7] * y) + h[8]; }

// The model of one 4-sample (header: "Solve").  False: a collinear triple in either image, a sample the homography takes
// through the plane at infinity, or no finite, invertible result.
__host__ __device__ inline bool hg_solve_minimal(const float4 *q, float *m) {
  // the four triples of either image
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = a + 1; b < 3; ++b)
#pragma unroll
      for (int c = b + 1; c < 4; ++c)
        if (hg_collinear(q[a].x, q[a].y, q[b].x, q[b].y, q[c].x, q[c].y) ||
            hg_collinear(q[a].z, q[a].w, q[b].z, q[b].w, q[c].z, q[c].w))
          return false;
  // Hartley normalisation of the sample: centroid, then sqrt(2) over the RMS distance to it
  float h1[3], h2[3];
  h1[0] = (((q[0].x + q[1].x) + q[2].x) + q[3].x) / 4.0f;
  h1[1] = (((q[0].y + q[1].y) + q[2].y) + q[3].y) / 4.0f;
  h2[0] = (((q[0].z + q[1].z) + q[2].z) + q[3].z) / 4.0f;
  h2[1] = (((q[0].w + q[1].w) + q[2].w) + q[3].w) / 4.0f;
  float d1 = 0.0f, d2 = 0.0f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float ax = q[s].x - h1[0], ay = q[s].y - h1[1], bx = q[s].z - h2[0], by = q[s].w - h2[1];
    d1 += ax * ax + ay * ay;
    d2 += bx * bx + by * by;
  }
  if (!(d1 > 0.0f && d2 > 0.0f)) return false;
  h1[2] = sqrtf(2.0f) / sqrtf(d1 / 4.0f);
  h2[2] = sqrtf(2.0f) / sqrtf(d2 / 4.0f);
  // per image the projective basis B = [l0 p0, l1 p1, l2 p2] with [p0 p1 p2] l = p3 by cofactors (Cramer's numerators;
  // the common denominator det [p0 p1 p2] scales B and is left out: H is defined up to scale)
  float bm[2][3][3];
#pragma unroll
  for (int im = 0; im < 2; ++im) {
    float x[4], y[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      x[s] = im ? (q[s].z - h2[0]) * h2[2] : (q[s].x - h1[0]) * h1[2];
      y[s] = im ? (q[s].w - h2[1]) * h2[2] : (q[s].y - h1[1]) * h1[2];
    }
    const float l0 = hg_tri(x[3], y[3], x[1], y[1], x[2], y[2]);
    const float l1 = hg_tri(x[0], y[0], x[3], y[3], x[2], y[2]);
    const float l2 = hg_tri(x[0], y[0], x[1], y[1], x[3], y[3]);
    const float l[3] = {l0, l1, l2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bm[im][0][c] = l[c] * x[c];
      bm[im][1][c] = l[c] * y[c];
      bm[im][2][c] = l[c];
    }
  }
  // H_hat = B2 adj(B1); row i of adj(B1) is column (i+1) x column (i+2) of B1
  float adj[3][3];
  {
    const float c0[3] = {bm[0][0][0], bm[0][1][0], bm[0][2][0]}, c1[3] = {bm[0][0][1], bm[0][1][1], bm[0][2][1]},
                c2[3] = {bm[0][0][2], bm[0][1][2], bm[0][2][2]};
    cross3(c1, c2, adj[0]);
    cross3(c2, c0, adj[1]);
    cross3(c0, c1, adj[2]);
  }
  float hh[9], h[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) hh[3 * r + c] = (bm[1][r][0] * adj[0][c] + bm[1][r][1] * adj[1][c]) + bm[1][r][2] * adj[2][c];
  hg_denormalise(hh, h1, h2, h);
  // sign: (H X1)_2 > 0 at sample point 0, and then at the other three as well
  const float w0 = hg_w(h, q[0].x, q[0].y);
  const float sg = w0 < 0.0f ? -1.0f : 1.0f;
  if (!hg_complete(h, sg, m)) return false;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (!(hg_w(m, q[s].x, q[s].y) > 0.0f)) return false;
  return true;
}

// squared symmetric transfer error of one correspondence under m = (H, G) (header: "Score"); +inf where either third
// coordinate is not positive
__host__ __device__ __forceinline__ float hg_dist2(const float *m, float4 q) {
  const float hx = (m[0] * q.x + m[1] * q.y) + m[2], hy = (m[3] * q.x + m[4] * q.y) + m[5], hw = (m[6] * q.x + m[7] * q.y) + m[8];
  const float gx = (m[9] * q.z + m[10] * q.w) + m[11], gy = (m[12] * q.z + m[13] * q.w) + m[14],
              gw = (m[15] * q.z + m[16] * q.w) + m[17];
  const float ax = q.z - hx / hw, ay = q.w - hy / hw, bx = q.x - gx / gw, by = q.y - gy / gw;
  const float d2 = ((ax * ax + ay * ay) + bx * bx) + by * by;
  return (hw > 0.0f && gw > 0.0f) ? d2 : INFINITY;
}

// ---- decomposition (header: mi_homography_pose) -------------------------------------------------------------------------------
struct HgPose {
  float r[4][9], t[4][3], n[4][3];   // the four candidates: 0 (R+, T+, N+), 1 (R-, T-, N-), 2 (R+, -T+, -N+), 3 (R-, -T-, -N-)
  float spread;                      // w1 - w3 of H^T H / w2
  bool rotation_only;                // spread <= HG_ROTATION_TOL: candidate 0 is (nearest rotation, 0, 0), the others copies
};

// one Newton step towards the nearest rotation, R (3 I - R^T R) / 2, as mi_recover_pose's
__host__ __device__ __forceinline__ void hg_newton(const float *r0, float *r) {
  float g[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      g[a][b] = (a == b ? 3.0f : 0.0f) - ((r0[a] * r0[b] + r0[3 + a] * r0[3 + b]) + r0[6 + a] * r0[6 + b]);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) r[3 * a + b] = 0.5f * ((r0[3 * a] * g[0][b] + r0[3 * a + 1] * g[1][b]) + r0[3 * a + 2] * g[2][b]);
}

// The four candidates of h (unit Frobenius norm, its sign already chosen).  False: no finite result.
__host__ __device__ inline bool hg_decompose(const float *h, HgPose &p) {
  float a[3][3], v[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[r][c] = (h[r] * h[c] + h[3 + r] * h[3 + c]) + h[6 + r] * h[6 + c];   // H^T H
  rg_jacobi<3>(a, v);
  // eigenvalues in descending order (the lower index first among equals), eigenvectors the matching columns of v
  float w[3] = {a[0][0], a[1][1], a[2][2]};
  int o[3] = {0, 1, 2};
#pragma unroll
  for (int pass = 0; pass < 2; ++pass)
#pragma unroll
    for (int k = 0; k < 2 - pass; ++k)
      if (w[k + 1] > w[k]) {
        const float tw = w[k]; w[k] = w[k + 1]; w[k + 1] = tw;
        const int to = o[k]; o[k] = o[k + 1]; o[k + 1] = to;
      }
  float e[3][3];                                                      // e[k]: eigenvector k, sign: largest component positive
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = o[k] == 0 ? v[r][0] : (o[k] == 1 ? v[r][1] : v[r][2]);
    float big = x[0];
    if (fabsf(x[1]) > fabsf(big)) big = x[1];
    if (fabsf(x[2]) > fabsf(big)) big = x[2];
    const float sg = big < 0.0f ? -1.0f : 1.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) e[k][r] = sg * x[r];
  }
  if (!(w[1] > 0.0f) || !(w[0] < INFINITY)) return false;
  const float inv = 1.0f / sqrtf(w[1]);
  float hs[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) hs[r][c] = h[3 * r + c] * inv;          // middle singular value 1
  const float w1 = w[0] / w[1], w3 = w[2] / w[1];
  p.spread = w1 - w3;
  p.rotation_only = !(p.spread > HG_ROTATION_TOL);
  float chk = 0.0f;
  if (p.rotation_only) {
    // the nearest rotation: H (H^T H)^(-1/2) = H sum_k e_k e_k^T / sqrt(w_k / w2), then the Newton step
    float s[3][3], r0[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        s[r][c] = ((e[0][r] * e[0][c]) / sqrtf(w1) + e[1][r] * e[1][c]) + (e[2][r] * e[2][c]) / sqrtf(w3);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) r0[3 * r + c] = (hs[r][0] * s[0][c] + hs[r][1] * s[1][c]) + hs[r][2] * s[2][c];
    hg_newton(r0, p.r[0]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int c = 0; c < 9; ++c) { p.r[k][c] = p.r[0][c]; chk += fabsf(p.r[k][c]); }
#pragma unroll
      for (int c = 0; c < 3; ++c) p.t[k][c] = p.n[k][c] = 0.0f;
    }
    return chk < INFINITY;
  }
  const float ca = sqrtf(fmaxf(1.0f - w3, 0.0f)), cb = sqrtf(fmaxf(w1 - 1.0f, 0.0f)), den = sqrtf(w1 - w3);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float u[3], nrm[3], hv[3], hu[3], hx[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) u[r] = (k ? ca * e[0][r] - cb * e[2][r] : ca * e[0][r] + cb * e[2][r]) / den;
    cross3(e[1], u, nrm);                                            // N = v2 x u
    matvec3(hs, e[1], hv);
    matvec3(hs, u, hu);
    cross3(hv, hu, hx);
    // R = W U^T with U = [v2, u, N], W = [H v2, H u, H v2 x H u]
    float r0[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) r0[3 * r + c] = (hv[r] * e[1][c] + hu[r] * u[c]) + hx[r] * nrm[c];
    hg_newton(r0, p.r[k]);
    // T = (H - R) N
#pragma unroll
    for (int r = 0; r < 3; ++r)
      p.t[k][r] = ((hs[r][0] - p.r[k][3 * r]) * nrm[0] + (hs[r][1] - p.r[k][3 * r + 1]) * nrm[1]) + (hs[r][2] - p.r[k][3 * r + 2]) * nrm[2];
#pragma unroll
    for (int c = 0; c < 9; ++c) { p.r[k + 2][c] = p.r[k][c]; chk += fabsf(p.r[k][c]); }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p.n[k][c] = nrm[c];
      p.t[k + 2][c] = -p.t[k][c];
      p.n[k + 2][c] = -nrm[c];
      chk += fabsf(p.t[k][c]) + fabsf(nrm[c]);
    }
  }
  return chk < INFINITY;
}

// a row passes under (R, T, N) when both depths, in units of the plane's distance, are positive: N . X1 > 0 and
// ((R X1) / (N . X1) + T)_2 > 0
__host__ __device__ __forceinline__ bool hg_in_front(const float *r, const float *t, const float *n, float4 q) {
  const float d1 = (n[0] * q.x + n[1] * q.y) + n[2];
  const float z2 = ((r[6] * q.x + r[7] * q.y) + r[8]) / d1 + t[2];
  return d1 > 0.0f && z2 > 0.0f;
}

// x2^T H x1 of one correspondence: its sign over the rows chooses the sign of H
__host__ __device__ __forceinline__ float hg_bilinear(const float *h, float4 q) {
  const float hx = (h[0] * q.x + h[1] * q.y) + h[2], hy = (h[3] * q.x + h[4] * q.y) + h[5], hw = (h[6] * q.x + h[7] * q.y) + h[8];
  return (q.z * hx + q.w * hy) + hw;
}

// the order of the four candidates: by passing count, descending; equal counts by the larger trace of R, then by index
__host__ __device__ __forceinline__ void hg_order(const int *cnt, const float *trace, int *order) {
#pragma unroll
  for (int k = 0; k < 4; ++k) order[k] = k;
#pragma unroll
  for (int pass = 0; pass < 3; ++pass)
#pragma unroll
    for (int k = 0; k < 3 - pass; ++k) {
      const int a = order[k], b = order[k + 1];
      const bool swap = cnt[b] > cnt[a] || (cnt[b] == cnt[a] && trace[b] > trace[a]);     // stable: index order among equals
      if (swap) { order[k] = b; order[k + 1] = a; }
    }
}

}  // namespace
