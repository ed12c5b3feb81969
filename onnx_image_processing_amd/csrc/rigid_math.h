// The arithmetic of K17 (rigid.hip; include/mi355x_match.h, "metric RGB-D pose"): Horn's closed-form absolute orientation
// (J. Opt. Soc. Am. A 4, 1987) with the quaternion taken by cyclic Jacobi, the degeneracy tests and the point-to-point
// score.  float32 arithmetic but for the 32 float64 products of the eigenvector correction, callable on the host as well
// (tests/native/rigid_host.cpp runs it without a GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

constexpr int RG_JACOBI_SWEEPS = 6;       // cyclic sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
constexpr float RG_DEGENERATE = 1e-6f;    // sin^2 of a sample's triangle / eigenvalue ratio of a set's scatter at or below this

// one staged correspondence: the point in frame 1 and in frame 2 (24 bytes)
struct alignas(8) RgRow {
  float a[3], b[3];
};

// Cyclic Jacobi on the symmetric N x N matrix a (both triangles stored and updated): RG_JACOBI_SWEEPS sweeps over the
// pairs p < q in row-major order; afterwards a's diagonal holds the eigenvalues and the columns of v the eigenvectors.
// A pair whose off-diagonal element is exactly 0 is skipped.  Fully unrolled inside a sweep: registers, no scratch.
template <int N>
__host__ __device__ __forceinline__ void rg_jacobi(float (*a)[N], float (*v)[N]) {
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) v[r][c] = r == c ? 1.0f : 0.0f;
#pragma unroll 1
  for (int sweep = 0; sweep < RG_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const float apq = a[p][q];
        if (apq != 0.0f) {
          const float theta = (a[q][q] - a[p][p]) / (2.0f * apq);
          const float t = (theta >= 0.0f ? 1.0f : -1.0f) / (fabsf(theta) + sqrtf(1.0f + theta * theta));
          const float c = 1.0f / sqrtf(1.0f + t * t), s = c * t;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const float akp = a[k][p], akq = a[k][q];
            a[k][p] = c * akp - s * akq;
            a[k][q] = s * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const float apk = a[p][k], aqk = a[q][k];
            a[p][k] = c * apk - s * aqk;
            a[q][k] = s * apk + c * aqk;
          }
          a[p][q] = 0.0f;
          a[q][p] = 0.0f;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const float vkp = v[k][p], vkq = v[k][q];
            v[k][p] = c * vkp - s * vkq;
            v[k][q] = s * vkp + c * vkq;
          }
        }
      }
  }
}

// the rotation R (row-major, 9 floats) that maximises sum b . (R a) for S = sum a b^T: Horn's 4x4 matrix, the unit
// eigenvector of its largest eigenvalue (the first maximum of the diagonal) with q0 >= 0, as a rotation matrix
__host__ __device__ inline void rg_rotation_from_scatter(const float (*s)[3], float *r) {
  float n[4][4], v[4][4];
  n[0][0] = (s[0][0] + s[1][1]) + s[2][2];
  n[0][1] = s[1][2] - s[2][1];
  n[0][2] = s[2][0] - s[0][2];
  n[0][3] = s[0][1] - s[1][0];
  n[1][1] = (s[0][0] - s[1][1]) - s[2][2];
  n[1][2] = s[0][1] + s[1][0];
  n[1][3] = s[2][0] + s[0][2];
  n[2][2] = (s[1][1] - s[0][0]) - s[2][2];
  n[2][3] = s[1][2] + s[2][1];
  n[3][3] = (s[2][2] - s[0][0]) - s[1][1];
#pragma unroll
  for (int p = 1; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < p; ++q) n[p][q] = n[q][p];
  float n0[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) n0[p][q] = n[p][q];
  rg_jacobi<4>(n, v);
  int m = 0;
  float best = n[0][0], q0 = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0];
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (n[c][c] > best) { best = n[c][c]; m = c; q0 = v[0][c]; qx = v[1][c]; qy = v[2][c]; qz = v[3][c]; }
  // One first-order correction against the matrix itself, its inner products in float64: the rotations' roundings perturb
  // N by a few eps |N|, which a minimal sample (three points span a plane, so N's eigenvalues come in +- pairs, and the two
  // largest of a slim triangle lie within a percent of each other) turns into 1e3 eps in q.  With the residual
  // w = N q - lambda_m q (which, unlike N q, is blind to the eps-sized non-orthogonality of the v_j),
  // q += sum over j != m of (v_j . w) / (lambda_m - lambda_j) v_j leaves the square of that error; w is the difference of
  // nearly equal vectors, hence the float64 products (16 + 16 of them: nothing next to the scoring loop).  The refit of a
  // set that spans space has well separated eigenvalues and does not need the step; it runs there too (once per round, one
  // code path, the same bits from the host program and both kernels).
  {
    const double qv[4] = {q0, qx, qy, qz};
    double w[4];
    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = ((((double)n0[k][0] * qv[0] + (double)n0[k][1] * qv[1]) + (double)n0[k][2] * qv[2]) + (double)n0[k][3] * qv[3]) -
             (double)best * qv[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double dot = (((double)v[0][j] * w[0] + (double)v[1][j] * w[1]) + (double)v[2][j] * w[2]) + (double)v[3][j] * w[3];
      const float den = best - n[j][j];
      const float coef = (j != m && den > 0.0f) ? (float)dot / den : 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] += coef * v[k][j];
    }
    q0 += d[0]; qx += d[1]; qy += d[2]; qz += d[3];
  }
  const float nn = sqrtf(((q0 * q0 + qx * qx) + qy * qy) + qz * qz);
  const float sg = q0 < 0.0f ? -1.0f : 1.0f;
  q0 = sg * q0 / nn; qx = sg * qx / nn; qy = sg * qy / nn; qz = sg * qz / nn;
  r[0] = ((q0 * q0 + qx * qx) - qy * qy) - qz * qz;
  r[1] = 2.0f * (qx * qy - q0 * qz);
  r[2] = 2.0f * (qx * qz + q0 * qy);
  r[3] = 2.0f * (qy * qx + q0 * qz);
  r[4] = ((q0 * q0 - qx * qx) + qy * qy) - qz * qz;
  r[5] = 2.0f * (qy * qz - q0 * qx);
  r[6] = 2.0f * (qz * qx - q0 * qy);
  r[7] = 2.0f * (qz * qy + q0 * qx);
  r[8] = ((q0 * q0 - qx * qx) - qy * qy) + qz * qz;
}

// rt = (R row-major, t): R from the centred products s, t = cb - R ca.  False when the result is not finite.
__host__ __device__ inline bool rg_finish(const float (*s)[3], const float *ca, const float *cb, float *rt) {
  rg_rotation_from_scatter(s, rt);
  float chk = 0.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    rt[9 + j] = cb[j] - ((rt[3 * j] * ca[0] + rt[3 * j + 1] * ca[1]) + rt[3 * j + 2] * ca[2]);
    chk += ((fabsf(rt[3 * j]) + fabsf(rt[3 * j + 1])) + fabsf(rt[3 * j + 2])) + fabsf(rt[9 + j]);
  }
  return chk < INFINITY;                      // false for NaN and infinities
}

// three points are degenerate when the triangle they span has sin^2 of the angle at p0 at or below RG_DEGENERATE (collinear
// or repeated points; not finite: degenerate)
__host__ __device__ inline bool rg_degenerate3(const float *p0, const float *p1, const float *p2) {
  const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  const float cc = (cx * cx + cy * cy) + cz * cz;
  const float n1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2], n2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
  return !(cc > RG_DEGENERATE * n1 * n2);
}

// (R, t) from one 3-sample (header: "Solve").  False: degenerate in either frame or no finite result.
__host__ __device__ inline bool rg_solve_minimal(const RgRow *q, float *rt) {
  if (rg_degenerate3(q[0].a, q[1].a, q[2].a) || rg_degenerate3(q[0].b, q[1].b, q[2].b)) return false;
  float ca[3], cb[3], s[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    ca[j] = ((q[0].a[j] + q[1].a[j]) + q[2].a[j]) / 3.0f;
    cb[j] = ((q[0].b[j] + q[1].b[j]) + q[2].b[j]) / 3.0f;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      s[i][j] = ((q[0].a[i] - ca[i]) * (q[0].b[j] - cb[j]) + (q[1].a[i] - ca[i]) * (q[1].b[j] - cb[j])) +
                (q[2].a[i] - ca[i]) * (q[2].b[j] - cb[j]);
  return rg_finish(s, ca, cb, rt);
}

// the second largest eigenvalue of the symmetric positive semi-definite c (upper triangle xx xy xz yy yz zz) is at or
// below RG_DEGENERATE times the largest: the points lie on a line (or in one place)
__host__ __device__ inline bool rg_scatter_degenerate(const float *c) {
  float a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}}, v[3][3];
  rg_jacobi<3>(a, v);
  const float l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
  const float hi = fmaxf(l0, fmaxf(l1, l2));
  const float mid = fmaxf(fminf(l0, l1), fminf(fmaxf(l0, l1), l2));        // the median, exactly
  return !(mid > RG_DEGENERATE * hi);
}

// squared distance of one correspondence under (R, t) (header: "Score")
__host__ __device__ __forceinline__ float rg_dist2(const float *rt, const RgRow &q) {
  const float u0 = (((rt[0] * q.a[0] + rt[1] * q.a[1]) + rt[2] * q.a[2]) + rt[9]) - q.b[0];
  const float u1 = (((rt[3] * q.a[0] + rt[4] * q.a[1]) + rt[5] * q.a[2]) + rt[10]) - q.b[1];
  const float u2 = (((rt[6] * q.a[0] + rt[7] * q.a[1]) + rt[8] * q.a[2]) + rt[11]) - q.b[2];
  return (u0 * u0 + u1 * u1) + u2 * u2;
}

}  // namespace
