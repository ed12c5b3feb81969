// 3x3 device helpers and the essential-manifold projection shared by K10 (essential.hip) and K15 (pose.hip).
// Semantics: reference pytorch_model/geometry/essential_matrix_estimator.py:175-248 (_project_onto_E_manifold).
// The two kernels differ only in how they obtain the dominant right singular vector va and the right null vector vc of E
// (K10: n_iter_manifold power-iteration steps, two lanes side by side; K15: repeated squaring in one lane); everything
// after that -- the right-handed bases, the singular values' mean, E = U diag(s, s, 0) V^T -- is em_manifold_from_vectors.
// Plain arithmetic, callable on the host as well (a CPU harness can check it without a GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

__host__ __device__ __forceinline__ float norm3(const float *v) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
__host__ __device__ __forceinline__ float det3(const float (*m)[3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
__host__ __device__ __forceinline__ float signf(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__host__ __device__ __forceinline__ void matvec3(const float (*a)[3], const float *v, float *out) {
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = (a[r][0] * v[0] + a[r][1] * v[1]) + a[r][2] * v[2];
}
__host__ __device__ __forceinline__ void unit3(float *v) {
  const float nn = norm3(v) + 1e-8f;
#pragma unroll
  for (int r = 0; r < 3; ++r) v[r] = v[r] / nn;
}
__host__ __device__ __forceinline__ void cross3(const float *a, const float *b, float *o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// E^T E and trace(E^T E) I - E^T E: the matrices whose dominant eigenvectors are va and vc (:190-215)
__host__ __device__ __forceinline__ void em_manifold_gram(const float (*e)[3], float (*bm)[3], float (*bs)[3]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) bm[r][c] = (e[0][r] * e[0][c] + e[1][r] * e[1][c]) + e[2][r] * e[2][c];
  const float lam3 = (bm[0][0] + bm[1][1]) + bm[2][2];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) bs[r][c] = (r == c ? lam3 : 0.0f) - bm[r][c];
}

// out = U diag(s, s, 0) V^T from E, its dominant right singular vector va and its right null vector vc (:217-248)
__host__ __device__ __forceinline__ void em_manifold_from_vectors(const float (*e)[3], const float *va, const float *vc,
                                                         float (*out)[3]) {
  float vb[3];
  cross3(vc, va, vb);
  unit3(vb);
  float vm[3][3] = {{va[0], vb[0], vc[0]}, {va[1], vb[1], vc[1]}, {va[2], vb[2], vc[2]}};   // columns v1 v2 v3
  const float sgn_v = signf(det3(vm));
  for (int r = 0; r < 3; ++r) vm[r][2] *= sgn_v;
  const float c0[3] = {vm[0][0], vm[1][0], vm[2][0]}, c1[3] = {vm[0][1], vm[1][1], vm[2][1]};
  float ev0[3], ev1[3], u3[3];
  matvec3(e, c0, ev0);
  matvec3(e, c1, ev1);
  const float sg1 = norm3(ev0), sg2 = norm3(ev1);
  const float s_avg = (sg1 + sg2) / 2.0f;
  float u1[3], u2[3];
  for (int r = 0; r < 3; ++r) { u1[r] = ev0[r] / (sg1 + 1e-8f); u2[r] = ev1[r] / (sg2 + 1e-8f); }
  cross3(u1, u2, u3);
  float um[3][3] = {{u1[0], u2[0], u3[0]}, {u1[1], u2[1], u3[1]}, {u1[2], u2[2], u3[2]}};
  const float sgn_u = signf(det3(um));
  for (int r = 0; r < 3; ++r) um[r][2] *= sgn_u;
  // E = U diag(s, s, 0) V^T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) out[r][c] = (um[r][0] * s_avg) * vm[c][0] + (um[r][1] * s_avg) * vm[c][1];
}

// squared Sampson distance of one correspondence (header: "Scoring"); +inf where the gradient vanishes.  K15 (pose.hip)
// scores with it, and K24's model selection (homography.hip) scores E with the same bits.
__host__ __device__ __forceinline__ float po_sampson(const float *e, float4 q) {
  const float ex0 = (e[0] * q.x + e[1] * q.y) + e[2], ex1 = (e[3] * q.x + e[4] * q.y) + e[5], ex2 = (e[6] * q.x + e[7] * q.y) + e[8];
  const float et0 = (e[0] * q.z + e[3] * q.w) + e[6], et1 = (e[1] * q.z + e[4] * q.w) + e[7];
  const float r = (q.z * ex0 + q.w * ex1) + ex2;
  const float den = ((ex0 * ex0 + ex1 * ex1) + et0 * et0) + et1 * et1;
  return den > 0.0f ? (r * r) / den : INFINITY;
}

// The unit eigenvector v of the smallest eigenvalue of the symmetric positive semi-definite 9x9 matrix mm (the normal
// equations of K15's and K24's linear refits) by shifted inverse iteration: the Cholesky factor of M + mu I,
// mu = 2e-6 trace(M) (above the rounding of M's entries, so the factor exists; far below the second smallest eigenvalue
// of a well-posed set), then EM_INVERSE_ITERS steps from the all-ones vector, each scaled to unit length.
constexpr int EM_INVERSE_ITERS = 6;
__host__ __device__ __forceinline__ void em_min_eigenvector9(const float (*mm)[9], float *v) {
  float tr = 0.0f;
#pragma unroll
  for (int r = 0; r < 9; ++r) tr += mm[r][r];
  const float mu = 2e-6f * tr;
  float l[9][9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    float d = mm[j][j] + mu;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= l[j][k] * l[j][k];
    d = sqrtf(fmaxf(d, 1e-30f));
    l[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < 9; ++i) {
      float t = mm[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= l[i][k] * l[j][k];
      l[i][j] = t / d;
    }
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) v[c] = 1.0f / 3.0f;
  for (int it = 0; it < EM_INVERSE_ITERS; ++it) {
    float y[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {                                     // L y = v
      float t = v[i];
#pragma unroll
      for (int k = 0; k < i; ++k) t -= l[i][k] * y[k];
      y[i] = t / l[i][i];
    }
#pragma unroll
    for (int i = 8; i >= 0; --i) {                                    // L^T x = y
      float t = y[i];
#pragma unroll
      for (int k = i + 1; k < 9; ++k) t -= l[k][i] * v[k];
      v[i] = t / l[i][i];
    }
    float nn = 0.0f;
#pragma unroll
    for (int c = 0; c < 9; ++c) nn += v[c] * v[c];
    nn = sqrtf(nn);
#pragma unroll
    for (int c = 0; c < 9; ++c) v[c] = v[c] / nn;
  }
}

}  // namespace
