// The arithmetic of K30 (sim3.hip; include/mi355x_match_sim3.h, "similarity alignment"): K17's Horn rotation
// (rigid_math.h, unchanged) with Umeyama's scale on top, the scale's range test and the two scores.  float32 arithmetic,
// callable on the host as well (tests/native/sim3_host.cpp runs it without a GPU).
// A model is 14 floats: R row-major, t, s, and inv_s = 1.0f / s (formed once per model; not stored in memory).
#pragma once
#include "rigid_math.h"

#include "../../include/mi355x_match_sim3.h"

namespace {

constexpr int S3_FLOATS = 14, S3_STORED = 13;

// false for NaN
__host__ __device__ __forceinline__ bool s3_scale_ok(float s) { return s >= MI_SIM3_MIN_SCALE && s <= MI_SIM3_MAX_SCALE; }

// s = num / den, t = cb - s (R ca), inv_s; m[0..8] holds R.  False: not finite or the scale outside its range.
__host__ __device__ inline bool s3_finish(float num, float den, const float *ca, const float *cb, float *m) {
  const float s = num / den;
  float chk = fabsf(s);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    m[9 + j] = cb[j] - s * ((m[3 * j] * ca[0] + m[3 * j + 1] * ca[1]) + m[3 * j + 2] * ca[2]);
    chk += ((fabsf(m[3 * j]) + fabsf(m[3 * j + 1])) + fabsf(m[3 * j + 2])) + fabsf(m[9 + j]);
  }
  m[12] = s;
  m[13] = 1.0f / s;
  return chk < INFINITY && s3_scale_ok(s);
}

// one row's term of num: b' . (R a') in the header's order
__host__ __device__ __forceinline__ float s3_num_term(const float *r, const float *a, const float *b) {
  const float r0 = (r[0] * a[0] + r[1] * a[1]) + r[2] * a[2];
  const float r1 = (r[3] * a[0] + r[4] * a[1]) + r[5] * a[2];
  const float r2 = (r[6] * a[0] + r[7] * a[1]) + r[8] * a[2];
  return (b[0] * r0 + b[1] * r1) + b[2] * r2;
}

// the model from one 3-sample (header: "Rotation", "Scale").  The centroids and S are rg_solve_minimal's expressions, so
// that R comes out in K17's bits.  False: degenerate in either frame, no finite result or the scale outside its range.
__host__ __device__ inline bool s3_solve_minimal(const RgRow *q, float *m) {
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
  rg_rotation_from_scatter(s, m);
  float num = 0.0f, den = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a[3] = {q[k].a[0] - ca[0], q[k].a[1] - ca[1], q[k].a[2] - ca[2]};
    const float b[3] = {q[k].b[0] - cb[0], q[k].b[1] - cb[1], q[k].b[2] - cb[2]};
    const float nk = s3_num_term(m, a, b), dk = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    num = k == 0 ? nk : num + nk;
    den = k == 0 ? dk : den + dk;
  }
  return s3_finish(num, den, ca, cb, m);
}

// Y = s (R X1) + t
__host__ __device__ __forceinline__ void s3_forward(const float *m, const float *x, float *y) {
#pragma unroll
  for (int j = 0; j < 3; ++j) y[j] = m[12] * ((m[3 * j] * x[0] + m[3 * j + 1] * x[1]) + m[3 * j + 2] * x[2]) + m[9 + j];
}

// squared distance of one correspondence in frame 2's units (header: "Metric MI_SIM3_POINT")
__host__ __device__ __forceinline__ float s3_point2(const float *m, const RgRow &q) {
  float y[3];
  s3_forward(m, q.a, y);
  const float u0 = y[0] - q.b[0], u1 = y[1] - q.b[1], u2 = y[2] - q.b[2];
  return (u0 * u0 + u1 * u1) + u2 * u2;
}

// symmetric reprojection error in normalised units (header: "Metric MI_SIM3_REPROJ"); +inf behind either camera
__host__ __device__ __forceinline__ float s3_reproj2(const float *m, const RgRow &q) {
  float y[3], w[3];
  s3_forward(m, q.a, y);
  const float v[3] = {q.b[0] - m[9], q.b[1] - m[10], q.b[2] - m[11]};
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = ((m[j] * v[0] + m[3 + j] * v[1]) + m[6 + j] * v[2]) * m[13];
  if (!(q.a[2] > 0.0f) || !(q.b[2] > 0.0f) || !(y[2] > 0.0f) || !(w[2] > 0.0f)) return INFINITY;
  const float p0 = y[0] / y[2] - q.b[0] / q.b[2], p1 = y[1] / y[2] - q.b[1] / q.b[2];
  const float g0 = w[0] / w[2] - q.a[0] / q.a[2], g1 = w[1] / w[2] - q.a[1] / q.a[2];
  const float e2 = p0 * p0 + p1 * p1, e1 = g0 * g0 + g1 * g1;
  return e1 + e2;
}

template <int METRIC>
__host__ __device__ __forceinline__ float s3_dist2(const float *m, const RgRow &q) {
  return METRIC == MI_SIM3_REPROJ ? s3_reproj2(m, q) : s3_point2(m, q);
}

}  // namespace
