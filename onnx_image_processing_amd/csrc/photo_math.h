// The arithmetic of K21 (photo.hip; include/mi355x_match.h, "direct RGB-D refinement"): the intensity record of a pixel, the
// bilinear footprint of a projected point, one pixel's row of the photometric system and the joint sums handed to K18's
// solve.  Per-pixel work is float32, the joint system float64.  Rotation, projection, solve and pose update are icp_math.h's.
// No HIP header is needed: a plain C++ compiler builds it for the host as well (tests/native/photo_host.cpp runs it
// without a GPU).
#pragma once
#include "icp_math.h"

namespace {

// the record (I, gx, gy, f) of a pixel with gray value c and axis neighbours l / r (x -+ 1), u / d (y -+ 1); `interior`:
// all four neighbours are inside the frame (otherwise they are not read and may hold anything).  false (and zeros) for a
// border pixel or when one of the five values is not finite.
ICP_HD bool photo_record(float c, float l, float r, float u, float d, bool interior, float *rec) {
  const bool ok = interior && fabsf(c) < INFINITY && fabsf(l) < INFINITY && fabsf(r) < INFINITY && fabsf(u) < INFINITY &&
                  fabsf(d) < INFINITY;
  rec[0] = ok ? c : 0.0f;
  rec[1] = ok ? 0.5f * (r - l) : 0.0f;
  rec[2] = ok ? 0.5f * (d - u) : 0.0f;
  rec[3] = ok ? 1.0f : 0.0f;
  return ok;
}

// the 2 x 2 footprint of q under the camera: its top-left pixel (x0, y0) and the weights a, b as floats, and K18's nearest
// pixel (px, py), which is one of the four.  false when q_z <= 0 or the footprint is not inside the w x h frame (NaN fails
// every comparison).
ICP_HD bool photo_footprint(const float *q, float fx, float fy, float cx, float cy, int w, int h, float *x0, float *y0, float *a,
                            float *b, float *px, float *py) {
  const float u = fx * (q[0] / q[2]) + cx, v = fy * (q[1] / q[2]) + cy;
  icp_project(q, fx, fy, cx, cy, w, h, px, py);
  *x0 = floorf(u);
  *y0 = floorf(v);
  *a = u - *x0;
  *b = v - *y0;
  return q[2] > 0.0f && *x0 >= 0.0f && *x0 <= (float)(w - 2) && *y0 >= 0.0f && *y0 <= (float)(h - 2);
}

ICP_HD float photo_blend(float c00, float c01, float c10, float c11, float a, float b) {
  const float top = c00 + a * (c01 - c00), bot = c10 + a * (c11 - c10);
  return top + b * (bot - top);
}

// the validity, occlusion and intensity gates and, for a survivor, the row J = [q x c, c] and the residual r = I2 - I1.
// c00 .. c11: the four records of frame 2 (row y0: c00 c01, row y0 + 1: c10 c11); v2: frame 2's vertex record at the
// nearest pixel; i1: frame 1's intensity.  false leaves J and r zero.
ICP_HD bool photo_row(const float *q, float i1, const float *c00, const float *c01, const float *c10, const float *c11, float a,
                      float b, const float *v2, float fx, float fy, float distance_threshold, float intensity_threshold, float *J,
                      float *r) {
  const float i2 = photo_blend(c00[0], c01[0], c10[0], c11[0], a, b);
  const float gx = photo_blend(c00[1], c01[1], c10[1], c11[1], a, b);
  const float gy = photo_blend(c00[2], c01[2], c10[2], c11[2], a, b);
  const float res = i2 - i1;
  const bool ok = c00[3] != 0.0f && c01[3] != 0.0f && c10[3] != 0.0f && c11[3] != 0.0f && v2[3] != 0.0f &&
                  fabsf(q[2] - v2[2]) <= distance_threshold && fabsf(res) <= intensity_threshold;
  const float k0 = (fx * gx) / q[2], k1 = (fy * gy) / q[2];
  const float k2 = -((k0 * q[0] + k1 * q[1]) / q[2]);
  J[0] = ok ? q[1] * k2 - q[2] * k1 : 0.0f;
  J[1] = ok ? q[2] * k0 - q[0] * k2 : 0.0f;
  J[2] = ok ? q[0] * k1 - q[1] * k0 : 0.0f;
  J[3] = ok ? k0 : 0.0f;
  J[4] = ok ? k1 : 0.0f;
  J[5] = ok ? k2 : 0.0f;
  *r = ok ? res : 0.0f;
  return ok;
}

// w * w in float64 of the float32 photo_weight
ICP_HD double photo_weight2(float w) { return (double)w * (double)w; }

// the joint system handed to icp_solve: s_k = g_k + w2 * p_k for A, b and sum r^2 (k < 28), the count the sum of both.
// p == nullptr (photo_weight 0): the geometric sums themselves.
ICP_HD void photo_joint(const double *g, const double *p, double w2, double *s) {
  for (int k = 0; k < 28; ++k) s[k] = p ? g[k] + w2 * p[k] : g[k];
  s[28] = p ? g[28] + p[28] : g[28];
}

}  // namespace
