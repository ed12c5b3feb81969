// The arithmetic of K32 (include/mi355x_match_flow.h: "Pyramid", "Sampling", "Tracking") shared by csrc/flow.hip and a host
// compile (tests/native/flow_host.cpp): float32, operation by operation as the header states it, built without contraction.
// Nothing here launches or reads a device.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi355x_match_flow.h"

#define FL_HD __host__ __device__ __forceinline__

// the geometry of a pyramid: sizes and FLOAT offsets of its levels (byte offsets are multiples of 256)
struct FlLevels {
  int h[MI_FLOW_MAX_LEVELS], w[MI_FLOW_MAX_LEVELS];
  long long off[MI_FLOW_MAX_LEVELS];
  long long total_bytes;
};

// false: levels outside 1 .. MI_FLOW_MAX_LEVELS, more than MI_FLOW_MAX_PIXELS pixels in level 0 or a level too small to hold a
// window of `radius`
static inline bool fl_levels(int batch, int h, int w, int levels, int radius, FlLevels *out) {
  if (levels < 1 || levels > MI_FLOW_MAX_LEVELS || (long long)batch * h * w > MI_FLOW_MAX_PIXELS) return false;
  long long bytes = 0;
  for (int l = 0; l < levels; ++l) {
    if ((h < w ? h : w) < 2 * radius + 3) return false;
    out->h[l] = h;
    out->w[l] = w;
    out->off[l] = bytes / 4;
    bytes += (long long)batch * h * w * 4;
    bytes = (bytes + 255) / 256 * 256;
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  out->total_bytes = bytes;
  return true;
}

FL_HD int fl_reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
FL_HD float fl_tap5(float a, float b, float c, float d, float e) { return ((a + e) + 4.0f * (b + d)) + 6.0f * c; }

// one pixel of level l+1 from level l (src: h x w), "Pyramid"
FL_HD float fl_pyr_down(const float *src, int h, int w, int y, int x) {
  int xs[5];
  for (int j = 0; j < 5; ++j) xs[j] = fl_reflect101(2 * x - 2 + j, w);
  float row[5];
  for (int j = 0; j < 5; ++j) {
    const float *s = src + (size_t)fl_reflect101(2 * y - 2 + j, h) * w;
    row[j] = fl_tap5(s[xs[0]], s[xs[1]], s[xs[2]], s[xs[3]], s[xs[4]]);
  }
  return fl_tap5(row[0], row[1], row[2], row[3], row[4]) * (1.0f / 256.0f);
}

// "Sampling": clamped in float before the conversion; any x, y (NaN, infinities, 1e30) gives indices inside the level
FL_HD float fl_sample(const float *f, int h, int w, float x, float y) {
  x = fminf(fmaxf(x, 0.0f), (float)(w - 1));
  y = fminf(fmaxf(y, 0.0f), (float)(h - 1));
  const float x0 = floorf(x), y0 = floorf(y);
  const float fx = x - x0, fy = y - y0;
  const int i0 = (int)x0, j0 = (int)y0;
  const int i1 = i0 + 1 < w ? i0 + 1 : w - 1, j1 = j0 + 1 < h ? j0 + 1 : h - 1;
  const float *r0 = f + (size_t)j0 * w, *r1 = f + (size_t)j1 * w;
  const float top = r0[i0] + fx * (r0[i1] - r0[i0]);
  const float bot = r1[i0] + fx * (r1[i1] - r1[i0]);
  return top + fy * (bot - top);
}

FL_HD bool fl_finite(float v) { return fabsf(v) < INFINITY; }            // false for NaN
// a position inside the closed frame; false for NaN
FL_HD bool fl_inside(float x, float y, int h, int w) { return x >= 0.0f && x <= (float)(w - 1) && y >= 0.0f && y <= (float)(h - 1); }

// window pixel q of radius r -> (dx, dy)
FL_HD void fl_pixel(int q, int r, int *dx, int *dy) {
  const int side = 2 * r + 1;
  *dy = q / side - r;
  *dx = q % side - r;
}

// the template and its gradients at one window pixel
FL_HD void fl_template(const float *f1, int h, int w, float cx, float cy, int dx, int dy, float *t, float *gx, float *gy) {
  const float x = cx + (float)dx, y = cy + (float)dy;
  *t = fl_sample(f1, h, w, x, y);
  *gx = 0.5f * (fl_sample(f1, h, w, cx + (float)(dx + 1), y) - fl_sample(f1, h, w, cx + (float)(dx - 1), y));
  *gy = 0.5f * (fl_sample(f1, h, w, x, cy + (float)(dy + 1)) - fl_sample(f1, h, w, x, cy + (float)(dy - 1)));
}

FL_HD float fl_min_eig(float gxx, float gxy, float gyy, int n) {
  const float dif = gxx - gyy;
  return ((gyy + gxx) - sqrtf(dif * dif + 4.0f * (gxy * gxy))) / (2.0f * (float)n);
}

// delta = G^-1 b by the closed 2x2 form
FL_HD void fl_step(float gxx, float gxy, float gyy, float det, float bx, float by, float *dx, float *dy) {
  *dx = (gyy * bx - gxy * by) / det;
  *dy = (gxx * by - gxy * bx) / det;
}

// "Loss": the inputs of a point that is never tracked
FL_HD bool fl_input_lost(float py, float px, bool has_guess, float gy, float gx, int h, int w) {
  if (!fl_finite(py) || !fl_finite(px) || !fl_inside(px, py, h, w)) return true;
  return has_guess && (!fl_finite(gy) || !fl_finite(gx));
}

// the cell of a point for mi_flow_replenish; the point is clamped into the frame in float first
FL_HD int fl_cell(float y, float x, int h, int w, int cell, int cells_x) {
  x = fminf(fmaxf(x, 0.0f), (float)(w - 1));
  y = fminf(fmaxf(y, 0.0f), (float)(h - 1));
  return ((int)y / cell) * cells_x + (int)x / cell;
}
