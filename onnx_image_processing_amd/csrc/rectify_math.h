// The arithmetic of K34 (include/mi355x_match_rectify.h: "Camera", "Forward model", "atan and tan", "Map", "Remap", "Points",
// "Stereo rig") shared by csrc/rectify.hip and a host compile (tests/native/rectify_host.cpp): float64 for the geometry,
// integers and float32 for the taps, operation by operation as the header states it; + - * / sqrt and floor only.  Nothing
// here launches or reads a device.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi355x_match_rectify.h"

#define RC_HD __host__ __device__ __forceinline__

// a camera as the kernels take it, by value: fx fy cx cy of k and k_new, the coefficients, the rotation (identity for NULL)
struct RcCamera {
  double fx, fy, cx, cy;
  double d[MI_RECTIFY_COEFFS];
  double r[9];
  double nfx, nfy, ncx, ncy;
  int model, has_new;
};

RC_HD bool rc_finite(double v) { return v - v == 0.0; }
RC_HD double rc_abs(double v) { return v < 0.0 ? -v : v; }

// "atan and tan": the odd Taylor polynomial through x^23 after the reciprocal and two half-angle reductions
RC_HD double rc_atan(double x) {
  const bool neg = x < 0.0;
  double a = neg ? -x : x;
  const bool recip = a > 1.0;
  if (recip) a = 1.0 / a;
  a = a / (1.0 + sqrt(1.0 + a * a));
  a = a / (1.0 + sqrt(1.0 + a * a));
  const double z = a * a;
  double p = 1.0 / 23.0;
  p = 1.0 / 21.0 - z * p;
  p = 1.0 / 19.0 - z * p;
  p = 1.0 / 17.0 - z * p;
  p = 1.0 / 15.0 - z * p;
  p = 1.0 / 13.0 - z * p;
  p = 1.0 / 11.0 - z * p;
  p = 1.0 / 9.0 - z * p;
  p = 1.0 / 7.0 - z * p;
  p = 1.0 / 5.0 - z * p;
  p = 1.0 / 3.0 - z * p;
  p = 1.0 - z * p;
  double v = 4.0 * (a * p);
  if (recip) v = 1.5707963267948966 - v;
  return neg ? -v : v;
}

// tan on 0 <= t <= MI_RECTIFY_MAX_THETA: sin through t^23 over cos through t^22, nested
RC_HD double rc_tan(double t) {
  const double z = t * t;
  double s = 1.0, c = 1.0;
  for (int m = 22; m >= 2; m -= 2) {
    s = 1.0 - z / (double)(m * (m + 1)) * s;
    c = 1.0 - z / (double)((m - 1) * m) * c;
  }
  return t * s / c;
}

// "Forward model": false where the pinhole model has no image
RC_HD bool rc_distort(const RcCamera &c, double x, double y, double *xd, double *yd) {
  const double r2 = x * x + y * y;
  const double *d = c.d;
  if (c.model == MI_RECTIFY_FISHEYE) {
    const double rr = sqrt(r2), th = rc_atan(rr), t2 = th * th;
    const double thd = th * (1.0 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3]))));
    const double s = rr > 0.0 ? thd / rr : 1.0;
    *xd = x * s;
    *yd = y * s;
    return true;
  }
  const double num = 1.0 + r2 * (d[0] + r2 * (d[1] + r2 * d[4])), den = 1.0 + r2 * (d[5] + r2 * (d[6] + r2 * d[7]));
  if (!(den > 0.0)) return false;
  const double radial = num / den, a = (2.0 * x) * y;
  *xd = x * radial + (d[2] * a + d[3] * (r2 + (2.0 * x) * x));
  *yd = y * radial + (d[2] * (r2 + (2.0 * y) * y) + d[3] * a);
  return true;
}

// "Map": the two map elements of destination pixel (v, u) and its mask byte
RC_HD void rc_map_pixel(const RcCamera &c, int src_h, int src_w, int v, int u, int32_t *qx, int32_t *qy, uint8_t *mask) {
  *qx = *qy = MI_RECTIFY_OUTSIDE;
  *mask = 0;
  const double xp = ((double)u - c.ncx) / c.nfx, yp = ((double)v - c.ncy) / c.nfy;
  const double *r = c.r;
  const double X0 = (r[0] * xp + r[3] * yp) + r[6], X1 = (r[1] * xp + r[4] * yp) + r[7], X2 = (r[2] * xp + r[5] * yp) + r[8];
  if (!(X2 > 0.0)) return;
  double xd, yd;
  if (!rc_distort(c, X0 / X2, X1 / X2, &xd, &yd)) return;
  const double sx = c.fx * xd + c.cx, sy = c.fy * yd + c.cy;
  const double tx = floor(sx * 32.0 + 0.5), ty = floor(sy * 32.0 + 0.5);
  if (!(tx >= -64.0 && tx < 32.0 * (double)(src_w + 1) && ty >= -64.0 && ty < 32.0 * (double)(src_h + 1))) return;
  const int ix = (int)tx, iy = (int)ty, X = ix >> 5, Y = iy >> 5;
  if (X < -1 || X >= src_w || Y < -1 || Y >= src_h) return;
  *qx = ix;
  *qy = iy;
  const int lastx = (ix & 31) ? X + 1 : X, lasty = (iy & 31) ? Y + 1 : Y;
  *mask = (uint8_t)(X >= 0 && lastx <= src_w - 1 && Y >= 0 && lasty <= src_h - 1);
}

// "Remap": one tap with the border rule
template <typename T>
RC_HD T rc_tap(const T *s, int src_h, int src_w, int Y, int X, T border) {
  return ((unsigned)X < (unsigned)src_w && (unsigned)Y < (unsigned)src_h) ? s[(size_t)Y * src_w + X] : border;
}

RC_HD uint8_t rc_blend(uint8_t p00, uint8_t p01, uint8_t p10, uint8_t p11, int ax, int ay) {
  return (uint8_t)(((int)p00 * (32 - ax) * (32 - ay) + (int)p01 * ax * (32 - ay) + (int)p10 * (32 - ax) * ay + (int)p11 * ax * ay + 512) >> 10);
}
RC_HD uint16_t rc_blend(uint16_t p00, uint16_t, uint16_t, uint16_t, int, int) { return p00; }      // refused before any launch
RC_HD float rc_blend(float p00, float p01, float p10, float p11, int ax, int ay) {
  if (!ax && !ay) return p00;
  const float wx = (float)ax / 32.0f, wy = (float)ay / 32.0f;
  const float top = ax ? p00 + (p01 - p00) * wx : p00;
  const float bot = ax ? p10 + (p11 - p10) * wx : p10;
  const float v = ay ? top + (bot - top) * wy : top;
  // which NaN an operation returns differs between processors; tested on the bits, which no compiler folds into the arithmetic
  const uint32_t bits = __builtin_bit_cast(uint32_t, v);
  return (bits & 0x7fffffffu) > 0x7f800000u ? __builtin_bit_cast(float, 0x7fc00000u) : v;
}

// one destination pixel of one frame s (src_h x src_w) from its map elements.  A tap of weight zero is read (inside the
// frame, or the border) but never enters the result.
template <typename T>
RC_HD T rc_remap_pixel(const T *s, int src_h, int src_w, int32_t qx, int32_t qy, bool linear, T border) {
  if (qx == MI_RECTIFY_OUTSIDE || qy == MI_RECTIFY_OUTSIDE) return border;
  if (!linear) {
    // 64-bit: any int32 is a legal map element
    const long long X = ((long long)qx + 16) >> 5, Y = ((long long)qy + 16) >> 5;
    return (X >= 0 && X < src_w && Y >= 0 && Y < src_h) ? s[(size_t)Y * src_w + (size_t)X] : border;
  }
  const int X = qx >> 5, Y = qy >> 5, ax = qx & 31, ay = qy & 31;
  // X + 1 cannot overflow: X <= 2^26
  return rc_blend(rc_tap(s, src_h, src_w, Y, X, border), rc_tap(s, src_h, src_w, Y, X + 1, border),
                  rc_tap(s, src_h, src_w, Y + 1, X, border), rc_tap(s, src_h, src_w, Y + 1, X + 1, border), ax, ay);
}

// "Points": one point; false (and out = 0, 0) on a failure
RC_HD bool rc_undistort_point(const RcCamera &c, float u, float v, int iterations, double max_residual_px, float *ox, float *oy) {
  *ox = 0.0f;
  *oy = 0.0f;
  const double *d = c.d;
  const double xd = ((double)u - c.cx) / c.fx, yd = ((double)v - c.cy) / c.fy;
  double x = xd, y = yd;
  if (c.model == MI_RECTIFY_FISHEYE) {
    const double thd = sqrt(xd * xd + yd * yd);
    double th = thd;
    for (int i = 0; i < iterations; ++i) {
      const double t2 = th * th;
      const double f = th * (1.0 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3])))) - thd;
      const double g = 1.0 + t2 * (3.0 * d[0] + t2 * (5.0 * d[1] + t2 * (7.0 * d[2] + t2 * (9.0 * d[3]))));
      th = th - f / g;
    }
    if (!(th >= 0.0 && th <= MI_RECTIFY_MAX_THETA)) return false;
    const double s = thd > 0.0 ? rc_tan(th) / thd : 1.0;
    x = xd * s;
    y = yd * s;
  } else {
    for (int i = 0; i < iterations; ++i) {
      const double r2 = x * x + y * y;
      const double num = 1.0 + r2 * (d[0] + r2 * (d[1] + r2 * d[4])), den = 1.0 + r2 * (d[5] + r2 * (d[6] + r2 * d[7]));
      const double icd = den / num, a = (2.0 * x) * y;
      const double nx = (xd - (d[2] * a + d[3] * (r2 + (2.0 * x) * x))) * icd;
      const double ny = (yd - (d[2] * (r2 + (2.0 * y) * y) + d[3] * a)) * icd;
      x = nx;
      y = ny;
    }
  }
  double bx, by;
  if (!rc_distort(c, x, y, &bx, &by)) return false;
  const double ex = (c.fx * bx + c.cx) - (double)u, ey = (c.fy * by + c.cy) - (double)v;
  if (!(ex * ex + ey * ey <= max_residual_px * max_residual_px)) return false;
  const double *r = c.r;
  const double X0 = (r[0] * x + r[1] * y) + r[2], X1 = (r[3] * x + r[4] * y) + r[5], X2 = (r[6] * x + r[7] * y) + r[8];
  if (!(X2 > 0.0)) return false;
  double px = X0 / X2, py = X1 / X2;
  if (c.has_new) {
    px = c.nfx * px + c.ncx;
    py = c.nfy * py + c.ncy;
  }
  const float fx32 = (float)px, fy32 = (float)py;
  if (!(fx32 - fx32 == 0.0f) || !(fy32 - fy32 == 0.0f)) return false;
  *ox = fx32;
  *oy = fy32;
  return true;
}

// "Camera": a legal camera matrix
inline bool rc_camera_ok(const double *k) {
  for (int i = 0; i < 9; ++i)
    if (!rc_finite(k[i])) return false;
  return k[0] > 0.0 && k[4] > 0.0 && k[1] == 0.0 && k[3] == 0.0 && k[6] == 0.0 && k[7] == 0.0 && k[8] == 1.0;
}

// MI_OK, or MI_E_PARAM for an unknown model, a bad camera, bad coefficients or a rotation that is not finite; fills *c.
// k_new may be NULL (has_new = 0).
inline int rc_camera(int model, const double *k, const double *dist, const double *r, const double *k_new, RcCamera *c) {
  if (model != MI_RECTIFY_PINHOLE && model != MI_RECTIFY_FISHEYE) return MI_E_PARAM;
  if (!rc_camera_ok(k) || (k_new && !rc_camera_ok(k_new))) return MI_E_PARAM;
  for (int i = 0; i < MI_RECTIFY_COEFFS; ++i) {
    if (!rc_finite(dist[i]) || (model == MI_RECTIFY_FISHEYE && i >= 4 && dist[i] != 0.0)) return MI_E_PARAM;
    c->d[i] = dist[i];
  }
  for (int i = 0; i < 9; ++i) {
    c->r[i] = r ? r[i] : (i % 4 == 0 ? 1.0 : 0.0);
    if (!rc_finite(c->r[i])) return MI_E_PARAM;
  }
  c->fx = k[0], c->fy = k[4], c->cx = k[2], c->cy = k[5];
  c->has_new = k_new != nullptr;
  c->nfx = k_new ? k_new[0] : 1.0, c->nfy = k_new ? k_new[4] : 1.0, c->ncx = k_new ? k_new[2] : 0.0, c->ncy = k_new ? k_new[5] : 0.0;
  c->model = model;
  return MI_OK;
}

// "Stereo rig": MI_OK or MI_E_PARAM; h, w are legal extents
inline int rc_stereo_rig(const double *k1, const double *k2, const double *r, const double *t, int h, int w, double *r1, double *r2,
                         double *k_new, double *baseline, double *fb) {
  if (!rc_camera_ok(k1) || !rc_camera_ok(k2)) return MI_E_PARAM;
  for (int i = 0; i < 9; ++i)
    if (!rc_finite(r[i])) return MI_E_PARAM;
  for (int i = 0; i < 3; ++i)
    if (!rc_finite(t[i])) return MI_E_PARAM;
  const double b = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  if (!(b > 0.0) || !rc_finite(b)) return MI_E_PARAM;
  double x[3], y[3], z[3];
  for (int i = 0; i < 3; ++i) x[i] = -((r[i] * t[0] + r[3 + i] * t[1]) + r[6 + i] * t[2]) / b;
  if (!(x[0] > 0.0 && x[0] >= rc_abs(x[1]))) return MI_E_PARAM;
  const double zm[3] = {r[6], r[7], 1.0 + r[8]};
  y[0] = zm[1] * x[2] - zm[2] * x[1];
  y[1] = zm[2] * x[0] - zm[0] * x[2];
  y[2] = zm[0] * x[1] - zm[1] * x[0];
  const double ny = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]), nz = sqrt((zm[0] * zm[0] + zm[1] * zm[1]) + zm[2] * zm[2]);
  if (!(ny > 1e-6 * nz)) return MI_E_PARAM;
  for (int i = 0; i < 3; ++i) y[i] = y[i] / ny;
  z[0] = x[1] * y[2] - x[2] * y[1];
  z[1] = x[2] * y[0] - x[0] * y[2];
  z[2] = x[0] * y[1] - x[1] * y[0];
  for (int j = 0; j < 3; ++j) {
    r1[j] = x[j];
    r1[3 + j] = y[j];
    r1[6 + j] = z[j];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r2[3 * i + j] = (r1[3 * i] * r[3 * j] + r1[3 * i + 1] * r[3 * j + 1]) + r1[3 * i + 2] * r[3 * j + 2];
  const double f = (k1[4] + k2[4]) / 2.0;
  const double kn[9] = {f, 0.0, ((double)w - 1.0) / 2.0, 0.0, f, ((double)h - 1.0) / 2.0, 0.0, 0.0, 1.0};
  for (int i = 0; i < 9; ++i) k_new[i] = kn[i];
  *baseline = b;
  *fb = f * b;
  return MI_OK;
}
