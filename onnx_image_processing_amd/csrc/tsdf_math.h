// The arithmetic of K19 (tsdf.hip; include/mi355x_match.h, "TSDF fusion"): a voxel's centre and its update by one depth
// sample, the trilinear sample of the volume, the ray's world point, the hit interpolation, the normal from the gradient
// and the composition of two poses.  Per-voxel and per-sample work is float32, the composition float64.  No HIP header is
// needed: a plain C++ compiler builds it for the host as well (tests/native/tsdf_host.cpp runs it without a GPU).
#pragma once
#include "icp_math.h"

#include <stddef.h>

namespace {

// centre of voxel `index` along one axis
ICP_HD float tsdf_centre(int index, float voxel_size, float origin) { return (((float)index + 0.5f) * voxel_size) + origin; }

// one depth sample d (already fetched at the voxel's nearest pixel) against a voxel at camera depth qz: the running mean of
// the truncated distance and the clamped weight.  false (nothing changes) when d is not finite, Z = d * z_scale is outside
// [min_depth, max_depth] or the voxel lies more than `truncation` behind the surface.
ICP_HD bool tsdf_fuse(float d, float z_scale, float min_depth, float max_depth, float qz, float truncation, float max_weight,
                      float *tsdf, float *weight) {
  const float z = d * z_scale;
  if (!(fabsf(d) < INFINITY) || !(z >= min_depth) || !(z <= max_depth)) return false;
  const float sdf = z - qz;
  if (!(sdf >= -truncation)) return false;
  const float f = fminf(1.0f, sdf / truncation);
  const float w = *weight;
  *tsdf = ((*tsdf) * w + f) / (w + 1.0f);
  *weight = fminf(w + 1.0f, max_weight);
  return true;
}

// records of two x-adjacent voxels: (tsdf, weight, tsdf, weight), one 16-byte load at 8-byte alignment on the device
struct TsdfPair {
  float t0, w0, t1, w1;
};
ICP_HD TsdfPair tsdf_pair(const float *vol, size_t voxel) {
#if defined(__HIPCC__)
  typedef float tsdf_f4 __attribute__((ext_vector_type(4), aligned(8)));
  const tsdf_f4 v = *reinterpret_cast<const tsdf_f4 *>(vol + 2 * voxel);
  return TsdfPair{v.x, v.y, v.z, v.w};
#else
  const float *p = vol + 2 * voxel;
  return TsdfPair{p[0], p[1], p[2], p[3]};
#endif
}

// trilinear sample of tsdf at the grid coordinate g (voxel centres at integers) of a volume of (nz, ny, nx) records, x
// fastest.  false (and *f = 0) unless the eight corners exist (0 <= floor(g_a) <= n_a - 2 on every axis; NaN fails) and all
// have weight > 0.  Along x, then y, then z, each as a + frac * (b - a).
ICP_HD bool tsdf_sample(const float *vol, int nx, int ny, int nz, const float *g, float *f) {
  *f = 0.0f;
  if (!(g[0] >= 0.0f && g[0] < (float)(nx - 1) && g[1] >= 0.0f && g[1] < (float)(ny - 1) && g[2] >= 0.0f && g[2] < (float)(nz - 1)))
    return false;
  const float bx = floorf(g[0]), by = floorf(g[1]), bz = floorf(g[2]);
  const float ax = g[0] - bx, ay = g[1] - by, az = g[2] - bz;
  const size_t base = ((size_t)(int)bz * (size_t)ny + (size_t)(int)by) * (size_t)nx + (size_t)(int)bx;
  const size_t row = (size_t)nx, slice = (size_t)nx * (size_t)ny;
  const TsdfPair p00 = tsdf_pair(vol, base), p10 = tsdf_pair(vol, base + row);
  const TsdfPair p01 = tsdf_pair(vol, base + slice), p11 = tsdf_pair(vol, base + slice + row);
  if (!(p00.w0 > 0.0f && p00.w1 > 0.0f && p10.w0 > 0.0f && p10.w1 > 0.0f && p01.w0 > 0.0f && p01.w1 > 0.0f && p11.w0 > 0.0f &&
        p11.w1 > 0.0f))
    return false;
  const float c00 = p00.t0 + ax * (p00.t1 - p00.t0), c10 = p10.t0 + ax * (p10.t1 - p10.t0);
  const float c01 = p01.t0 + ax * (p01.t1 - p01.t0), c11 = p11.t0 + ax * (p11.t1 - p11.t0);
  const float c0 = c00 + ay * (c10 - c00), c1 = c01 + ay * (c11 - c01);
  *f = c0 + az * (c1 - c0);
  return true;
}

// grid coordinate of the camera-frame point (xn s, yn s, s) under the world-to-camera pose (R, t): c = X_c - t,
// X_w = R^T c with each component (R_0j c_0 + R_1j c_1) + R_2j c_2, g = (X_w - origin) / voxel_size - 0.5
ICP_HD void tsdf_grid_point(float xn, float yn, float s, const float *R, const float *t, const float *origin, float voxel_size,
                            float *g) {
  const float c[3] = {xn * s - t[0], yn * s - t[1], s - t[2]};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float xw = (R[j] * c[0] + R[3 + j] * c[1]) + R[6 + j] * c[2];
    g[j] = (xw - origin[j]) / voxel_size - 0.5f;
  }
}

// depth of the zero crossing between the samples (s_prev, f_prev > 0) and (s_prev + step, f <= 0)
ICP_HD float tsdf_hit(float s_prev, float step, float f_prev, float f) { return s_prev + step * (f_prev / (f_prev - f)); }

// the normal at grid coordinate g: the central difference of the trilinear field over +- one voxel per axis (all six samples
// valid), rotated into the camera frame, normalised, turned towards the camera (v is the vertex).  false and zeros otherwise.
ICP_HD bool tsdf_normal(const float *vol, int nx, int ny, int nz, const float *g, const float *R, const float *v, float *n) {
  n[0] = n[1] = n[2] = 0.0f;
  float grad[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float hi[3] = {g[0], g[1], g[2]}, lo[3] = {g[0], g[1], g[2]}, fh, fl;
    hi[a] = g[a] + 1.0f;
    lo[a] = g[a] - 1.0f;
    ok = tsdf_sample(vol, nx, ny, nz, hi, &fh) && ok;
    ok = tsdf_sample(vol, nx, ny, nz, lo, &fl) && ok;
    grad[a] = fh - fl;
  }
  if (!ok) return false;
  float m[3];
  icp_rotate(R, grad, m);
  const float len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  if (!(len2 > 0.0f) || !(len2 < INFINITY)) return false;
  const float len = sqrtf(len2);
  const float e[3] = {m[0] / len, m[1] / len, m[2] / len};
  const float facing = (e[0] * v[0] + e[1] * v[1]) + e[2] * v[2];
  const float s = facing > 0.0f ? -1.0f : 1.0f;
  n[0] = s * e[0];
  n[1] = s * e[1];
  n[2] = s * e[2];
  return true;
}

// (Ra, ta) o (Rb, tb): R = Ra Rb, t = Ra tb + ta; products and the (a + b) + c sums in float64, rounded to float32
ICP_HD void tsdf_compose(const float *ra, const float *ta, const float *rb, const float *tb, float *r, float *t) {
  float ro[9], to[3];
  for (int i = 0; i < 3; ++i) {
    const double a0 = (double)ra[i * 3], a1 = (double)ra[i * 3 + 1], a2 = (double)ra[i * 3 + 2];
    for (int j = 0; j < 3; ++j) ro[i * 3 + j] = (float)((a0 * (double)rb[j] + a1 * (double)rb[3 + j]) + a2 * (double)rb[6 + j]);
    to[i] = (float)(((a0 * (double)tb[0] + a1 * (double)tb[1]) + a2 * (double)tb[2]) + (double)ta[i]);
  }
  for (int i = 0; i < 9; ++i) r[i] = ro[i];
  for (int i = 0; i < 3; ++i) t[i] = to[i];
}

}  // namespace
