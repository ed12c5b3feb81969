// The arithmetic of K22 (tsdf_gray.hip; include/mi355x_match.h, "TSDF intensity"): the gate and the running mean of a voxel's
// gray value beside K19's update, the world point of a camera-frame point, and the weight-normalised trilinear blend of the
// intensity volume over the observed corners of a cell.  float32 with nothing fused.  No HIP header is needed: a plain C++
// compiler builds it for the host as well (tests/native/tsdf_gray_host.cpp runs it without a GPU).
#pragma once
#include "tsdf_math.h"

namespace {

// after tsdf_fuse(d, ...) returned `fused` for the voxel at camera depth qz: true when the voxel lies inside the truncation
// band in front of the surface too (sdf <= truncation; behind it tsdf_fuse has already refused).  sdf has tsdf_fuse's bits.
ICP_HD bool tsdf_gray_band(bool fused, float d, float z_scale, float qz, float truncation) {
  const float sdf = d * z_scale - qz;
  return fused && sdf <= truncation;
}

// one gray sample g (already fetched at the voxel's nearest pixel, the depth sample's own pixel) into the running mean and
// the clamped weight of a voxel inside the band.  false (nothing changes) when g is not finite.
ICP_HD bool tsdf_gray_fuse(float g, float max_weight, float *gray, float *gweight) {
  if (!(fabsf(g) < INFINITY)) return false;
  const float w = *gweight;
  *gray = ((*gray) * w + g) / (w + 1.0f);
  *gweight = fminf(w + 1.0f, max_weight);
  return true;
}

// the world point of the camera-frame point p under the world-to-camera pose (R, t): c = p - t, X_w = R^T c with each
// component (R_0j c_0 + R_1j c_1) + R_2j c_2: tsdf_grid_point's operations, so a raycast vertex (xn s, yn s, s) gets the
// raycast's own bits
ICP_HD void tsdf_gray_world(const float *p, const float *R, const float *t, float *xw) {
  const float c[3] = {p[0] - t[0], p[1] - t[1], p[2] - t[2]};
#pragma unroll
  for (int j = 0; j < 3; ++j) xw[j] = (R[j] * c[0] + R[3 + j] * c[1]) + R[6 + j] * c[2];
}

// the intensity at the world point xw of an intensity volume of (nz, ny, nx) records (gray, gweight), x fastest: the grid
// coordinate g = (xw - origin) / voxel_size - 0.5 must lie in [0, n - 1] on every axis (NaN fails); the cell is b =
// min(floor(g), n - 2), so that the last layer is reached with a = 1; over the corners m = 0..7 (x is bit 0, y bit 1, z bit 2)
// with the weight (wx * wy) * wz, num and den are the running sums of w gray and w over the corners with gweight > 0.
// false (and *I = 0) unless den > 0.
ICP_HD bool tsdf_gray_sample(const float *ivol, int nx, int ny, int nz, const float *xw, const float *origin, float voxel_size,
                             float *I) {
  *I = 0.0f;
  const int n[3] = {nx, ny, nz};
  float b[3], a[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float g = (xw[k] - origin[k]) / voxel_size - 0.5f;
    if (!(g >= 0.0f && g <= (float)(n[k] - 1))) return false;
    b[k] = fminf(floorf(g), (float)(n[k] - 2));
    a[k] = g - b[k];
  }
  const size_t base = ((size_t)(int)b[2] * (size_t)ny + (size_t)(int)b[1]) * (size_t)nx + (size_t)(int)b[0];
  const size_t row = (size_t)nx, slice = (size_t)nx * (size_t)ny;
  const TsdfPair p[4] = {tsdf_pair(ivol, base), tsdf_pair(ivol, base + row), tsdf_pair(ivol, base + slice),
                         tsdf_pair(ivol, base + slice + row)};
  const float wx[2] = {1.0f - a[0], a[0]}, wy[2] = {1.0f - a[1], a[1]}, wz[2] = {1.0f - a[2], a[2]};
  float num = 0.0f, den = 0.0f;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const TsdfPair &q = p[m >> 1];
    const float gray = (m & 1) ? q.t1 : q.t0, gw = (m & 1) ? q.w1 : q.w0;
    const float w = (wx[m & 1] * wy[(m >> 1) & 1]) * wz[m >> 2];
    if (gw > 0.0f) {
      num = num + w * gray;
      den = den + w;
    }
  }
  if (!(den > 0.0f)) return false;
  *I = num / den;
  return true;
}

}  // namespace
