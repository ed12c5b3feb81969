// What K21 (photo.hip) shares with K18 (icp.hip): the slab geometry, the host-side checks and the launches of K18i and K18r,
// whose kernels live in icp.hip alone.
#pragma once
#include "common.h"

#include <math.h>

struct IcpCam {
  float fx, fy, cx, cy;
};

// K18i over `batch` pairs and K18r over the slabs of `stride` into slabs[(pair * max_slabs + slab) * ICP_REC ...], defined in
// icp.hip.  pose64 / state as icp_reduce_kernel takes them (either may be null).
int icp_init_launch(const float *r0, const float *t0, int batch, double *pose, int *state, int *steps, hipStream_t s);
int icp_reduce_launch(const float4 *v1, const float4 *n1, const float4 *v2, const float4 *n2, const float *r, const float *t,
                      const double *pose64, const int *state, int batch, int h, int w, int stride, int max_slabs, IcpCam cam,
                      float thr2, float cos_thr, double *slabs, hipStream_t s);

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_PER_LANE = 8;
constexpr int ICP_SLAB = ICP_THREADS * ICP_PER_LANE;       // sampled pixels per workgroup
constexpr int ICP_REC = 32;                                // doubles per slab record (29 used)

inline int icp_shape_status(int batch, int h, int w) {
  if (batch < 1 || h < 3 || w < 3) return MI_E_SHAPE;
  if (batch > 65535) return MI_E_PARAM;
  if ((long long)batch * h * w >= 0x80000000LL) return MI_E_SHAPE;
  return MI_OK;
}
inline bool icp_stride_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }
inline bool icp_positive(float v) { return v > 0.0f && v < INFINITY; }
inline int icp_gate_status(float fx, float fy, float cx, float cy, float distance_threshold, float angle_threshold) {
  if (!icp_positive(fx) || !icp_positive(fy) || !(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY) ||
      !icp_positive(distance_threshold) || !(angle_threshold > 0.0f) || !(angle_threshold <= 3.14159274f))
    return MI_E_PARAM;
  return MI_OK;
}
inline int icp_samples(int h, int w, int s, int *ws) {
  *ws = (w + s - 1) / s;
  return ((h + s - 1) / s) * *ws;
}

}  // namespace
