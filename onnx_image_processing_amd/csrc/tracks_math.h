// The arithmetic of K28's triangulation (tracks.hip; include/mi355x_match.h, "Triangulation"): one landmark from all
// the frames that see it -- the point closest to the viewing rays in the least-squares sense, by the symmetric 3x3 cofactor
// inverse under K25's pivot rule -- and its gates.  float64 throughout, only + - * / and sqrt, every sum in the order the
// header states.  Like icp_math.h it is plain C++: any C++ compiler builds all of it (hipcc adds the HIP markers).
// tests/native/tracks_host.cpp runs it without a GPU against tests/tracks_oracle.py.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>      // first: the HIP markers icp_math.h uses under hipcc
#endif
#include "icp_math.h"     // ICP_HD, ICP_PIVOT_RATIO

#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace {

struct TrkPoint {
  double X[3];         // zeros when the solve is unusable
  double e2max;        // +inf when undefined
  double cos_par;      // 1 when undefined
  int seen;
  bool usable, front, ok;
};

// d = R^T m / |m| for m = (x, y, 1); R row-major
ICP_HD void trk_ray(const float *R, float xf, float yf, double *d) {
  const double x = xf, y = yf;
  const double n = sqrt((x * x + y * y) + 1.0);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = (((double)R[k] * x + (double)R[3 + k] * y) + (double)R[6 + k]) / n;
}

// r (F, 3, 3), t (F, 3) of the window; obs + f * obs_stride: the (x, y) of frame f; vis[f * vis_stride]: its byte.
ICP_HD void trk_triangulate(const float *r, const float *t, const float *obs, size_t obs_stride, const uint8_t *vis,
                            size_t vis_stride, int F, int min_views, float max_e2, float max_cos, TrkPoint &o) {
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};      // A: 00 01 02 11 12 22
  o.seen = 0;
  for (int f = 0; f < F; ++f) {
    if (!vis[f * vis_stride]) continue;
    ++o.seen;
    const float *R = r + f * 9, *T = t + f * 3;
    double d[3], c[3];
    trk_ray(R, obs[f * obs_stride], obs[f * obs_stride + 1], d);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = -(((double)R[k] * (double)T[0] + (double)R[3 + k] * (double)T[1]) + (double)R[6 + k] * (double)T[2]);
    const double P[6] = {1.0 - d[0] * d[0], 0.0 - d[0] * d[1], 0.0 - d[0] * d[2], 1.0 - d[1] * d[1], 0.0 - d[1] * d[2], 1.0 - d[2] * d[2]};
#pragma unroll
    for (int k = 0; k < 6; ++k) A[k] += P[k];
    b[0] += (P[0] * c[0] + P[1] * c[1]) + P[2] * c[2];
    b[1] += (P[1] * c[0] + P[3] * c[1]) + P[4] * c[2];
    b[2] += (P[2] * c[0] + P[4] * c[1]) + P[5] * c[2];
  }
  const double C[6] = {A[3] * A[5] - A[4] * A[4], A[2] * A[4] - A[1] * A[5], A[1] * A[4] - A[2] * A[3],
                       A[0] * A[5] - A[2] * A[2], A[1] * A[2] - A[0] * A[4], A[0] * A[3] - A[1] * A[1]};
  const double det = (A[0] * C[0] + A[1] * C[1]) + A[2] * C[2];
  const double p1 = C[5] / A[0], p2 = det / C[5];
  double dmax = A[0] > A[3] ? A[0] : A[3];
  dmax = A[5] > dmax ? A[5] : dmax;
  const double thr = ICP_PIVOT_RATIO * dmax;
  o.usable = dmax > 0.0 && A[0] > thr && p1 > thr && p2 > thr;              // a NaN pivot fails its comparison
  o.X[0] = ((C[0] * b[0] + C[1] * b[1]) + C[2] * b[2]) / det;
  o.X[1] = ((C[1] * b[0] + C[3] * b[1]) + C[4] * b[2]) / det;
  o.X[2] = ((C[2] * b[0] + C[4] * b[1]) + C[5] * b[2]) / det;
#pragma unroll
  for (int k = 0; k < 3; ++k) o.usable = o.usable && fabs(o.X[k]) < INFINITY;
  if (!o.usable) o.X[0] = o.X[1] = o.X[2] = 0.0;
  o.front = true;
  o.e2max = o.usable ? 0.0 : (double)INFINITY;
  o.cos_par = 1.0;
  for (int f = 0; f < F; ++f) {
    if (!vis[f * vis_stride]) continue;
    const float *R = r + f * 9, *T = t + f * 3;
    if (o.usable) {
      double q[3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
        q[i] = (((double)R[3 * i] * o.X[0] + (double)R[3 * i + 1] * o.X[1]) + (double)R[3 * i + 2] * o.X[2]) + (double)T[i];
      if (q[2] > 0.0) {
        const double u = q[0] / q[2] - (double)obs[f * obs_stride], v = q[1] / q[2] - (double)obs[f * obs_stride + 1];
        const double e2 = u * u + v * v;
        o.e2max = e2 > o.e2max ? e2 : o.e2max;
        if (!(e2 < INFINITY)) o.e2max = (double)INFINITY;                    // NaN included
      } else {
        o.front = false;
        o.e2max = (double)INFINITY;
      }
    }
    double da[3];
    trk_ray(R, obs[f * obs_stride], obs[f * obs_stride + 1], da);
    for (int g = f + 1; g < F; ++g) {
      if (!vis[g * vis_stride]) continue;
      double db[3];
      trk_ray(r + g * 9, obs[g * obs_stride], obs[g * obs_stride + 1], db);
      const double cs = (da[0] * db[0] + da[1] * db[1]) + da[2] * db[2];
      o.cos_par = cs < o.cos_par ? cs : o.cos_par;
    }
  }
  o.ok = o.seen >= min_views && o.usable && o.front && o.e2max <= (double)max_e2 && o.cos_par <= (double)max_cos;
}

}  // namespace
