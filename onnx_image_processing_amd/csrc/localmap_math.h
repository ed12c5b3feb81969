// The arithmetic of K29 (localmap.hip; include/mi355x_match.h): a landmark's projection and its in-view gates, the
// window test, the key of a keypoint, the best-two pair and its order-independent merge, K26's vote as the candidate test, the
// claim key, and the median distance of a view for the representative descriptor.  float64 geometry in the header's stated
// operation order, integers everywhere else.  Like tracks_math.h it is plain C++: any C++ compiler builds all of it (hipcc adds
// the HIP markers).  tests/native/localmap_host.cpp runs it without a GPU against tests/localmap_oracle.py.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>      // first: the HIP markers icp_math.h uses under hipcc
#endif
#include "icp_math.h"     // ICP_HD

#include <math.h>
#include <stdint.h>

namespace {

constexpr int LM_MAX_FRAMES = 16;
constexpr uint32_t LM_EMPTY = 0xffffffffu;           // "no keypoint": above every key (hamming <= 512, j < 1024)
constexpr int LM_NO_CLAIM = 0x7fffffff;              // above every claim key (d1 <= 512, l < 2048)

struct LmProj {
  double u, v;
  bool in_view;
};

// R (3, 3) row-major, T (3), cam = fx, fy, cx, cy, X (3); every float32 is widened exactly
ICP_HD LmProj lm_project(const float *R, const float *T, const float *cam, const float *X, bool valid, int height, int width,
                         float min_depth, float max_depth) {
  double q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    q[i] = (((double)R[3 * i] * (double)X[0] + (double)R[3 * i + 1] * (double)X[1]) + (double)R[3 * i + 2] * (double)X[2]) + (double)T[i];
  const double z = q[2];
  LmProj p;
  p.u = (double)cam[0] * (q[0] / z) + (double)cam[2];
  p.v = (double)cam[1] * (q[1] / z) + (double)cam[3];
  const bool finite = fabs(q[0]) < INFINITY && fabs(q[1]) < INFINITY && fabs(q[2]) < INFINITY;        // a NaN fails its comparison
  p.in_view = valid && finite && z >= (double)min_depth && z <= (double)max_depth && p.u >= 0.0 && p.u <= (double)(width - 1) &&
              p.v >= 0.0 && p.v <= (double)(height - 1);
  return p;
}

// r2 = (double)radius * (double)radius; a NaN coordinate is outside
ICP_HD bool lm_in_window(float ky, float kx, double u, double v, double r2) {
  const double du = (double)kx - u, dv = (double)ky - v;
  return du * du + dv * dv <= r2;
}

ICP_HD int lm_popcount(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

ICP_HD uint32_t lm_key(int hamming, int j) { return (uint32_t)hamming << 16 | (uint32_t)j; }

// (k1 <= k2): the two smallest keys seen so far.  Keys of different keypoints differ, so neither the order of the pushes nor
// that of the merges changes the result.
struct LmPair {
  uint32_t k1, k2;
};

ICP_HD void lm_push(LmPair &p, uint32_t key) {
  const uint32_t hi = key > p.k1 ? key : p.k1;
  p.k1 = key < p.k1 ? key : p.k1;
  p.k2 = hi < p.k2 ? hi : p.k2;
}

ICP_HD LmPair lm_merge(LmPair a, LmPair b) {
  LmPair r;
  const uint32_t hi = a.k1 > b.k1 ? a.k1 : b.k1, lo2 = a.k2 < b.k2 ? a.k2 : b.k2;
  r.k1 = a.k1 < b.k1 ? a.k1 : b.k1;
  r.k2 = hi < lo2 ? hi : lo2;
  return r;
}

ICP_HD void lm_decode(LmPair p, int num_bits, int *d1, int *j1, int *d2) {
  *d1 = p.k1 == LM_EMPTY ? num_bits + 1 : (int)(p.k1 >> 16);
  *j1 = p.k1 == LM_EMPTY ? -1 : (int)(p.k1 & 0xffffu);
  *d2 = p.k2 == LM_EMPTY ? num_bits + 1 : (int)(p.k2 >> 16);
}

// K26's vote: one float32 multiply, one compare
ICP_HD bool lm_candidate(int d1, int d2, int max_distance, float ratio) { return d1 <= max_distance && (float)d1 < ratio * (float)d2; }

ICP_HD int lm_claim_key(int d1, int l) { return d1 << 16 | l; }
ICP_HD int lm_claim_landmark(int claim) { return claim == LM_NO_CLAIM ? -1 : (claim & 0xffff); }

// element (n - 1) / 2 of the ascending list of the distances d[b] over the views b (bit b of `views`, n of them, n >= 1): the
// distance whose rank under (distance, b) is (n - 1) / 2.  Fully unrolled: d stays in registers.
ICP_HD int lm_median(const int (&d)[LM_MAX_FRAMES], unsigned views, int n) {
  const int want = (n - 1) / 2;
  int med = 0;
#pragma unroll
  for (int b = 0; b < LM_MAX_FRAMES; ++b) {
    int rank = 0;
#pragma unroll
    for (int c = 0; c < LM_MAX_FRAMES; ++c) rank += ((views >> c) & 1u) && (d[c] < d[b] || (d[c] == d[b] && c < b)) ? 1 : 0;
    if (((views >> b) & 1u) && rank == want) med = d[b];
  }
  return med;
}

// the key the representative minimises
ICP_HD int lm_rep_key(int med, int frame) { return med << 8 | frame; }

}  // namespace
