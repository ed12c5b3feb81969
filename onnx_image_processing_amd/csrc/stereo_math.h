// The arithmetic of K33 (include/mi355x_match_stereo.h: "Census", "Cost", "Paths", "Selection", "Depth") shared by
// csrc/stereo.hip and a host compile (tests/native/stereo_host.cpp): integers from the census bits to the aggregated volume,
// float32 for the sub-pixel step and the division, operation by operation as the header states it.  Nothing here launches or
// reads a device.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi355x_match_stereo.h"

#define ST_HD __host__ __device__ __forceinline__

// a neighbour disparity that does not exist (d - 1 at d = 0, d + 1 at d = D - 1): above every L_r + P1, far below overflow
#define ST_ABSENT 0x3fff

// the eight directions (dy, dx) in the header's order
static const int ST_DIRS[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};

ST_HD int st_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// "Census": the 62 compares of pixel (y, x) of one frame g (h x w), replicate border.  T is uint8_t or float.
template <typename T>
ST_HD uint64_t st_census(const T *g, int h, int w, int y, int x) {
  const T c = g[(size_t)y * w + x];
  uint64_t bits = 0;
  int k = 0;
  for (int dy = -3; dy <= 3; ++dy) {
    const T *row = g + (size_t)st_clamp(y + dy, h - 1) * w;
    for (int dx = -4; dx <= 4; ++dx) {
      if (dy == 0 && dx == 0) continue;
      bits |= (uint64_t)(row[st_clamp(x + dx, w - 1)] < c ? 1 : 0) << k;
      ++k;
    }
  }
  return bits;
}

// "Cost" from the left census word and the right one at x - d; `inside` is x - d >= 0
ST_HD int st_cost(uint64_t left, uint64_t right, bool inside) {
  return inside ? __builtin_popcountll(left ^ right) : MI_STEREO_COST_OUTSIDE;
}

ST_HD int st_min(int a, int b) { return a < b ? a : b; }

// "Paths": L_r(p, d) from the cost and the predecessor's L_r at d, d - 1, d + 1 (ST_ABSENT where there is none) and minimum m
ST_HD int st_path_step(int c, int prev, int prev_lo, int prev_hi, int m, int p1, int p2) {
  return c + st_min(st_min(prev, m + p2), st_min(prev_lo, prev_hi) + p1) - m;
}

// the number of path lines of one image in direction (dy, dx), and the first pixel of line i: the pixels whose predecessor
// is outside the frame.  Lines 0 .. w - 1 (dy != 0) start on the first row of the walk, the others on its first column.
ST_HD int st_lines(int h, int w, int dy, int dx) { return dy == 0 ? h : (dx == 0 ? w : w + h - 1); }
ST_HD void st_line_start(int i, int h, int w, int dy, int dx, int *y, int *x) {
  if (dy == 0) {
    *y = i;
    *x = dx > 0 ? 0 : w - 1;
  } else if (i < w) {
    *y = dy > 0 ? 0 : h - 1;
    *x = i;
  } else {
    *y = dy > 0 ? 1 + (i - w) : h - 2 - (i - w);
    *x = dx > 0 ? 0 : w - 1;
  }
}

// "Selection": the key whose minimum is the lowest S and, among equals, the lowest d (S <= 2552, d <= 255)
ST_HD uint32_t st_key(int s, int d) { return ((uint32_t)s << 8) | (uint32_t)d; }
ST_HD int st_key_d(uint32_t key) { return (int)(key & 255u); }
ST_HD int st_key_s(uint32_t key) { return (int)(key >> 8); }

// does disparity d with sum s make the winner (d_best, s_best) not unique?
ST_HD bool st_rival(int s, int d, int s_best, int d_best, int uniqueness) {
  const int gap = d > d_best ? d - d_best : d_best - d;
  return gap > 1 && s * (100 - uniqueness) < s_best * 100;
}

// the left-right test of a pixel at column x with winner d_best; dR(y, x - d_best) is read only when x - d_best is a column of
// the right view beyond its first MI_STEREO_BORDER
ST_HD bool st_lr_fails(int x, int d_best, const int16_t *right_row, int lr_max_diff) {
  if (x - d_best < MI_STEREO_BORDER) return true;
  const int diff = (int)right_row[x - d_best] - d_best;
  return (diff < 0 ? -diff : diff) > lr_max_diff;
}

// the parabola through S(d* - 1), S(d*), S(d* + 1); s_lo, s_hi are not read at d* = 0 and d* = D - 1
ST_HD float st_subpixel(int d_best, int D, int s_lo, int s_best, int s_hi) {
  if (d_best <= 0 || d_best >= D - 1) return (float)d_best;
  const int den = s_lo + s_hi - 2 * s_best;
  const float offset = den > 0 ? (float)(s_lo - s_hi) / (float)(2 * den) : 0.0f;
  return (float)d_best + offset;
}

// "Depth"
ST_HD float st_depth(float disparity, float fb, float min_disparity) { return disparity >= min_disparity ? fb / disparity : 0.0f; }
