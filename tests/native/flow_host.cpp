// Host harness for the arithmetic of csrc/flow.hip (no GPU is touched: nothing is launched): csrc/flow_math.h -- the pyramid's
// tap sums, the clamped bilinear sample, the template, the 2x2 solve, the loss rules, the cell of a point -- driven as the
// kernels drive it: 64 lanes that each add their window pixels in index order, then the neighbour tree.
// tests/test_flow_host.py compiles it with hipcc, plain and under the host sanitizers, and compares its output with
// tests/flow_oracle.py.  Raw little-endian float32 / int32 on both standard streams.
//   flow_host pyr H W LEVELS < frame                    H*W floats -> the levels one after the other, unpadded
//   flow_host track H W LEVELS RADIUS MAXIT EPS MINEIG K GUESS < frame1 frame2 keypoints [guesses]
//                                                       -> K records {float y2, x2, residual; int32 status, code, iterations}
//   flow_host cells H W CELL N < points                 N (y, x) pairs -> N int32 cells
#include "../../onnx_image_processing_amd/csrc/flow_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool read_floats(std::vector<float> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(float), n, stdin) == n;
}

static std::vector<std::vector<float>> build_pyramid(const std::vector<float> &frame, const FlLevels &lv, int levels) {
  std::vector<std::vector<float>> p((size_t)levels);
  p[0] = frame;
  for (int l = 1; l < levels; ++l) {
    p[(size_t)l].resize((size_t)lv.h[l] * lv.w[l]);
    for (int y = 0; y < lv.h[l]; ++y)
      for (int x = 0; x < lv.w[l]; ++x)
        p[(size_t)l][(size_t)y * lv.w[l] + x] = fl_pyr_down(p[(size_t)l - 1].data(), lv.h[l - 1], lv.w[l - 1], y, x);
  }
  return p;
}

static float tree(float *p) {                                            // wave_sum_dpp's order
  for (int o = 1; o < 64; o <<= 1)
    for (int l = 0; l < 64; l += 2 * o) p[l] += p[l + o];
  return p[0];
}

struct Record {
  float y, x, residual;
  int32_t status, code, iterations;
};

// fl_track_kernel, lane by lane
static Record track_point(const std::vector<std::vector<float>> &p1, const std::vector<std::vector<float>> &p2, const FlLevels &lv,
                          int levels, int r, int max_it, float eps2, float min_eigen, float py, float px, bool has_guess, float gy0,
                          float gx0) {
  const int n = (2 * r + 1) * (2 * r + 1), nj = (n + 63) / 64;
  int lost = fl_input_lost(py, px, has_guess, gy0, gx0, lv.h[0], lv.w[0]) ? MI_FLOW_PADDING : MI_FLOW_OK;
  const float top = 1.0f / (float)(1 << (levels - 1));
  float dx = gx0 * top, dy = gy0 * top, mean_abs = 0.0f;
  int its = 0;
  std::vector<float> t((size_t)nj * 64), gx((size_t)nj * 64), gy((size_t)nj * 64);
  std::vector<int> qx((size_t)nj * 64), qy((size_t)nj * 64);
  for (int q = 0; q < nj * 64; ++q) fl_pixel(q < n ? q : 0, r, &qx[(size_t)q], &qy[(size_t)q]);
  for (int l = levels - 1; l >= 0 && lost == MI_FLOW_OK; --l) {
    const int h = lv.h[l], w = lv.w[l];
    const float *f1 = p1[(size_t)l].data(), *f2 = p2[(size_t)l].data();
    const float scale = 1.0f / (float)(1 << l);
    const float cx = px * scale, cy = py * scale;
    float sxx[64], sxy[64], syy[64];
    for (int lane = 0; lane < 64; ++lane) {
      sxx[lane] = sxy[lane] = syy[lane] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        const size_t q = (size_t)lane + 64 * (size_t)j;
        if ((int)q < n) {
          fl_template(f1, h, w, cx, cy, qx[q], qy[q], &t[q], &gx[q], &gy[q]);
          sxx[lane] += gx[q] * gx[q];
          sxy[lane] += gx[q] * gy[q];
          syy[lane] += gy[q] * gy[q];
        }
      }
    }
    const float gxx = tree(sxx), gxy = tree(sxy), gyy = tree(syy);
    if (!(fl_min_eig(gxx, gxy, gyy, n) >= min_eigen)) {
      lost = MI_FLOW_FLAT;
      break;
    }
    const float det = gxx * gyy - gxy * gxy;
    for (int it = 0; it < max_it; ++it) {
      const float ox = cx + dx, oy = cy + dy;
      float sbx[64], sby[64], sab[64];
      for (int lane = 0; lane < 64; ++lane) {
        sbx[lane] = sby[lane] = sab[lane] = 0.0f;
        for (int j = 0; j < nj; ++j) {
          const size_t q = (size_t)lane + 64 * (size_t)j;
          if ((int)q < n) {
            const float e = t[q] - fl_sample(f2, h, w, ox + (float)qx[q], oy + (float)qy[q]);
            sbx[lane] += e * gx[q];
            sby[lane] += e * gy[q];
            sab[lane] += fabsf(e);
          }
        }
      }
      const float bx = tree(sbx), by = tree(sby);
      mean_abs = tree(sab) / (float)n;
      float sx, sy;
      fl_step(gxx, gxy, gyy, det, bx, by, &sx, &sy);
      dx += sx;
      dy += sy;
      ++its;
      if (sx * sx + sy * sy < eps2) break;
    }
    const float ex = cx + dx, ey = cy + dy;
    if (!fl_finite(ex) || !fl_finite(ey) || !fl_inside(ex, ey, h, w)) {
      lost = MI_FLOW_LEFT;
      break;
    }
    if (l > 0) {
      dx = 2.0f * dx;
      dy = 2.0f * dy;
    }
  }
  const bool ok = lost == MI_FLOW_OK;
  return Record{ok ? py + dy : -1.0f, ok ? px + dx : -1.0f, ok ? mean_abs : 0.0f, ok ? 1 : 0, lost, ok ? its : 0};
}

int main(int argc, char **argv) {
  if (argc >= 5 && !strcmp(argv[1], "pyr")) {
    const int h = atoi(argv[2]), w = atoi(argv[3]), levels = atoi(argv[4]);
    FlLevels lv;
    std::vector<float> frame;
    if (h < 1 || w < 1 || h > 4096 || w > 4096 || !fl_levels(1, h, w, levels, 1, &lv) || !read_floats(frame, (size_t)h * w)) return 2;
    for (const auto &level : build_pyramid(frame, lv, levels)) fwrite(level.data(), sizeof(float), level.size(), stdout);
    return 0;
  }
  if (argc == 11 && !strcmp(argv[1], "track")) {
    const int h = atoi(argv[2]), w = atoi(argv[3]), levels = atoi(argv[4]), r = atoi(argv[5]), max_it = atoi(argv[6]);
    const float eps = strtof(argv[7], nullptr), min_eigen = strtof(argv[8], nullptr);
    const int k = atoi(argv[9]), has_guess = atoi(argv[10]);
    FlLevels lv;
    if (h < 1 || w < 1 || h > 4096 || w > 4096 || r < 1 || r > MI_FLOW_MAX_RADIUS || !fl_levels(1, h, w, levels, r, &lv) || k < 0 ||
        k > 65536 || max_it < 1)
      return 2;
    std::vector<float> f1, f2, kp, guess;
    if (!read_floats(f1, (size_t)h * w) || !read_floats(f2, (size_t)h * w) || !read_floats(kp, (size_t)k * 2) ||
        !read_floats(guess, has_guess ? (size_t)k * 2 : 0))
      return 2;
    const auto p1 = build_pyramid(f1, lv, levels), p2 = build_pyramid(f2, lv, levels);
    for (int i = 0; i < k; ++i) {
      const Record rec = track_point(p1, p2, lv, levels, r, max_it, eps * eps, min_eigen, kp[2 * (size_t)i], kp[2 * (size_t)i + 1],
                                     has_guess != 0, has_guess ? guess[2 * (size_t)i] : 0.0f, has_guess ? guess[2 * (size_t)i + 1] : 0.0f);
      fwrite(&rec, sizeof(rec), 1, stdout);
    }
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "cells")) {
    const int h = atoi(argv[2]), w = atoi(argv[3]), cell = atoi(argv[4]), n = atoi(argv[5]);
    std::vector<float> pts;
    if (h < 1 || w < 1 || cell < 1 || n < 0 || n > 65536 || !read_floats(pts, (size_t)n * 2)) return 2;
    for (int i = 0; i < n; ++i) {
      const int32_t c = fl_cell(pts[2 * (size_t)i], pts[2 * (size_t)i + 1], h, w, cell, (w + cell - 1) / cell);
      fwrite(&c, sizeof(c), 1, stdout);
    }
    return 0;
  }
  fprintf(stderr, "usage: flow_host pyr H W LEVELS | track H W LEVELS RADIUS MAXIT EPS MINEIG K GUESS | cells H W CELL N\n");
  return 1;
}
