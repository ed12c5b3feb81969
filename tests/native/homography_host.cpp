// Host harness for the arithmetic of csrc/homography.hip (no GPU is touched: nothing is launched): the shared sampler
// (csrc/pose_sampler.h) and the minimal solve, transfer error and decomposition of csrc/homography_math.h, exactly the code
// the kernels run.  tests/test_homography_host.py compiles it with hipcc and compares its output with
// tests/homography_oracle.py.
//   homography_host ranks                 prints "seed b h nv r0 r1 r2 r3" for nv in (4, 5, 64, 97), 50 hypotheses each
//   homography_host solve < samples       4 lines "x1 y1 x2 y2" per sample -> one line "ok m(18)" per sample
//   homography_host score < model+rows    18 floats, then lines "x1 y1 x2 y2" -> one d^2 per row
//   homography_host pose < h+rows         "n", 9 floats, n lines "x1 y1 x2 y2" -> "ok rotation_only spread", then 4 lines
//                                         "count R(9) t(3) n(3)" in slot order (serial counts; every row is masked in)
#include "../../onnx_image_processing_amd/csrc/homography_math.h"
#include "../../onnx_image_processing_amd/csrc/pose_sampler.h"

#include <cstdio>
#include <cstring>
#include <vector>

static bool read_row(float4 &q) { return scanf("%f %f %f %f", &q.x, &q.y, &q.z, &q.w) == 4; }

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "ranks")) {
    for (int nv : {4, 5, 64, 97})
      for (unsigned h = 0; h < 50; ++h) {
        int pick[4];
        po_sample_ranks<4>(5u, 1u, h, nv, pick);
        printf("5 1 %u %d %d %d %d %d\n", h, nv, pick[0], pick[1], pick[2], pick[3]);
      }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "solve")) {
    float4 q[4];
    for (;;) {
      for (int s = 0; s < 4; ++s)
        if (!read_row(q[s])) return 0;
      float m[18];
      const bool ok = hg_solve_minimal(q, m);
      printf("%d", ok ? 1 : 0);
      for (int c = 0; c < 18; ++c) printf(" %.9g", ok ? m[c] : 0.0f);
      printf("\n");
    }
  }
  if (argc == 2 && !strcmp(argv[1], "score")) {
    float m[18];
    for (int c = 0; c < 18; ++c)
      if (scanf("%f", &m[c]) != 1) return 2;
    float4 q;
    while (read_row(q)) printf("%.9g\n", hg_dist2(m, q));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "pose")) {
    int n;
    while (scanf("%d", &n) == 1) {
      if (n < 0 || n > 4096) return 2;
      float h[9], fro = 0.0f;
      for (int c = 0; c < 9; ++c) {
        if (scanf("%f", &h[c]) != 1) return 2;
        fro += h[c] * h[c];
      }
      std::vector<float4> rows((size_t)n);
      for (int i = 0; i < n; ++i)
        if (!read_row(rows[(size_t)i])) return 2;
      bool usable = fro > 0.0f && fro < INFINITY;
      const float sc = 1.0f / sqrtf(fro);
      for (int c = 0; c < 9; ++c) h[c] = usable ? h[c] * sc : 0.0f;
      int pos = 0;
      for (const float4 &q : rows) pos += hg_bilinear(h, q) > 0.0f ? 1 : 0;
      if (2 * pos < n)
        for (int c = 0; c < 9; ++c) h[c] = -h[c];
      HgPose p = {};
      usable = usable && hg_decompose(h, p);
      int cnt[4] = {0, 0, 0, 0}, order[4];
      float trace[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int k = 0; k < 4 && usable; ++k) {
        for (const float4 &q : rows) cnt[k] += (p.rotation_only || hg_in_front(p.r[k], p.t[k], p.n[k], q)) ? 1 : 0;
        trace[k] = (p.r[k][0] + p.r[k][4]) + p.r[k][8];
      }
      hg_order(cnt, trace, order);
      const bool ok = usable && cnt[order[0]] >= HG_MIN_POSE_ROWS;
      printf("%d %d %.9g\n", ok ? 1 : 0, (ok && p.rotation_only) ? 1 : 0, usable ? p.spread : 0.0f);
      for (int s = 0; s < 4; ++s) {
        const int k = order[s];
        printf("%d", ok ? cnt[k] : 0);
        for (int c = 0; c < 9; ++c) printf(" %.9g", ok ? p.r[k][c] : (c % 4 == 0 ? 1.0f : 0.0f));
        for (int c = 0; c < 3; ++c) printf(" %.9g", ok ? p.t[k][c] : 0.0f);
        for (int c = 0; c < 3; ++c) printf(" %.9g", ok ? p.n[k][c] : 0.0f);
        printf("\n");
      }
    }
    return 0;
  }
  fprintf(stderr, "usage: homography_host ranks | solve | score | pose  (input on stdin)\n");
  return 1;
}
