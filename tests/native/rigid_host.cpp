// Host harness for the arithmetic of csrc/rigid.hip (no GPU is touched: nothing is launched): the shared sampler
// (csrc/pose_sampler.h) and the Horn solve, degeneracy tests and score of csrc/rigid_math.h, exactly the code the kernels
// run.  tests/test_rigid_host.py compiles it with hipcc and compares its output with tests/rigid_oracle.py.
//   rigid_host draws                    prints "seed b h slot value" for a fixed grid of arguments, slots 0 .. 2
//   rigid_host ranks                    prints "seed b h nv r0 r1 r2" for nv in (3, 4, 64, 97), 50 hypotheses each
//   rigid_host solve < samples          3 lines "ax ay az bx by bz" per sample -> one line "ok R(9) t(3)" per sample
//   rigid_host fit < sets               "n" then n lines "ax ay az bx by bz" -> "ok R(9) t(3) rms" (two passes, serial sums)
#include "../../onnx_image_processing_amd/csrc/pose_sampler.h"
#include "../../onnx_image_processing_amd/csrc/rigid_math.h"

#include <cstdio>
#include <cstring>
#include <vector>

static bool read_row(RgRow &q) {
  return scanf("%f %f %f %f %f %f", &q.a[0], &q.a[1], &q.a[2], &q.b[0], &q.b[1], &q.b[2]) == 6;
}

static void print_rt(bool ok, const float *rt) {
  printf("%d", ok ? 1 : 0);
  for (int i = 0; i < 12; ++i) printf(" %.9g", ok ? rt[i] : 0.0f);
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "draws")) {
    for (unsigned seed : {0u, 5u, 0xFFFFFFFFu})
      for (unsigned b : {0u, 2u, 65534u})
        for (unsigned h : {0u, 63u, 199u, 65535u})
          for (unsigned s = 0; s < 3; ++s) printf("%u %u %u %u %u\n", seed, b, h, s, po_draw(seed, b, h, s));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "ranks")) {
    for (int nv : {3, 4, 64, 97})
      for (unsigned h = 0; h < 50; ++h) {
        int pick[3];
        po_sample_ranks<3>(5u, 1u, h, nv, pick);
        printf("5 1 %u %d %d %d %d\n", h, nv, pick[0], pick[1], pick[2]);
      }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "solve")) {
    RgRow q[3];
    for (;;) {
      for (int s = 0; s < 3; ++s)
        if (!read_row(q[s])) return 0;
      float rt[12];
      const bool ok = rg_solve_minimal(q, rt);
      print_rt(ok, rt);
      printf("\n");
    }
  }
  if (argc == 2 && !strcmp(argv[1], "fit")) {
    int n;
    while (scanf("%d", &n) == 1) {
      if (n < 0 || n > 4096) return 2;
      std::vector<RgRow> rows((size_t)n);
      for (int i = 0; i < n; ++i)
        if (!read_row(rows[(size_t)i])) return 2;
      float rt[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      bool ok = n >= 3;
      float rms = 0.0f;
      if (ok) {
        float ca[3] = {0.0f, 0.0f, 0.0f}, cb[3] = {0.0f, 0.0f, 0.0f}, acc[21];
        for (const RgRow &q : rows)
          for (int j = 0; j < 3; ++j) { ca[j] += q.a[j]; cb[j] += q.b[j]; }
        for (int j = 0; j < 3; ++j) { ca[j] = ca[j] / (float)n; cb[j] = cb[j] / (float)n; }
        for (int k = 0; k < 21; ++k) acc[k] = 0.0f;
        for (const RgRow &q : rows) {
          const float a[3] = {q.a[0] - ca[0], q.a[1] - ca[1], q.a[2] - ca[2]}, b[3] = {q.b[0] - cb[0], q.b[1] - cb[1], q.b[2] - cb[2]};
          int k = 0;
          for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) acc[k++] += a[r] * b[c];
          for (int r = 0; r < 3; ++r)
            for (int c = r; c < 3; ++c) { acc[k] += a[r] * a[c]; acc[k + 6] += b[r] * b[c]; ++k; }
        }
        ok = !rg_scatter_degenerate(acc + 9) && !rg_scatter_degenerate(acc + 15);
        if (ok) {
          const float s[3][3] = {{acc[0], acc[1], acc[2]}, {acc[3], acc[4], acc[5]}, {acc[6], acc[7], acc[8]}};
          ok = rg_finish(s, ca, cb, rt);
        }
        if (ok) {
          float sum = 0.0f;
          for (const RgRow &q : rows) sum += rg_dist2(rt, q);
          rms = sqrtf(sum / (float)n);
        }
      }
      print_rt(ok, rt);
      printf(" %.9g\n", rms);
    }
    return 0;
  }
  fprintf(stderr, "usage: rigid_host draws | ranks | solve | fit  (input on stdin)\n");
  return 1;
}
