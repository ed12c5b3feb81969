// Host harness for the arithmetic of csrc/ba.hip (no GPU is touched: nothing is launched): one observation's lines, a
// landmark's damped 3x3 inverse and the packed LDL^T solve of csrc/ba_math.h, exactly the code the kernels run.
// tests/test_ba_host.py compiles it with hipcc -- once more with the host sanitizers -- and compares its output with
// tests/ba_oracle.py.
//   ba_host lines < rows    one line "huber", one line rt(12), then lines "X Y Z u v" ->
//                           "ok ju(6) jv(6) xu(3) xv(3) ru rv e2 w rho" per row (zeros, e2 = rho = inf where ok = 0), then
//                           "rho e2" of ba_rho, the cost's own form
//   ba_host inv3 < rows     lines "lambda v00 v01 v02 v11 v12 v22" -> "ok vi(6)"
//   ba_host ldlt < system   "n", the n (n + 1) / 2 elements of the packed upper triangle, the n of b -> "ok x(n)"; repeated
// %.9g prints a float32 and %.17g a float64 so that reading them back returns the same bits.
#include "../../onnx_image_processing_amd/csrc/ba_math.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "lines")) {
    float huber, rt[12], X[3], u, v;
    if (scanf("%f", &huber) != 1) return 2;
    for (int i = 0; i < 12; ++i)
      if (scanf("%f", &rt[i]) != 1) return 2;
    while (scanf("%f %f %f %f %f", &X[0], &X[1], &X[2], &u, &v) == 5) {
      BaLine q;
      const bool ok = ba_line(rt, X, u, v, huber, q);
      printf("%d", ok ? 1 : 0);
      for (int i = 0; i < 6; ++i) printf(" %.9g", ok ? q.ju[i] : 0.0f);
      for (int i = 0; i < 6; ++i) printf(" %.9g", ok ? q.jv[i] : 0.0f);
      for (int i = 0; i < 3; ++i) printf(" %.9g", ok ? q.xu[i] : 0.0f);
      for (int i = 0; i < 3; ++i) printf(" %.9g", ok ? q.xv[i] : 0.0f);
      printf(" %.9g %.9g %.9g %.9g %.9g", ok ? q.ru : 0.0f, ok ? q.rv : 0.0f, ok ? q.e2 : INFINITY, ok ? q.w : 0.0f, q.rho);
      float e2;
      const float rho = ba_rho(rt, X, u, v, huber, &e2);
      printf(" %.9g %.9g\n", rho, e2);
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "inv3")) {
    float lambda, V[6];
    while (scanf("%f %f %f %f %f %f %f", &lambda, &V[0], &V[1], &V[2], &V[3], &V[4], &V[5]) == 7) {
      float vi[6];
      const bool ok = ba_inv3(V, lambda, vi);
      printf("%d", ok ? 1 : 0);
      for (int i = 0; i < 6; ++i) printf(" %.9g", vi[i]);
      printf("\n");
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "ldlt")) {
    int n;
    while (scanf("%d", &n) == 1) {
      if (n < 0 || n > 96) return 2;                       // 6 * MI_BA_MAX_FRAMES
      std::vector<double> a((size_t)n * (n + 1) / 2 + 1), x((size_t)n + 1);
      for (int i = 0; i < n * (n + 1) / 2; ++i)
        if (scanf("%lf", &a[i]) != 1) return 2;
      for (int i = 0; i < n; ++i)
        if (scanf("%lf", &x[i]) != 1) return 2;
      const bool ok = ba_ldlt_solve(a.data(), x.data(), n, 0, 1, [] {});
      printf("%d", ok ? 1 : 0);
      for (int i = 0; i < n; ++i) printf(" %.17g", ok ? x[i] : 0.0);
      printf("\n");
    }
    return 0;
  }
  fprintf(stderr, "usage: ba_host lines | inv3 | ldlt  (input on stdin)\n");
  return 1;
}
