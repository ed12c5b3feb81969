// Host harness for the arithmetic of csrc/icp.hip (plain C++: csrc/icp_math.h needs no HIP header and nothing is launched):
// the vertex and normal of the surfel maps, one pixel's row of the point-to-plane system, the LDL^T solve and the Rodrigues
// update, exactly the code the kernels run.  tests/test_icp_host.py compiles it and compares its output with
// tests/icp_oracle.py.  Every mode reads records from stdin until it ends and prints one line per record (%.9g floats,
// %.17g doubles):
//   icp_host vertex   d x y kinv(6) z_scale min max                                   -> ok vx vy vz
//   icp_host normal   max_jump c(3) l(3) r(3) u(3) d(3)                               -> ok nx ny nz
//   icp_host row      R(9) t(3) v1(3) n1(3) v2(3) n2(3) fx fy cx cy w h thr2 cos_thr  -> ok px py J(6) r   (ok: 0 rejected by
//                                                                        the projection, 1 by the gates, 2 survivor)
//   icp_host solve    min_count sums(29)                                              -> ok ratio x(6)
//   icp_host exp      omega(3)                                                        -> E(9)
//   icp_host update   pose(12) x(6)                                                   -> pose(12)
#include "../../onnx_image_processing_amd/csrc/icp_math.h"

#include <cstdio>
#include <cstring>

template <typename T>
static bool read_n(T *p, int n, const char *fmt) {
  for (int i = 0; i < n; ++i)
    if (scanf(fmt, &p[i]) != 1) return false;
  return true;
}
static bool rf(float *p, int n) { return read_n(p, n, "%f"); }
static bool rd(double *p, int n) { return read_n(p, n, "%lf"); }

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: icp_host vertex | normal | row | solve | exp | update  (records on stdin)\n");
    return 1;
  }
  const char *mode = argv[1];
  if (!strcmp(mode, "vertex")) {
    float a[12], v[3];
    while (rf(a, 12)) {
      const bool ok = icp_vertex(a[0], a[1], a[2], a + 3, a[9], a[10], a[11], v);
      printf("%d %.9g %.9g %.9g\n", ok ? 1 : 0, v[0], v[1], v[2]);
    }
    return 0;
  }
  if (!strcmp(mode, "normal")) {
    float a[16], n[3];
    while (rf(a, 16)) {
      const bool ok = icp_normal(a + 1, a + 4, a + 7, a + 10, a + 13, a[0], n);
      printf("%d %.9g %.9g %.9g\n", ok ? 1 : 0, n[0], n[1], n[2]);
    }
    return 0;
  }
  if (!strcmp(mode, "row")) {
    float a[32];
    while (rf(a, 32)) {
      const float *R = a, *t = a + 9, *v1 = a + 12, *n1 = a + 15, *v2 = a + 18, *n2 = a + 21;
      float q[3], rn[3], px, py, J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, r = 0.0f;
      icp_rotate(R, v1, q);
      for (int j = 0; j < 3; ++j) q[j] += t[j];
      icp_rotate(R, n1, rn);
      int ok = icp_project(q, a[24], a[25], a[26], a[27], (int)a[28], (int)a[29], &px, &py) ? 1 : 0;
      if (ok) ok += icp_row(q, rn, v2, n2, a[30], a[31], J, &r) ? 1 : 0;
      printf("%d %.9g %.9g", ok, px, py);
      for (int j = 0; j < 6; ++j) printf(" %.9g", J[j]);
      printf(" %.9g\n", r);
    }
    return 0;
  }
  if (!strcmp(mode, "solve")) {
    double a[30], x[6], ratio;
    while (rd(a, 30)) {
      const bool ok = icp_solve(a + 1, (int)a[0], x, &ratio);
      printf("%d %.17g", ok ? 1 : 0, ratio);
      for (int j = 0; j < 6; ++j) printf(" %.17g", x[j]);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(mode, "exp")) {
    double w[3], e[9];
    while (rd(w, 3)) {
      icp_exp(w, e);
      for (int j = 0; j < 9; ++j) printf("%s%.17g", j ? " " : "", e[j]);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(mode, "update")) {
    double a[18];
    while (rd(a, 18)) {
      icp_update_pose(a, a + 12);
      for (int j = 0; j < 12; ++j) printf("%s%.17g", j ? " " : "", a[j]);
      printf("\n");
    }
    return 0;
  }
  fprintf(stderr, "unknown mode %s\n", mode);
  return 1;
}
