// Host harness for the arithmetic of csrc/pgo.hip (no GPU is touched: nothing is launched): one edge's residual, lines,
// blocks and gradient parts, and a node's preconditioner solve of csrc/pgo_math.h, exactly the code the kernels run.
// tests/test_pgo_host.py compiles it with hipcc -- once more with the host sanitizers -- and compares its output with
// tests/pgo_oracle.py.
//   pgo_host edge < rows      one line "huber", then lines "ri(9) ti(3) rj(9) tj(3) rz(9) tz(3) info(36)" ->
//                             "e(6) chi2 w rho Ji(36) Jj(36) Hii(36) Hjj(36) Hij(36) gi(6) gj(6)" per row
//   pgo_host precond < rows   lines "lambda D(36) r(6)" -> "ok z(6)" (zeros where the block fails the pivot rule)
// Built as plain C++ (no HIP header) it has the edge mode alone.
// %.9g prints a float32 so that reading it back returns the same bits.
#include "../../onnx_image_processing_amd/csrc/pgo_math.h"

#include <cstdio>
#include <cstring>

static bool read_floats(float *v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%f", &v[i]) != 1) return false;
  return true;
}

static void print_floats(const float *v, int n) {
  for (int i = 0; i < n; ++i) printf(" %.9g", v[i]);
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "edge")) {
    float huber, in[72];
    if (scanf("%f", &huber) != 1) return 2;
    while (read_floats(in, 72)) {
      PgoEdge o;
      float O[36], oe[6], w, rho, Ji[36], Jj[36], A[36], Hii[36], Hjj[36], Hij[36], gi[6], gj[6];
      pgo_residual(in, in + 9, in + 12, in + 21, in + 24, in + 33, o);
      pgo_omega(in + 36, O);
      const float chi2 = pgo_chi2(O, o.e, oe);
      pgo_rho(chi2, huber, &w, &rho);
      pgo_lines(o, Ji, Jj);
      pgo_omega_j(O, Jj, A);
      pgo_jt_a(Jj, A, w, true, Hjj);
      pgo_jt_a(Ji, A, w, false, Hij);
      pgo_omega_j(O, Ji, A);
      pgo_jt_a(Ji, A, w, true, Hii);
      pgo_jt_v(Ji, oe, w, gi);
      pgo_jt_v(Jj, oe, w, gj);
      print_floats(o.e, 6);
      printf(" %.9g %.9g %.9g", chi2, w, rho);
      print_floats(Ji, 36); print_floats(Jj, 36); print_floats(Hii, 36); print_floats(Hjj, 36); print_floats(Hij, 36);
      print_floats(gi, 6); print_floats(gj, 6);
      printf("\n");
    }
    return 0;
  }
#if defined(__HIPCC__)                                      // the factorisation is ba_math.h's, which needs hipcc
  if (argc == 2 && !strcmp(argv[1], "precond")) {
    float in[43];
    while (read_floats(in, 43)) {
      float fac[21], z[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      double work[27];
      const bool ok = pgo_block_factor(in + 1, in[0], fac, work);
      if (ok) pgo_ldlt_apply(fac, in + 37, z);
      printf("%d", ok ? 1 : 0);
      print_floats(z, 6);
      printf("\n");
    }
    return 0;
  }
#endif
  fprintf(stderr, "usage: pgo_host edge | precond  (input on stdin)\n");
  return 1;
}
