// Host harness for the arithmetic of csrc/simgraph.hip (no GPU is touched: nothing is launched): one Sim(3) edge's residual,
// lines, blocks and gradient parts, a node's preconditioner solve, the state update and the map correction of
// csrc/simgraph_math.h, exactly the code the kernels run.  tests/test_simgraph_host.py compiles it with hipcc -- once more
// with the host sanitizers -- and compares its output with tests/simgraph_oracle.py.
//   simgraph_host edge < rows      one line "huber", then lines "si ri(9) ti(3) sj rj(9) tj(3) sz rz(9) tz(3) info(49)" ->
//                                  "e(7) chi2 w rho Ji(49) Jj(49) Hii(49) Hjj(49) Hij(49) gi(7) gj(7)" per row
//   simgraph_host update < rows    lines "R(9) t(3) s x(7)" (float64) -> "R(9) t(3) s" (%.17g)
//   simgraph_host correct < rows   lines "r_old(9) t_old(3) s r(9) t(3) x(3)" -> "r_out(9) t_out(3) x_out(3)"
//   simgraph_host precond < rows   lines "lambda D(49) r(7)" -> "ok z(7)" (zeros where the block fails the pivot rule)
// Built as plain C++ (no HIP header) it lacks the precond mode.
// %.9g prints a float32 so that reading it back returns the same bits.
#include "../../onnx_image_processing_amd/csrc/simgraph_math.h"

#include <cstdio>
#include <cstring>

static bool read_floats(float *v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%f", &v[i]) != 1) return false;
  return true;
}

static bool read_doubles(double *v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%lf", &v[i]) != 1) return false;
  return true;
}

static void print_floats(const float *v, int n) {
  for (int i = 0; i < n; ++i) printf(" %.9g", v[i]);
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "edge")) {
    float huber, in[88];
    if (scanf("%f", &huber) != 1) return 2;
    while (read_floats(in, 88)) {
      SgEdge o;
      float O[49], oe[7], w, rho, Ji[49], Jj[49], A[49], Hii[49], Hjj[49], Hij[49], gi[7], gj[7];
      sg_residual(in[0], in + 1, in + 10, in[13], in + 14, in + 23, in[26], in + 27, in + 36, o);
      sg_omega(in + 39, O);
      const float chi2 = sg_chi2(O, o.e, oe);
      pgo_rho(chi2, huber, &w, &rho);
      sg_lines(o, Ji, Jj);
      sg_omega_j(O, Jj, A);
      sg_jt_a(Jj, A, w, true, Hjj);
      sg_jt_a(Ji, A, w, false, Hij);
      sg_omega_j(O, Ji, A);
      sg_jt_a(Ji, A, w, true, Hii);
      sg_jt_v(Ji, oe, w, gi);
      sg_jt_v(Jj, oe, w, gj);
      print_floats(o.e, 7);
      printf(" %.9g %.9g %.9g", chi2, w, rho);
      print_floats(Ji, 49); print_floats(Jj, 49); print_floats(Hii, 49); print_floats(Hjj, 49); print_floats(Hij, 49);
      print_floats(gi, 7); print_floats(gj, 7);
      printf("\n");
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "update")) {
    double in[20];
    while (read_doubles(in, 20)) {
      sg_update(in, in + 13);
      for (int i = 0; i < 13; ++i) printf(" %.17g", in[i]);
      printf("\n");
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "correct")) {
    float in[28];
    while (read_floats(in, 28)) {
      float r_out[9], t_out[3], x_out[3];
      sg_correct_pose(in[12], in + 13, in + 22, r_out, t_out);
      sg_correct_point(in, in + 9, in[12], in + 13, in + 22, in + 25, x_out);
      print_floats(r_out, 9); print_floats(t_out, 3); print_floats(x_out, 3);
      printf("\n");
    }
    return 0;
  }
#if defined(__HIPCC__)                                      // the factorisation is ba_math.h's, which needs hipcc
  if (argc == 2 && !strcmp(argv[1], "precond")) {
    float in[57];
    while (read_floats(in, 57)) {
      float fac[28], z[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      double work[35];
      const bool ok = sg_block_factor(in + 1, in[0], fac, work);
      if (ok) sg_ldlt_apply(fac, in + 50, z);
      printf("%d", ok ? 1 : 0);
      print_floats(z, 7);
      printf("\n");
    }
    return 0;
  }
#endif
  fprintf(stderr, "usage: simgraph_host edge | update | correct | precond  (input on stdin)\n");
  return 1;
}
