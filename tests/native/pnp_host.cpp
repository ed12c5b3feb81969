// Host harness for the arithmetic of csrc/pnp.hip (no GPU is touched: nothing is launched): the shared sampler with four
// slots (csrc/pose_sampler.h) and the P3P solver, reprojection score and Jacobian lines of csrc/pnp_math.h, exactly the
// code the kernels run.  tests/test_pnp_host.py compiles it with hipcc and compares its output with tests/pnp_oracle.py.
//   pnp_host ranks                 prints "seed b h nv r0 r1 r2 r3" for nv in (4, 5, 64, 97), 50 hypotheses each
//   pnp_host solve < samples       4 lines "X Y Z u v" per sample -> "S ok rt(12)" (the chosen pose), then for c = 0 .. 3
//                                  "C c ok l(3) rt(12) d2" (every candidate; d2: its distance on the fourth row)
//   pnp_host score < rows          one line rt(12), then lines "X Y Z u v" -> one d2 per row
//   pnp_host lines < rows          one line rt(12), then lines "X Y Z u v" -> "ok ju(6) jv(6) ru rv" per row
// %.9g prints a float32 so that reading it back returns the same bits.
#include "../../onnx_image_processing_amd/csrc/pose_sampler.h"
#include "../../onnx_image_processing_amd/csrc/pnp_math.h"

#include <cstdio>
#include <cstring>

static bool read_row(PnpRow &q) { return scanf("%f %f %f %f %f", &q.X[0], &q.X[1], &q.X[2], &q.u, &q.v) == 5; }

static bool read_rt(float *rt) {
  for (int i = 0; i < 12; ++i)
    if (scanf("%f", &rt[i]) != 1) return false;
  return true;
}

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
    PnpRow q[4];
    for (;;) {
      for (int s = 0; s < 4; ++s)
        if (!read_row(q[s])) return 0;
      float rt[12];
      const bool ok = pnp_solve_minimal(q, rt);
      printf("S %d", ok ? 1 : 0);
      for (int i = 0; i < 12; ++i) printf(" %.9g", ok ? rt[i] : 0.0f);
      printf("\n");
      PnpSetup S;
      const bool sok = pnp_setup(q, S);
      for (int c = 0; c < 4; ++c) {
        float l[3] = {0.0f, 0.0f, 0.0f}, cand[12];
        const bool cok = sok && pnp_candidate(q, S, c, l, cand);
        printf("C %d %d", c, cok ? 1 : 0);
        for (int i = 0; i < 3; ++i) printf(" %.9g", cok ? l[i] : 0.0f);
        for (int i = 0; i < 12; ++i) printf(" %.9g", cok ? cand[i] : 0.0f);
        printf(" %.9g\n", cok ? pnp_dist2(cand, q[3]) : 0.0f);
      }
    }
  }
  if (argc == 2 && (!strcmp(argv[1], "score") || !strcmp(argv[1], "lines"))) {
    const bool lines = !strcmp(argv[1], "lines");
    float rt[12];
    if (!read_rt(rt)) return 2;
    PnpRow q;
    while (read_row(q)) {
      if (!lines) {
        printf("%.9g\n", pnp_dist2(rt, q));
        continue;
      }
      float ju[6], jv[6], ru, rv;
      const bool ok = pnp_lines(rt, q, ju, jv, &ru, &rv);
      printf("%d", ok ? 1 : 0);
      for (int i = 0; i < 6; ++i) printf(" %.9g", ju[i]);
      for (int i = 0; i < 6; ++i) printf(" %.9g", jv[i]);
      printf(" %.9g %.9g\n", ru, rv);
    }
    return 0;
  }
  fprintf(stderr, "usage: pnp_host ranks | solve | score | lines  (input on stdin)\n");
  return 1;
}
