// Host harness for the arithmetic of csrc/tracks.hip's triangulation (no GPU is touched: nothing is launched):
// csrc/tracks_math.h's trk_triangulate, exactly the code the kernel runs.  tests/test_tracks_host.py compiles it with hipcc,
// as plain C++ and once more with the host sanitizers, and compares its output with tests/tracks_oracle.py.
//   tracks_host tri < windows    per window one line "F L min_views max_e2 max_cos", F lines "r(9) t(3)", then L lines of F
//                                triples "vis x y"  ->  per landmark "ok usable front seen X(3) e2max cos_par"
// The arrays are laid out as the kernel sees them: obs (F, L, 2), vis (F, L), a landmark's frames L entries apart.
// %.9g prints a float32 so that reading it back returns the same bits; %.17g does the same for a float64.
#include "../../onnx_image_processing_amd/csrc/tracks_math.h"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "tri")) {
    int F, L, min_views;
    float max_e2, max_cos;
    while (scanf("%d %d %d %f %f", &F, &L, &min_views, &max_e2, &max_cos) == 5) {
      if (F < 1 || F > 16 || L < 1 || L > 4096) return 2;
      std::vector<float> r((size_t)F * 9), t((size_t)F * 3), obs((size_t)F * L * 2);
      std::vector<uint8_t> vis((size_t)F * L);
      for (int f = 0; f < F; ++f) {
        for (int k = 0; k < 9; ++k)
          if (scanf("%f", &r[f * 9 + k]) != 1) return 2;
        for (int k = 0; k < 3; ++k)
          if (scanf("%f", &t[f * 3 + k]) != 1) return 2;
      }
      for (int l = 0; l < L; ++l)
        for (int f = 0; f < F; ++f) {
          int v;
          const size_t at = (size_t)f * L + l;
          if (scanf("%d %f %f", &v, &obs[2 * at], &obs[2 * at + 1]) != 3) return 2;
          vis[at] = (uint8_t)v;
        }
      for (int l = 0; l < L; ++l) {
        TrkPoint o;
        trk_triangulate(r.data(), t.data(), obs.data() + 2 * l, (size_t)L * 2, vis.data() + l, (size_t)L, F, min_views, max_e2, max_cos, o);
        printf("%d %d %d %d %.17g %.17g %.17g %.17g %.17g\n", o.ok ? 1 : 0, o.usable ? 1 : 0, o.front ? 1 : 0, o.seen, o.X[0], o.X[1],
               o.X[2], o.e2max, o.cos_par);
      }
    }
    return 0;
  }
  fprintf(stderr, "usage: tracks_host tri  (input on stdin)\n");
  return 1;
}
