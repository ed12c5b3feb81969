// Host harness for the host-callable pieces of csrc/pose.hip (no GPU is touched: nothing is launched): the sampler's
// hash and the minimal 8-point solver, exactly the code the kernels run per lane.  tests/test_pose_host.py compiles it
// with hipcc and compares its output with tests/pose_oracle.py.
//   pose_host draws                     prints "seed b h slot value" for a fixed grid of arguments
//   pose_host solve < samples           8 lines "x1 y1 x2 y2" per sample -> one line "ok e0 .. e8" per sample
//   pose_host pose < cases              "e0 .. e8 dist n" then n lines "x1 y1 x2 y2" -> "usable t(3) Ra(9) Rb(9) count(4)"
//   pose_host tri < points              "P1(12) P2(12) n" then n lines "x1 y1 x2 y2" -> n lines "finite X Y Z"
#include "../../onnx_image_processing_amd/csrc/pose.hip"

#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "draws")) {
    for (unsigned seed : {0u, 5u, 0xFFFFFFFFu})
      for (unsigned b : {0u, 2u, 65534u})
        for (unsigned h : {0u, 63u, 199u, 65535u})
          for (unsigned s = 0; s < 8; ++s) printf("%u %u %u %u %u\n", seed, b, h, s, po_draw(seed, b, h, s));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "solve")) {
    std::vector<float> work(81 * 64);                      // the lane's work area: word w at work[w * 64 + lane]
    float4 q[8];
    for (int sample = 0;; ++sample) {
      for (int s = 0; s < 8; ++s)
        if (scanf("%f %f %f %f", &q[s].x, &q[s].y, &q[s].z, &q[s].w) != 4) return 0;
      float e[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      const bool ok = po_solve_minimal(q, work.data() + sample % 64, e);
      printf("%d", ok ? 1 : 0);
      for (int i = 0; i < 9; ++i) printf(" %.9g", e[i]);
      printf("\n");
    }
  }
  if (argc == 2 && !strcmp(argv[1], "pose")) {
    float e[9], dist;
    int n;
    while (scanf("%f %f %f %f %f %f %f %f %f %f %d", e, e + 1, e + 2, e + 3, e + 4, e + 5, e + 6, e + 7, e + 8, &dist, &n) == 11) {
      float t[3], rot[2][3][3];
      const bool usable = po_decompose(e, t, rot);
      int count[4] = {0, 0, 0, 0};
      for (int i = 0; i < n; ++i) {
        float4 q;
        if (scanf("%f %f %f %f", &q.x, &q.y, &q.z, &q.w) != 4) return 2;
        for (int k = 0; k < 4; ++k) {                      // the kernel's candidate order
          const float sg = k < 2 ? 1.0f : -1.0f;
          const float tk[3] = {sg * t[0], sg * t[1], sg * t[2]};
          count[k] += (usable && po_in_front(rot[k & 1], tk, q, dist)) ? 1 : 0;
        }
      }
      printf("%d %.9g %.9g %.9g", usable ? 1 : 0, t[0], t[1], t[2]);
      for (int w = 0; w < 2; ++w)
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) printf(" %.9g", rot[w][r][c]);
      printf(" %d %d %d %d\n", count[0], count[1], count[2], count[3]);
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "tri")) {
    float p1[12], p2[12];
    int n;
    for (int i = 0; i < 12; ++i) if (scanf("%f", p1 + i) != 1) return 2;
    for (int i = 0; i < 12; ++i) if (scanf("%f", p2 + i) != 1) return 2;
    if (scanf("%d", &n) != 1) return 2;
    for (int i = 0; i < n; ++i) {
      float x1, y1, x2, y2, out[3];
      if (scanf("%f %f %f %f", &x1, &y1, &x2, &y2) != 4) return 2;
      const bool ok = po_triangulate_point(p1, p2, x1, y1, x2, y2, out);
      printf("%d %.9g %.9g %.9g\n", ok ? 1 : 0, out[0], out[1], out[2]);
    }
    return 0;
  }
  fprintf(stderr, "usage: pose_host draws | solve | pose | tri  (input on stdin)\n");
  return 1;
}
