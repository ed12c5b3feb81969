// Host harness for the arithmetic of csrc/sim3.hip (no GPU is touched: nothing is launched): the shared sampler
// (csrc/pose_sampler.h), K17's Horn solve (csrc/rigid_math.h) and the scale, range test and scores of csrc/sim3_math.h,
// exactly the code the kernels run.  tests/test_sim3_host.py compiles it with hipcc and compares its output with
// tests/sim3_oracle.py.
//   sim3_host solve < samples           3 lines "ax ay az bx by bz" per sample -> "ok R(9) t(3) s same" per sample; same = 1
//                                       when R is rg_solve_minimal's, bit for bit, or both refuse on K17's grounds
//   sim3_host fit < sets                "n" then n rows -> "ok R(9) t(3) s" (the refit's passes, serial sums)
//   sim3_host hyp METRIC THR SEED B H < set    "n" then n rows -> H lines "ok cost count R(9) t(3) s": the hypothesis kernel's
//                                       lane, hypothesis by hypothesis (sample, solve, serial score in index order)
//   sim3_host rmse METRIC THR < model+set      13 floats (R, t, s), "n", n rows -> "count rmse": the selection kernel's inlier
//                                       count and root-mean-square d^2 (64 strided partial sums, then a tree)
#include "../../onnx_image_processing_amd/csrc/pose_sampler.h"
#include "../../onnx_image_processing_amd/csrc/sim3_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool read_row(RgRow &q) {
  return scanf("%f %f %f %f %f %f", &q.a[0], &q.a[1], &q.a[2], &q.b[0], &q.b[1], &q.b[2]) == 6;
}

static void print_model(bool ok, const float *m) {
  printf("%d", ok ? 1 : 0);
  for (int i = 0; i < S3_STORED; ++i) printf(" %.9g", ok ? m[i] : 0.0f);
}

static bool read_set(std::vector<RgRow> &rows) {
  int n;
  if (scanf("%d", &n) != 1) return false;
  if (n < 0 || n > 4096) exit(2);
  rows.resize((size_t)n);
  for (int i = 0; i < n; ++i)
    if (!read_row(rows[(size_t)i])) exit(2);
  return true;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "solve")) {
    RgRow q[3];
    for (;;) {
      for (int s = 0; s < 3; ++s)
        if (!read_row(q[s])) return 0;
      float m[S3_FLOATS], rt[12];
      const bool ok = s3_solve_minimal(q, m);
      const bool rigid_ok = rg_solve_minimal(q, rt);
      bool same = ok ? (rigid_ok && !memcmp(m, rt, 9 * sizeof(float))) : true;
      print_model(ok, m);
      printf(" %d\n", same ? 1 : 0);
    }
  }
  if (argc == 2 && !strcmp(argv[1], "fit")) {
    std::vector<RgRow> rows;
    while (read_set(rows)) {
      const int n = (int)rows.size();
      float m[S3_FLOATS];
      for (int i = 0; i < S3_FLOATS; ++i) m[i] = 0.0f;
      bool ok = n >= 3;
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
          rg_rotation_from_scatter(s, m);
          float num = 0.0f;
          for (const RgRow &q : rows) {
            const float a[3] = {q.a[0] - ca[0], q.a[1] - ca[1], q.a[2] - ca[2]}, b[3] = {q.b[0] - cb[0], q.b[1] - cb[1], q.b[2] - cb[2]};
            num += s3_num_term(m, a, b);
          }
          ok = s3_finish(num, (acc[9] + acc[12]) + acc[14], ca, cb, m);
        }
      }
      print_model(ok, m);
      printf("\n");
    }
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "hyp")) {
    const int metric = atoi(argv[2]);
    const float thr = strtof(argv[3], nullptr), thr2 = thr * thr;
    const unsigned seed = (unsigned)strtoul(argv[4], nullptr, 10), b = (unsigned)strtoul(argv[5], nullptr, 10);
    const int H = atoi(argv[6]);
    std::vector<RgRow> rows;
    if (!read_set(rows) || (metric != MI_SIM3_POINT && metric != MI_SIM3_REPROJ) || H < 1) return 2;
    const int nv = (int)rows.size();
    for (int h = 0; h < H; ++h) {
      float m[S3_FLOATS];
      bool ok = nv >= 3;
      if (ok) {
        int pick[3];
        po_sample_ranks<3>(seed, b, (unsigned)h, nv, pick);
        const RgRow q[3] = {rows[(size_t)pick[0]], rows[(size_t)pick[1]], rows[(size_t)pick[2]]};
        ok = s3_solve_minimal(q, m);
      }
      float cost = INFINITY;
      int count = 0;
      if (ok) {
        cost = 0.0f;
        for (const RgRow &q : rows) {
          const float d2 = metric == MI_SIM3_REPROJ ? s3_dist2<MI_SIM3_REPROJ>(m, q) : s3_dist2<MI_SIM3_POINT>(m, q);
          count += d2 <= thr2 ? 1 : 0;
          cost += fminf(d2, thr2);
        }
        if (!(cost < INFINITY)) { ok = false; cost = INFINITY; count = 0; }
      }
      printf("%d %.9g %d", ok ? 1 : 0, cost, count);
      for (int i = 0; i < S3_STORED; ++i) printf(" %.9g", ok ? m[i] : 0.0f);
      printf("\n");
    }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "rmse")) {
    const int metric = atoi(argv[2]);
    const float thr = strtof(argv[3], nullptr), thr2 = thr * thr;
    float m[S3_FLOATS];
    for (int i = 0; i < S3_STORED; ++i)
      if (scanf("%f", &m[i]) != 1) return 2;
    m[13] = 1.0f / m[12];
    std::vector<RgRow> rows;
    if (!read_set(rows) || (metric != MI_SIM3_POINT && metric != MI_SIM3_REPROJ)) return 2;
    float part[64];
    for (int l = 0; l < 64; ++l) part[l] = 0.0f;
    int count = 0;
    for (size_t i = 0; i < rows.size(); ++i) {
      const float d2 = metric == MI_SIM3_REPROJ ? s3_dist2<MI_SIM3_REPROJ>(m, rows[i]) : s3_dist2<MI_SIM3_POINT>(m, rows[i]);
      if (d2 <= thr2) { ++count; part[i & 63] += d2; }
    }
    for (int o = 1; o < 64; o <<= 1)
      for (int l = 0; l < 64; l += 2 * o) part[l] += part[l + o];
    printf("%d %.9g\n", count, count ? sqrtf(part[0] / (float)count) : 0.0f);
    return 0;
  }
  fprintf(stderr, "usage: sim3_host solve | fit | hyp METRIC THR SEED B H | rmse METRIC THR  (input on stdin)\n");
  return 1;
}
