// Host harness for the arithmetic of csrc/localmap.hip (no GPU is touched: nothing is launched): csrc/localmap_math.h's
// projection, window test, keys, best-two pair, merge, candidate test, claims and median, exactly the code the kernels run, in
// the kernels' order of work: the keypoints of a landmark are dealt to 64 "lanes" whose pairs are merged in butterfly order, and
// a slot's distance table is ranked row by row.  tests/test_localmap_host.py compiles it with hipcc, as plain C++ and once more
// with the host sanitizers, and compares its output with tests/localmap_oracle.py.
//   localmap_host match < items   per item "L K W height width min_depth max_depth radius max_distance ratio", "r(9) t(3) cam(4)",
//                                 L lines "valid x y z words(W)", K lines "valid ky kx words(W)"
//                                 ->  L lines "state lm_kp lm_distance d2 proj(2) match_keypoints(2)" (floats as their bit
//                                 patterns), then one line of K kp_lm and one line of 5 counts
//   localmap_host desc < windows  per window "F K L W", F * K lines "words(W)", F lines of L track_kp
//                                 ->  L lines "rep_frame rep_median words(W)"
// %.9g prints a float32 so that reading it back returns the same bits.
#include "../../onnx_image_processing_amd/csrc/localmap_math.h"

#include <cstdio>
#include <cstring>
#include <vector>

static unsigned bits_of(float x) {
  unsigned u;
  memcpy(&u, &x, 4);
  return u;
}

static int run_match() {
  int L, K, W, height, width, max_distance;
  float min_depth, max_depth, radius, ratio;
  while (scanf("%d %d %d %d %d %f %f %f %d %f", &L, &K, &W, &height, &width, &min_depth, &max_depth, &radius, &max_distance, &ratio) == 10) {
    if (L < 1 || L > 2048 || K < 1 || K > 1024 || (W != 8 && W != 16)) return 2;
    const int num_bits = 32 * W;
    float pose[16];
    for (int i = 0; i < 16; ++i)
      if (scanf("%f", &pose[i]) != 1) return 2;
    const float *R = pose, *T = pose + 9, *cam = pose + 12;
    std::vector<float> X((size_t)L * 3), kp((size_t)K * 2);
    std::vector<uint32_t> rep((size_t)L * W), kb((size_t)K * W);
    std::vector<int> pv(L), kv(K);
    for (int l = 0; l < L; ++l) {
      if (scanf("%d %f %f %f", &pv[l], &X[3 * l], &X[3 * l + 1], &X[3 * l + 2]) != 4) return 2;
      for (int w = 0; w < W; ++w)
        if (scanf("%u", &rep[(size_t)l * W + w]) != 1) return 2;
    }
    for (int j = 0; j < K; ++j) {
      if (scanf("%d %f %f", &kv[j], &kp[2 * j], &kp[2 * j + 1]) != 3) return 2;
      for (int w = 0; w < W; ++w)
        if (scanf("%u", &kb[(size_t)j * W + w]) != 1) return 2;
    }
    const double r2 = (double)radius * (double)radius;
    std::vector<int> claim(K, LM_NO_CLAIM), state(L), d1s(L), d2s(L), j1s(L);
    std::vector<LmProj> proj(L);
    for (int l = 0; l < L; ++l) {
      proj[l] = lm_project(R, T, cam, &X[3 * l], pv[l] != 0, height, width, min_depth, max_depth);
      d1s[l] = d2s[l] = num_bits + 1;
      j1s[l] = -1;
      state[l] = 0;
      if (!proj[l].in_view) continue;
      LmPair lanes[64], next[64];
      for (int i = 0; i < 64; ++i) lanes[i].k1 = lanes[i].k2 = LM_EMPTY;
      for (int j = 0; j < K; ++j) {
        if (!kv[j] || !lm_in_window(kp[2 * j], kp[2 * j + 1], proj[l].u, proj[l].v, r2)) continue;
        int h = 0;
        for (int w = 0; w < W; ++w) h += lm_popcount(rep[(size_t)l * W + w] ^ kb[(size_t)j * W + w]);
        lm_push(lanes[j & 63], lm_key(h, j));
      }
      for (int o = 32; o > 0; o >>= 1) {
        for (int i = 0; i < 64; ++i) next[i] = lm_merge(lanes[i], lanes[i ^ o]);
        memcpy(lanes, next, sizeof(lanes));
      }
      lm_decode(lanes[0], num_bits, &d1s[l], &j1s[l], &d2s[l]);
      if (j1s[l] < 0) {
        state[l] = 1;
      } else if (lm_candidate(d1s[l], d2s[l], max_distance, ratio)) {
        state[l] = 4;
        const int key = lm_claim_key(d1s[l], l);
        if (key < claim[j1s[l]]) claim[j1s[l]] = key;
      } else {
        state[l] = 2;
      }
    }
    int counts[5] = {0, 0, 0, 0, 0};
    for (int l = 0; l < L; ++l) {
      if (state[l] == 4 && lm_claim_landmark(claim[j1s[l]]) != l) state[l] = 3;
      const bool kept = state[l] == 4;
      ++counts[state[l]];
      printf("%d %d %d %d %u %u %u %u\n", state[l], kept ? j1s[l] : -1, state[l] >= 2 ? d1s[l] : num_bits + 1, d2s[l],
             bits_of(proj[l].in_view ? (float)proj[l].v : -1.0f), bits_of(proj[l].in_view ? (float)proj[l].u : -1.0f),
             bits_of(kept ? kp[2 * j1s[l]] : -1.0f), bits_of(kept ? kp[2 * j1s[l] + 1] : -1.0f));
    }
    for (int j = 0; j < K; ++j) printf("%d ", lm_claim_landmark(claim[j]));
    printf("\n%d %d %d %d %d\n", counts[0], counts[1], counts[2], counts[3], counts[4]);
  }
  return 0;
}

static int run_desc() {
  int F, K, L, W;
  while (scanf("%d %d %d %d", &F, &K, &L, &W) == 4) {
    if (F < 1 || F > LM_MAX_FRAMES || K < 1 || K > 1024 || L < 1 || L > 2048 || (W != 8 && W != 16)) return 2;
    std::vector<uint32_t> bits((size_t)F * K * W);
    std::vector<int> tk((size_t)F * L);
    for (size_t i = 0; i < bits.size(); ++i)
      if (scanf("%u", &bits[i]) != 1) return 2;
    for (size_t i = 0; i < tk.size(); ++i)
      if (scanf("%d", &tk[i]) != 1) return 2;
    for (int l = 0; l < L; ++l) {
      unsigned views = 0;
      for (int f = 0; f < F; ++f)
        if (tk[(size_t)f * L + l] >= 0 && tk[(size_t)f * L + l] < K) views |= 1u << f;
      const int n = lm_popcount(views);
      int best = 0x7fffffff;
      for (int a = 0; a < F; ++a) {
        if (!((views >> a) & 1u)) continue;
        int d[LM_MAX_FRAMES];
        for (int b = 0; b < LM_MAX_FRAMES; ++b) {
          d[b] = 0;
          if (!((views >> b) & 1u)) continue;                 // a row's entries outside the views are never read
          for (int w = 0; w < W; ++w)
            d[b] += lm_popcount(bits[((size_t)a * K + tk[(size_t)a * L + l]) * W + w] ^ bits[((size_t)b * K + tk[(size_t)b * L + l]) * W + w]);
        }
        const int key = lm_rep_key(lm_median(d, views, n), a);
        best = key < best ? key : best;
      }
      const int frame = n ? (best & 0xff) : -1;
      printf("%d %d", frame, n ? best >> 8 : 32 * W + 1);
      for (int w = 0; w < W; ++w) printf(" %u", n ? bits[((size_t)frame * K + tk[(size_t)frame * L + l]) * W + w] : 0u);
      printf("\n");
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "match")) return run_match();
  if (argc == 2 && !strcmp(argv[1], "desc")) return run_desc();
  fprintf(stderr, "usage: localmap_host match | desc  (input on stdin)\n");
  return 1;
}
