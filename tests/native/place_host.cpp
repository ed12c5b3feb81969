// Host harness for the arithmetic of csrc/place.hip (no GPU is touched: nothing is launched): the column key, the best-two
// pair with its push and merge, the decode, the vote predicate and the selection key of csrc/place_math.h, exactly the code
// the kernels run.  tests/test_place_host.py compiles it with hipcc -- once more with the host sanitizers -- and compares
// its output with tests/place_oracle.py.
//   place_host merge < sets   repeated: a line "num_bits pop_q n" (n <= 7), then n lines "j pop_d dot valid".  Every ORDER
//                             of the n columns is pushed sequentially, and at every split point the two parts are pushed
//                             apart and merged; -> "d1 j1 d2 j2 orders mismatches": the decoded pair of the given order,
//                             the number of (order, split) forms tried and how many gave other bits
//   place_host vote < rows    lines "d1 d2 max_distance ratio" -> "0" / "1"
//   place_host key < rows     lines "votes index" -> "key votes index" (the key in decimal, and what it decodes to)
#include "../../onnx_image_processing_amd/csrc/place_math.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

static bool same(PlacePair a, PlacePair b) { return memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "merge")) {
    int num_bits, pop_q, n;
    while (scanf("%d %d %d", &num_bits, &pop_q, &n) == 3) {
      if (n < 0 || n > 7) return 2;
      std::vector<float> key((size_t)n);
      for (int c = 0; c < n; ++c) {
        int j, pop_d, dot, valid;
        if (scanf("%d %d %d %d", &j, &pop_d, &dot, &valid) != 4) return 2;
        if (j < 0 || j >= PLACE_MAX_K) return 2;
        key[c] = place_col_start(pop_d, j, valid != 0) + (float)dot;
      }
      const PlacePair empty = {-INFINITY, -INFINITY};
      PlacePair first = empty;
      for (int c = 0; c < n; ++c) place_push(first, key[c]);
      std::vector<int> order((size_t)n);
      for (int c = 0; c < n; ++c) order[c] = c;
      long forms = 0, bad = 0;
      do {
        for (int split = 0; split <= n; ++split) {
          PlacePair a = empty, b = empty;
          for (int c = 0; c < split; ++c) place_push(a, key[order[c]]);
          for (int c = split; c < n; ++c) place_push(b, key[order[c]]);
          ++forms;
          if (!same(place_merge(a, b), first) || !same(place_merge(b, a), first)) ++bad;
        }
      } while (std::next_permutation(order.begin(), order.end()));
      int d1, j1, d2, j2;
      place_decode(first.m1, pop_q, num_bits, &d1, &j1);
      place_decode(first.m2, pop_q, num_bits, &d2, &j2);
      printf("%d %d %d %d %ld %ld\n", d1, j1, d2, j2, forms, bad);
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "vote")) {
    int d1, d2, max_distance;
    float ratio;
    while (scanf("%d %d %d %f", &d1, &d2, &max_distance, &ratio) == 4)
      printf("%d\n", place_votes_for(d1, d2, max_distance, ratio) ? 1 : 0);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "key")) {
    long long votes, index;
    while (scanf("%lld %lld", &votes, &index) == 2) {
      const uint64_t k = place_select_key((int32_t)votes, (uint32_t)index);
      printf("%llu %d %d\n", (unsigned long long)k, place_key_votes(k), place_key_index(k));
    }
    return 0;
  }
  fprintf(stderr, "usage: place_host merge | vote | key  (input on stdin)\n");
  return 1;
}
