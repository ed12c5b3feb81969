// The arithmetic of K26 (place.hip; include/mi355x_match.h, "loop-closure retrieval"): the key a database column gets, the
// best-two pair a query row keeps and its order-independent merge, the vote predicate and the selection key.  Host and
// device; tests/native/place_host.cpp runs it without a GPU against tests/place_oracle.py.
//
// The key.  The header orders the columns of a query row by hamming << 16 | j, smallest first.  With
// hamming = pop(q) + pop(d_j) - 2 dot and pop(q) fixed for the row, that is the order of
//     g_j = dot - pop(d_j) / 2 + (1023 - j) / 2048,        LARGEST first:
// dot - pop / 2 is a multiple of 1/2 in [-256, 256], the index term a multiple of 2^-11 below 1/2, so g_j is a multiple of
// 2^-11 below 2^9 in magnitude -- 21 bits, exact in float32 -- and g orders first by hamming and then by the lower index.
// The MFMA accumulator STARTS at -pop(d_j) / 2 + (1023 - j) / 2048 and adds the 0 / 1 products (every partial sum is such
// a multiple, so exact), so the matrix core hands over the finished key and the epilogue is the two instructions of
// place_push per product.  An invalid or padding column starts at -PLACE_INVALID_HALF instead: whatever its dot product, it
// decodes to a distance above every descriptor length, which is how ABSENT is recognised.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int PLACE_MAX_K = 1024;                  // descriptors per frame; j < 1024 is what the index term relies on
constexpr float PLACE_INVALID_HALF = 4096.0f;      // "pop / 2" of an invalid column: distance >= 8192 - 2 * 512

__host__ __device__ __forceinline__ float place_col_start(int pop, int j, bool valid) {
  return (valid ? -0.5f * (float)pop : -PLACE_INVALID_HALF) + (float)(PLACE_MAX_K - 1 - j) * (1.0f / 2048.0f);
}

// (m1 >= m2): the two largest keys seen so far; empty = -inf.  Keys of different columns differ, so the result does not
// depend on the order of the pushes.
struct PlacePair {
  float m1, m2;
};

__host__ __device__ __forceinline__ float place_med3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fmed3f(a, b, c);
#else
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
#endif
}

__host__ __device__ __forceinline__ void place_push(PlacePair &p, float x) {
  p.m2 = place_med3(p.m1, p.m2, x);                // m1 >= m2: the median is the second largest of the three
  p.m1 = fmaxf(p.m1, x);
}

// the two largest of the union of two pairs over disjoint column sets
__host__ __device__ __forceinline__ PlacePair place_merge(PlacePair a, PlacePair b) {
  PlacePair r;
  r.m1 = fmaxf(a.m1, b.m1);
  r.m2 = fmaxf(fminf(a.m1, b.m1), fmaxf(a.m2, b.m2));
  return r;
}

// key -> (distance, index) for a query row of popcount pop_q; distance > num_bits: no such column (ABSENT, -1)
__host__ __device__ __forceinline__ void place_decode(float m, int pop_q, int num_bits, int *d, int *j) {
  if (!(m > -2.0f * PLACE_INVALID_HALF)) {         // -inf: nothing was pushed
    *d = num_bits + 1;
    *j = -1;
    return;
  }
  const int u = (int)(m * 2048.0f) + (8192 << 10);           // (2 dot - pop_d + 8192) << 10 | (1023 - j)
  const int dist = pop_q - ((u >> 10) - 8192);
  const bool have = dist <= num_bits;
  *d = have ? dist : num_bits + 1;
  *j = have ? (PLACE_MAX_K - 1) - (u & (PLACE_MAX_K - 1)) : -1;
}

// d2 = num_bits + 1 when there is no second column
__host__ __device__ __forceinline__ bool place_votes_for(int d1, int d2, int max_distance, float ratio) {
  return d1 <= max_distance && (float)d1 < ratio * (float)d2;
}

// selection: larger key first = (votes descending, index ascending); never 0 for an index below 2^31
__host__ __device__ __forceinline__ uint64_t place_select_key(int32_t votes, uint32_t index) {
  return ((uint64_t)((uint32_t)votes ^ 0x80000000u) << 32) | (uint32_t)~index;
}
__host__ __device__ __forceinline__ int32_t place_key_votes(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
__host__ __device__ __forceinline__ int32_t place_key_index(uint64_t key) { return (int32_t)~(uint32_t)key; }

}  // namespace
