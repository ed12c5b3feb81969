// The counter-based sampler of the RANSAC kernels (include/mi355x_match.h, "Sampling"), called by ransac_wave.h's
// hypothesis kernel for K15 (pose.hip: 8 ranks per hypothesis), K17 (rigid.hip: 3 ranks) and K23 (pnp.hip: 4 ranks, three
// rows to solve and one to pick the candidate).  Integer arithmetic only, callable on the host as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__host__ __device__ inline uint32_t po_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t po_draw(uint32_t seed, uint32_t b, uint32_t h, uint32_t slot) {
  return po_mix(po_mix(po_mix(seed + 0x9E3779B9u) + b) + (h * 8u + slot));
}

// K distinct ranks among nv >= K rows, slots 0 .. K-1 in turn: r = draw mod (nv - s), then every rank already taken, in
// ascending order, at or below r moves r up by one
template <int K>
__host__ __device__ __forceinline__ void po_sample_ranks(uint32_t seed, uint32_t b, uint32_t h, int nv, int *pick) {
  int sorted[K];
#pragma unroll
  for (int s = 0; s < K; ++s) sorted[s] = 0x7fffffff;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    int r = (int)(po_draw(seed, b, h, (uint32_t)s) % (uint32_t)(nv - s));
#pragma unroll
    for (int j = 0; j < K; ++j) r += (j < s && r >= sorted[j]) ? 1 : 0;      // skip the ranks already taken (ascending)
    pick[s] = r;
    int x = r;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int lo = sorted[j] < x ? sorted[j] : x, hi = sorted[j] < x ? x : sorted[j];
      sorted[j] = lo;
      x = hi;
    }
  }
}

}  // namespace
