// The arithmetic of K35 (include/mi355x_match_filter.h: "Validity and adjacency", "Components", "Speckle", "Median") shared by
// csrc/filter.hip and a host compile (tests/native/filter_host.cpp): the validity and join rules, the union-find over a small
// memory policy (the kernels run it on LDS and on global memory with atomics, the host program sequentially on an array), the
// rules that say which unions are implied by a neighbour's, the float key and the median's sorting network.  Nothing here
// launches or reads a device.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi355x_match_filter.h"

#define FT_HD __host__ __device__ __forceinline__

#define FT_TILE_W MI_FILTER_TILE_W
#define FT_TILE_H MI_FILTER_TILE_H
#define FT_TILE (FT_TILE_W * FT_TILE_H)

// "Validity and adjacency": the rule of one call, for float32 and for uint8 values
struct FtRule {
  float min_valid, max_diff;
  int min_valid_u8, max_diff_u8;
};
FT_HD bool ft_valid(float v, const FtRule &r) { return v >= r.min_valid; }
FT_HD bool ft_valid(uint8_t v, const FtRule &r) { return (int)v >= r.min_valid_u8; }
// both pixels valid is the caller's to know
FT_HD bool ft_near(float a, float b, const FtRule &r) { return fabsf(a - b) <= r.max_diff; }
FT_HD bool ft_near(uint8_t a, uint8_t b, const FtRule &r) {
  const int d = (int)a - (int)b;
  return (d < 0 ? -d : d) <= r.max_diff_u8;
}
template <typename T>
FT_HD bool ft_joined(T a, T b, const FtRule &r) {
  return ft_valid(a, r) && ft_valid(b, r) && ft_near(a, b, r);
}

// ---- union-find over a memory policy M: int load(int i), void store(int i, int v), int atomic_min(int i, int v) (returns the
// old value).  parent[i] <= i always, parent[i] == i marks a root, and a parent is only ever replaced by a SMALLER element of the
// same set: a chain strictly decreases, so every loop below ends after at most `cap` = h * w trips by itself; the explicit cap
// is the belt to those braces -- at the cap a loop gives up and leaves a wrong answer, which a test catches, instead of spinning.
// A load that returns an older parent (another thread's union in flight) still returns an element of the same set.
template <typename M>
FT_HD int ft_find(M &m, int i, int cap) {
  for (int trip = 0; trip < cap; ++trip) {
    const int p = m.load(i);
    if (p == i) break;
    i = p;
  }
  return i;
}

// join the sets of a and b under the smaller root.  A retry happens only after atomic_min returned something smaller than the
// element it was applied to (that element was no root any more): the pair (old parent, lo) is then what is left to join.
template <typename M>
FT_HD void ft_unite(M &m, int a, int b, int cap) {
  for (int trip = 0; trip < cap; ++trip) {
    a = ft_find(m, a, cap);
    b = ft_find(m, b, cap);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = m.atomic_min(hi, lo);
    if (old == hi) return;                                                // hi was a root and now hangs under lo
    a = old;
    b = lo;
  }
}

// the sequential memory of the host program
struct FtHostMem {
  int *p;
  int load(int i) const { return p[i]; }
  void store(int i, int v) { p[i] = v; }
  int atomic_min(int i, int v) {
    const int old = p[i];
    if (v < old) p[i] = v;
    return old;
  }
};

// a row of up to 64 pixels: bit i of `joined_left` says pixel i is joined to pixel i - 1 (bit 0 is 0).  The first pixel of the
// run that holds pixel `lane`.
FT_HD int ft_run_start(uint64_t joined_left, int lane) {
  const uint64_t starts = ~joined_left & ((2ull << lane) - 1ull);         // bit 0 is always set
  return 63 - __builtin_clzll(starts);
}

// Two pixels A, B joined across a line (two rows of a tile, or a tile border) and the pair A', B' before them along that line:
// the union of A and B is implied by that of A' and B' when A ~ A', B ~ B' and A' ~ B' are joined and A ~ A', B ~ B' lie inside
// one tile each (those unions are made by the tile's own labelling, never skipped).  A constant plane then makes one union per
// row and per border segment, not one per pixel on the same two roots.
FT_HD bool ft_implied(bool a_joined_before, bool b_joined_before, bool before_joined_across) {
  return a_joined_before && b_joined_before && before_joined_across;
}

// the index in the frame of the local element `e` (row e / 64, column e % 64) of tile (ty, tx)
FT_HD int ft_global_index(int e, int ty, int tx, int w) { return (ty * FT_TILE_H + e / FT_TILE_W) * w + tx * FT_TILE_W + e % FT_TILE_W; }

// the border pair `k` of a frame (see ft_border_pairs): pixel a, pixel b = its right or lower neighbour across a tile border,
// and whether the pair before it along the border (one row up, or one column left) lies in the same two tiles
FT_HD int ft_border_pairs(int h, int w) { return ((w - 1) / FT_TILE_W) * h + ((h - 1) / FT_TILE_H) * w; }
FT_HD void ft_border_pair(int k, int h, int w, int *a, int *b, int *step, bool *same_tiles) {
  const int vertical = ((w - 1) / FT_TILE_W) * h;
  if (k < vertical) {
    const int x = (k / h + 1) * FT_TILE_W, y = k % h;
    *a = y * w + x - 1;
    *b = y * w + x;
    *step = w;
    *same_tiles = y % FT_TILE_H != 0;
  } else {
    k -= vertical;
    const int y = (k / w + 1) * FT_TILE_H, x = k % w;
    *a = (y - 1) * w + x;
    *b = y * w + x;
    *step = 1;
    *same_tiles = x % FT_TILE_W != 0;
  }
}
template <typename T>
FT_HD bool ft_border_union_wanted(const T *g, int a, int b, int step, bool same_tiles, const FtRule &r) {
  if (!ft_joined(g[a], g[b], r)) return false;
  return !(same_tiles && ft_implied(ft_joined(g[a - step], g[a], r), ft_joined(g[b - step], g[b], r), ft_joined(g[a - step], g[b - step], r)));
}

// "Speckle"
FT_HD bool ft_speckle_keeps(bool valid, int size, int max_size) { return valid && size > max_size; }

// ---- "Median" -------------------------------------------------------------------------------------------------------------------------
FT_HD uint32_t ft_bits(float v) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = v;
  return c.u;
}
FT_HD float ft_float(uint32_t u) {
  union {
    float f;
    uint32_t u;
  } c;
  c.u = u;
  return c.f;
}
// the monotone key of a float and its inverse; 0xFFFFFFFF is the key of a NaN only, which is never valid
FT_HD uint32_t ft_key(float v) {
  const uint32_t u = ft_bits(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FT_HD float ft_unkey(uint32_t k) { return ft_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
FT_HD int ft_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// pixel (y, x) of one frame g (h x w): K x K taps with a replicate border, invalid taps as 0xFFFFFFFF, an odd-even transposition
// network over the K K keys (every index a constant once unrolled: registers only), then the key of rank (n - 1) / 2
template <int K>
FT_HD float ft_median(const float *g, int h, int w, int y, int x, float min_valid, float invalid_value) {
  constexpr int N = K * K, R = K / 2;
  if (!(g[(size_t)y * w + x] >= min_valid)) return invalid_value;
  uint32_t a[N];
  int n = 0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
    const float *row = g + (size_t)ft_clamp(y + dy, h - 1) * w;
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const float v = row[ft_clamp(x + dx, w - 1)];
      const bool ok = v >= min_valid;
      a[(dy + R) * K + dx + R] = ok ? ft_key(v) : 0xffffffffu;
      n += ok ? 1 : 0;
    }
  }
#pragma unroll
  for (int round = 0; round < N; ++round) {
#pragma unroll
    for (int i = round & 1; i + 1 < N; i += 2) {
      const uint32_t lo = a[i] < a[i + 1] ? a[i] : a[i + 1], hi = a[i] < a[i + 1] ? a[i + 1] : a[i];
      a[i] = lo;
      a[i + 1] = hi;
    }
  }
  const int rank = (n - 1) / 2;
  uint32_t key = a[0];
#pragma unroll
  for (int j = 1; j < N; ++j) key = j == rank ? a[j] : key;
  return ft_unkey(key);
}
