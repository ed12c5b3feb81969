// K33 stereo depth (include/mi355x_match_stereo.h): census transform, semi-global aggregation of the Hamming cost, disparity
// selection with its tests, depth, batched over rectified pairs under K30's contract.  The arithmetic is csrc/stereo_math.h's.
//
// K33a  st_census_kernel<T>        one thread per pixel; the 62 neighbours through the L1 (a wave's rows are contiguous).
// K33b  st_path_kernel<NPL, FIRST> one launch per direction.  A wave walks one path line; lane t holds the NPL = D / 64
//       consecutive disparities t NPL .. t NPL + NPL - 1, so that a pixel's volume row is one coalesced store of 2 D bytes and
//       the d - 1 / d + 1 neighbours are registers but for one wave shift each way.  The cost is popcount(xor) of the left
//       census word (one address for the wave) and the right row's words x - d (consecutive addresses, descending); it is
//       never stored.  m is an integer wave minimum on the DPP path.  The previous pixel's L_r stays in registers; the census
//       words and volume rows of the next ST_AHEAD pixels are in flight while the recurrence of this one runs (a wave has one
//       line and the recurrence is serial, so what hides the memory latency is how far ahead it fetches).  FIRST writes the volume, the other launches add to it: every element has one owner thread per launch, so
//       the adds are plain.  Four waves of a workgroup take neighbouring lines (columns for the vertical and diagonal
//       directions), whose census words and volume rows are neighbours in memory.
// K33c  st_right_kernel<NPL>       one wave per image row walks x; the running minimum of the right pixel xr = x - d sits in
//       the lane of d and moves one disparity up per pixel, so the diagonal S(y, xr + d, d) is read as coalesced volume rows,
//       ST_AHEAD of them in flight.
// K33d  st_left_kernel<NPL>        one wave per pixel, 16 pixels one after the other with ST_AHEAD rows in flight: wave argmin on
//       a (S, d) key, the uniqueness vote by ballot, then lane 0 does the left-right test and the sub-pixel step.
// K33e  st_depth_kernel            one thread per pixel.
// Integer arithmetic and two float32 divisions; no atomics; nothing depends on the order of arrival: bitwise reproducible.
#include "common.h"
#include "stereo_math.h"

#include <math.h>

namespace {

constexpr int ST_WAVES = 4;
constexpr int ST_STRIP = 16;                                              // pixels per wave of K33d
constexpr int ST_AHEAD = 4;                                               // pixels a wave fetches ahead of the one it works on

// NPL uint16 of one lane as one aligned vector
template <int NPL>
struct StRow;
template <>
struct StRow<1> {
  typedef uint16_t T;
};
template <>
struct StRow<2> {
  typedef unsigned short T __attribute__((ext_vector_type(2)));
};
template <>
struct StRow<4> {
  typedef unsigned short T __attribute__((ext_vector_type(4)));
};
__device__ __forceinline__ int st_get(uint16_t v, int) { return v; }
template <typename V>
__device__ __forceinline__ int st_get(const V &v, int j) {
  return v[j];
}
__device__ __forceinline__ void st_set(uint16_t &v, int, int s) { v = (uint16_t)s; }
template <typename V>
__device__ __forceinline__ void st_set(V &v, int j, int s) {
  v[j] = (unsigned short)s;
}

// lane i takes lane i - 1's value and lane 0 `fill` (wave_shr:1); lane i takes lane i + 1's and lane 63 `fill` (wave_shl:1):
// a lane without a source keeps `old`, which is the fill
__device__ __forceinline__ int st_lane_up(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int st_lane_down(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false); }

// the minimum over the wave in every lane; common.h's wave_max_dpp in integers (values below 2^31)
#define ST_DPP(v, ctrl, rmask) __builtin_amdgcn_update_dpp(v, v, ctrl, rmask, 0xf, false)
__device__ __forceinline__ int st_wave_min(int v) {
  v = min(v, ST_DPP(v, 0xB1, 0xf));     // quad_perm [1,0,3,2]
  v = min(v, ST_DPP(v, 0x4E, 0xf));     // quad_perm [2,3,0,1]
  v = min(v, ST_DPP(v, 0x141, 0xf));    // row_half_mirror
  v = min(v, ST_DPP(v, 0x140, 0xf));    // row_mirror
  v = min(v, ST_DPP(v, 0x142, 0xa));    // row_bcast15 into rows 1 and 3
  v = min(v, ST_DPP(v, 0x143, 0xc));    // row_bcast31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}

template <typename T>
__global__ __launch_bounds__(256) void st_census_kernel(const T *__restrict__ gray, size_t n, int h, int w, uint64_t *__restrict__ census) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const size_t row = p / (size_t)w;
  const int x = (int)(p - row * w), y = (int)(row % (size_t)h);
  census[p] = st_census(gray + (row - y) * w, h, w, y, x);
}

// what a lane needs of pixel (y, x), as loaded: the left census word, the right row's words at x - d for its NPL disparities
// (the address clamped into the row where x - d < 0; st_cost does not read that word) and, unless FIRST, the volume row the
// new sums are added to.  Nothing is computed from them at fetch time, so that the loads stay in flight.
template <int NPL>
struct StPixel {
  uint64_t left, right[NPL];
  typename StRow<NPL>::T old;
};
template <int NPL, bool FIRST>
__device__ __forceinline__ void st_fetch(const uint64_t *__restrict__ cl, const uint64_t *__restrict__ cr, const uint16_t *volume, int w,
                                         int y, int x, int d0, StPixel<NPL> *px) {
  const size_t row = (size_t)y * w;
  px->left = cl[row + x];
#pragma unroll
  for (int j = 0; j < NPL; ++j) px->right[j] = cr[row + max(x - (d0 + j), 0)];
  if (!FIRST) px->old = *reinterpret_cast<const typename StRow<NPL>::T *>(volume + (row + x) * (size_t)(64 * NPL) + d0);
}

// the index of this thread's wave in its workgroup as a scalar: everything derived from it (the line, its pixels, the loop
// bounds) is then wave-uniform for the compiler too, which makes the branches scalar
__device__ __forceinline__ int st_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

template <int NPL, bool FIRST>
__global__ __launch_bounds__(64 * ST_WAVES) void st_path_kernel(const uint64_t *__restrict__ cl, const uint64_t *__restrict__ cr, int batch,
                                                                int h, int w, int dy, int dx, int lines, int p1, int p2,
                                                                uint16_t *volume) {
  typedef typename StRow<NPL>::T Row;
  const int lane = threadIdx.x & 63, d0 = lane * NPL;
  const long long line = (long long)blockIdx.x * ST_WAVES + st_wave();
  if (line >= (long long)batch * lines) return;
  const size_t image = (size_t)(line / lines) * h * w;
  cl += image;
  cr += image;
  volume += image * (size_t)(64 * NPL);
  // a zero the compiler takes for a per-lane value: the left census word, one address for the whole wave, then comes by a
  // vector load that stays in flight with the others; as a scalar load its wait is placed right behind it, once per pixel
  int lane_zero;
  asm("v_mov_b32 %0, 0" : "=v"(lane_zero));
  cl += lane_zero;
  int y, x;
  st_line_start((int)(line % lines), h, w, dy, dx, &y, &x);
  const int ny = dy == 0 ? w : (dy > 0 ? h - y : y + 1), nx = dx == 0 ? h : (dx > 0 ? w - x : x + 1);
  const int n = min(ny, nx);                                                         // the pixels of this line
  // a ring of the next ST_AHEAD pixels: slot k serves the pixels k, k + ST_AHEAD, ...
  StPixel<NPL> ring[ST_AHEAD];
  int prev[NPL], m = 0;
#pragma unroll
  for (int k = 0; k < ST_AHEAD; ++k) {
    ring[k].old = Row();
    if (k < n) st_fetch<NPL, FIRST>(cl, cr, volume, w, y + k * dy, x + k * dx, d0, &ring[k]);
  }
  for (int s0 = 0; s0 < n; s0 += ST_AHEAD) {
#pragma unroll
    for (int k = 0; k < ST_AHEAD; ++k) {
      const int s = s0 + k;
      if (s >= n) break;
      const int py = y + s * dy, px = x + s * dx;
      int c[NPL], l[NPL];
#pragma unroll
      for (int j = 0; j < NPL; ++j) c[j] = st_cost(ring[k].left, ring[k].right[j], px - (d0 + j) >= 0);
      const Row old = ring[k].old;
      if (s + ST_AHEAD < n) st_fetch<NPL, FIRST>(cl, cr, volume, w, py + ST_AHEAD * dy, px + ST_AHEAD * dx, d0, &ring[k]);
      if (s == 0) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) l[j] = c[j];
      } else {
        const int below = st_lane_up(prev[NPL - 1], ST_ABSENT), above = st_lane_down(prev[0], ST_ABSENT);
#pragma unroll
        for (int j = 0; j < NPL; ++j)
          l[j] = st_path_step(c[j], prev[j], j == 0 ? below : prev[j - 1], j == NPL - 1 ? above : prev[j + 1], m, p1, p2);
      }
      int lo = l[0];
      Row out;
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        lo = min(lo, l[j]);
        prev[j] = l[j];
        st_set(out, j, FIRST ? l[j] : st_get(old, j) + l[j]);
      }
      *reinterpret_cast<Row *>(volume + ((size_t)py * w + px) * (size_t)(64 * NPL) + d0) = out;
      if (s + 1 < n) m = st_wave_min(lo);
    }
  }
}

template <int NPL>
__global__ __launch_bounds__(64 * ST_WAVES) void st_right_kernel(const uint16_t *__restrict__ volume, long long rows, int w,
                                                                 int16_t *__restrict__ right) {
  typedef typename StRow<NPL>::T Row;
  constexpr int D = 64 * NPL;
  const int lane = threadIdx.x & 63, d0 = lane * NPL;
  const long long row = (long long)blockIdx.x * ST_WAVES + st_wave();
  if (row >= rows) return;
  volume += (size_t)row * w * D + d0;
  right += (size_t)row * w;
  // best[j]: the running minimum key of the right pixel xr = x - (d0 + j) over the disparities 0 .. d0 + j.  A pixel's
  // minimum starts in lane 0 at x = xr and moves one disparity up per step; those of xr < 0 are never written.
  uint32_t best[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) best[j] = 0xffffffffu;
  Row ring[ST_AHEAD];                                                                // the next ST_AHEAD volume rows
#pragma unroll
  for (int k = 0; k < ST_AHEAD; ++k) ring[k] = k < w ? *reinterpret_cast<const Row *>(volume + (size_t)k * D) : Row();
  for (int x0 = 0; x0 < w; x0 += ST_AHEAD) {
#pragma unroll
    for (int k = 0; k < ST_AHEAD; ++k) {
      const int x = x0 + k;
      if (x >= w) break;
      const Row s = ring[k];
      if (x + ST_AHEAD < w) ring[k] = *reinterpret_cast<const Row *>(volume + (size_t)(x + ST_AHEAD) * D);
      const uint32_t carry = (uint32_t)st_lane_up((int)best[NPL - 1], -1);
#pragma unroll
      for (int j = NPL - 1; j > 0; --j) best[j] = best[j - 1];
      best[0] = carry;
#pragma unroll
      for (int j = 0; j < NPL; ++j) best[j] = min(best[j], st_key(st_get(s, j), d0 + j));
      if (lane == 63 && x - (D - 1) >= 0 && x < w - 1) right[x - (D - 1)] = (int16_t)st_key_d(best[NPL - 1]);   // d = D - 1 was its last
    }
  }
#pragma unroll
  for (int j = 0; j < NPL; ++j)                                                      // x = w - 1 was the last of all that are left
    if (w - 1 - (d0 + j) >= 0) right[w - 1 - (d0 + j)] = (int16_t)st_key_d(best[j]);
}

template <int NPL>
__global__ __launch_bounds__(64 * ST_WAVES) void st_left_kernel(const uint16_t *__restrict__ volume, size_t pixels, int w, int uniqueness,
                                                                int lr_max_diff, const int16_t *__restrict__ right,
                                                                float *__restrict__ disparity, uint8_t *__restrict__ code) {
  typedef typename StRow<NPL>::T Row;
  constexpr int D = 64 * NPL;
  const int lane = threadIdx.x & 63, d0 = lane * NPL;
  const size_t p0 = ((size_t)blockIdx.x * ST_WAVES + st_wave()) * ST_STRIP;
  if (p0 >= pixels) return;
  const int count = pixels - p0 < (size_t)ST_STRIP ? (int)(pixels - p0) : ST_STRIP;
  Row ring[ST_AHEAD];                                                                // the next ST_AHEAD pixels' volume rows
#pragma unroll
  for (int k = 0; k < ST_AHEAD; ++k) ring[k] = k < count ? *reinterpret_cast<const Row *>(volume + (p0 + k) * D + d0) : Row();
  for (int i0 = 0; i0 < count; i0 += ST_AHEAD) {
#pragma unroll
    for (int k = 0; k < ST_AHEAD; ++k) {
      const int i = i0 + k;
      if (i >= count) break;
      const size_t p = p0 + i;
      const Row s = ring[k];
      if (i + ST_AHEAD < count) ring[k] = *reinterpret_cast<const Row *>(volume + (p + ST_AHEAD) * D + d0);
      uint32_t key = 0xffffffffu;
#pragma unroll
      for (int j = 0; j < NPL; ++j) key = min(key, st_key(st_get(s, j), d0 + j));
      key = (uint32_t)st_wave_min((int)key);                                         // below 2^20
      const int d_best = st_key_d(key), s_best = st_key_s(key);
      bool rival = false;
#pragma unroll
      for (int j = 0; j < NPL; ++j) rival |= st_rival(st_get(s, j), d0 + j, s_best, d_best, uniqueness);
      const bool not_unique = __ballot(rival) != 0ull;
      if (lane == 0) {
        const int x = (int)(p % (size_t)w);
        int result = MI_STEREO_OK;
        if (not_unique)
          result = MI_STEREO_NOT_UNIQUE;
        else if (lr_max_diff >= 0 && st_lr_fails(x, d_best, right + (p - x), lr_max_diff))
          result = MI_STEREO_LR;
        float disp = -1.0f;
        if (result == MI_STEREO_OK) {
          const bool inner = d_best > 0 && d_best < D - 1;
          const uint16_t *at = volume + p * D + d_best;
          disp = st_subpixel(d_best, D, inner ? at[-1] : 0, s_best, inner ? at[1] : 0);
        }
        disparity[p] = disp;
        code[p] = (uint8_t)result;
      }
    }
  }
}

__global__ __launch_bounds__(256) void st_depth_kernel(const float *__restrict__ disparity, size_t n, float fb, float min_disparity,
                                                       float *__restrict__ depth) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) depth[i] = st_depth(disparity[i], fb, min_disparity);
}

inline bool st_aligned(const void *p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

// MI_E_SHAPE / MI_E_PARAM of a frame batch; *pixels = batch h w (below MI_STEREO_MAX_PIXELS)
inline int st_frames_status(int batch, int h, int w, long long *pixels) {
  if (batch < 1 || h < 1 || w < 1) return MI_E_SHAPE;
  const long long rows = (long long)batch * h;
  if (rows >= MI_STEREO_MAX_PIXELS || rows * w >= MI_STEREO_MAX_PIXELS) return MI_E_PARAM;
  *pixels = rows * w;
  return MI_OK;
}

template <int NPL>
int st_aggregate(const uint64_t *cl, const uint64_t *cr, int batch, int h, int w, int paths, int p1, int p2, uint16_t *volume,
                 hipStream_t s) {
  for (int r = 0; r < paths; ++r) {
    const int dy = ST_DIRS[r][0], dx = ST_DIRS[r][1], lines = st_lines(h, w, dy, dx);
    const dim3 grid((unsigned)(((long long)batch * lines + ST_WAVES - 1) / ST_WAVES)), block(64 * ST_WAVES);
    if (r == 0)
      hipLaunchKernelGGL((st_path_kernel<NPL, true>), grid, block, 0, s, cl, cr, batch, h, w, dy, dx, lines, p1, p2, volume);
    else
      hipLaunchKernelGGL((st_path_kernel<NPL, false>), grid, block, 0, s, cl, cr, batch, h, w, dy, dx, lines, p1, p2, volume);
    MI_CHECK_LAUNCH();
  }
  return MI_OK;
}

template <int NPL>
int st_select(const uint16_t *volume, long long rows, int w, int uniqueness, int lr_max_diff, float *disparity, int16_t *right,
              uint8_t *code, hipStream_t s) {
  const dim3 block(64 * ST_WAVES);
  if (right) {
    hipLaunchKernelGGL(st_right_kernel<NPL>, dim3((unsigned)((rows + ST_WAVES - 1) / ST_WAVES)), block, 0, s, volume, rows, w, right);
    MI_CHECK_LAUNCH();
  }
  const size_t pixels = (size_t)rows * w, waves = (pixels + ST_STRIP - 1) / ST_STRIP;
  hipLaunchKernelGGL(st_left_kernel<NPL>, dim3((unsigned)((waves + ST_WAVES - 1) / ST_WAVES)), block, 0, s, volume, pixels, w, uniqueness,
                     lr_max_diff, right, disparity, code);
  return mi_launch_status();
}

}  // namespace

extern "C" int mi_stereo_census(const void *gray, int gray_is_u8, int batch, int h, int w, uint64_t *census, mi_stream_t stream) {
  MI_ENTER();
  if (!gray || !census) return MI_E_NULL;
  long long n;
  if (const int st = st_frames_status(batch, h, w, &n)) return st;
  if (!st_aligned(census, 8) || (!gray_is_u8 && !st_aligned(gray, 4))) return MI_E_ALIGN;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (gray_is_u8)
    hipLaunchKernelGGL(st_census_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, static_cast<const uint8_t *>(gray), (size_t)n, h, w, census);
  else
    hipLaunchKernelGGL(st_census_kernel<float>, grid, block, 0, (hipStream_t)stream, static_cast<const float *>(gray), (size_t)n, h, w, census);
  return mi_launch_status();
}

extern "C" size_t mi_stereo_workspace_bytes(int, int, int, int, int) { return 0; }

extern "C" int mi_stereo_aggregate(const uint64_t *census_left, const uint64_t *census_right, int batch, int h, int w, int D,
                                   int paths, int p1, int p2, uint16_t *volume, void *workspace, size_t workspace_bytes,
                                   mi_stream_t stream) {
  MI_ENTER();
  if (!census_left || !census_right || !volume) return MI_E_NULL;
  long long n;
  if (const int st = st_frames_status(batch, h, w, &n)) return st;
  if ((D != 64 && D != 128 && D != 256) || (paths != 4 && paths != 8) || p1 < 0 || p1 > p2 || p2 > 255) return MI_E_PARAM;
  if (n * D >= MI_STEREO_MAX_VOLUME) return MI_E_PARAM;
  if (!st_aligned(census_left, 8) || !st_aligned(census_right, 8) || !st_aligned(volume, 16)) return MI_E_ALIGN;
  if (workspace_bytes < mi_stereo_workspace_bytes(batch, h, w, D, paths)) return MI_E_CAPACITY;
  (void)workspace;
  hipStream_t s = (hipStream_t)stream;
  switch (D) {
    case 64: return st_aggregate<1>(census_left, census_right, batch, h, w, paths, p1, p2, volume, s);
    case 128: return st_aggregate<2>(census_left, census_right, batch, h, w, paths, p1, p2, volume, s);
    default: return st_aggregate<4>(census_left, census_right, batch, h, w, paths, p1, p2, volume, s);
  }
}

extern "C" int mi_stereo_select(const uint16_t *volume, int batch, int h, int w, int D, int uniqueness, int lr_max_diff,
                                float *disparity, int16_t *disparity_right, uint8_t *code, mi_stream_t stream) {
  MI_ENTER();
  if (!volume || !disparity || !code || (!disparity_right && lr_max_diff >= 0)) return MI_E_NULL;
  long long n;
  if (const int st = st_frames_status(batch, h, w, &n)) return st;
  if ((D != 64 && D != 128 && D != 256) || uniqueness < 0 || uniqueness > 100 || n * D >= MI_STEREO_MAX_VOLUME) return MI_E_PARAM;
  if (!st_aligned(volume, 16) || !st_aligned(disparity, 4) || !st_aligned(disparity_right, 2)) return MI_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const long long rows = (long long)batch * h;
  switch (D) {
    case 64: return st_select<1>(volume, rows, w, uniqueness, lr_max_diff, disparity, disparity_right, code, s);
    case 128: return st_select<2>(volume, rows, w, uniqueness, lr_max_diff, disparity, disparity_right, code, s);
    default: return st_select<4>(volume, rows, w, uniqueness, lr_max_diff, disparity, disparity_right, code, s);
  }
}

extern "C" int mi_stereo_depth(const float *disparity, int batch, int h, int w, float fb, float min_disparity, float *depth,
                               mi_stream_t stream) {
  MI_ENTER();
  if (!disparity || !depth) return MI_E_NULL;
  long long n;
  if (const int st = st_frames_status(batch, h, w, &n)) return st;
  if (!(fb > 0.0f) || !(fb < INFINITY) || !(min_disparity > 0.0f) || !(min_disparity < INFINITY)) return MI_E_PARAM;
  if (!st_aligned(disparity, 4) || !st_aligned(depth, 4)) return MI_E_ALIGN;
  hipLaunchKernelGGL(st_depth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, disparity, (size_t)n, fb,
                     min_disparity, depth);
  return mi_launch_status();
}
