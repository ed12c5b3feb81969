// K34 camera rectification (include/mi355x_match_rectify.h): the sampling map of a camera, the remap of a batch of frames
// through it, the undistortion of keypoints and, on the host, the rectifying rotations of a stereo rig, under K30's contract.
// The arithmetic is csrc/rectify_math.h's.
//
// K34a  rc_map_kernel          one thread per destination pixel; float64, about 80 operations and four divisions.  It runs
//       once per camera.
// K34b  rc_remap_kernel<T, VEC> the hot path: a gather with a compact footprint, bound by memory.  A lane owns four consecutive
//       destination pixels of a row, a workgroup of 256 a tile of 64 x 16 destination pixels, whose source footprint (a few
//       KiB for a real lens) stays in the CU's L1 between the taps of neighbouring lanes.  The lane's eight map elements are
//       loaded once (VEC: two 16-byte loads) and kept in registers while the workgroup walks RC_FRAMES frames of the batch:
//       the map's traffic is an eighth of a frame's, and the frames of one tile run together.  VEC (w a multiple of 4, map and
//       dst on 16 bytes): the four results leave in one store (a dword of uint8, 8 bytes of uint16, 16 bytes of float32).
//       The taps themselves are element loads through the L1, bounds-checked one by one: no index leaves the frame.
// K34c  rc_points_kernel       one thread per point, float64.
// No atomics; every output element has one owner thread: bitwise reproducible.
#include "common.h"
#include "rectify_math.h"

#include <math.h>

namespace {

constexpr int RC_TILE_W = 64, RC_TILE_H = 16, RC_PX = 4;                    // a lane's pixels; 16 x 16 lanes
constexpr int RC_FRAMES = 8;                                                // frames a workgroup walks with its map in registers

__global__ __launch_bounds__(256) void rc_map_kernel(RcCamera cam, int src_h, int src_w, int h, int w, int32_t *__restrict__ map,
                                                     uint8_t *__restrict__ mask) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)h * w) return;
  const int v = (int)(p / (size_t)w), u = (int)(p - (size_t)v * w);
  int32_t qx, qy;
  uint8_t m;
  rc_map_pixel(cam, src_h, src_w, v, u, &qx, &qy, &m);
  *reinterpret_cast<int2 *>(map + 2 * p) = make_int2(qx, qy);
  if (mask) mask[p] = m;
}

template <typename T>
struct RcQuad;
template <>
struct RcQuad<uint8_t> {
  typedef uint32_t V;
};
template <>
struct RcQuad<uint16_t> {
  typedef uint2 V;
};
template <>
struct RcQuad<float> {
  typedef float4 V;
};

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void rc_remap_kernel(const T *__restrict__ src, int batch, int src_h, int src_w,
                                                       const int32_t *__restrict__ map, int h, int w, int tiles_x, bool linear, T border,
                                                       T *__restrict__ dst) {
  const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * tiles_x);
  const int x0 = tile_x * RC_TILE_W + (int)(threadIdx.x & 15) * RC_PX, y = tile_y * RC_TILE_H + (int)(threadIdx.x >> 4);
  if (y >= h || x0 >= w) return;
  const size_t p0 = (size_t)y * w + x0;
  const int count = VEC ? RC_PX : min(RC_PX, w - x0);                       // VEC: w is a multiple of RC_PX
  int32_t q[2 * RC_PX];
  if (VEC) {
    const int4 a = *reinterpret_cast<const int4 *>(map + 2 * p0), b = *reinterpret_cast<const int4 *>(map + 2 * p0 + 4);
    q[0] = a.x, q[1] = a.y, q[2] = a.z, q[3] = a.w, q[4] = b.x, q[5] = b.y, q[6] = b.z, q[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < RC_PX; ++j) {
      const int2 e = j < count ? *reinterpret_cast<const int2 *>(map + 2 * (p0 + j)) : make_int2(0, 0);
      q[2 * j] = e.x, q[2 * j + 1] = e.y;
    }
  }
  const size_t src_frame = (size_t)src_h * src_w, dst_frame = (size_t)h * w;
  const int f0 = (int)blockIdx.y * RC_FRAMES, f1 = min(f0 + RC_FRAMES, batch);
  for (int f = f0; f < f1; ++f) {
    const T *s = src + (size_t)f * src_frame;
    T *d = dst + (size_t)f * dst_frame + p0;
    T out[RC_PX];
#pragma unroll
    for (int j = 0; j < RC_PX; ++j) out[j] = (VEC || j < count) ? rc_remap_pixel(s, src_h, src_w, q[2 * j], q[2 * j + 1], linear, border) : border;
    if (VEC) {
      typename RcQuad<T>::V packed;
      __builtin_memcpy(&packed, out, sizeof(packed));
      *reinterpret_cast<typename RcQuad<T>::V *>(d) = packed;
    } else {
#pragma unroll
      for (int j = 0; j < RC_PX; ++j)
        if (j < count) d[j] = out[j];
    }
  }
}

__global__ __launch_bounds__(256) void rc_points_kernel(RcCamera cam, const float *__restrict__ pts, size_t n, int iterations,
                                                        double max_residual_px, float *__restrict__ out, uint8_t *__restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float ox, oy;
  const bool good = rc_undistort_point(cam, pts[2 * i], pts[2 * i + 1], iterations, max_residual_px, &ox, &oy);
  out[2 * i] = ox;
  out[2 * i + 1] = oy;
  ok[i] = (uint8_t)good;
}

inline bool rc_aligned(const void *p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

template <typename T>
int rc_remap(const void *src, int batch, int src_h, int src_w, const int32_t *map, int h, int w, bool linear, double border_value, void *dst,
             hipStream_t s) {
  const int tiles_x = (w + RC_TILE_W - 1) / RC_TILE_W, tiles_y = (h + RC_TILE_H - 1) / RC_TILE_H;
  const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)((batch + RC_FRAMES - 1) / RC_FRAMES)), block(256);
  const bool vec = w % RC_PX == 0 && rc_aligned(map, 16) && rc_aligned(dst, 16);
  if (vec)
    hipLaunchKernelGGL((rc_remap_kernel<T, true>), grid, block, 0, s, static_cast<const T *>(src), batch, src_h, src_w, map, h, w, tiles_x,
                       linear, (T)border_value, static_cast<T *>(dst));
  else
    hipLaunchKernelGGL((rc_remap_kernel<T, false>), grid, block, 0, s, static_cast<const T *>(src), batch, src_h, src_w, map, h, w, tiles_x,
                       linear, (T)border_value, static_cast<T *>(dst));
  return mi_launch_status();
}

inline bool rc_extent_small(int v) { return v < 1; }
inline bool rc_extent_large(int v) { return v > MI_RECTIFY_MAX_DIM; }

}  // namespace

extern "C" int mi_rectify_map(int model, const double *k, const double *dist, const double *r, const double *k_new, int src_h, int src_w,
                              int h, int w, int32_t *map, uint8_t *mask, mi_stream_t stream) {
  MI_ENTER();
  if (!k || !dist || !k_new || !map) return MI_E_NULL;
  if (rc_extent_small(src_h) || rc_extent_small(src_w) || rc_extent_small(h) || rc_extent_small(w)) return MI_E_SHAPE;
  if (rc_extent_large(src_h) || rc_extent_large(src_w) || rc_extent_large(h) || rc_extent_large(w)) return MI_E_PARAM;
  RcCamera cam;
  if (const int st = rc_camera(model, k, dist, r, k_new, &cam)) return st;
  if (!rc_aligned(map, 8)) return MI_E_ALIGN;
  const size_t n = (size_t)h * w;
  hipLaunchKernelGGL(rc_map_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cam, src_h, src_w, h, w, map, mask);
  return mi_launch_status();
}

extern "C" int mi_rectify_remap(const void *src, int type, int batch, int src_h, int src_w, const int32_t *map, int h, int w,
                                int interpolation, double border_value, void *dst, mi_stream_t stream) {
  MI_ENTER();
  if (!src || !map || !dst) return MI_E_NULL;
  if (batch < 1 || rc_extent_small(src_h) || rc_extent_small(src_w) || rc_extent_small(h) || rc_extent_small(w)) return MI_E_SHAPE;
  if (batch > MI_RECTIFY_MAX_BATCH || rc_extent_large(src_h) || rc_extent_large(src_w) || rc_extent_large(h) || rc_extent_large(w)) return MI_E_PARAM;
  if (type != MI_RECTIFY_U8 && type != MI_RECTIFY_U16 && type != MI_RECTIFY_F32) return MI_E_PARAM;
  if (interpolation != MI_RECTIFY_NEAREST && interpolation != MI_RECTIFY_LINEAR) return MI_E_PARAM;
  if (type == MI_RECTIFY_U16 && interpolation == MI_RECTIFY_LINEAR) return MI_E_PARAM;
  if (type != MI_RECTIFY_F32) {
    const double top = type == MI_RECTIFY_U8 ? 255.0 : 65535.0;
    if (!(border_value >= 0.0 && border_value <= top) || floor(border_value) != border_value) return MI_E_PARAM;
  }
  const uintptr_t element = type == MI_RECTIFY_U8 ? 1 : (type == MI_RECTIFY_U16 ? 2 : 4);
  if (!rc_aligned(src, element) || !rc_aligned(dst, element) || !rc_aligned(map, 8)) return MI_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const bool linear = interpolation == MI_RECTIFY_LINEAR;
  switch (type) {
    case MI_RECTIFY_U8: return rc_remap<uint8_t>(src, batch, src_h, src_w, map, h, w, linear, border_value, dst, s);
    case MI_RECTIFY_U16: return rc_remap<uint16_t>(src, batch, src_h, src_w, map, h, w, linear, border_value, dst, s);
    default: return rc_remap<float>(src, batch, src_h, src_w, map, h, w, linear, border_value, dst, s);
  }
}

extern "C" int mi_rectify_points(const float *pts, int batch, int n, int model, const double *k, const double *dist, const double *r,
                                 const double *k_new, int iterations, double max_residual_px, float *out, uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts || !k || !dist || !out || !ok) return MI_E_NULL;
  if (batch < 1 || n < 1) return MI_E_SHAPE;
  if ((long long)batch * n > MI_RECTIFY_MAX_POINTS) return MI_E_PARAM;
  RcCamera cam;
  if (const int st = rc_camera(model, k, dist, r, k_new, &cam)) return st;
  if (iterations < 1 || iterations > MI_RECTIFY_MAX_ITERATIONS) return MI_E_PARAM;
  if (!(max_residual_px > 0.0) || !rc_finite(max_residual_px)) return MI_E_PARAM;
  if (!rc_aligned(pts, 4) || !rc_aligned(out, 4)) return MI_E_ALIGN;
  const size_t total = (size_t)batch * n;
  hipLaunchKernelGGL(rc_points_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cam, pts, total, iterations,
                     max_residual_px, out, ok);
  return mi_launch_status();
}

extern "C" int mi_rectify_stereo_rig(const double *k1, const double *k2, const double *r, const double *t, int h, int w, double *r1,
                                     double *r2, double *k_new, double *baseline, double *fb) {
  if (!k1 || !k2 || !r || !t || !r1 || !r2 || !k_new || !baseline || !fb) return MI_E_NULL;
  if (rc_extent_small(h) || rc_extent_small(w)) return MI_E_SHAPE;
  if (rc_extent_large(h) || rc_extent_large(w)) return MI_E_PARAM;
  return rc_stereo_rig(k1, k2, r, t, h, w, r1, r2, k_new, baseline, fb);
}
