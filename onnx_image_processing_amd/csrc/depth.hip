// K13 depth front end (reference pytorch_model/depth/): depth frames -> points (+ normals), and depth re-rendered in
// the colour camera's frame.  Batched over frames, every launch on `stream`, nothing read back, no workspace.
//
// K13a  depth_points_kernel   one workgroup per 128 x 8 pixel tile of one frame.  The depth tile with its one-pixel
//       apron (zero outside the frame) and the tile's slices of the two tables go to LDS; each thread forms four
//       neighbouring pixels' points d * (u_tab[w], v_tab[h], z_scale) and, if asked, their normals from the 3 x 6 depth
//       neighbourhood (the point image is never read back).  The interleaved xyz rows are staged in LDS and leave as
//       full-width contiguous stores (16 B per lane when w % 4 == 0 and the outputs are 16-byte aligned, 4 B otherwise).
//       HBM traffic: 4 (2 for uint16) bytes in, 12 or 24 out per pixel.
// K13b  depth_align: fill (sentinel) -> splat -> finish (sentinel -> 0).  The z-buffer is the output itself: positive
//       floats order as their bit patterns, so "nearest surface wins" is a uint32 atomicMin (integer vector atomics
//       only; no float atomics, no cross-workgroup waits): bitwise reproducible, identical alone or batched, and the
//       fill pass makes the result independent of what the output buffer held.  A tile-local LDS z-buffer in front
//       of the global atomics takes most of them away (depth_align_splat_kernel).
// Built with -ffp-contract=off and IEEE division: the products and the projection below round exactly as the
// reference's op-by-op float32 arithmetic does.
#include "common.h"

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_TW = 128;                    // tile width: 32 threads x 4 pixels
constexpr int DP_TH = 8;                      // tile height: one row per 32 threads
constexpr int DP_AW = DP_TW + 2;              // with apron
constexpr int DP_AH = DP_TH + 2;
constexpr unsigned DA_SENTINEL = 0xFFFFFFFFu; // above every float bit pattern a source may write (< 10000.0f)

template <typename T>
__device__ __forceinline__ float dp_load(const T *p) {
  return (float)*p;                           // uint16 -> float32 is exact
}

// stage[DP_TH][3 * DP_TW] floats -> rows of the interleaved output; `valid_w` pixels per row, `rows` rows.  PER_ROW > 0:
// the row length in store units is a compile-time constant (a full-width tile), which keeps the index division cheap.
template <int PER_ROW, typename V>
__device__ __forceinline__ void dp_store_units(const float *stage, float *out, long long pix0, int w, int per_row_rt, int rows) {
  constexpr int N = sizeof(V) / sizeof(float);
  const int per_row = PER_ROW > 0 ? PER_ROW : per_row_rt;
  for (int i = threadIdx.x; i < rows * per_row; i += DP_THREADS) {
    const int r = i / per_row, c = i - r * per_row;
    *reinterpret_cast<V *>(out + (pix0 + (long long)r * w) * 3 + N * c) = *reinterpret_cast<const V *>(stage + r * (3 * DP_TW) + N * c);
  }
}
__device__ __forceinline__ void dp_store_rows(const float *stage, float *out, long long pix0, int w, int valid_w, int rows,
                                              bool vec) {
  if (vec) {                                  // w % 4 == 0: every row piece starts and ends on 16 bytes
    if (valid_w == DP_TW)
      dp_store_units<3 * DP_TW / 4, float4>(stage, out, pix0, w, 0, rows);
    else
      dp_store_units<0, float4>(stage, out, pix0, w, valid_w * 3 / 4, rows);
  } else {
    if (valid_w == DP_TW)
      dp_store_units<3 * DP_TW, float>(stage, out, pix0, w, 0, rows);
    else
      dp_store_units<0, float>(stage, out, pix0, w, valid_w * 3, rows);
  }
}

template <typename T, bool NORMALS>
__global__ __launch_bounds__(DP_THREADS) void depth_points_kernel(const T *__restrict__ depth, int h, int w, int tiles_x,
                                                                   int tiles_y, const float *__restrict__ u_tab,
                                                                   const float *__restrict__ v_tab, float z_scale,
                                                                   float *__restrict__ points, float *__restrict__ normals,
                                                                   int vec) {
  __shared__ float sd[DP_AH][DP_AW];
  __shared__ float su[DP_AW];
  __shared__ float sv[DP_AH];
  __shared__ __attribute__((aligned(16))) float stage[DP_TH * 3 * DP_TW];

  const unsigned tile = blockIdx.x;
  const int txi = (int)(tile % (unsigned)tiles_x);
  const unsigned rest = tile / (unsigned)tiles_x;
  const int tyi = (int)(rest % (unsigned)tiles_y);
  const long long frame = rest / (unsigned)tiles_y;
  const int x0 = txi * DP_TW, y0 = tyi * DP_TH;
  const T *src = depth + frame * h * w;

  for (int i = threadIdx.x; i < DP_AH * DP_AW; i += DP_THREADS) {
    const int r = i / DP_AW, c = i - r * DP_AW;
    const int gy = y0 - 1 + r, gx = x0 - 1 + c;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    sd[r][c] = in ? dp_load(src + (long long)gy * w + gx) : 0.0f;
  }
  if (threadIdx.x < DP_AW) {
    const int gx = x0 - 1 + (int)threadIdx.x;
    su[threadIdx.x] = (gx >= 0 && gx < w) ? u_tab[gx] : 0.0f;
  } else if (threadIdx.x < DP_AW + DP_AH) {
    const int r = (int)threadIdx.x - DP_AW;
    const int gy = y0 - 1 + r;
    sv[r] = (gy >= 0 && gy < h) ? v_tab[gy] : 0.0f;
  }
  __syncthreads();

  const int ty = threadIdx.x >> 5;            // tile row
  const int tx = (threadIdx.x & 31) * 4;      // first of the thread's four pixels
  const int rows = min(DP_TH, h - y0), valid_w = min(DP_TW, w - x0);
  const long long pix0 = (frame * h + y0) * w + x0;

  // the points: exactly d * u_tab[w], d * v_tab[h], d * z_scale
  const float vy = sv[ty + 1];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float d = sd[ty + 1][tx + k + 1];
    float *o = stage + ty * (3 * DP_TW) + 3 * (tx + k);
    o[0] = d * su[tx + k + 1];
    o[1] = d * vy;
    o[2] = d * z_scale;
  }
  __syncthreads();
  dp_store_rows(stage, points, pix0, w, valid_w, rows, vec != 0);

  if (NORMALS) {
    // s = X + Y + Z of the 3 x 6 neighbourhood (0 outside the frame: the apron's depth is 0 and its table entries are 0)
    float s[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float vr = sv[ty + r];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const float d = sd[ty + r][tx + c];
        s[r][c] = (d * su[tx + c] + d * vr) + d * z_scale;
      }
    }
    __syncthreads();                          // the point rows have left the staging buffer
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // cross-correlation with sobel_v = [[1,0,-1],[2,0,-2],[1,0,-1]] and sobel_h = [[1,2,1],[0,0,0],[-1,-2,-1]]
      const float dx = ((s[0][k] - s[0][k + 2]) + 2.0f * (s[1][k] - s[1][k + 2])) + (s[2][k] - s[2][k + 2]);
      const float dy = ((s[0][k] - s[2][k]) + 2.0f * (s[0][k + 1] - s[2][k + 1])) + (s[0][k + 2] - s[2][k + 2]);
      const float inv = 1.0f / sqrtf((dx * dx + dy * dy) + 1.0f);     // one IEEE division, three products (<= 2.5 eps in all)
      float *o = stage + ty * (3 * DP_TW) + 3 * (tx + k);
      o[0] = dx * inv;
      o[1] = dy * inv;
      o[2] = -inv;
    }
    __syncthreads();
    dp_store_rows(stage, normals, pix0, w, valid_w, rows, vec != 0);
  }
}

__global__ __launch_bounds__(256) void depth_align_fill_kernel(unsigned *__restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out[i] = DA_SENTINEL;
}

__global__ __launch_bounds__(256) void depth_align_finish_kernel(unsigned *__restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total && out[i] == DA_SENTINEL) out[i] = 0u;
}

struct DaCamera {
  float cx, cy, fx, fy;
};

// The splat behind a tile-local z-buffer: a workgroup takes 64 x 16 source pixels (a thread: one column, four rows),
// finds the smallest target column / row any of them offers, resolves every target inside the DL_WW x DL_WH window that
// starts there with LDS atomics, and sends one global atomicMin per window pixel that was written (targets outside the
// window -- a depth edge whose parallax throws them far -- go to global memory directly).  The minimum is order-free, so
// the result does not depend on which path a target took.  Measured on 16 frames of 480x640 against one global
// atomicMin per target (up to four per source): 0.026 ms instead of 0.170 ms per launch, the same bits.
constexpr int DL_SW = 64, DL_SH = 16, DL_ROWS = DL_SH / 4;
constexpr int DL_WW = 96, DL_WH = 24;

template <typename T>
__global__ __launch_bounds__(256) void depth_align_splat_kernel(const T *__restrict__ depth, int h, int w, int tiles_x,
                                                                    int tiles_y, const float *__restrict__ u_tab,
                                                                    const float *__restrict__ v_tab, float z_scale,
                                                                    DaCamera cam, const float *__restrict__ rot,
                                                                    const float *__restrict__ trans,
                                                                    unsigned *__restrict__ out) {
  __shared__ unsigned win[DL_WH * DL_WW];
  __shared__ int org[2];
  const unsigned tile = blockIdx.x;
  const int txi = (int)(tile % (unsigned)tiles_x);
  const unsigned rest = tile / (unsigned)tiles_x;
  const int tyi = (int)(rest % (unsigned)tiles_y);
  const long long frame = rest / (unsigned)tiles_y;
  for (int i = threadIdx.x; i < DL_WH * DL_WW; i += 256) win[i] = DA_SENTINEL;
  if (threadIdx.x < 2) org[threadIdx.x] = 0x7FFFFFFF;
  __syncthreads();

  const int sx = txi * DL_SW + (int)(threadIdx.x & 63);
  const float r0 = rot[0], r1 = rot[1], r2 = rot[2], r3 = rot[3], r4 = rot[4], r5 = rot[5], r6 = rot[6], r7 = rot[7], r8 = rot[8];
  const float t0 = trans[0], t1 = trans[1], t2 = trans[2];
  unsigned bits[DL_ROWS];
  int tx0[DL_ROWS], tx1[DL_ROWS], ty0[DL_ROWS], ty1[DL_ROWS];
  bool live[DL_ROWS];
  int minx = 0x7FFFFFFF, miny = 0x7FFFFFFF;
#pragma unroll
  for (int k = 0; k < DL_ROWS; ++k) {
    const int sy = tyi * DL_SH + (int)(threadIdx.x >> 6) + 4 * k;
    live[k] = false;
    if (sx < w && sy < h) {
      const float d = dp_load(depth + (frame * h + sy) * w + sx);
      if (d > 0.0f && d < 10000.0f) {
        const float X = d * u_tab[sx], Y = d * v_tab[sy], Z = d * z_scale;
        const float x = ((X * r0 + Y * r3) + Z * r6) + t0;
        const float y = ((X * r1 + Y * r4) + Z * r7) + t1;
        const float z = ((X * r2 + Y * r5) + Z * r8) + t2;
        float px = x / z * cam.fx + cam.cx;
        float py = y / z * cam.fy + cam.cy;
        if (z == 0.0f) px = py = 0.0f;
        if (px >= 0.0f && px < (float)w && py >= 0.0f && py < (float)h) {
          live[k] = true;
          bits[k] = __float_as_uint(d);
          tx0[k] = (int)(px - 0.5f);
          tx1[k] = (int)(px + 0.5f);
          ty0[k] = (int)(py - 0.5f);
          ty1[k] = (int)(py + 0.5f);
          minx = min(minx, tx0[k]);
          miny = min(miny, ty0[k]);
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    minx = min(minx, __shfl_xor(minx, o, 64));
    miny = min(miny, __shfl_xor(miny, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&org[0], minx);
    atomicMin(&org[1], miny);
  }
  __syncthreads();
  const int ox = org[0], oy = org[1];
  unsigned *o = out + frame * h * w;
  auto offer = [&](int tx, int ty, unsigned b) {       // 0 <= tx - ox, 0 <= ty - oy by construction
    const int lx = tx - ox, ly = ty - oy;
    if (lx < DL_WW && ly < DL_WH)
      atomicMin(&win[ly * DL_WW + lx], b);
    else
      atomicMin(o + (long long)ty * w + tx, b);
  };
#pragma unroll
  for (int k = 0; k < DL_ROWS; ++k) {
    if (!live[k]) continue;
    const bool ex = tx1[k] != tx0[k] && tx1[k] < w, ey = ty1[k] != ty0[k] && ty1[k] < h;
    offer(tx0[k], ty0[k], bits[k]);
    if (ex) offer(tx1[k], ty0[k], bits[k]);
    if (ey) offer(tx0[k], ty1[k], bits[k]);
    if (ex && ey) offer(tx1[k], ty1[k], bits[k]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DL_WH * DL_WW; i += 256) {
    const unsigned v = win[i];
    if (v != DA_SENTINEL) {                             // written, hence a target inside the frame
      const int ly = i / DL_WW, lx = i - ly * DL_WW;
      atomicMin(o + (long long)(oy + ly) * w + (ox + lx), v);
    }
  }
}

int dp_shape_status(int batch, int h, int w) {
  if (batch < 1 || h < 1 || w < 1) return MI_E_SHAPE;
  if ((long long)batch * h * w >= (1ll << 31)) return MI_E_SHAPE;
  return MI_OK;
}

}  // namespace

extern "C" int mi_depth_to_points(const void *depth, int depth_is_u16, int batch, int h, int w, const float *u_tab,
                                  const float *v_tab, float z_scale, float *out_points, float *out_normals,
                                  mi_stream_t stream) {
  MI_ENTER();
  if (!depth || !u_tab || !v_tab || !out_points) return MI_E_NULL;
  if (const int e = dp_shape_status(batch, h, w)) return e;
  if (depth_is_u16 != 0 && depth_is_u16 != 1) return MI_E_PARAM;
  if ((uintptr_t)depth % (depth_is_u16 ? 2 : 4) != 0 || (uintptr_t)u_tab % 4 != 0 || (uintptr_t)v_tab % 4 != 0 ||
      (uintptr_t)out_points % 4 != 0 || (uintptr_t)out_normals % 4 != 0)
    return MI_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int tiles_x = ceil_div(w, DP_TW), tiles_y = ceil_div(h, DP_TH);
  const long long tiles = (long long)batch * tiles_x * tiles_y;       // < 2^31: every tile holds a pixel
  const int vec = (w % 4 == 0 && (uintptr_t)out_points % 16 == 0 && (uintptr_t)out_normals % 16 == 0) ? 1 : 0;
  const dim3 grid((unsigned)tiles), block(DP_THREADS);
  if (depth_is_u16) {
    const uint16_t *d = static_cast<const uint16_t *>(depth);
    if (out_normals)
      hipLaunchKernelGGL((depth_points_kernel<uint16_t, true>), grid, block, 0, s, d, h, w, tiles_x, tiles_y, u_tab, v_tab,
                         z_scale, out_points, out_normals, vec);
    else
      hipLaunchKernelGGL((depth_points_kernel<uint16_t, false>), grid, block, 0, s, d, h, w, tiles_x, tiles_y, u_tab, v_tab,
                         z_scale, out_points, out_normals, vec);
  } else {
    const float *d = static_cast<const float *>(depth);
    if (out_normals)
      hipLaunchKernelGGL((depth_points_kernel<float, true>), grid, block, 0, s, d, h, w, tiles_x, tiles_y, u_tab, v_tab,
                         z_scale, out_points, out_normals, vec);
    else
      hipLaunchKernelGGL((depth_points_kernel<float, false>), grid, block, 0, s, d, h, w, tiles_x, tiles_y, u_tab, v_tab,
                         z_scale, out_points, out_normals, vec);
  }
  return mi_launch_status();
}

extern "C" int mi_depth_align(const void *depth, int depth_is_u16, int batch, int h, int w, const float *u_tab,
                              const float *v_tab, float z_scale, float rgb_cx, float rgb_cy, float rgb_fx, float rgb_fy,
                              const float *rotation, const float *translation, float *out, mi_stream_t stream) {
  MI_ENTER();
  if (!depth || !u_tab || !v_tab || !rotation || !translation || !out) return MI_E_NULL;
  if (const int e = dp_shape_status(batch, h, w)) return e;
  if (depth_is_u16 != 0 && depth_is_u16 != 1) return MI_E_PARAM;
  if ((uintptr_t)depth % (depth_is_u16 ? 2 : 4) != 0 || (uintptr_t)u_tab % 4 != 0 || (uintptr_t)v_tab % 4 != 0 ||
      (uintptr_t)rotation % 4 != 0 || (uintptr_t)translation % 4 != 0 || (uintptr_t)out % 4 != 0)
    return MI_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long total = (long long)batch * h * w;
  unsigned *zbuf = reinterpret_cast<unsigned *>(out);
  const dim3 flat((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(depth_align_fill_kernel, flat, block, 0, s, zbuf, total);
  MI_CHECK_LAUNCH();
  const int tiles_x = ceil_div(w, DL_SW), tiles_y = ceil_div(h, DL_SH);
  const dim3 grid((unsigned)((long long)batch * tiles_x * tiles_y));
  const DaCamera cam{rgb_cx, rgb_cy, rgb_fx, rgb_fy};
  if (depth_is_u16)
    hipLaunchKernelGGL(depth_align_splat_kernel<uint16_t>, grid, block, 0, s, static_cast<const uint16_t *>(depth), h, w,
                       tiles_x, tiles_y, u_tab, v_tab, z_scale, cam, rotation, translation, zbuf);
  else
    hipLaunchKernelGGL(depth_align_splat_kernel<float>, grid, block, 0, s, static_cast<const float *>(depth), h, w, tiles_x,
                       tiles_y, u_tab, v_tab, z_scale, cam, rotation, translation, zbuf);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(depth_align_finish_kernel, flat, block, 0, s, zbuf, total);
  return mi_launch_status();
}
