// K32 feature tracking (include/mi355x_match_flow.h): pyramidal Lucas-Kanade in the inverse form, the forward-backward test
// and the refill of lost slots, batched over frames under K30's contract.  The arithmetic is csrc/flow_math.h's.
//
// K32a  fl_convert_kernel / fl_down_kernel   level 0 from the frame; level l+1 from level l, one thread per output pixel
//                                            (25 reads that the L1 / L2 serve: neighbours share 15 of them).
// K32b  fl_track_kernel<NJ>                  one wave per keypoint, four waves to a workgroup, all levels in one launch.  Lane t
//       holds the template and both gradients of the window pixels t, t + 64, ... in registers (NJ = ceil((2r+1)^2 / 64) of
//       them, 21 registers at r = 10): no LDS.  Each iteration gathers frame 2's four neighbours per pixel through the L1
//       (a window is at most 23 x 23 floats and is re-read every iteration), folds b and |e| across the wave on the DPP path
//       and takes the step in every lane; all that decides a branch is wave-uniform, and a wave whose point converges or is
//       lost leaves at once.
// K32c  fl_check_kernel                      one thread per keypoint.
// K32d  fl_replenish_kernel                  one workgroup per image: cell winners by integer LDS atomicMin, ranks by ballot scans.
// fp32; built with -ffp-contract=off; no floating-point atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "flow_math.h"

#include <limits.h>
#include <math.h>

#include <atomic>

namespace {

constexpr int FL_WAVES = 4;

__global__ __launch_bounds__(256) void fl_convert_kernel(const void *__restrict__ gray, int is_u8, size_t n, float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = is_u8 ? (float)static_cast<const uint8_t *>(gray)[i] : static_cast<const float *>(gray)[i];
}

__global__ __launch_bounds__(256) void fl_down_kernel(const float *__restrict__ src, int h, int w, float *__restrict__ dst, int h2,
                                                      int w2) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (x >= w2 || y >= h2) return;
  dst[((size_t)b * h2 + y) * w2 + x] = fl_pyr_down(src + (size_t)b * h * w, h, w, y, x);
}

struct FlTrackArgs {
  FlLevels lv;
  int levels, k, radius, max_iterations;
  float eps2, min_eigen;
};

template <int NJ>
__global__ __launch_bounds__(64 * FL_WAVES) void fl_track_kernel(const float *__restrict__ pyr1, const float *__restrict__ pyr2,
                                                                 const float *__restrict__ kp1, const float *__restrict__ guess,
                                                                 FlTrackArgs a, float *__restrict__ kp2, uint8_t *__restrict__ status,
                                                                 uint8_t *__restrict__ code, float *__restrict__ residual,
                                                                 int *__restrict__ iterations) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int i = blockIdx.x * FL_WAVES + (threadIdx.x >> 6);            // wave-uniform
  if (i >= a.k) return;
  const size_t slot = (size_t)b * a.k + i;
  const float py = kp1[slot * 2], px = kp1[slot * 2 + 1];
  const float gy0 = guess ? guess[slot * 2] : 0.0f, gx0 = guess ? guess[slot * 2 + 1] : 0.0f;
  const int r = a.radius, n = (2 * r + 1) * (2 * r + 1);
  int lost = fl_input_lost(py, px, guess != nullptr, gy0, gx0, a.lv.h[0], a.lv.w[0]) ? MI_FLOW_PADDING : MI_FLOW_OK;
  const float top = 1.0f / (float)(1 << (a.levels - 1));
  float dx = gx0 * top, dy = gy0 * top, mean_abs = 0.0f;
  int its = 0;
  int qx[NJ], qy[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) fl_pixel(lane + 64 * j < n ? lane + 64 * j : 0, r, &qx[j], &qy[j]);
  for (int l = a.levels - 1; l >= 0 && lost == MI_FLOW_OK; --l) {
    const int h = a.lv.h[l], w = a.lv.w[l];
    const float *f1 = pyr1 + a.lv.off[l] + (size_t)b * h * w, *f2 = pyr2 + a.lv.off[l] + (size_t)b * h * w;
    const float scale = 1.0f / (float)(1 << l);
    const float cx = px * scale, cy = py * scale;
    float t[NJ], gx[NJ], gy[NJ], sxx = 0.0f, sxy = 0.0f, syy = 0.0f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      t[j] = gx[j] = gy[j] = 0.0f;
      if (lane + 64 * j < n) {
        fl_template(f1, h, w, cx, cy, qx[j], qy[j], &t[j], &gx[j], &gy[j]);
        sxx += gx[j] * gx[j];
        sxy += gx[j] * gy[j];
        syy += gy[j] * gy[j];
      }
    }
    const float gxx = wave_sum_dpp(sxx), gxy = wave_sum_dpp(sxy), gyy = wave_sum_dpp(syy);
    if (!(fl_min_eig(gxx, gxy, gyy, n) >= a.min_eigen)) {
      lost = MI_FLOW_FLAT;
      break;
    }
    const float det = gxx * gyy - gxy * gxy;
    for (int it = 0; it < a.max_iterations; ++it) {
      const float ox = cx + dx, oy = cy + dy;
      float sbx = 0.0f, sby = 0.0f, sab = 0.0f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (lane + 64 * j < n) {
          const float e = t[j] - fl_sample(f2, h, w, ox + (float)qx[j], oy + (float)qy[j]);
          sbx += e * gx[j];
          sby += e * gy[j];
          sab += fabsf(e);
        }
      const float bx = wave_sum_dpp(sbx), by = wave_sum_dpp(sby);
      mean_abs = wave_sum_dpp(sab) / (float)n;
      float sx, sy;
      fl_step(gxx, gxy, gyy, det, bx, by, &sx, &sy);
      dx += sx;
      dy += sy;
      ++its;
      if (sx * sx + sy * sy < a.eps2) break;
    }
    const float ex = cx + dx, ey = cy + dy;
    if (!fl_finite(ex) || !fl_finite(ey) || !fl_inside(ex, ey, h, w)) {
      lost = MI_FLOW_LEFT;
      break;
    }
    if (l > 0) {
      dx = 2.0f * dx;
      dy = 2.0f * dy;
    }
  }
  if (lane == 0) {
    const bool ok = lost == MI_FLOW_OK;
    kp2[slot * 2] = ok ? py + dy : -1.0f;
    kp2[slot * 2 + 1] = ok ? px + dx : -1.0f;
    status[slot] = ok ? 1 : 0;
    code[slot] = (uint8_t)lost;
    residual[slot] = ok ? mean_abs : 0.0f;
    iterations[slot] = ok ? its : 0;
  }
}

__global__ __launch_bounds__(256) void fl_check_kernel(const float *__restrict__ kp1, const float *__restrict__ back,
                                                       const uint8_t *__restrict__ sf, const uint8_t *__restrict__ sb, size_t n,
                                                       float max_distance, uint8_t *__restrict__ status, float *__restrict__ fb) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool both = sf[i] != 0 && sb[i] != 0;
  const float dy = back[2 * i] - kp1[2 * i], dx = back[2 * i + 1] - kp1[2 * i + 1];
  const float dist = sqrtf(dy * dy + dx * dx);
  status[i] = both && dist <= max_distance ? 1 : 0;
  fb[i] = both ? dist : INFINITY;
}

// ---- K32d -------------------------------------------------------------------------------------------------------------------
constexpr int FL_RT = 256;
extern __shared__ __align__(16) unsigned char fl_lds[];

// the number of set flags in the threads before this one, and in the whole block (256 threads, 4 waves); two barriers
__device__ __forceinline__ int fl_block_rank(bool flag, int *wave_tot, int &total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();                                                       // the previous round's readers are done
  if (lane == 0) wave_tot[wv] = __popcll(m);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int v = 0; v < FL_RT / 64; ++v) {
    if (v < wv) base += wave_tot[v];
    total += wave_tot[v];
  }
  return base + before;
}

__global__ __launch_bounds__(FL_RT) void fl_replenish_kernel(const float *__restrict__ kp, const uint8_t *__restrict__ st,
                                                             const float *__restrict__ cand, const int *__restrict__ cand_count, int k,
                                                             int n_cand, int h, int w, int cell, int cells_x, int cells,
                                                             float *__restrict__ kp_out, uint8_t *__restrict__ is_new,
                                                             int *__restrict__ counts) {
  int *win = reinterpret_cast<int *>(fl_lds);                            // cells: the lowest candidate index, -1 under a live keypoint
  int *lost_slot = win + cells;                                          // k: the lost slots in ascending order
  int *wave_tot = lost_slot + k;                                         // FL_RT / 64
  const int b = blockIdx.x, tid = threadIdx.x;
  kp += (size_t)b * k * 2;
  st += (size_t)b * k;
  cand += (size_t)b * n_cand * 2;
  kp_out += (size_t)b * k * 2;
  is_new += (size_t)b * k;
  for (int c = tid; c < cells; c += FL_RT) win[c] = INT_MAX;
  __syncthreads();
  int n_live = 0, n_lost = 0;
  for (int i0 = 0; i0 < k; i0 += FL_RT) {                                // block-uniform trip count
    const int i = i0 + tid;
    const bool in = i < k, live = in && st[i] != 0;
    float y = -1.0f, x = -1.0f;
    if (live) {
      y = kp[2 * i];
      x = kp[2 * i + 1];
      win[fl_cell(y, x, h, w, cell, cells_x)] = -1;                      // every writer stores the same value
    }
    if (in) {
      kp_out[2 * i] = y;
      kp_out[2 * i + 1] = x;
      is_new[i] = 0;
    }
    int tot;
    const int rank = fl_block_rank(in && !live, wave_tot, tot);
    if (in && !live) lost_slot[n_lost + rank] = i;
    n_lost += tot;
    n_live += min(FL_RT, k - i0) - tot;
  }
  __syncthreads();
  int nc = cand_count[b];
  nc = nc < 0 ? 0 : (nc > n_cand ? n_cand : nc);
  for (int i = tid; i < nc; i += FL_RT) {
    const float y = cand[2 * i], x = cand[2 * i + 1];
    if (fl_finite(y) && fl_finite(x) && y >= 0.0f && x >= 0.0f) atomicMin(&win[fl_cell(y, x, h, w, cell, cells_x)], i);
  }
  __syncthreads();
  int n_acc = 0;
  for (int i0 = 0; i0 < nc; i0 += FL_RT) {
    const int i = i0 + tid;
    float y = -1.0f, x = -1.0f;
    bool acc = false;
    if (i < nc) {
      y = cand[2 * i];
      x = cand[2 * i + 1];
      acc = fl_finite(y) && fl_finite(x) && y >= 0.0f && x >= 0.0f && win[fl_cell(y, x, h, w, cell, cells_x)] == i;
    }
    int tot;
    const int rank = n_acc + fl_block_rank(acc, wave_tot, tot);
    if (acc && rank < n_lost) {
      const int s = lost_slot[rank];
      kp_out[2 * s] = y;
      kp_out[2 * s + 1] = x;
      is_new[s] = 1;
    }
    n_acc += tot;
  }
  if (tid == 0) {
    counts[3 * b] = n_live;
    counts[3 * b + 1] = n_acc;
    counts[3 * b + 2] = n_acc < n_lost ? n_acc : n_lost;
  }
}

inline size_t fl_replenish_lds(int cells, int k) { return ((size_t)cells + (size_t)k + FL_RT / 64) * sizeof(int); }

// every pointer on a 4-byte boundary (null counts as aligned): the float and int32 arrays
inline bool fl_aligned4(std::initializer_list<const void *> ps) {
  for (const void *p : ps)
    if (((uintptr_t)p % 4) != 0) return false;
  return true;
}

inline int fl_batch_status(int batch, int k) {
  if (batch < 1 || k < 1) return MI_E_SHAPE;
  if (batch > 65535 || k > MI_FLOW_MAX_K) return MI_E_PARAM;
  return MI_OK;
}

template <int NJ>
int fl_launch_track(const float *pyr1, const float *pyr2, const float *kp1, const float *guess, int batch, const FlTrackArgs &a,
                    float *kp2, uint8_t *status, uint8_t *code, float *residual, int32_t *iterations, hipStream_t s) {
  hipLaunchKernelGGL(fl_track_kernel<NJ>, dim3((unsigned)ceil_div(a.k, FL_WAVES), (unsigned)batch), dim3(64 * FL_WAVES), 0, s, pyr1,
                     pyr2, kp1, guess, a, kp2, status, code, residual, iterations);
  return mi_launch_status();
}

}  // namespace

extern "C" size_t mi_flow_pyramid_bytes(int batch, int h, int w, int levels) {
  FlLevels lv;
  if (batch < 1 || batch > 65535 || h < 1 || w < 1 || h > 32768 || w > 32768 || !fl_levels(batch, h, w, levels, 1, &lv)) return 0;
  return (size_t)lv.total_bytes;
}

extern "C" int mi_flow_pyramid(const void *gray, int gray_is_u8, int batch, int h, int w, int levels, float *pyramid,
                               size_t pyramid_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!gray || !pyramid) return MI_E_NULL;
  if (batch < 1 || h < 1 || w < 1) return MI_E_SHAPE;
  FlLevels lv;
  if (batch > 65535 || h > 32768 || w > 32768 || !fl_levels(batch, h, w, levels, 1, &lv)) return MI_E_PARAM;
  if (((uintptr_t)pyramid % 16) != 0 || (!gray_is_u8 && ((uintptr_t)gray % 4) != 0)) return MI_E_ALIGN;
  if (pyramid_bytes < (size_t)lv.total_bytes) return MI_E_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)batch * h * w;
  hipLaunchKernelGGL(fl_convert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gray, gray_is_u8, n, pyramid);
  MI_CHECK_LAUNCH();
  for (int l = 1; l < levels; ++l) {
    hipLaunchKernelGGL(fl_down_kernel, dim3((unsigned)ceil_div(lv.w[l], 64), (unsigned)ceil_div(lv.h[l], 4), (unsigned)batch), dim3(256),
                       0, s, pyramid + lv.off[l - 1], lv.h[l - 1], lv.w[l - 1], pyramid + lv.off[l], lv.h[l], lv.w[l]);
    MI_CHECK_LAUNCH();
  }
  return MI_OK;
}

extern "C" int mi_flow_track(const float *pyr1, const float *pyr2, const float *keypoints1, const float *guess, int batch, int h,
                             int w, int levels, int k, int radius, int max_iterations, float epsilon, float min_eigen,
                             float *keypoints2, uint8_t *status, uint8_t *code, float *residual, int32_t *iterations,
                             mi_stream_t stream) {
  MI_ENTER();
  if (!pyr1 || !pyr2 || !keypoints1 || !keypoints2 || !status || !code || !residual || !iterations) return MI_E_NULL;
  if (h < 1 || w < 1) return MI_E_SHAPE;
  if (const int st = fl_batch_status(batch, k)) return st;
  FlTrackArgs a;
  if (radius < 1 || radius > MI_FLOW_MAX_RADIUS || h > 32768 || w > 32768 || !fl_levels(batch, h, w, levels, radius, &a.lv))
    return MI_E_PARAM;
  if (max_iterations < 1 || max_iterations > MI_FLOW_MAX_ITERATIONS) return MI_E_PARAM;
  if (!(epsilon > 0.0f) || !(epsilon < INFINITY) || !(min_eigen >= 0.0f) || !(min_eigen < INFINITY)) return MI_E_PARAM;
  if (!mi_aligned16({pyr1, pyr2}) || !fl_aligned4({keypoints1, guess, keypoints2, residual, iterations})) return MI_E_ALIGN;
  a.levels = levels;
  a.k = k;
  a.radius = radius;
  a.max_iterations = max_iterations;
  a.eps2 = epsilon * epsilon;
  a.min_eigen = min_eigen;
  hipStream_t s = (hipStream_t)stream;
  switch (ceil_div((2 * radius + 1) * (2 * radius + 1), 64)) {
    case 1: return fl_launch_track<1>(pyr1, pyr2, keypoints1, guess, batch, a, keypoints2, status, code, residual, iterations, s);
    case 2: return fl_launch_track<2>(pyr1, pyr2, keypoints1, guess, batch, a, keypoints2, status, code, residual, iterations, s);
    case 3: return fl_launch_track<3>(pyr1, pyr2, keypoints1, guess, batch, a, keypoints2, status, code, residual, iterations, s);
    case 4: return fl_launch_track<4>(pyr1, pyr2, keypoints1, guess, batch, a, keypoints2, status, code, residual, iterations, s);
    case 5: return fl_launch_track<5>(pyr1, pyr2, keypoints1, guess, batch, a, keypoints2, status, code, residual, iterations, s);
    case 6: return fl_launch_track<6>(pyr1, pyr2, keypoints1, guess, batch, a, keypoints2, status, code, residual, iterations, s);
    default: return fl_launch_track<7>(pyr1, pyr2, keypoints1, guess, batch, a, keypoints2, status, code, residual, iterations, s);
  }
}

extern "C" int mi_flow_check(const float *keypoints1, const float *keypoints_back, const uint8_t *status_fwd,
                             const uint8_t *status_bwd, int batch, int k, float max_distance, uint8_t *status, float *fb_distance,
                             mi_stream_t stream) {
  MI_ENTER();
  if (!keypoints1 || !keypoints_back || !status_fwd || !status_bwd || !status || !fb_distance) return MI_E_NULL;
  if (const int st = fl_batch_status(batch, k)) return st;
  if (!(max_distance >= 0.0f) || !(max_distance < INFINITY)) return MI_E_PARAM;
  if (!fl_aligned4({keypoints1, keypoints_back, fb_distance})) return MI_E_ALIGN;
  const size_t n = (size_t)batch * k;
  hipLaunchKernelGGL(fl_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keypoints1, keypoints_back,
                     status_fwd, status_bwd, n, max_distance, status, fb_distance);
  return mi_launch_status();
}

extern "C" int mi_flow_replenish(const float *keypoints, const uint8_t *status, const float *candidates, const int32_t *cand_count,
                                 int batch, int k, int n_cand, int h, int w, int cell, float *keypoints_out, uint8_t *is_new,
                                 int32_t *counts, mi_stream_t stream) {
  MI_ENTER();
  if (!keypoints || !status || !candidates || !cand_count || !keypoints_out || !is_new || !counts) return MI_E_NULL;
  if (n_cand < 1 || h < 1 || w < 1) return MI_E_SHAPE;
  if (const int st = fl_batch_status(batch, k)) return st;
  if (n_cand > MI_FLOW_MAX_CANDIDATES || h > 32768 || w > 32768 || cell < 1) return MI_E_PARAM;
  const long long cells_x = (w + cell - 1) / cell, cells_y = (h + cell - 1) / cell;
  if (cells_x * cells_y > MI_FLOW_MAX_CELLS) return MI_E_PARAM;
  if (!fl_aligned4({keypoints, candidates, cand_count, keypoints_out, counts})) return MI_E_ALIGN;
  const int cells = (int)(cells_x * cells_y);
  const size_t lds = fl_replenish_lds(cells, k);
  if (lds > 64 * 1024) {
    // More than the default 64 KB of dynamic LDS needs the kernel's attribute raised, once per DEVICE (the attribute belongs
    // to the device's copy of the function).  One bit per device; two threads that race here both set the same value.
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipGetLastError();
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (!(raised.load(std::memory_order_acquire) & bit)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fl_replenish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)fl_replenish_lds(MI_FLOW_MAX_CELLS, MI_FLOW_MAX_K));
      if (e != hipSuccess) return (int)e;
      raised.fetch_or(bit, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(fl_replenish_kernel, dim3((unsigned)batch), dim3(FL_RT), lds, (hipStream_t)stream, keypoints, status, candidates,
                     cand_count, k, n_cand, h, w, cell, (int)cells_x, cells, keypoints_out, is_new, counts);
  return mi_launch_status();
}
