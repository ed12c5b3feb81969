// K35 disparity post-filters (include/mi355x_match_filter.h): connected components of a frame, the speckle filter and the median,
// batched under K33's contract.  The arithmetic and the union-find are csrc/filter_math.h's.
//
// K35a  ft_local_kernel<T>    one workgroup of four waves labels a 64 x 16 tile in LDS.  A wave owns four rows with the row in its
//       lanes: a ballot of "joined to the left" gives every pixel the start of its run without a loop, so a row costs no union at
//       all; unions are made only between rows, and only where the pixel to the left does not imply the same one (ft_implied): a
//       constant tile makes 15.  Every pixel then finds its local root (read-only), the local counts are added up in LDS, one add
//       per wave and row where the whole row has one root.  Written out: parent = the frame index of the local root (-1 on an
//       invalid pixel), count = the local component's size at the local root and 0 elsewhere.  Both arrays are the workspace; every
//       word is written here, so it may hold anything on entry.
// K35b  ft_border_kernel<T>   one thread per pixel pair across a tile border: the unions between tiles, on global memory with
//       atomicMin, again only where the pair before it along the border does not imply it.
// K35c  ft_count_kernel       one thread per pixel; a local root that is not the root of its component finds the root, hangs itself
//       under it and adds its local count there: one atomicAdd per local component and tile, never one per pixel.
// K35d  ft_labels_kernel / ft_speckle_kernel   one thread per pixel: at most two hops to the root, then the outputs.
// K35e  ft_median_kernel<K>   one thread per pixel, the taps through the L1, the keys in registers.
// Integer atomics only, on a minimum and on a count: nothing depends on the order of arrival; bitwise reproducible.
// Every device loop is ft_find's or ft_unite's: bounded by the strictly decreasing chain and capped at h * w trips.
#include "common.h"
#include "filter_math.h"

#include <math.h>

namespace {

constexpr int FT_WAVES = 4;
constexpr int FT_ROWS = FT_TILE_H / FT_WAVES;                               // rows of a tile per wave

// the forest of one tile in LDS
struct FtLdsMem {
  int *p;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ void store(int i, int v) { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int atomic_min(int i, int v) { return atomicMin(p + i, v); }
};
// the forest of one frame in global memory: loads that another compute unit's atomicMin must reach go past the L1
struct FtGlobalMem {
  int *p;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void store(int i, int v) { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int atomic_min(int i, int v) { return atomicMin(p + i, v); }
};

__device__ __forceinline__ float ft_lane_up(float v) { return __shfl_up(v, 1); }
__device__ __forceinline__ uint8_t ft_lane_up(uint8_t v) { return (uint8_t)__shfl_up((int)v, 1); }
__device__ __forceinline__ bool ft_lane_up(bool v) { return __shfl_up((int)v, 1) != 0; }

template <typename T>
__global__ __launch_bounds__(64 * FT_WAVES) void ft_local_kernel(const T *__restrict__ values, int h, int w, int tiles_x, int tiles_y,
                                                                 FtRule rule, int *__restrict__ parent, int *__restrict__ count) {
  __shared__ int lab[FT_TILE], cnt[FT_TILE];
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x), rest = (int)(blockIdx.x / (unsigned)tiles_x);
  const int ty = rest % tiles_y;
  const size_t frame = (size_t)(rest / tiles_y) * h * w;
  values += frame;
  parent += frame;
  count += frame;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cap = h * w;
  const int x = tx * FT_TILE_W + lane, row0 = wave * FT_ROWS;
  FtLdsMem mem{lab};
  // the wave's rows and the one below them; ok[j] is "inside the tile and the frame, and valid"
  T v[FT_ROWS + 1];
  bool ok[FT_ROWS + 1], left[FT_ROWS + 1];
#pragma unroll
  for (int j = 0; j <= FT_ROWS; ++j) {
    const int r = row0 + j, y = ty * FT_TILE_H + r;
    const bool inside = x < w && y < h && r < FT_TILE_H;
    v[j] = inside ? values[(size_t)y * w + x] : T(0);
    ok[j] = inside && ft_valid(v[j], rule);
    const T v_left = ft_lane_up(v[j]);
    const bool ok_left = ft_lane_up(ok[j]);
    left[j] = lane > 0 && ok[j] && ok_left && ft_near(v_left, v[j], rule);
  }
#pragma unroll
  for (int j = 0; j < FT_ROWS; ++j) {
    const int e = (row0 + j) * FT_TILE_W + lane;
    const uint64_t joined_left = __ballot(left[j]);
    lab[e] = ok[j] ? (row0 + j) * FT_TILE_W + ft_run_start(joined_left, lane) : -1;
    cnt[e] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FT_ROWS; ++j) {
    const int e = (row0 + j) * FT_TILE_W + lane;
    const bool down = ok[j] && ok[j + 1] && ft_near(v[j], v[j + 1], rule);
    const bool before_down = lane > 0 && ft_lane_up(down);
    if (down && !ft_implied(left[j], left[j + 1], before_down)) ft_unite(mem, e, e + FT_TILE_W, cap);
  }
  __syncthreads();
  int root[FT_ROWS];
#pragma unroll
  for (int j = 0; j < FT_ROWS; ++j) root[j] = ok[j] ? ft_find(mem, (row0 + j) * FT_TILE_W + lane, cap) : -1;    // nothing writes the forest now
#pragma unroll
  for (int j = 0; j < FT_ROWS; ++j) {
    const uint64_t active = __ballot(ok[j]);
    if (active == 0) continue;
    const int lead = __ffsll((long long)active) - 1, lead_root = __shfl(root[j], lead);
    if (__ballot(ok[j] && root[j] == lead_root) == active) {
      if (lane == lead) atomicAdd(&cnt[lead_root], __popcll(active));
    } else if (ok[j]) {
      atomicAdd(&cnt[root[j]], 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FT_ROWS; ++j) {
    const int r = row0 + j, y = ty * FT_TILE_H + r, e = r * FT_TILE_W + lane;
    if (x >= w || y >= h) continue;
    const size_t p = (size_t)y * w + x;
    parent[p] = ok[j] ? ft_global_index(root[j], ty, tx, w) : -1;
    count[p] = (ok[j] && root[j] == e) ? cnt[e] : 0;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ft_border_kernel(const T *__restrict__ values, int h, int w, int pairs, long long total, FtRule rule,
                                                        int *parent) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t frame = (size_t)(i / pairs) * h * w;
  int a, b, step;
  bool same_tiles;
  ft_border_pair((int)(i % pairs), h, w, &a, &b, &step, &same_tiles);
  if (!ft_border_union_wanted(values + frame, a, b, step, same_tiles, rule)) return;
  FtGlobalMem mem{parent + frame};
  ft_unite(mem, a, b, h * w);
}

__global__ __launch_bounds__(256) void ft_count_kernel(int *parent, int *count, int hw, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % hw);
  const int c = count[i];                       // > 0 on local roots only; only the root of a component is added to, and it skips below
  if (c <= 0) return;
  FtGlobalMem mem{parent + (i - q)};
  const int r = ft_find(mem, q, hw);
  if (r == q) return;
  mem.store(q, r);                              // a smaller element of the same set: the next kernel reaches the root in two hops
  atomicAdd(count + (i - q) + r, c);
}

__global__ __launch_bounds__(256) void ft_labels_kernel(int *parent, const int *__restrict__ count, int hw, long long total,
                                                        int32_t *__restrict__ labels, int32_t *__restrict__ sizes) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % hw);
  FtGlobalMem mem{parent + (i - q)};
  const bool valid = parent[i] >= 0;
  const int r = valid ? ft_find(mem, q, hw) : MI_FILTER_NO_LABEL;
  labels[i] = r;
  if (sizes) sizes[i] = valid ? count[(i - q) + r] : 0;
}

__global__ __launch_bounds__(256) void ft_speckle_kernel(const float *in, int *parent, const int *__restrict__ count, int hw, long long total,
                                                         int max_size, float invalid_value, float *out, uint8_t *__restrict__ removed) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % hw);
  FtGlobalMem mem{parent + (i - q)};
  const bool valid = parent[i] >= 0;
  const float v = in[i];                        // out may be in: this thread alone reads and writes element i
  const bool keep = ft_speckle_keeps(valid, valid ? count[(i - q) + ft_find(mem, q, hw)] : 0, max_size);
  out[i] = keep ? v : invalid_value;
  if (removed) removed[i] = (uint8_t)(valid && !keep);
}

template <int K>
__global__ __launch_bounds__(256) void ft_median_kernel(const float *__restrict__ in, int h, int w, long long total, float min_valid,
                                                        float invalid_value, float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long row = i / w;
  const int x = (int)(i - row * w), y = (int)(row % h);
  out[i] = ft_median<K>(in + (row - y) * w, h, w, y, x, min_valid, invalid_value);
}

inline bool ft_aligned(const void *p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

// MI_E_SHAPE / MI_E_PARAM of a frame batch; *pixels = batch h w (below MI_FILTER_MAX_PIXELS)
inline int ft_frames_status(int batch, int h, int w, long long *pixels) {
  if (batch < 1 || h < 1 || w < 1) return MI_E_SHAPE;
  const long long rows = (long long)batch * h;
  if (rows >= MI_FILTER_MAX_PIXELS || rows * w >= MI_FILTER_MAX_PIXELS) return MI_E_PARAM;
  *pixels = rows * w;
  return MI_OK;
}

// the rule of a call, or false for parameters the header refuses
inline bool ft_rule(int type, float min_valid, float max_diff, FtRule *rule) {
  if (!(max_diff >= 0.0f) || !(max_diff < INFINITY) || min_valid != min_valid) return false;
  rule->min_valid = min_valid;
  rule->max_diff = max_diff;
  rule->min_valid_u8 = rule->max_diff_u8 = 0;
  if (type == MI_FILTER_F32) return true;
  if (type != MI_FILTER_U8) return false;
  if (!(min_valid >= 0.0f) || min_valid > 256.0f || max_diff > 255.0f || min_valid != floorf(min_valid) || max_diff != floorf(max_diff)) return false;
  rule->min_valid_u8 = (int)min_valid;
  rule->max_diff_u8 = (int)max_diff;
  return true;
}

inline unsigned ft_blocks(long long n) { return (unsigned)((n + 255) / 256); }

// K35a to K35c: the forest and the counts of every frame into the workspace
template <typename T>
int ft_forest(const T *values, int batch, int h, int w, long long n, const FtRule &rule, int *parent, int *count, hipStream_t s) {
  const int tiles_x = (w + FT_TILE_W - 1) / FT_TILE_W, tiles_y = (h + FT_TILE_H - 1) / FT_TILE_H;
  const long long tiles = (long long)batch * tiles_y * tiles_x;
  hipLaunchKernelGGL(ft_local_kernel<T>, dim3((unsigned)tiles), dim3(64 * FT_WAVES), 0, s, values, h, w, tiles_x, tiles_y, rule, parent, count);
  MI_CHECK_LAUNCH();
  const int pairs = ft_border_pairs(h, w);                                 // a matter of the shape, not of the data
  if (pairs > 0) {
    const long long total = (long long)batch * pairs;
    hipLaunchKernelGGL(ft_border_kernel<T>, dim3(ft_blocks(total)), dim3(256), 0, s, values, h, w, pairs, total, rule, parent);
    MI_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ft_count_kernel, dim3(ft_blocks(n)), dim3(256), 0, s, parent, count, h * w, n);
  return mi_launch_status();
}

inline size_t ft_workspace_bytes(long long n) { return ((size_t)n * 8 + 15) / 16 * 16; }

}  // namespace

extern "C" size_t mi_filter_workspace_bytes(int batch, int h, int w) {
  long long n;
  return ft_frames_status(batch, h, w, &n) ? 0 : ft_workspace_bytes(n);
}

extern "C" int mi_filter_components(const void *values, int type, int batch, int h, int w, float min_valid, float max_diff, int32_t *labels,
                                    int32_t *sizes, void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!values || !labels || !workspace) return MI_E_NULL;
  long long n;
  if (const int st = ft_frames_status(batch, h, w, &n)) return st;
  FtRule rule;
  if (!ft_rule(type, min_valid, max_diff, &rule)) return MI_E_PARAM;
  if ((type == MI_FILTER_F32 && !ft_aligned(values, 4)) || !ft_aligned(labels, 4) || !ft_aligned(sizes, 4) || !ft_aligned(workspace, 16))
    return MI_E_ALIGN;
  if (workspace_bytes < ft_workspace_bytes(n)) return MI_E_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  int *parent = static_cast<int *>(workspace), *count = parent + n;
  const int st = type == MI_FILTER_U8 ? ft_forest(static_cast<const uint8_t *>(values), batch, h, w, n, rule, parent, count, s)
                                      : ft_forest(static_cast<const float *>(values), batch, h, w, n, rule, parent, count, s);
  if (st != MI_OK) return st;
  hipLaunchKernelGGL(ft_labels_kernel, dim3(ft_blocks(n)), dim3(256), 0, s, parent, count, h * w, n, labels, sizes);
  return mi_launch_status();
}

extern "C" int mi_filter_speckle(const float *in, int batch, int h, int w, float min_valid, float max_diff, int max_size, float invalid_value,
                                 float *out, uint8_t *removed, void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!in || !out || !workspace) return MI_E_NULL;
  long long n;
  if (const int st = ft_frames_status(batch, h, w, &n)) return st;
  FtRule rule;
  if (!ft_rule(MI_FILTER_F32, min_valid, max_diff, &rule) || max_size < 0 || invalid_value >= min_valid) return MI_E_PARAM;
  if (!ft_aligned(in, 4) || !ft_aligned(out, 4) || !ft_aligned(workspace, 16)) return MI_E_ALIGN;
  if (workspace_bytes < ft_workspace_bytes(n)) return MI_E_CAPACITY;
  hipStream_t s = (hipStream_t)stream;
  int *parent = static_cast<int *>(workspace), *count = parent + n;
  if (const int st = ft_forest(in, batch, h, w, n, rule, parent, count, s)) return st;
  hipLaunchKernelGGL(ft_speckle_kernel, dim3(ft_blocks(n)), dim3(256), 0, s, in, parent, count, h * w, n, max_size, invalid_value, out, removed);
  return mi_launch_status();
}

extern "C" int mi_filter_median(const float *in, int batch, int h, int w, int k, float min_valid, float invalid_value, float *out,
                                mi_stream_t stream) {
  MI_ENTER();
  if (!in || !out) return MI_E_NULL;
  long long n;
  if (const int st = ft_frames_status(batch, h, w, &n)) return st;
  if ((k != 3 && k != 5) || min_valid != min_valid || invalid_value >= min_valid || in == out) return MI_E_PARAM;
  if (!ft_aligned(in, 4) || !ft_aligned(out, 4)) return MI_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  if (k == 3)
    hipLaunchKernelGGL(ft_median_kernel<3>, dim3(ft_blocks(n)), dim3(256), 0, s, in, h, w, n, min_valid, invalid_value, out);
  else
    hipLaunchKernelGGL(ft_median_kernel<5>, dim3(ft_blocks(n)), dim3(256), 0, s, in, h, w, n, min_valid, invalid_value, out);
  return mi_launch_status();
}
