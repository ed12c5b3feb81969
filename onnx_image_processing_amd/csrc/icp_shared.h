// What the dense linearisations share: K18 (icp.hip) and K21 (photo.hip).
//
// The slab reduction (K18r, K21r).  Grid (slabs, pairs), 256 threads; a slab is ICP_SLAB = 2048 consecutive SAMPLED pixels of
// the stride's grid (row-major over ceil(h / s) x ceil(w / s)): a function of (h, w, s) only.  Lane l takes the samples
// l, l + 256, ... of its slab in this order (ICP_PER_LANE = 8 of them) into 28 float32 accumulators and an integer count.
// Both kernels are the same sequence around their own ROW, the one thing in which they differ: the pose in float32 (r / t, or
// the workspace's float64 pose rounded to float32), then per sample
//   icp_sample_pixel   sample `it` of the lane: whether it exists, and its source pixel at a clamped, always valid address
//   (the row)          the kernel's own: from the source pixel, `in`, R, T and the camera to ok, J[6] and res.  K18: normal
//                      rotation, icp_project, the gather of frame 2's surfel, icp_row.  K21: photo_footprint, the four
//                      footprint records and the nearest vertex, photo_row.  A gather is clamped to a valid address as well,
//                      so the eight iterations carry no branch and their loads overlap.
//   (the sums)         zeros for a rejected row, icp_accumulate, the count; and at the end
//   icp_store_slab     wave_sum_dpp per accumulator, the 4 waves through LDS in wave order in float64, and the 29 float64
//                      partials stored with plain stores into the slab's 256-byte record.  No atomics.
// The loop over the lane's samples is written out in each kernel, around its row, and is not a template over a row functor:
// a loop or a row that reaches the kernel through an inlined callee keeps a branch per sample and loses the overlap of the
// next sample's streamed loads with the current gather (32 waits on memory for 19; DESIGN.md, K21, "Reduction").
// The pose load and the zero-and-accumulate step are written out too: as helpers they cost K18r 2 and K21r 6 VGPRs.
// The two terms are not fused into one kernel either: 56 accumulators would cost K18r a wave per SIMD (ibid., "Layout").
//
// The solve step (K18s, K21s): icp_column_sum, icp_step and icp_write_pose; K21s forms its joint sums between the first and
// the second.  Host side: the workspace (one carve; K18 has one slab array, K21 two), the checks, the slab geometry of a
// launch (icp_reduce_job) and the refine driver.  K18i and K18r live in icp.hip alone; K21 reaches them through
// icp_init_launch / icp_reduce_launch.
#pragma once
#include "common.h"
#include "icp_math.h"

#include <math.h>

struct IcpCam {
  float fx, fy, cx, cy;
};

// One launch of a slab reduction, beside its maps and gates.  The pose comes from r / t (float32: the linearise entries)
// or, when pose64 is given, from the workspace's float64 pose (the refine entries); state: the freeze words, or null.
struct IcpReduceJob {
  const float *r, *t;
  const double *pose64;
  const int *state;
  int h, w, stride, ws, samples, nslabs, max_slabs;          // ws, samples, nslabs: icp_reduce_job's, from (h, w, stride)
  IcpCam cam;
  double *slabs;                                             // slabs[(pair * max_slabs + slab) * ICP_REC ...]
};

// K18r's maps and gates: the surfel maps of both frames, the squared distance gate and the cosine of the angle gate.
struct IcpMaps {
  const float4 *vertex1, *normal1, *vertex2, *normal2;
  float thr2, cos_thr;
};

// K18i over `batch` pairs and K18r over the job's slabs, defined in icp.hip.
int icp_init_launch(const float *r0, const float *t0, int batch, double *pose, int *state, int *steps, hipStream_t s);
int icp_reduce_launch(const IcpMaps &m, const IcpReduceJob &job, int batch, hipStream_t s);

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_PER_LANE = 8;
constexpr int ICP_SLAB = ICP_THREADS * ICP_PER_LANE;       // sampled pixels per workgroup
constexpr int ICP_REC = 32;                                // doubles per slab record (29 used)

enum { ICP_MODE_STEP = 0, ICP_MODE_SUMS = 1, ICP_MODE_FINAL = 2 };   // of K18s and K21s

// ---- the slab reduction (K18r, K21r) ---------------------------------------------------------------------------------------
// sample it * ICP_THREADS + tid of `slab`: *in when it is one of the stride's `samples` (ws of them per row), and the offset
// of its source pixel in a w-wide frame; a sample past the end gets pixel 0
__device__ __forceinline__ size_t icp_sample_pixel(int slab, int it, int tid, int samples, int ws, int stride, int w, bool *in) {
  const int s = slab * ICP_SLAB + it * ICP_THREADS + tid;
  *in = s < samples;
  const int sc = *in ? s : 0;                                // a clamped, always valid address
  const int ys = sc / ws, xs = sc - ys * ws;
  return (size_t)(ys * stride) * (size_t)w + (size_t)(xs * stride);
}

// the workgroup's 28 sums and its count into the slab's record `rec`; part: the workgroup's 4 x ICP_REC doubles of LDS
__device__ __forceinline__ void icp_store_slab(const float *acc, int count, double (*part)[ICP_REC], double *__restrict__ rec) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 28; ++k) {
    const float sum = wave_sum_dpp(acc[k]);
    if (lane == 0) part[wave][k] = (double)sum;
  }
  int c = count;                                             // integers: exact in any order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) part[wave][28] = (double)c;
  __syncthreads();
  if (tid < ICP_SUMS) rec[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// ---- the solve step (K18s, K21s) -------------------------------------------------------------------------------------------
// column `lane` (< ICP_SUMS) of pair b's slab records, added in slab order
__device__ __forceinline__ double icp_column_sum(const double *__restrict__ slabs, int b, int nslabs, int max_slabs, int lane) {
  double a = 0.0;
  for (int k = 0; k < nslabs; ++k) a += slabs[((size_t)b * max_slabs + k) * ICP_REC + lane];
  return a;
}

// mode STEP, one lane: solve the sums s and move pair b's pose; a failed solve or a pose that is not finite freezes the pair
__device__ __forceinline__ void icp_step(const double *s, int min_count, int b, double *__restrict__ pose, int *__restrict__ state,
                                         int *__restrict__ steps) {
  double x[6], ratio;
  if (icp_solve(s, min_count, x, &ratio)) {
    double p[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) p[k] = pose[(size_t)b * 12 + k];
    icp_update_pose(p, x);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) finite = finite && fabs(p[k]) < INFINITY;
    if (finite) {
#pragma unroll
      for (int k = 0; k < 12; ++k) pose[(size_t)b * 12 + k] = p[k];
      steps[b] += 1;
      return;
    }
  }
  state[b] = 1;
}

// mode FINAL, one lane: pair b's pose in float32 and the 6x6 information matrix of the sums s (zeros unless `finite`)
__device__ __forceinline__ void icp_write_pose(const double *s, bool finite, int b, const double *__restrict__ pose,
                                               float *__restrict__ r, float *__restrict__ t, float *__restrict__ information) {
  for (int k = 0; k < 9; ++k) r[(size_t)b * 9 + k] = (float)pose[(size_t)b * 12 + k];
  for (int k = 0; k < 3; ++k) t[(size_t)b * 3 + k] = (float)pose[(size_t)b * 12 + 9 + k];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      const float v = finite ? (float)s[k] : 0.0f;
      information[(size_t)b * 36 + i * 6 + j] = v;
      information[(size_t)b * 36 + j * 6 + i] = v;
      ++k;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline int icp_shape_status(int batch, int h, int w) {
  if (batch < 1 || h < 3 || w < 3) return MI_E_SHAPE;
  if (batch > 65535) return MI_E_PARAM;
  if ((long long)batch * h * w >= 0x80000000LL) return MI_E_SHAPE;
  return MI_OK;
}
inline bool icp_stride_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }
inline bool icp_positive(float v) { return v > 0.0f && v < INFINITY; }
inline int icp_gate_status(float fx, float fy, float cx, float cy, float distance_threshold, float angle_threshold) {
  if (!icp_positive(fx) || !icp_positive(fy) || !(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY) ||
      !icp_positive(distance_threshold) || !(angle_threshold > 0.0f) || !(angle_threshold <= 3.14159274f))
    return MI_E_PARAM;
  return MI_OK;
}
inline int icp_schedule_status(const int32_t *strides, const int32_t *iterations, int stages, int min_correspondences) {
  if (stages < 1 || stages > MI_ICP_MAX_STAGES || min_correspondences < 1) return MI_E_PARAM;
  int all = 0;
  for (int i = 0; i < stages; ++i) {
    if (!icp_stride_ok(strides[i]) || iterations[i] < 0 || iterations[i] > MI_ICP_MAX_ITERATIONS) return MI_E_PARAM;
    all += iterations[i];
  }
  return all > MI_ICP_MAX_ITERATIONS ? MI_E_PARAM : MI_OK;
}

inline IcpMaps icp_maps(const float *vertex1, const float *normal1, const float *vertex2, const float *normal2,
                        float distance_threshold, float angle_threshold) {
  return IcpMaps{reinterpret_cast<const float4 *>(vertex1), reinterpret_cast<const float4 *>(normal1),
                 reinterpret_cast<const float4 *>(vertex2), reinterpret_cast<const float4 *>(normal2),
                 distance_threshold * distance_threshold, (float)cos((double)angle_threshold)};
}

// The slabs of `stride`: ICP_SLAB consecutive sampled pixels of the stride's grid, row-major over ceil(h / s) x ceil(w / s).
inline IcpReduceJob icp_reduce_job(const float *r, const float *t, const double *pose64, const int *state, int h, int w, int stride,
                                   IcpCam cam, int max_slabs, double *slabs) {
  IcpReduceJob j{r, t, pose64, state, h, w, stride, 0, 0, 0, max_slabs, cam, slabs};
  j.ws = ceil_div(w, stride);
  j.samples = ceil_div(h, stride) * j.ws;
  j.nslabs = ceil_div(j.samples, ICP_SLAB);
  return j;
}

// The workspace of mi_icp_* (slab_arrays = 1) and of mi_rgbd_* / mi_photo_* (2: geometric, then photometric).
struct IcpWork {
  double *pose, *slabs[2];
  int *state, *steps;
  int max_slabs;
  size_t total;
};
inline IcpWork icp_carve(void *ws, int batch, int h, int w, int slab_arrays) {
  char *base = static_cast<char *>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
  IcpWork k = {};
  k.max_slabs = ceil_div(h * w, ICP_SLAB);                   // stride 1
  k.pose = reinterpret_cast<double *>(take((size_t)batch * 12 * sizeof(double)));
  for (int a = 0; a < slab_arrays; ++a)
    k.slabs[a] = reinterpret_cast<double *>(take((size_t)batch * k.max_slabs * ICP_REC * sizeof(double)));
  k.state = reinterpret_cast<int *>(take((size_t)batch * sizeof(int)));
  k.steps = reinterpret_cast<int *>(take((size_t)batch * sizeof(int)));
  k.total = off;
  return k;
}

// The refinement's launches: linearise(stride, mode) for every iteration of every stage in mode STEP, then once more at the
// last stage's stride in mode FINAL.
template <class Linearise>
int icp_refine_drive(const int32_t *strides, const int32_t *iterations, int stages, Linearise linearise) {
  for (int st = 0; st < stages; ++st)
    for (int it = 0; it < iterations[st]; ++it)
      if (const int e = linearise(strides[st], ICP_MODE_STEP)) return e;
  return linearise(strides[stages - 1], ICP_MODE_FINAL);
}

}  // namespace
