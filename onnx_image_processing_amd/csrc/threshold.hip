// K14 thresholds (reference pytorch_model/threshold/): histogram -> Otsu / multi-Otsu threshold search -> apply.
// Batched over frames, every launch on `stream`, nothing read back, thresholds stay in device memory.
//
// K14a  th_hist_kernel     a workgroup takes 16 KB of one frame as 16-byte loads (a scalar head and tail where a frame
//       does not start or end on 16 bytes).  Each thread folds runs of equal neighbouring values into one (bin, count)
//       before it touches the histogram -- images repeat values, a constant frame is the worst case -- and adds into
//       a workgroup-private uint32 histogram in LDS that is replicated up to 8 times (copy = lane & 7, copies of one
//       bin in neighbouring banks), then flushes the non-empty bins with one 64-bit integer atomic each.  Above
//       TH_LDS_MAX_BINS bins the runs go to global memory directly.  Integer atomics only: bitwise reproducible.
// K14b  th_otsu_kernel     one workgroup per frame: totals, then a tiled int64 scan of hist and value * hist over the
//       bins, the float32 between-class score per bin in the reference's operation order, first-maximum reduction.
// K14c  multi-Otsu         th_prefix_kernel (the two int64 prefix sums, to the workspace) -> th_multi_search_kernel
//       (every thread unranks the first of a contiguous run of combination ranks and steps to the lexicographic
//       successor from there; the score of a candidate is O(n_class^2) from prefix sums in LDS, fp64 in a fixed order;
//       reduction on (score descending, rank ascending) through wave and workgroup to one partial per workgroup) ->
//       th_multi_finish_kernel (partials of a frame -> best rank -> thresholds).  No floating-point atomics, no
//       cross-workgroup waits.
// K14d  th_apply_kernel    one pass: label = number of thresholds below the pixel, or the two-valued image.
// Built with -ffp-contract=off and IEEE division (float32 and float64).
#include "common.h"

namespace {

constexpr int TH_THREADS = 256;
constexpr int TH_LDS_WORDS = 8192;            // 32 KB of uint32 counters per workgroup
constexpr int TH_LDS_MAX_BINS = 4096;         // above: global atomics (measured: DESIGN.md K14)
constexpr int TH_MAX_COPIES_LOG2 = 3;
constexpr int TH_VECS_PER_THREAD = 4;         // 16-byte loads per thread: 16 KB of frame per workgroup
constexpr int TH_MAX_BINS = MI_THRESHOLD_MAX_BINS;
constexpr int TH_MAX_CLASSES = MI_THRESHOLD_MAX_CLASSES;
constexpr int TH_MULTI_LDS_BINS = 2047;       // prefix sums of up to this many bins live in LDS (2 x 16 KB)
constexpr int TH_RANKS_PER_THREAD = 16;       // target run length of the combination sweep

__host__ __device__ inline int th_elem_size(int dtype) { return dtype == MI_PIX_U8 ? 1 : dtype == MI_PIX_U16 ? 2 : 4; }

// bin index of a value, -1 when it is not counted (outside [min_val, min_val + bins), NaN, beyond the int32 range)
template <typename T>
__device__ __forceinline__ int th_bin(T v, int min_val, int bins) {
  const long long d = (long long)v - min_val;
  return (d >= 0 && d < bins) ? (int)d : -1;
}
template <>
__device__ __forceinline__ int th_bin<float>(float v, int min_val, int bins) {
  if (!(fabsf(v) < 2147483648.0f)) return -1;           // NaN, infinities and what int32 cannot hold
  const long long d = (long long)(int)v - min_val;      // truncation toward zero, as .to(torch.int64)
  return (d >= 0 && d < bins) ? (int)d : -1;
}

struct ThLdsAcc {
  unsigned *h;
  int shift, copy;
  __device__ __forceinline__ void add(int bin, unsigned n) const { atomicAdd(&h[(bin << shift) + copy], n); }
};
struct ThGlobalAcc {
  unsigned long long *h;
  __device__ __forceinline__ void add(int bin, unsigned n) const { atomicAdd(&h[bin], (unsigned long long)n); }
};

// runs of equal bins become one add
template <typename Acc>
struct ThRun {
  int cur = -1;
  unsigned n = 0;
  __device__ __forceinline__ void push(int bin, const Acc &a) {
    if (bin != cur) {
      if (cur >= 0) a.add(cur, n);
      cur = bin;
      n = 0;
    }
    ++n;
  }
  __device__ __forceinline__ void flush(const Acc &a) {
    if (cur >= 0) a.add(cur, n);
    cur = -1;
    n = 0;
  }
};

template <typename T, typename Acc>
__device__ __forceinline__ void th_hist_chunk(const T *p, long long len, int min_val, int bins, const Acc &acc) {
  constexpr int VEC = 16 / (int)sizeof(T);
  long long lead = (long long)(((16 - (uintptr_t)p % 16) % 16) / sizeof(T));   // p is aligned to sizeof(T)
  if (lead > len) lead = len;
  const long long nvec = (len - lead) / VEC, tail0 = lead + nvec * VEC;
  ThRun<Acc> run;
  if ((long long)threadIdx.x < lead) run.push(th_bin<T>(p[threadIdx.x], min_val, bins), acc);
  for (long long v = threadIdx.x; v < nvec; v += TH_THREADS) {
    const uint4 raw = *reinterpret_cast<const uint4 *>(p + lead + v * VEC);
    T vals[VEC];
    __builtin_memcpy(vals, &raw, 16);
#pragma unroll
    for (int k = 0; k < VEC; ++k) run.push(th_bin<T>(vals[k], min_val, bins), acc);
  }
  for (long long i = tail0 + threadIdx.x; i < len; i += TH_THREADS) run.push(th_bin<T>(p[i], min_val, bins), acc);
  run.flush(acc);
}

template <typename T, bool LDS>
__global__ __launch_bounds__(TH_THREADS) void th_hist_kernel(const T *__restrict__ frames, long long pixels, long long chunk,
                                                              unsigned blocks_per_frame, int min_val, int bins,
                                                              int copies_log2, unsigned long long *__restrict__ hist) {
  __shared__ unsigned sh[LDS ? TH_LDS_WORDS : 1];
  const long long frame = blockIdx.x / blocks_per_frame;
  const long long start = (long long)(blockIdx.x % blocks_per_frame) * chunk;
  const long long len = min(chunk, pixels - start);
  const T *p = frames + frame * pixels + start;
  unsigned long long *out = hist + frame * bins;
  if (LDS) {
    const int words = bins << copies_log2;                // <= TH_LDS_WORDS by the host's choice of copies_log2
    for (int i = threadIdx.x; i < words; i += TH_THREADS) sh[i] = 0u;
    __syncthreads();
    th_hist_chunk<T>(p, len, min_val, bins, ThLdsAcc{sh, copies_log2, (int)(threadIdx.x & ((1u << copies_log2) - 1u))});
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += TH_THREADS) {
      unsigned sum = 0;
      for (int c = 0; c < (1 << copies_log2); ++c) sum += sh[(b << copies_log2) + c];
      if (sum) atomicAdd(&out[b], (unsigned long long)sum);
    }
  } else {
    th_hist_chunk<T>(p, len, min_val, bins, ThGlobalAcc{out});
  }
}

// ---- workgroup scan of two int64 series (blockDim.x <= 1024; every thread calls) ------------------------------------
// in: this thread's pair; out: the inclusive prefix over the threads before and including it; tot_*: the workgroup's sums
__device__ __forceinline__ void th_block_scan2(long long &a, long long &b, long long (*s_wave)[16], long long &tot_a,
                                               long long &tot_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long ua = __shfl_up(a, o, 64), ub = __shfl_up(b, o, 64);
    if (lane >= o) {
      a += ua;
      b += ub;
    }
  }
  __syncthreads();                                        // the previous use of s_wave has been read
  if (lane == 63) {
    s_wave[0][wave] = a;
    s_wave[1][wave] = b;
  }
  __syncthreads();
  long long pa = 0, pb = 0;
  tot_a = 0;
  tot_b = 0;
  for (int w = 0; w < waves; ++w) {
    const long long xa = s_wave[0][w], xb = s_wave[1][w];
    if (w < wave) {
      pa += xa;
      pb += xb;
    }
    tot_a += xa;
    tot_b += xb;
  }
  a += pa;
  b += pb;
}

__global__ __launch_bounds__(1024) void th_otsu_kernel(const long long *__restrict__ hist, int bins, int min_val,
                                                       int *__restrict__ thresh) {
  __shared__ long long s_wave[2][16];
  __shared__ float s_var[16];
  __shared__ int s_idx[16];
  const long long *h = hist + (long long)blockIdx.x * bins;
  const int T = blockDim.x;
  long long n = 0, f = 0, N, F;
  for (int b = threadIdx.x; b < bins; b += T) {
    const long long c = h[b];
    n += c;
    f += ((long long)min_val + b) * c;
  }
  th_block_scan2(n, f, s_wave, N, F);

  long long carry_n = 0, carry_f = 0;
  float best = -1.0f;                                     // every score is >= 0 (NaN becomes 0)
  int best_idx = 0x7FFFFFFF;
  for (int base = 0; base < bins; base += T) {
    const int b = base + (int)threadIdx.x;
    const long long c = b < bins ? h[b] : 0;
    long long nb = c, fb = ((long long)min_val + b) * c, tn, tf;
    th_block_scan2(nb, fb, s_wave, tn, tf);
    nb += carry_n;
    fb += carry_f;
    carry_n += tn;
    carry_f += tf;
    if (b < bins) {
      const long long nw = N - nb, fw = F - fb;
      const float mean_bk = (float)fb / (float)nb;
      const float mean_wh = (float)fw / (float)nw;
      const float d = mean_bk - mean_wh;
      float var = (float)(nb * nw) * (d * d);
      if (var != var) var = 0.0f;
      if (var > best) {                                   // strict: the first maximum of this thread's ascending bins
        best = var;
        best_idx = b;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(best_idx, o, 64);
    if (ov > best || (ov == best && oi < best_idx)) {
      best = ov;
      best_idx = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    s_var[threadIdx.x >> 6] = best;
    s_idx[threadIdx.x >> 6] = best_idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (T + 63) / 64; ++w)
      if (s_var[w] > best || (s_var[w] == best && s_idx[w] < best_idx)) {
        best = s_var[w];
        best_idx = s_idx[w];
      }
    thresh[blockIdx.x] = min_val + best_idx;
  }
}

// ---- multi-Otsu ---------------------------------------------------------------------------------------------------------

// prefix[frame]: pn[0 .. bins], ps[0 .. bins]: pn[b] = sum of hist[0 .. b), ps[b] = sum of (min_val + i) * hist[i] over the same
__global__ __launch_bounds__(1024) void th_prefix_kernel(const long long *__restrict__ hist, int bins, int min_val,
                                                         long long *__restrict__ prefix) {
  __shared__ long long s_wave[2][16];
  const long long *h = hist + (long long)blockIdx.x * bins;
  long long *pn = prefix + (long long)blockIdx.x * 2 * (bins + 1), *ps = pn + bins + 1;
  const int T = blockDim.x;
  if (threadIdx.x == 0) {
    pn[0] = 0;
    ps[0] = 0;
  }
  long long carry_n = 0, carry_f = 0;
  for (int base = 0; base < bins; base += T) {
    const int b = base + (int)threadIdx.x;
    const long long c = b < bins ? h[b] : 0;
    long long nb = c, fb = ((long long)min_val + b) * c, tn, tf;
    th_block_scan2(nb, fb, s_wave, tn, tf);
    if (b < bins) {
      pn[b + 1] = carry_n + nb;
      ps[b + 1] = carry_f + fb;
    }
    carry_n += tn;
    carry_f += tf;
  }
}

// C(a, b) for 0 <= b <= 4, exact whenever the result fits (every call below stays <= C(bins - 1, n_class - 1) < 2^31)
__host__ __device__ inline unsigned long long th_binom(long long a, int b) {
  if (a < b) return 0ull;
  unsigned long long r = 1ull;
  if (b >= 1) r = (unsigned long long)a;
  if (b >= 2) r = r * (unsigned long long)(a - 1) / 2ull;
  if (b >= 3) r = r * (unsigned long long)(a - 2) / 3ull;
  if (b >= 4) r = r * (unsigned long long)(a - 3) / 4ull;
  return r;
}

// rank -> the rank-th K-subset of {1 .. M} in lexicographic order (the order of itertools.combinations)
template <int K>
__host__ __device__ inline void th_unrank(unsigned long long rank, int M, int *th) {
  int lo = 1;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int r = K - 1 - j;                              // elements still to place after this one
    const unsigned long long base = th_binom(M - lo + 1, r + 1);
    // subsets whose element j lies in [lo, c): base - C(M - c + 1, r + 1); the largest c that keeps it <= rank
    int l = lo, h = M - r;
    while (l < h) {
      const int mid = l + (h - l + 1) / 2;
      if (base - th_binom(M - mid + 1, r + 1) <= rank)
        l = mid;
      else
        h = mid - 1;
    }
    th[j] = l;
    rank -= base - th_binom(M - l + 1, r + 1);
    lo = l + 1;
  }
}

template <int K>
__device__ __forceinline__ void th_next(int M, int *th) {
  bool done = false;
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {
    if (!done && th[j] < M - (K - 1 - j)) {
      ++th[j];
#pragma unroll
      for (int i = j + 1; i < K; ++i) th[i] = th[j] + (i - j);
      done = true;
    }
  }
}

template <int NC>
__device__ __forceinline__ double th_multi_score(const long long *pn, const long long *ps, const int *th, int bins) {
  long long n[NC];
  double m[NC];
  bool empty = false;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int lo = i == 0 ? 0 : th[i - 1], hi = i == NC - 1 ? bins : th[i];
    n[i] = pn[hi] - pn[lo];
    empty |= n[i] == 0;
    m[i] = (double)(ps[hi] - ps[lo]) / (double)n[i];
  }
  if (empty) return 0.0;
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int j = i + 1; j < NC; ++j) {
      const double d = m[i] - m[j];
      v = v + ((double)n[i] * (double)n[j]) * (d * d);
    }
  return v;
}

struct ThPartial {
  double v;
  unsigned long long rank;
};
__device__ __forceinline__ bool th_better(double v, unsigned long long r, double bv, unsigned long long br) {
  return v > bv || (v == bv && r < br);
}
// workgroup reduction on (v descending, rank ascending); the result is valid in thread 0
__device__ __forceinline__ void th_reduce_best(double &v, unsigned long long &r, ThPartial *s_part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const unsigned long long orr = __shfl_xor(r, o, 64);
    if (th_better(ov, orr, v, r)) {
      v = ov;
      r = orr;
    }
  }
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ThPartial{v, r};
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < TH_THREADS / 64; ++w)
      if (th_better(s_part[w].v, s_part[w].rank, v, r)) {
        v = s_part[w].v;
        r = s_part[w].rank;
      }
}

template <int NC, bool LDS>
__global__ __launch_bounds__(TH_THREADS) void th_multi_search_kernel(const long long *__restrict__ prefix, int bins,
                                                                     unsigned long long combos, unsigned blocks_per_frame,
                                                                     unsigned long long per_thread,
                                                                     ThPartial *__restrict__ partials) {
  constexpr int K = NC - 1;
  __shared__ long long s_pn[LDS ? TH_MULTI_LDS_BINS + 1 : 1], s_ps[LDS ? TH_MULTI_LDS_BINS + 1 : 1];
  __shared__ ThPartial s_part[TH_THREADS / 64];
  const unsigned frame = blockIdx.x / blocks_per_frame, blk = blockIdx.x % blocks_per_frame;
  const long long *pn = prefix + (long long)frame * 2 * (bins + 1), *ps = pn + bins + 1;
  if (LDS) {
    for (int i = threadIdx.x; i <= bins; i += TH_THREADS) {
      s_pn[i] = pn[i];
      s_ps[i] = ps[i];
    }
    __syncthreads();
    pn = s_pn;
    ps = s_ps;
  }
  const int M = bins - 1;
  double best = -1.0;                                     // every score is >= 0
  unsigned long long best_rank = ~0ull;
  unsigned long long r = ((unsigned long long)blk * TH_THREADS + threadIdx.x) * per_thread;
  const unsigned long long end = min(combos, r + per_thread);
  if (r < end) {
    int th[K];
    th_unrank<K>(r, M, th);
    for (;;) {
      const double v = th_multi_score<NC>(pn, ps, th, bins);
      if (v > best) {                                     // strict: the smallest rank among equals
        best = v;
        best_rank = r;
      }
      if (++r >= end) break;
      th_next<K>(M, th);
    }
  }
  th_reduce_best(best, best_rank, s_part);
  if (threadIdx.x == 0) partials[blockIdx.x] = ThPartial{best, best_rank};
}

template <int NC>
__device__ __forceinline__ void th_write_thresholds(unsigned long long rank, int bins, int min_val, int *out) {
  int th[NC - 1];
  th_unrank<NC - 1>(rank, bins - 1, th);
#pragma unroll
  for (int k = 0; k < NC - 1; ++k) out[k] = min_val + th[k] - 1;       // inclusive upper bound of class k
}

__global__ __launch_bounds__(TH_THREADS) void th_multi_finish_kernel(const ThPartial *__restrict__ partials,
                                                                     unsigned blocks_per_frame, int bins, int min_val,
                                                                     int n_class, int *__restrict__ thresholds) {
  __shared__ ThPartial s_part[TH_THREADS / 64];
  const ThPartial *p = partials + (size_t)blockIdx.x * blocks_per_frame;
  double best = -1.0;
  unsigned long long best_rank = ~0ull;
  for (unsigned i = threadIdx.x; i < blocks_per_frame; i += TH_THREADS)
    if (th_better(p[i].v, p[i].rank, best, best_rank)) {
      best = p[i].v;
      best_rank = p[i].rank;
    }
  th_reduce_best(best, best_rank, s_part);
  if (threadIdx.x == 0) {
    int *out = thresholds + (size_t)blockIdx.x * (n_class - 1);
    switch (n_class) {
      case 2: th_write_thresholds<2>(best_rank, bins, min_val, out); break;
      case 3: th_write_thresholds<3>(best_rank, bins, min_val, out); break;
      case 4: th_write_thresholds<4>(best_rank, bins, min_val, out); break;
      default: th_write_thresholds<5>(best_rank, bins, min_val, out); break;
    }
  }
}

// ---- apply ----------------------------------------------------------------------------------------------------------------

template <typename TI>
__device__ __forceinline__ bool th_above(TI v, int t) { return (long long)v > (long long)t; }
template <>
__device__ __forceinline__ bool th_above<float>(float v, int t) { return v > (float)t; }
template <typename TI>
__device__ __forceinline__ bool th_not_above(TI v, int t) { return (long long)v <= (long long)t; }
template <>
__device__ __forceinline__ bool th_not_above<float>(float v, int t) { return v <= (float)t; }     // false for NaN

template <typename T, int V>
struct __attribute__((aligned(sizeof(T) * V))) ThVec {
  T v[V];
};

template <typename TI, typename TO, int V>
__global__ __launch_bounds__(TH_THREADS) void th_apply_kernel(const TI *__restrict__ frames, long long pixels,
                                                               unsigned blocks_per_frame, const int *__restrict__ thresholds,
                                                               int n_thresh, int binary, TO low, TO high,
                                                               TO *__restrict__ out) {
  const long long frame = blockIdx.x / blocks_per_frame;
  const long long unit = (long long)(blockIdx.x % blocks_per_frame) * TH_THREADS + threadIdx.x;
  const long long i0 = unit * V;
  if (i0 >= pixels) return;
  int t[TH_MAX_CLASSES - 1];
#pragma unroll
  for (int k = 0; k < TH_MAX_CLASSES - 1; ++k) t[k] = k < n_thresh ? thresholds[frame * n_thresh + k] : 0;
  const long long at = frame * pixels + i0;
  const ThVec<TI, V> in = *reinterpret_cast<const ThVec<TI, V> *>(frames + at);   // V == 1, or pixels % V == 0 and aligned
  ThVec<TO, V> o;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (binary) {
      o.v[j] = th_not_above<TI>(in.v[j], t[0]) ? low : high;
    } else {
      int label = 0;
#pragma unroll
      for (int k = 0; k < TH_MAX_CLASSES - 1; ++k) label += (k < n_thresh && th_above<TI>(in.v[j], t[k])) ? 1 : 0;
      o.v[j] = (TO)label;
    }
  }
  *reinterpret_cast<ThVec<TO, V> *>(out + at) = o;
}

template <typename TI, typename TO>
int th_apply_launch(const void *frames, int batch, long long pixels, const int *thresholds, int n_thresh, int binary, int low,
                    int high, void *out, hipStream_t s) {
  const bool vec = pixels % 4 == 0 && (uintptr_t)frames % (4 * sizeof(TI)) == 0 && (uintptr_t)out % (4 * sizeof(TO)) == 0;
  const long long units = vec ? pixels / 4 : pixels;
  const long long bpf = (units + TH_THREADS - 1) / TH_THREADS;
  if (bpf * batch >= (1ll << 31)) return MI_E_SHAPE;
  const dim3 grid((unsigned)(bpf * batch)), block(TH_THREADS);
  const TI *in = static_cast<const TI *>(frames);
  TO *o = static_cast<TO *>(out);
  if (vec)
    hipLaunchKernelGGL((th_apply_kernel<TI, TO, 4>), grid, block, 0, s, in, pixels, (unsigned)bpf, thresholds, n_thresh, binary,
                       (TO)low, (TO)high, o);
  else
    hipLaunchKernelGGL((th_apply_kernel<TI, TO, 1>), grid, block, 0, s, in, pixels, (unsigned)bpf, thresholds, n_thresh, binary,
                       (TO)low, (TO)high, o);
  return mi_launch_status();
}

template <typename TI>
int th_apply_out(int out_dtype, const void *frames, int batch, long long pixels, const int *thresholds, int n_thresh,
                 int binary, int low, int high, void *out, hipStream_t s) {
  switch (out_dtype) {
    case MI_PIX_U8: return th_apply_launch<TI, uint8_t>(frames, batch, pixels, thresholds, n_thresh, binary, low, high, out, s);
    case MI_PIX_I32: return th_apply_launch<TI, int32_t>(frames, batch, pixels, thresholds, n_thresh, binary, low, high, out, s);
    default: return th_apply_launch<TI, float>(frames, batch, pixels, thresholds, n_thresh, binary, low, high, out, s);
  }
}

bool th_dtype_ok(int dtype) { return dtype == MI_PIX_U8 || dtype == MI_PIX_U16 || dtype == MI_PIX_I32 || dtype == MI_PIX_F32; }

int th_frames_status(int dtype, int batch, long long pixels) {
  if (!th_dtype_ok(dtype)) return MI_E_PARAM;
  if (batch < 1 || pixels < 1) return MI_E_SHAPE;
  if (pixels > (1ll << 62) / batch) return MI_E_SHAPE;
  return MI_OK;
}

// number of candidates C(bins - 1, n_class - 1), 0 when the request is outside the limits
unsigned long long th_multi_combos(int bins, int n_class) {
  if (n_class < 2 || n_class > TH_MAX_CLASSES || bins < n_class || bins > TH_MAX_BINS) return 0ull;
  unsigned long long c = 1ull;                            // C(M, k) built up as C(M - k + i, i): exact at every step
  const int M = bins - 1, k = n_class - 1;
  for (int i = 1; i <= k; ++i) {
    c = c * (unsigned long long)(M - k + i) / (unsigned long long)i;
    if (c > 0x7FFFFFFFull * 65536ull) return 0ull;        // already hopeless; keeps the product inside 64 bits
  }
  return c <= 0x7FFFFFFFull ? c : 0ull;
}

unsigned th_multi_blocks(unsigned long long combos, int batch) {
  const unsigned long long want = (combos + (unsigned long long)TH_THREADS * TH_RANKS_PER_THREAD - 1) /
                                  ((unsigned long long)TH_THREADS * TH_RANKS_PER_THREAD);
  const unsigned long long cap = batch >= 4096 ? 1ull : 4096ull / (unsigned long long)batch;
  return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

size_t th_multi_prefix_bytes(int batch, int bins) { return (size_t)batch * 2 * ((size_t)bins + 1) * sizeof(long long); }

template <int NC>
void th_multi_search_launch(bool lds, dim3 grid, hipStream_t s, const long long *prefix, int bins, unsigned long long combos,
                            unsigned bpf, unsigned long long per_thread, ThPartial *partials) {
  if (lds)
    hipLaunchKernelGGL((th_multi_search_kernel<NC, true>), grid, dim3(TH_THREADS), 0, s, prefix, bins, combos, bpf, per_thread,
                       partials);
  else
    hipLaunchKernelGGL((th_multi_search_kernel<NC, false>), grid, dim3(TH_THREADS), 0, s, prefix, bins, combos, bpf, per_thread,
                       partials);
}

}  // namespace

extern "C" int mi_histogram(const void *frames, int dtype, int batch, long long pixels, int min_val, int bins,
                            int64_t *hist, mi_stream_t stream) {
  MI_ENTER();
  if (!frames || !hist) return MI_E_NULL;
  if (const int e = th_frames_status(dtype, batch, pixels)) return e;
  if (bins < 1 || bins > TH_MAX_BINS) return MI_E_SHAPE;
  if ((uintptr_t)frames % th_elem_size(dtype) != 0 || (uintptr_t)hist % 8 != 0) return MI_E_ALIGN;
  const long long chunk = (long long)TH_THREADS * TH_VECS_PER_THREAD * (16 / th_elem_size(dtype));
  const long long bpf = (pixels + chunk - 1) / chunk;
  if (bpf > ((1ll << 31) - 1) / batch) return MI_E_SHAPE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int e = mi_zero_async(hist, (size_t)batch * bins * sizeof(int64_t), s)) return e;
  const bool lds = bins <= TH_LDS_MAX_BINS;
  int copies_log2 = 0;
  while (copies_log2 < TH_MAX_COPIES_LOG2 && ((long long)bins << (copies_log2 + 1)) <= TH_LDS_WORDS) ++copies_log2;
  const dim3 grid((unsigned)(bpf * batch)), block(TH_THREADS);
  unsigned long long *h = reinterpret_cast<unsigned long long *>(hist);
#define TH_HIST_LAUNCH(T)                                                                                                  \
  do {                                                                                                                     \
    if (lds)                                                                                                               \
      hipLaunchKernelGGL((th_hist_kernel<T, true>), grid, block, 0, s, static_cast<const T *>(frames), pixels, chunk,      \
                         (unsigned)bpf, min_val, bins, copies_log2, h);                                                    \
    else                                                                                                                   \
      hipLaunchKernelGGL((th_hist_kernel<T, false>), grid, block, 0, s, static_cast<const T *>(frames), pixels, chunk,     \
                         (unsigned)bpf, min_val, bins, copies_log2, h);                                                    \
  } while (0)
  switch (dtype) {
    case MI_PIX_U8: TH_HIST_LAUNCH(uint8_t); break;
    case MI_PIX_U16: TH_HIST_LAUNCH(uint16_t); break;
    case MI_PIX_I32: TH_HIST_LAUNCH(int32_t); break;
    default: TH_HIST_LAUNCH(float); break;
  }
#undef TH_HIST_LAUNCH
  return mi_launch_status();
}

extern "C" int mi_otsu_threshold(const int64_t *hist, int batch, int bins, int min_val, int32_t *thresh, mi_stream_t stream) {
  MI_ENTER();
  if (!hist || !thresh) return MI_E_NULL;
  if (batch < 1 || bins < 1 || bins > TH_MAX_BINS) return MI_E_SHAPE;
  if ((long long)min_val + bins - 1 > 0x7FFFFFFFll) return MI_E_PARAM;
  if ((uintptr_t)hist % 8 != 0 || (uintptr_t)thresh % 4 != 0) return MI_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(th_otsu_kernel, dim3((unsigned)batch), dim3(bins <= 256 ? 256 : 1024), 0, s,
                     reinterpret_cast<const long long *>(hist), bins, min_val, thresh);
  return mi_launch_status();
}

extern "C" size_t mi_multi_otsu_workspace_bytes(int batch, int bins, int n_class) {
  const unsigned long long combos = th_multi_combos(bins, n_class);
  if (batch < 1 || combos == 0) return 0;
  return th_multi_prefix_bytes(batch, bins) + (size_t)batch * th_multi_blocks(combos, batch) * sizeof(ThPartial);
}

extern "C" int mi_multi_otsu_threshold(const int64_t *hist, int batch, int bins, int min_val, int n_class,
                                       int32_t *thresholds, void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!hist || !thresholds || !workspace) return MI_E_NULL;
  if (batch < 1 || bins < 1) return MI_E_SHAPE;
  if (n_class < 2 || n_class > TH_MAX_CLASSES) return MI_E_PARAM;
  const unsigned long long combos = th_multi_combos(bins, n_class);
  if (combos == 0) return MI_E_SHAPE;                     // n_class > bins, bins > 65536, or more than 2^31 - 1 candidates
  if ((long long)min_val + bins - 1 > 0x7FFFFFFFll) return MI_E_PARAM;
  if ((uintptr_t)hist % 8 != 0 || (uintptr_t)thresholds % 4 != 0 || (uintptr_t)workspace % 8 != 0) return MI_E_ALIGN;
  if (workspace_bytes < mi_multi_otsu_workspace_bytes(batch, bins, n_class)) return MI_E_CAPACITY;
  const unsigned bpf = th_multi_blocks(combos, batch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  long long *prefix = static_cast<long long *>(workspace);
  ThPartial *partials = reinterpret_cast<ThPartial *>(static_cast<char *>(workspace) + th_multi_prefix_bytes(batch, bins));
  hipLaunchKernelGGL(th_prefix_kernel, dim3((unsigned)batch), dim3(bins <= 256 ? 256 : 1024), 0, s,
                     reinterpret_cast<const long long *>(hist), bins, min_val, prefix);
  MI_CHECK_LAUNCH();
  const unsigned long long threads = (unsigned long long)bpf * TH_THREADS;
  const unsigned long long per_thread = (combos + threads - 1) / threads;
  const dim3 grid(bpf * (unsigned)batch);
  const bool lds = bins <= TH_MULTI_LDS_BINS;
  switch (n_class) {
    case 2: th_multi_search_launch<2>(lds, grid, s, prefix, bins, combos, bpf, per_thread, partials); break;
    case 3: th_multi_search_launch<3>(lds, grid, s, prefix, bins, combos, bpf, per_thread, partials); break;
    case 4: th_multi_search_launch<4>(lds, grid, s, prefix, bins, combos, bpf, per_thread, partials); break;
    default: th_multi_search_launch<5>(lds, grid, s, prefix, bins, combos, bpf, per_thread, partials); break;
  }
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(th_multi_finish_kernel, dim3((unsigned)batch), dim3(TH_THREADS), 0, s, partials, bpf, bins, min_val, n_class,
                     thresholds);
  return mi_launch_status();
}

extern "C" int mi_threshold_apply(const void *frames, int dtype, int batch, long long pixels, const int32_t *thresholds,
                                  int n_thresh, int out_dtype, int binary, int low, int high, void *out, mi_stream_t stream) {
  MI_ENTER();
  if (!frames || !thresholds || !out) return MI_E_NULL;
  if (const int e = th_frames_status(dtype, batch, pixels)) return e;
  if (n_thresh < 1 || n_thresh > TH_MAX_CLASSES - 1 || (binary != 0 && binary != 1)) return MI_E_PARAM;
  if (out_dtype != MI_PIX_U8 && out_dtype != MI_PIX_I32 && out_dtype != MI_PIX_F32) return MI_E_PARAM;
  if (binary ? n_thresh != 1 : out_dtype != MI_PIX_U8) return MI_E_PARAM;
  if ((uintptr_t)frames % th_elem_size(dtype) != 0 || (uintptr_t)thresholds % 4 != 0 ||
      (uintptr_t)out % th_elem_size(out_dtype) != 0)
    return MI_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MI_PIX_U8: return th_apply_out<uint8_t>(out_dtype, frames, batch, pixels, thresholds, n_thresh, binary, low, high, out, s);
    case MI_PIX_U16: return th_apply_out<uint16_t>(out_dtype, frames, batch, pixels, thresholds, n_thresh, binary, low, high, out, s);
    case MI_PIX_I32: return th_apply_out<int32_t>(out_dtype, frames, batch, pixels, thresholds, n_thresh, binary, low, high, out, s);
    default: return th_apply_out<float>(out_dtype, frames, batch, pixels, thresholds, n_thresh, binary, low, high, out, s);
  }
}
