// K29 local-map tracking (include/mi355x_match.h): a representative descriptor per landmark slot, and the landmarks
// of a batch item projected into one frame by a predicted pose and matched, each inside a window round its projection.
//
// K29a localmap_descriptors_kernel: 16 lanes per slot, lane f = frame f.  A lane gathers its view's W words; W width-16
//   shuffles per other frame give it its row of the distance table (registers, fully unrolled); localmap_math.h's lm_median
//   ranks the row; a width-16 min-reduction of med << 8 | f picks the view, whose words lane w < W writes.
// K29b localmap_match_kernel: one workgroup of 1024 threads per item; no workgroup ever waits for another.
//   stage      the frame into dynamic LDS: the keypoints' two floats (a NaN pair for an invalid keypoint: it is in no
//              window), their bits TRANSPOSED, word w of keypoint j at w * (K | 1) + j (the odd pitch spreads the staging
//              writes over the banks; a wave's read of one word of 64 consecutive keypoints is conflict-free), one claim
//              word per keypoint (LM_NO_CLAIM), five counters.
//   match      every wave takes a contiguous chunk of ceil(L / 16) <= 128 landmarks, 64 at a time: lane i projects landmark
//              i of the group (float64, lm_project), writes its proj and loads its W descriptor words.  The in-view ballot is
//              walked bit by bit: u, v and the W words of landmark i are read out of lane i, the lanes stride over the
//              keypoints, the window test runs on all of them and the Hamming distance only inside the window; the lanes'
//              best-two pairs are merged across the wave.  A candidate claims its keypoint by an LDS atomicMin of
//              d1 << 16 | l.  Lane i keeps landmark i's (state, d1, j1) in a register.
//   write      after a barrier that every thread reaches: lane i finishes landmark i (kept iff the claim word of j1 names it)
//              and writes its outputs; the states are counted by ballot and LDS atomicAdd; kp_lm is the claim words decoded.
// Built with -ffp-contract=off.  No global atomics; the LDS atomics are integer and order-independent (header): bitwise
// reproducible.
#include "common.h"
#include "localmap_math.h"

#include <math.h>

namespace {

constexpr int LM_THREADS = 1024, LM_WAVES = LM_THREADS / 64;
constexpr int LM_GROUPS = 2;                         // groups of 64 landmarks per wave: 16 waves x 2 x 64 = 2048
static_assert(LM_WAVES * LM_GROUPS * 64 == MI_LOCALMAP_MAX_LANDMARKS, "a lane keeps the result of LM_GROUPS landmarks");
static_assert(MI_LOCALMAP_MAX_LANDMARKS <= 1 << 16 && MI_LOCALMAP_MAX_KEYPOINTS <= 1 << 10, "claim: d1 << 16 | l; packed: 10 bits of j1 + 1");
static_assert(MI_LOCALMAP_MAX_FRAMES == LM_MAX_FRAMES && MI_LOCALMAP_MAX_LANDMARKS == MI_BA_MAX_LANDMARKS, "the header's limits");
constexpr int LM_DESC_THREADS = 256;
constexpr unsigned LM_NAN_BITS = 0x7fc00000u;
constexpr size_t LM_HEAD_BYTES = 32;                 // five counters, padded to keep what follows 16-byte aligned

__host__ __device__ inline int lm_pitch(int K) { return K | 1; }
size_t lm_lds_bytes(int K, int W) { return LM_HEAD_BYTES + (size_t)K * 12 + (size_t)W * lm_pitch(K) * 4; }

extern __shared__ __align__(16) unsigned char lm_lds[];

// a landmark's result between the two passes: state (3 bits) | d1 (10 bits, ABSENT <= 513) << 3 | (j1 + 1) << 13
__device__ __forceinline__ int lm_pack(int state, int d1, int j1) { return state | d1 << 3 | (j1 + 1) << 13; }

template <int W>
__global__ __launch_bounds__(LM_THREADS) void localmap_match_kernel(
    const float *__restrict__ points, const uint8_t *__restrict__ point_valid, const uint32_t *__restrict__ rep_bits,
    const float *__restrict__ r, const float *__restrict__ t, const float *__restrict__ cam, const float *__restrict__ kp,
    const uint8_t *__restrict__ kp_valid, const uint32_t *__restrict__ kp_bits, int L, int K, int height, int width, float min_depth,
    float max_depth, float radius, int max_distance, float ratio, float *__restrict__ proj, uint8_t *__restrict__ lm_state,
    int32_t *__restrict__ lm_kp, int32_t *__restrict__ lm_distance, float *__restrict__ match_keypoints, int32_t *__restrict__ kp_lm,
    int32_t *__restrict__ counts) {
  constexpr int num_bits = 32 * W;
  const int Kp = lm_pitch(K);
  int *cnt = reinterpret_cast<int *>(lm_lds);
  uint32_t *kpw = reinterpret_cast<uint32_t *>(lm_lds + LM_HEAD_BYTES);          // (K, 2): ky, kx
  int *claim = reinterpret_cast<int *>(kpw + 2 * (size_t)K);
  uint32_t *kpb = reinterpret_cast<uint32_t *>(claim + K);                        // (W, Kp)
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  points += b * (size_t)L * 3;
  if (point_valid) point_valid += b * (size_t)L;
  rep_bits += b * (size_t)L * W;
  r += b * 9;
  t += b * 3;
  cam += b * 4;
  kp += b * (size_t)K * 2;
  if (kp_valid) kp_valid += b * (size_t)K;
  kp_bits += b * (size_t)K * W;
  proj += b * (size_t)L * 2;
  lm_state += b * (size_t)L;
  lm_kp += b * (size_t)L;
  lm_distance += b * (size_t)L;
  match_keypoints += b * (size_t)L * 2;
  kp_lm += b * (size_t)K;

  // ---- stage ---------------------------------------------------------------------------------------------------------------------
  if (tid < 5) cnt[tid] = 0;
  for (int j = tid; j < K; j += LM_THREADS) {
    const bool ok = !kp_valid || kp_valid[j];
    kpw[2 * j] = ok ? __float_as_uint(kp[2 * j]) : LM_NAN_BITS;
    kpw[2 * j + 1] = ok ? __float_as_uint(kp[2 * j + 1]) : LM_NAN_BITS;
    claim[j] = LM_NO_CLAIM;
  }
  for (int idx = tid; idx < K * W; idx += LM_THREADS) {
    const int j = idx / W, w = idx - j * W;
    kpb[w * Kp + j] = kp_bits[idx];
  }
  __syncthreads();

  // ---- match ---------------------------------------------------------------------------------------------------------------------
  const double r2 = (double)radius * (double)radius;
  const int chunk = (L + LM_WAVES - 1) / LM_WAVES;                                // <= 128 = LM_GROUPS * 64
  const int l0 = wave * chunk, l1 = l0 + chunk < L ? l0 + chunk : L;
  int mine[LM_GROUPS];
#pragma unroll
  for (int g = 0; g < LM_GROUPS; ++g) {
    const int lg = l0 + g * 64, l = lg + lane;
    mine[g] = lm_pack(0, num_bits + 1, -1);
    if (lg >= l1) continue;                                                       // wave-uniform
    const bool live = l < l1;
    LmProj p;
    p.u = p.v = 0.0;
    p.in_view = false;
    uint32_t rep[W];
#pragma unroll
    for (int w = 0; w < W; ++w) rep[w] = 0;
    if (live) {
      p = lm_project(r, t, cam, points + 3 * (size_t)l, !point_valid || point_valid[l], height, width, min_depth, max_depth);
      proj[2 * (size_t)l] = p.in_view ? (float)p.v : -1.0f;
      proj[2 * (size_t)l + 1] = p.in_view ? (float)p.u : -1.0f;
      if (p.in_view) {
#pragma unroll
        for (int w = 0; w < W; ++w) rep[w] = rep_bits[(size_t)l * W + w];
      }
    }
    unsigned long long todo = __ballot(live && p.in_view);
    while (todo) {                                                                // wave-uniform
      const int i = __ffsll(todo) - 1;
      todo &= todo - 1;
      const double u = __shfl(p.u, i, 64), v = __shfl(p.v, i, 64);
      uint32_t rw[W];
#pragma unroll
      for (int w = 0; w < W; ++w) rw[w] = (uint32_t)__builtin_amdgcn_readlane((int)rep[w], i);
      LmPair best;
      best.k1 = best.k2 = LM_EMPTY;
      for (int j = lane; j < K; j += 64) {
        if (lm_in_window(__uint_as_float(kpw[2 * j]), __uint_as_float(kpw[2 * j + 1]), u, v, r2)) {
          int h = 0;
#pragma unroll
          for (int w = 0; w < W; ++w) h += lm_popcount(rw[w] ^ kpb[w * Kp + j]);
          lm_push(best, lm_key(h, j));
        }
      }
      int packed = lm_pack(1, num_bits + 1, -1);
      if (__any(best.k1 != LM_EMPTY)) {                                           // wave-uniform
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          LmPair other;
          other.k1 = (uint32_t)__shfl_xor((int)best.k1, o, 64);
          other.k2 = (uint32_t)__shfl_xor((int)best.k2, o, 64);
          best = lm_merge(best, other);
        }
        int d1, j1, d2;
        lm_decode(best, num_bits, &d1, &j1, &d2);
        const bool cand = lm_candidate(d1, d2, max_distance, ratio);
        if (cand && lane == 0) atomicMin(&claim[j1], lm_claim_key(d1, lg + i));
        packed = lm_pack(cand ? 4 : 2, d1, j1);
      }
      if (lane == i) mine[g] = packed;
    }
  }
  __syncthreads();                                   // every claim has landed

  // ---- write ---------------------------------------------------------------------------------------------------------------------
#pragma unroll
  for (int g = 0; g < LM_GROUPS; ++g) {
    const int lg = l0 + g * 64, l = lg + lane;
    if (lg >= l1) continue;                                                       // wave-uniform
    const bool live = l < l1;
    int state = mine[g] & 7;
    const int d1 = (mine[g] >> 3) & 1023, j1 = (mine[g] >> 13) - 1;
    if (live) {
      if (state == 4 && lm_claim_landmark(claim[j1]) != l) state = 3;
      const bool kept = state == 4;
      lm_state[l] = (uint8_t)state;
      lm_kp[l] = kept ? j1 : -1;
      lm_distance[l] = state >= 2 ? d1 : num_bits + 1;
      match_keypoints[2 * (size_t)l] = kept ? __uint_as_float(kpw[2 * j1]) : -1.0f;
      match_keypoints[2 * (size_t)l + 1] = kept ? __uint_as_float(kpw[2 * j1 + 1]) : -1.0f;
    }
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int n = __popcll(__ballot(live && state == s));
      if (lane == 0 && n) atomicAdd(&cnt[s], n);
    }
  }
  for (int j = tid; j < K; j += LM_THREADS) kp_lm[j] = lm_claim_landmark(claim[j]);
  __syncthreads();
  if (tid < 5) counts[b * 5 + tid] = cnt[tid];
}

template <int W>
__global__ __launch_bounds__(LM_DESC_THREADS) void localmap_descriptors_kernel(
    const uint32_t *__restrict__ bits, const int32_t *__restrict__ track_kp, int F, int K, int L, uint32_t *__restrict__ rep_bits,
    int32_t *__restrict__ rep_frame, int32_t *__restrict__ rep_median) {
  constexpr int num_bits = 32 * W;
  const int f = threadIdx.x & 15, slot = blockIdx.x * (LM_DESC_THREADS / 16) + (threadIdx.x >> 4);
  const size_t b = blockIdx.y;
  const bool live = slot < L;                        // nobody leaves early: the shuffles below want the whole wave
  int k = -1;
  if (live && f < F) k = track_kp[(b * F + f) * L + slot];
  const bool view = k >= 0 && k < K;
  uint32_t w[W];
#pragma unroll
  for (int i = 0; i < W; ++i) w[i] = view ? bits[((b * F + f) * K + (size_t)k) * W + i] : 0u;
  const unsigned views = (unsigned)(__ballot(view) >> (threadIdx.x & 48)) & 0xffffu;
  const int n = __popc(views);
  int d[LM_MAX_FRAMES];
#pragma unroll
  for (int g = 0; g < LM_MAX_FRAMES; ++g) {
    int h = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) h += lm_popcount(w[i] ^ (uint32_t)__shfl((int)w[i], g, 16));
    d[g] = h;
  }
  int key = view ? lm_rep_key(lm_median(d, views, n), f) : 0x7fffffff;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const int other = __shfl_xor(key, o, 16);
    key = other < key ? other : key;
  }
  const int best = n ? (key & 0xff) : 0;
  uint32_t out = 0;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const uint32_t word = (uint32_t)__shfl((int)w[i], best, 16);
    if (f == i) out = word;
  }
  if (live) {
    const size_t at = b * L + slot;
    if (f < W) rep_bits[at * W + f] = n ? out : 0u;
    if (f == 0) {
      rep_frame[at] = n ? best : -1;
      rep_median[at] = n ? key >> 8 : num_bits + 1;
    }
  }
}

int lm_shape_status(int batch, int landmarks, int keypoints) {
  if (batch < 1 || landmarks < 1 || keypoints < 1) return MI_E_SHAPE;
  if (batch > 65535 || landmarks > MI_LOCALMAP_MAX_LANDMARKS || keypoints > MI_LOCALMAP_MAX_KEYPOINTS) return MI_E_PARAM;
  return MI_OK;
}

template <int W>
int lm_launch_match(const float *points, const uint8_t *point_valid, const uint32_t *rep_bits, const float *r, const float *t,
                    const float *cam, const float *kp, const uint8_t *kp_valid, const uint32_t *kp_bits, int batch, int L, int K,
                    int height, int width, float min_depth, float max_depth, float radius, int max_distance, float ratio, float *proj,
                    uint8_t *lm_state, int32_t *lm_kp, int32_t *lm_distance, float *match_keypoints, int32_t *kp_lm, int32_t *counts,
                    hipStream_t stream) {
  const size_t lds = lm_lds_bytes(K, W);
  static size_t allowed = 64 * 1024;                     // raised once, to what the keypoint cap needs (pgo.hip's pattern)
  if (lds > allowed) {
    const size_t most = lm_lds_bytes(MI_LOCALMAP_MAX_KEYPOINTS, W);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(localmap_match_kernel<W>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    if (e != hipSuccess) return (int)e;
    allowed = most;
  }
  hipLaunchKernelGGL(localmap_match_kernel<W>, dim3((unsigned)batch), dim3(LM_THREADS), lds, stream, points, point_valid, rep_bits, r, t,
                     cam, kp, kp_valid, kp_bits, L, K, height, width, min_depth, max_depth, radius, max_distance, ratio, proj, lm_state,
                     lm_kp, lm_distance, match_keypoints, kp_lm, counts);
  return mi_launch_status();
}

}  // namespace

extern "C" int mi_localmap_descriptors(const uint32_t *bits, const int32_t *track_kp, int batch, int frames, int keypoints,
                                       int landmarks, int num_bits, uint32_t *rep_bits, int32_t *rep_frame, int32_t *rep_median,
                                       mi_stream_t stream) {
  MI_ENTER();
  if (!bits || !track_kp || !rep_bits || !rep_frame || !rep_median) return MI_E_NULL;
  if (frames < 1) return MI_E_SHAPE;
  if (const int s = lm_shape_status(batch, landmarks, keypoints)) return s;
  if (frames > MI_LOCALMAP_MAX_FRAMES || (num_bits != 256 && num_bits != 512)) return MI_E_PARAM;
  const dim3 grid((unsigned)ceil_div(landmarks, LM_DESC_THREADS / 16), (unsigned)batch);
  if (num_bits == 256)
    hipLaunchKernelGGL(localmap_descriptors_kernel<8>, grid, dim3(LM_DESC_THREADS), 0, (hipStream_t)stream, bits, track_kp, frames, keypoints,
                       landmarks, rep_bits, rep_frame, rep_median);
  else
    hipLaunchKernelGGL(localmap_descriptors_kernel<16>, grid, dim3(LM_DESC_THREADS), 0, (hipStream_t)stream, bits, track_kp, frames, keypoints,
                       landmarks, rep_bits, rep_frame, rep_median);
  return mi_launch_status();
}

extern "C" int mi_localmap_match(const float *points, const uint8_t *point_valid, const uint32_t *rep_bits, const float *r,
                                 const float *t, const float *cam, const float *kp, const uint8_t *kp_valid, const uint32_t *kp_bits,
                                 int batch, int landmarks, int keypoints, int num_bits, int height, int width, float min_depth,
                                 float max_depth, float radius, int max_distance, float ratio, float *proj, uint8_t *lm_state,
                                 int32_t *lm_kp, int32_t *lm_distance, float *match_keypoints, int32_t *kp_lm, int32_t *counts,
                                 mi_stream_t stream) {
  MI_ENTER();
  if (!points || !rep_bits || !r || !t || !cam || !kp || !kp_bits || !proj || !lm_state || !lm_kp || !lm_distance || !match_keypoints ||
      !kp_lm || !counts)
    return MI_E_NULL;
  if (const int s = lm_shape_status(batch, landmarks, keypoints)) return s;
  if (num_bits != 256 && num_bits != 512) return MI_E_PARAM;
  if (!(min_depth > 0.0f) || !(min_depth < max_depth) || !(max_depth < INFINITY) || !(radius > 0.0f) || !(radius < INFINITY) ||
      max_distance < 0 || max_distance > num_bits || !(ratio > 0.0f) || !(ratio <= 1.0f) || height < 1 || width < 1)
    return MI_E_PARAM;
  if (num_bits == 256)
    return lm_launch_match<8>(points, point_valid, rep_bits, r, t, cam, kp, kp_valid, kp_bits, batch, landmarks, keypoints, height, width,
                              min_depth, max_depth, radius, max_distance, ratio, proj, lm_state, lm_kp, lm_distance, match_keypoints, kp_lm,
                              counts, (hipStream_t)stream);
  return lm_launch_match<16>(points, point_valid, rep_bits, r, t, cam, kp, kp_valid, kp_bits, batch, landmarks, keypoints, height, width,
                             min_depth, max_depth, radius, max_distance, ratio, proj, lm_state, lm_kp, lm_distance, match_keypoints, kp_lm,
                             counts, (hipStream_t)stream);
}
