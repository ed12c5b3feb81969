// K28 landmark tracks (include/mi355x_match.h): the pairwise matches of a window of frames -> landmark tracks in the
// form K25 reads, and the N-view triangulation of every track, batched over independent windows.
//
// K28a tracks_build_kernel: one workgroup of 1024 threads per window; no workgroup ever waits for another.
//   edges      every match record -> the workspace: its two nodes packed into one int32, -1 for padding.  Once per launch.
//   label      label[n] in dynamic LDS, n at the start.  A round: every active edge finds the roots of its ends and hooks
//              the larger under the smaller (LDS atomicMin); then every node jumps to its root.  Labels only decrease and a
//              node's label stays inside its component, so a racy read sees a valid ancestor.  Rounds repeat until a
//              workgroup-uniform "changed" flag stays clear after a barrier that every thread reaches; every productive
//              round removes a root, which bounds the loop by the node count.  At the fixed point the root of a component
//              is its smallest node, whatever order the hooks landed in.
//   stats      per root (aux[n], the second LDS array) the mask of its nodes' frames and their count (LDS atomicOr /
//              atomicAdd): conflict <=> count > popcount(mask).
//   order      nodes in contiguous chunks per thread; for each length F .. min_views a block prefix sum over the threads'
//              counts of eligible roots of that length: slots in (length descending, label ascending).
//   write      empty slots first (at the kernel's start), then every node of a kept component writes its own column entry.
// K28b tracks_triangulate_kernel: one thread per landmark, tracks_math.h's trk_triangulate, float64.
// Built with -ffp-contract=off.  No global atomics; the LDS atomics are integer and order-independent (header): bitwise
// reproducible.
#include "common.h"
#include "tracks_math.h"

#include <math.h>

namespace {

constexpr int TRK_THREADS = 1024, TRK_WAVES = TRK_THREADS / 64;
constexpr int TRK_TRI_THREADS = 128;
constexpr int TRK_NODE_BITS = 14;                    // F K <= 16 * 1024 = 2^14 nodes
static_assert(MI_TRACKS_MAX_FRAMES * MI_TRACKS_MAX_KEYPOINTS == 1 << TRK_NODE_BITS, "an edge packs two nodes into 28 bits");
static_assert(MI_TRACKS_MAX_FRAMES == MI_BA_MAX_FRAMES && MI_TRACKS_MAX_FRAMES <= 16, "the frame mask is the low half of aux");
// aux[n] while the statistics are collected: count << 16 | frame mask (count <= 2^14).  Once a root is judged, its code:
constexpr int TRK_DONE = (int)0x80000000;            // | length << 16 | (slot + 2); slot -2: conflicting, -1: no slot

struct TrkShared {
  int wave_sum[TRK_WAVES];
  int changed;
  int counts[3];                                     // components of >= 2 nodes, conflicting, eligible
};
constexpr size_t TRK_SHARED_BYTES = (sizeof(TrkShared) + 15) & ~(size_t)15;

__host__ __device__ inline size_t trk_ws_bytes(int pairs, int matches) { return ((size_t)pairs * matches * 4 + 15) & ~(size_t)15; }
size_t trk_lds_bytes(int nodes) { return TRK_SHARED_BYTES + (size_t)2 * nodes * sizeof(int); }

extern __shared__ __align__(16) unsigned char trk_lds[];

__device__ __forceinline__ int trk_find(const int *label, int x) {
  int p = __atomic_load_n(&label[x], __ATOMIC_RELAXED);
  while (p != x) {
    x = p;
    p = __atomic_load_n(&label[x], __ATOMIC_RELAXED);
  }
  return x;
}

// exclusive prefix sum of v over the workgroup's threads in thread order, and the total; two barriers
__device__ __forceinline__ int trk_block_scan(TrkShared &S, int v, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  __syncthreads();                                   // the previous scan's wave_sum has been read by everyone
  if (lane == 63) S.wave_sum[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < TRK_WAVES; ++w) {
    const int s = S.wave_sum[w];
    before += w < wave ? s : 0;
    all += s;
  }
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(TRK_THREADS) void tracks_build_kernel(
    const int32_t *__restrict__ pair_frames, const int32_t *__restrict__ match_ij, const uint8_t *__restrict__ match_valid,
    const uint8_t *__restrict__ kp_valid, const float *__restrict__ keypoints, int F, int K, int P, int M, int min_views, int L,
    int32_t *__restrict__ track_kp, uint8_t *__restrict__ vis, float *__restrict__ track_keypoints, int32_t *__restrict__ track_len,
    int32_t *__restrict__ kp_track, int32_t *__restrict__ counts, void *__restrict__ ws) {
  TrkShared &S = *reinterpret_cast<TrkShared *>(trk_lds);
  int *label = reinterpret_cast<int *>(trk_lds + TRK_SHARED_BYTES);
  const int N = F * K, E = P * M;
  int *aux = label + N;
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x;
  int32_t *edge = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(ws) + b * trk_ws_bytes(P, M));
  pair_frames += b * P * 2;
  match_ij += b * (size_t)E * 2;
  match_valid += b * (size_t)E;
  if (kp_valid) kp_valid += b * (size_t)N;
  keypoints += b * (size_t)N * 2;
  track_kp += b * (size_t)F * L;
  vis += b * (size_t)F * L;
  track_keypoints += b * (size_t)F * L * 2;
  track_len += b * (size_t)L;
  kp_track += b * (size_t)N;

  // ---- empty slots, identity labels, the edges ----------------------------------------------------------------------------
  for (int idx = tid; idx < F * L; idx += TRK_THREADS) {
    track_kp[idx] = -1;
    vis[idx] = 0;
    track_keypoints[2 * (size_t)idx] = 0.0f;
    track_keypoints[2 * (size_t)idx + 1] = 0.0f;
  }
  for (int s = tid; s < L; s += TRK_THREADS) track_len[s] = 0;
  for (int n = tid; n < N; n += TRK_THREADS) {
    label[n] = n;
    aux[n] = 0;
  }
  if (tid < 3) S.counts[tid] = 0;
  for (int e = tid; e < E; e += TRK_THREADS) {
    int packed = -1;
    if (match_valid[e]) {
      const int p = e / M;
      const int fa = pair_frames[2 * p], fb = pair_frames[2 * p + 1];
      if (fa >= 0 && fa < F && fb >= 0 && fb < F && fa != fb) {
        const int i = match_ij[2 * (size_t)e], j = match_ij[2 * (size_t)e + 1];
        if (i >= 0 && i < K && j >= 0 && j < K) {
          const int u = fa * K + i, v = fb * K + j;
          if (!kp_valid || (kp_valid[u] && kp_valid[v])) packed = u << TRK_NODE_BITS | v;
        }
      }
    }
    edge[e] = packed;
  }

  // ---- labels: hook, jump, until nothing changes ----------------------------------------------------------------------------
#pragma unroll 1
  for (int round = 0; round <= N; ++round) {
    if (tid == 0) S.changed = 0;
    __syncthreads();                                 // (also orders the edge stores above before the loads below)
    bool hooked = false;
    for (int e = tid; e < E; e += TRK_THREADS) {
      const int packed = edge[e];
      if (packed < 0) continue;
      const int ru = trk_find(label, packed >> TRK_NODE_BITS), rv = trk_find(label, packed & ((1 << TRK_NODE_BITS) - 1));
      if (ru != rv) {
        atomicMin(&label[ru > rv ? ru : rv], ru < rv ? ru : rv);
        hooked = true;
      }
    }
    if (hooked) atomicOr(&S.changed, 1);
    __syncthreads();
    const int changed = S.changed;                   // the same in every thread
    if (!changed) break;
    for (int n = tid; n < N; n += TRK_THREADS) {
      const int root = trk_find(label, n);
      __atomic_store_n(&label[n], root, __ATOMIC_RELAXED);
    }
    __syncthreads();
  }

  // ---- per root: frame mask and node count -------------------------------------------------------------------------------------
  for (int n = tid; n < N; n += TRK_THREADS) {
    const int root = label[n];
    if (root != n) {                                 // a singleton stays 0: its root adds nothing either
      atomicOr(&aux[root], 1 << (n / K));
      atomicAdd(&aux[root], 1 << 16);
    }
  }
  __syncthreads();
  // a root with members adds itself; everything that gets no slot is judged here
  const int chunk = (N + TRK_THREADS - 1) / TRK_THREADS, n0 = tid * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
  {
    int big = 0, conflicting = 0;
    for (int n = n0; n < n1; ++n) {
      int a = aux[n];
      if (label[n] != n || a == 0) {                 // not a root, or a singleton
        aux[n] = TRK_DONE | 1;
        continue;
      }
      a = (a | 1 << (n / K)) + (1 << 16);
      const int count = a >> 16, mask = a & 0xffff;
      ++big;
      if (count > __popc(mask)) {
        ++conflicting;
        aux[n] = TRK_DONE | 0;
      } else if (count < min_views) {
        aux[n] = TRK_DONE | 1;
      } else {
        aux[n] = a;                                  // eligible: count == popcount(mask) <= F
      }
    }
    if (big) atomicAdd(&S.counts[0], big);
    if (conflicting) atomicAdd(&S.counts[1], conflicting);
  }

  // ---- slots: length descending, label ascending ---------------------------------------------------------------------------------
  int placed = 0;
#pragma unroll 1
  for (int len = F; len >= min_views; --len) {
    int mine = 0;
    for (int n = n0; n < n1; ++n) {
      const int a = aux[n];
      mine += (a >= 0 && (a >> 16) == len) ? 1 : 0;
    }
    int total;
    int slot = placed + trk_block_scan(S, mine, &total);
    if (mine)
      for (int n = n0; n < n1; ++n) {
        const int a = aux[n];
        if (a >= 0 && (a >> 16) == len) {
          aux[n] = TRK_DONE | len << 16 | (slot < L ? slot + 2 : 1);
          ++slot;
        }
      }
    placed += total;
  }
  __syncthreads();                                   // every code is in place; the empty slots written at the start are ordered before

  // ---- write ----------------------------------------------------------------------------------------------------------------------
  for (int n = tid; n < N; n += TRK_THREADS) {
    const int code = aux[label[n]];
    const int slot = (code & 0xffff) - 2;
    kp_track[n] = slot;
    if (slot >= 0) {
      const int f = n / K, k = n - f * K;
      const size_t at = (size_t)f * L + slot;
      track_kp[at] = k;
      vis[at] = 1;
      track_keypoints[2 * at] = keypoints[2 * (size_t)n];
      track_keypoints[2 * at + 1] = keypoints[2 * (size_t)n + 1];
      if (label[n] == n) track_len[slot] = (code >> 16) & 0x7fff;
    }
  }
  if (tid == 0) {
    counts[b * 4] = S.counts[0];
    counts[b * 4 + 1] = S.counts[1];
    counts[b * 4 + 2] = placed;
    counts[b * 4 + 3] = placed < L ? placed : L;
  }
}

__global__ __launch_bounds__(TRK_TRI_THREADS) void tracks_triangulate_kernel(
    const float *__restrict__ r, const float *__restrict__ t, const float *__restrict__ obs, const uint8_t *__restrict__ vis, int F,
    int L, int min_views, float max_e2, float max_cos, float *__restrict__ points, uint8_t *__restrict__ point_ok,
    uint8_t *__restrict__ vis_out, float *__restrict__ e2max, float *__restrict__ cos_par) {
  const int l = blockIdx.x * TRK_TRI_THREADS + threadIdx.x;
  if (l >= L) return;
  const size_t b = blockIdx.y;
  obs += (b * F * L + l) * 2;
  vis += b * F * L + l;
  TrkPoint o;
  trk_triangulate(r + b * F * 9, t + b * F * 3, obs, (size_t)L * 2, vis, (size_t)L, F, min_views, max_e2, max_cos, o);
  const size_t at = b * L + l;
  points[3 * at] = (float)o.X[0];
  points[3 * at + 1] = (float)o.X[1];
  points[3 * at + 2] = (float)o.X[2];
  point_ok[at] = o.ok ? 1 : 0;
  e2max[at] = (float)o.e2max;
  cos_par[at] = (float)o.cos_par;
  for (int f = 0; f < F; ++f) vis_out[b * F * L + (size_t)f * L + l] = (o.ok && vis[(size_t)f * L]) ? 1 : 0;
}

int trk_batch_status(int batch, int frames, int landmarks) {
  if (batch < 1 || frames < 2 || landmarks < 1) return MI_E_SHAPE;
  if (batch > 65535 || frames > MI_TRACKS_MAX_FRAMES || landmarks > MI_BA_MAX_LANDMARKS) return MI_E_PARAM;
  return MI_OK;
}
int trk_shape_status(int batch, int frames, int keypoints, int pairs, int matches, int landmarks) {
  if (batch < 1 || frames < 2 || landmarks < 1 || keypoints < 1 || pairs < 1 || matches < 1) return MI_E_SHAPE;
  if (const int s = trk_batch_status(batch, frames, landmarks)) return s;
  if (keypoints > MI_TRACKS_MAX_KEYPOINTS || pairs > MI_TRACKS_MAX_PAIRS || matches > MI_TRACKS_MAX_MATCHES) return MI_E_PARAM;
  return MI_OK;
}

}  // namespace

extern "C" size_t mi_tracks_workspace_bytes(int batch, int frames, int keypoints, int pairs, int matches, int landmarks) {
  if (trk_shape_status(batch, frames, keypoints, pairs, matches, landmarks) != MI_OK) return 0;
  return (size_t)batch * trk_ws_bytes(pairs, matches);
}

extern "C" int mi_tracks_build(const int32_t *pair_frames, const int32_t *match_ij, const uint8_t *match_valid,
                               const uint8_t *kp_valid, const float *keypoints, int batch, int frames, int keypoints_per_frame,
                               int pairs, int matches, int min_views, int landmarks, int32_t *track_kp, uint8_t *vis,
                               float *track_keypoints, int32_t *track_len, int32_t *kp_track, int32_t *counts, void *workspace,
                               size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pair_frames || !match_ij || !match_valid || !keypoints || !track_kp || !vis || !track_keypoints || !track_len || !kp_track ||
      !counts || !workspace)
    return MI_E_NULL;
  if (const int s = trk_shape_status(batch, frames, keypoints_per_frame, pairs, matches, landmarks)) return s;
  if (min_views < 2 || min_views > frames) return MI_E_PARAM;
  if (((uintptr_t)workspace % 16) != 0) return MI_E_ALIGN;
  if (workspace_bytes < mi_tracks_workspace_bytes(batch, frames, keypoints_per_frame, pairs, matches, landmarks)) return MI_E_CAPACITY;
  const size_t lds = trk_lds_bytes(frames * keypoints_per_frame);
  static size_t allowed = 64 * 1024;                     // raised once, to what the node cap needs (pgo.hip's pattern)
  if (lds > allowed) {
    const size_t most = trk_lds_bytes(MI_TRACKS_MAX_FRAMES * MI_TRACKS_MAX_KEYPOINTS);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(tracks_build_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    if (e != hipSuccess) return (int)e;
    allowed = most;
  }
  hipLaunchKernelGGL(tracks_build_kernel, dim3((unsigned)batch), dim3(TRK_THREADS), lds, (hipStream_t)stream, pair_frames, match_ij,
                     match_valid, kp_valid, keypoints, frames, keypoints_per_frame, pairs, matches, min_views, landmarks, track_kp, vis,
                     track_keypoints, track_len, kp_track, counts, workspace);
  return mi_launch_status();
}

extern "C" int mi_tracks_triangulate(const float *r, const float *t, const float *obs, const uint8_t *vis, int batch, int frames,
                                     int landmarks, int min_views, float max_e2, float max_cos, float *points, uint8_t *point_ok,
                                     uint8_t *vis_out, float *e2max, float *cos_par, mi_stream_t stream) {
  MI_ENTER();
  if (!r || !t || !obs || !vis || !points || !point_ok || !vis_out || !e2max || !cos_par) return MI_E_NULL;
  if (const int s = trk_batch_status(batch, frames, landmarks)) return s;
  if (min_views < 2 || min_views > frames || !(max_e2 > 0.0f) || !(max_e2 < INFINITY) || !(max_cos > -1.0f) || !(max_cos <= 1.0f))
    return MI_E_PARAM;
  hipLaunchKernelGGL(tracks_triangulate_kernel, dim3((unsigned)((landmarks + TRK_TRI_THREADS - 1) / TRK_TRI_THREADS), (unsigned)batch),
                     dim3(TRK_TRI_THREADS), 0, (hipStream_t)stream, r, t, obs, vis, frames, landmarks, min_views, max_e2, max_cos, points,
                     point_ok, vis_out, e2max, cos_par);
  return mi_launch_status();
}
