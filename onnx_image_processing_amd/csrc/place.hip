// K26: loop-closure retrieval on packed BAD descriptors (include/mi355x_match.h, "loop-closure retrieval").
//
// K26a place_votes_kernel -- a workgroup keeps ONE query frame's descriptors and popcounts in LDS and walks the keyframes
//   of its slots in 128-column tiles.  The dot products go through v_mfma_f32_32x32x64_f8f6f4 on K5's nibble expansion
//   (cost.hip: a set bit is the FP4 value 1.0, so the fp32 sum is the popcount of a & b, exact).  The DATABASE descriptors
//   are the A operand and the QUERY descriptors the B operand: in the 32x32 accumulator layout a lane then owns one query
//   row (lane & 31) and its 16 registers are 16 database columns.  The accumulator starts at the column's part of the key
//   (place_math.h), so what the matrix core returns IS the key and the epilogue per product is v_med3_f32 + v_max_f32 on
//   the row's best-two pair, which lives in registers across the accumulator registers, the four 32-column blocks and all
//   column tiles of a keyframe.  A query row belongs to one wave (32-row block b to wave b & 3), so the only merges are the
//   one between the two half-waves (the same query row, rows 4 lh .. of every 8 columns) at the end of a keyframe, and the
//   workgroup sum of the votes.  Nothing but the votes (and, on request, the per-row nearest neighbour) reaches memory; a
//   keyframe's descriptors are read from memory once per (query, slot), the next tile's loads in flight under the MFMAs.
// K26b place_select_kernel -- one workgroup per query, C rounds of a workgroup maximum over 64-bit keys.
#include "common.h"
#include "place_math.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// K5's expansion restated (cost.hip, nibbles_fp4): dword d of the operand takes the bits d, d + 4, d + 8, ... of w where
// they sit, as the nibble 0x2 = 1.0 (E2M1).  Both operands use the same order, so which k a bit lands on does not matter.
__device__ __forceinline__ v8i place_nibbles(uint32_t w) {
  v8i r;
  r[0] = (int)((w << 1) & 0x22222222u);
  r[1] = (int)(w & 0x22222222u);
  r[2] = (int)((w >> 1) & 0x22222222u);
  r[3] = (int)((w >> 2) & 0x22222222u);
  r[4] = r[5] = r[6] = r[7] = 0;
  return r;
}

constexpr int PV_T = 128;            // database columns per tile
constexpr int PV_MAX_GRID_X = 1024;  // workgroups per query: each walks the slots blockIdx.x, + gridDim.x, ...

__host__ __device__ constexpr int pv_round32(int k) { return (k + 31) & ~31; }
// LDS: cst [128] float | wave votes [4] int | sa [128][W + 1] | sq [round32(kq)][W + 1] | pq [round32(kq)] int16
__host__ __device__ constexpr size_t pv_lds_bytes(int words, int kq) {
  return (size_t)(PV_T + 4) * 4 + (size_t)(PV_T + pv_round32(kq)) * (words + 1) * 4 + (size_t)pv_round32(kq) * 2;
}

// W: words per descriptor (8 / 16).  QB: 32-row query blocks per wave, kq <= 128 QB.
template <int W, int QB>
__global__ __launch_bounds__(256) void place_votes_kernel(const uint32_t *__restrict__ db_bits, const uint8_t *__restrict__ db_valid,
                                                          int kd, const uint32_t *__restrict__ q_bits,
                                                          const uint8_t *__restrict__ q_valid, int kq,
                                                          const int32_t *__restrict__ frame_index, int slots, int max_distance,
                                                          float ratio, int32_t *__restrict__ votes, int32_t *__restrict__ nn_index,
                                                          int32_t *__restrict__ nn_distance, uint8_t *__restrict__ nn_vote) {
  extern __shared__ uint32_t lds_u[];
  constexpr int WP = W + 1;                            // +1 word: conflict-free column reads (K5)
  constexpr int NUM_BITS = 32 * W, ABSENT = NUM_BITS + 1;
  constexpr int CPR = W / 4;                           // 16-byte chunks per descriptor
  constexpr int CPT = PV_T * CPR / 256;                // chunks per thread and tile: 1 / 2
  const int kq_pad = pv_round32(kq);
  float *cst = reinterpret_cast<float *>(lds_u);       // [128] the accumulator start of the tile's columns
  int *wave_votes = reinterpret_cast<int *>(lds_u + PV_T);
  uint32_t *sa = lds_u + PV_T + 4;                     // [128][WP] database tile
  uint32_t *sq = sa + PV_T * WP;                       // [kq_pad][WP] the query frame
  int16_t *pq = reinterpret_cast<int16_t *>(sq + kq_pad * WP);   // [kq_pad] popcount, -1 = invalid row

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int q = blockIdx.y;

  // ---- the query frame, once per workgroup
  {
    const uint32_t *qg = q_bits + (size_t)q * kq * W;
    for (int i = t; i < kq_pad * W; i += 256) {
      const int r = i / W, c = i - r * W;
      sq[r * WP + c] = r < kq ? qg[i] : 0u;
    }
    __syncthreads();
    for (int r = t; r < kq_pad; r += 256) {
      int pop = 0;
#pragma unroll
      for (int c = 0; c < W; ++c) pop += __popc(sq[r * WP + c]);
      const bool ok = r < kq && (!q_valid || q_valid[(size_t)q * kq + r] != 0);
      pq[r] = (int16_t)(ok ? pop : -1);
    }
  }

  const int ntiles = (kd + PV_T - 1) / PV_T;
  uint4 pre[CPT];
  bool pre_valid = false;
  auto fetch = [&](int f, int tile) {                  // tile `tile` of keyframe f into registers
    const int j0 = tile * PV_T;
    const uint4 *src = reinterpret_cast<const uint4 *>(db_bits + ((size_t)f * kd + j0) * W);
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int ch = t + 256 * c;
      pre[c] = make_uint4(0u, 0u, 0u, 0u);
      if (j0 + ch / CPR < kd) pre[c] = src[ch];
    }
    pre_valid = t < PV_T && j0 + t < kd && (!db_valid || db_valid[(size_t)f * kd + j0 + t] != 0);
  };

  for (int slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int f = frame_index ? frame_index[(size_t)q * slots + slot] : slot;
    const size_t out0 = ((size_t)q * slots + slot) * kq;
    if (f < 0) {                                       // an empty slot (workgroup-uniform)
      if (t == 0) votes[(size_t)q * slots + slot] = 0;
      if (nn_index)
        for (int i = t; i < kq; i += 256) {
          nn_index[out0 + i] = -1;
          nn_distance[out0 + i] = ABSENT;
          nn_vote[out0 + i] = 0;
        }
      continue;
    }
    PlacePair best[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) best[qi].m1 = best[qi].m2 = -INFINITY;

    fetch(f, 0);
    for (int tile = 0; tile < ntiles; ++tile) {
      __syncthreads();                                 // the previous tile's readers are done (and the query is in LDS)
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int ch = t + 256 * c;
        const int r = ch / CPR, col = (ch - r * CPR) * 4;
        uint32_t *d = sa + r * WP + col;
        d[0] = pre[c].x; d[1] = pre[c].y; d[2] = pre[c].z; d[3] = pre[c].w;
      }
      const bool col_valid = pre_valid;
      __syncthreads();
      if (t < PV_T) {
        int pop = 0;
#pragma unroll
        for (int c = 0; c < W; ++c) pop += __popc(sa[t * WP + c]);
        cst[t] = place_col_start(pop, tile * PV_T + t, col_valid);
      }
      if (tile + 1 < ntiles) fetch(f, tile + 1);       // in flight during the MFMAs below
      __syncthreads();

#pragma unroll
      for (int qi = 0; qi < QB; ++qi) {
        const int qblk = wave + 4 * qi;
        if (qblk * 32 < kq) {                          // wave-uniform
          v16f acc[4];
#pragma unroll
          for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int g = 0; g < 4; ++g) {              // register e = 4 g + i is column 32 blk + 8 g + 4 lh + i
              const float4 c4 = *reinterpret_cast<const float4 *>(cst + 32 * blk + 8 * g + 4 * lh);
              acc[blk][4 * g + 0] = c4.x; acc[blk][4 * g + 1] = c4.y; acc[blk][4 * g + 2] = c4.z; acc[blk][4 * g + 3] = c4.w;
            }
          const uint32_t *qrow = sq + (qblk * 32 + lr) * WP + lh;
          const uint32_t *arow = sa + lr * WP + lh;
#pragma unroll
          for (int ks = 0; ks < W / 2; ++ks) {
            const v8i fb = place_nibbles(qrow[2 * ks]);
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
              const v8i fa = place_nibbles(arow[blk * 32 * WP + 2 * ks]);
              acc[blk] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa, fb, acc[blk], 4, 4, 0, 0, 0, 0);
            }
          }
#pragma unroll
          for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int e = 0; e < 16; ++e) place_push(best[qi], acc[blk][e]);
        }
      }
    }

    // ---- the keyframe is done: the two half-waves hold the same query rows over different columns
    int count = 0;
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
      const int qblk = wave + 4 * qi;
      if (qblk * 32 < kq) {
        PlacePair other;
        other.m1 = __shfl_xor(best[qi].m1, 32, 64);
        other.m2 = __shfl_xor(best[qi].m2, 32, 64);
        const PlacePair r = place_merge(best[qi], other);
        const int row = qblk * 32 + lr;
        const int pop = pq[row];
        int d1, j1, d2, j2;
        place_decode(r.m1, pop, NUM_BITS, &d1, &j1);
        place_decode(r.m2, pop, NUM_BITS, &d2, &j2);
        const bool row_ok = pop >= 0;                  // false for the padding rows too
        if (!row_ok) { d1 = ABSENT; j1 = -1; }
        const bool vote = row_ok && lh == 0 && place_votes_for(d1, d2, max_distance, ratio);
        if (nn_index && lh == 0 && row < kq) {
          nn_index[out0 + row] = j1;
          nn_distance[out0 + row] = d1;
          nn_vote[out0 + row] = vote ? 1 : 0;
        }
        count += __popcll(__ballot(vote));
      }
    }
    if (lane == 0) wave_votes[wave] = count;
    __syncthreads();
    if (t == 0) votes[(size_t)q * slots + slot] = (wave_votes[0] + wave_votes[1]) + (wave_votes[2] + wave_votes[3]);
    // wave_votes is rewritten only after the barriers of the next slot's first tile
  }
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    const uint64_t w = ((uint64_t)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void place_select_kernel(const int32_t *__restrict__ votes, int n,
                                                           const int32_t *__restrict__ excl_lo,
                                                           const int32_t *__restrict__ excl_hi, int min_votes, int c,
                                                           int32_t *__restrict__ cand_index, int32_t *__restrict__ cand_votes) {
  __shared__ uint64_t wmax[2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = blockIdx.x;
  const int32_t *v = votes + (size_t)q * n;
  const int lo = excl_lo ? excl_lo[q] : 0, hi = excl_lo ? excl_hi[q] : 0;
  uint64_t prev = ~0ull;                               // round r takes the largest key below round r - 1's
  for (int r = 0; r < c; ++r) {
    uint64_t best = 0;                                 // no key is 0
    if (prev != 0)                                     // workgroup-uniform: nothing is left after an empty round
      for (int i = t; i < n; i += 256) {
        const int32_t vi = v[i];
        if (vi >= min_votes && !(i >= lo && i < hi)) {
          const uint64_t key = place_select_key(vi, (uint32_t)i);
          if (key < prev && key > best) best = key;
        }
      }
    best = wave_max_u64(best);
    if (lane == 0) wmax[r & 1][wave] = best;
    __syncthreads();                                   // two buffers: round r + 1 writes the other one
    const uint64_t a = wmax[r & 1][0], b = wmax[r & 1][1], d = wmax[r & 1][2], e = wmax[r & 1][3];
    const uint64_t ab = a > b ? a : b, de = d > e ? d : e;
    best = ab > de ? ab : de;
    if (t == 0) {
      cand_index[(size_t)q * c + r] = best ? place_key_index(best) : -1;
      cand_votes[(size_t)q * c + r] = best ? place_key_votes(best) : 0;
    }
    prev = best;
  }
}

template <typename K>
int pv_allow_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return MI_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  return e == hipSuccess ? MI_OK : (int)e;
}

template <int W, int QB>
int pv_launch(const uint32_t *db_bits, const uint8_t *db_valid, int kd, const uint32_t *q_bits, const uint8_t *q_valid, int q,
              int kq, const int32_t *frame_index, int slots, int max_distance, float ratio, int32_t *votes, int32_t *nn_index,
              int32_t *nn_distance, uint8_t *nn_vote, hipStream_t stream) {
  const size_t lds = pv_lds_bytes(W, kq);
  static size_t allowed = 64 * 1024;                   // per instantiation; raised once (a repeated call would be harmless)
  if (lds > allowed) {
    const int e = pv_allow_lds(place_votes_kernel<W, QB>, pv_lds_bytes(W, 128 * QB));
    if (e != MI_OK) return e;
    allowed = pv_lds_bytes(W, 128 * QB);
  }
  const dim3 grid((unsigned)(slots < PV_MAX_GRID_X ? slots : PV_MAX_GRID_X), (unsigned)q);
  hipLaunchKernelGGL((place_votes_kernel<W, QB>), grid, dim3(256), lds, stream, db_bits, db_valid, kd, q_bits, q_valid, kq,
                     frame_index, slots, max_distance, ratio, votes, nn_index, nn_distance, nn_vote);
  return mi_launch_status();
}

template <int W>
int pv_dispatch(const uint32_t *db_bits, const uint8_t *db_valid, int kd, const uint32_t *q_bits, const uint8_t *q_valid, int q,
                int kq, const int32_t *frame_index, int slots, int max_distance, float ratio, int32_t *votes, int32_t *nn_index,
                int32_t *nn_distance, uint8_t *nn_vote, hipStream_t stream) {
#define PV_GO(QB) \
  return pv_launch<W, QB>(db_bits, db_valid, kd, q_bits, q_valid, q, kq, frame_index, slots, max_distance, ratio, votes, nn_index, \
                          nn_distance, nn_vote, stream)
  if (kq <= 128) PV_GO(1);
  if (kq <= 256) PV_GO(2);
  if (kq <= 512) PV_GO(4);
  PV_GO(8);
#undef PV_GO
}

}  // namespace

extern "C" int mi_place_votes(const uint32_t *db_bits, const uint8_t *db_valid, int n, int kd, const uint32_t *q_bits,
                              const uint8_t *q_valid, int q, int kq, const int32_t *frame_index, int slots, int num_bits,
                              int max_distance, float ratio, int32_t *votes, int32_t *nn_index, int32_t *nn_distance,
                              uint8_t *nn_vote, mi_stream_t stream) {
  MI_ENTER();
  if (!db_bits || !q_bits || !votes) return MI_E_NULL;
  if ((nn_index != nullptr) != (nn_distance != nullptr) || (nn_index != nullptr) != (nn_vote != nullptr)) return MI_E_NULL;
  if (n < 1 || kd < 1 || q < 1 || kq < 1 || slots < 1) return MI_E_SHAPE;
  if (!frame_index && slots != n) return MI_E_SHAPE;
  if (n > MI_PLACE_MAX_KEYFRAMES || kd > MI_PLACE_MAX_DESCRIPTORS || kq > MI_PLACE_MAX_DESCRIPTORS || q > 65535) return MI_E_PARAM;
  if (num_bits != 256 && num_bits != 512) return MI_E_PARAM;
  if (max_distance < 0 || max_distance > num_bits || !(ratio > 0.0f && ratio <= 1.0f)) return MI_E_PARAM;
  if (((uintptr_t)db_bits % 16) != 0 || ((uintptr_t)q_bits % 4) != 0 || ((uintptr_t)votes % 4) != 0 ||
      ((uintptr_t)frame_index % 4) != 0 || ((uintptr_t)nn_index % 4) != 0 || ((uintptr_t)nn_distance % 4) != 0)
    return MI_E_ALIGN;
  if (num_bits == 256)
    return pv_dispatch<8>(db_bits, db_valid, kd, q_bits, q_valid, q, kq, frame_index, slots, max_distance, ratio, votes, nn_index,
                          nn_distance, nn_vote, (hipStream_t)stream);
  return pv_dispatch<16>(db_bits, db_valid, kd, q_bits, q_valid, q, kq, frame_index, slots, max_distance, ratio, votes, nn_index,
                         nn_distance, nn_vote, (hipStream_t)stream);
}

extern "C" int mi_place_select(const int32_t *votes, int q, int n, const int32_t *excl_lo, const int32_t *excl_hi, int min_votes,
                               int num_candidates, int32_t *cand_index, int32_t *cand_votes, mi_stream_t stream) {
  MI_ENTER();
  if (!votes || !cand_index || !cand_votes || (excl_lo != nullptr) != (excl_hi != nullptr)) return MI_E_NULL;
  if (q < 1 || n < 1) return MI_E_SHAPE;
  if (n > MI_PLACE_MAX_KEYFRAMES || num_candidates < 1 || num_candidates > MI_PLACE_MAX_CANDIDATES) return MI_E_PARAM;
  if (((uintptr_t)votes % 4) != 0 || ((uintptr_t)excl_lo % 4) != 0 || ((uintptr_t)excl_hi % 4) != 0 ||
      ((uintptr_t)cand_index % 4) != 0 || ((uintptr_t)cand_votes % 4) != 0)
    return MI_E_ALIGN;
  hipLaunchKernelGGL(place_select_kernel, dim3((unsigned)q), dim3(256), 0, (hipStream_t)stream, votes, n, excl_lo, excl_hi,
                     min_votes, num_candidates, cand_index, cand_votes);
  return mi_launch_status();
}
