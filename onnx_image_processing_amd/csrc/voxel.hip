// K12 voxel-grid downsampling (reference pointcloud/voxel_downsampling.py:16-104) for a batch of ragged clouds.
//
// One call, every launch on `stream`, nothing read back to the host:
//   init      (1 block)   sanitised offsets, per-cloud min / max slots
//   minmax    (points)    per-cloud min / max of floor(p / leaf) over columns 0-2 (64-bit integer atomics, one per wave)
//   plan      (1 block)   per-cloud extents, the key's significant bits, cloud-relative segment tiles
//   keys      (points)    64-bit key per point (wrapping uint64 arithmetic; sign bit flipped when a cloud overflows),
//                         payload = point index
//   radix     3 launches per 8-bit digit: tile histograms, per-digit scans of the tile counts, stable scatter (ranks
//                         within a wave from 64-bit ballots).  Key digits first (passes at or above the device-known bit
//                         count return at once), cloud-id digits last; which buffer holds the result follows from the
//                         number of active passes, which every kernel derives from the plan.
//   seg_count (tiles)     segment starts per tile, tiles of 256 sorted rows that restart at each cloud's first row
//   seg_scan  (1 block)   voxel numbering per cloud, M_b
//   seg_sum   (tiles)     fp64 segmented scan of the gathered points inside each tile; voxels that end in their tile
//                         are written as (float)(sum / count); pieces of voxels that cross a tile edge are kept
//   seg_fixup (tiles)     voxels spanning tiles: the pieces summed by one workgroup in a fixed tree order
// No float atomics, no cross-workgroup waits, no hipMemset: every result is bitwise reproducible and a cloud's results do
// not depend on what else is in the batch (all summation tiles are cloud-relative).  Addresses only ever come from
// indices, sanitised offsets and scan results; key digits index 256-entry LDS tables through an 8-bit mask.
#include "common.h"

namespace {

constexpr int VX_THREADS = 256;
constexpr int RADIX_ITEMS = 16;                               // per thread
constexpr int RADIX_TILE = VX_THREADS * RADIX_ITEMS;          // 4096 keys; one wave ranks 1024 contiguous keys
constexpr int SEG_TILE = VX_THREADS;                          // one sorted row per thread
constexpr int KEY_PASSES = 8;

struct VxPlan {
  int nbits;          // significant key bits over the batch (64 when any cloud's key overflows int64)
  int ntiles;         // segment tiles over the batch
  int pad[2];
};
struct VxCloud {      // per cloud: the minima and the key's strides
  long long mn[3];
  unsigned long long d1, d2;
  unsigned long long flip;
};

struct VxLayout {
  VxPlan *plan;
  long long *soff;          // B+1 sanitised offsets
  long long *mm;            // B x 6: min0..2, max0..2
  VxCloud *cloud;           // B
  int *tile_start;          // B+1
  unsigned *mcount;         // B: voxels per cloud
  unsigned long long *keys[2];
  unsigned *idx[2];
  unsigned *counts;         // 256 x radix tiles
  unsigned *dtot;           // 256
  unsigned *tflags;         // segment tiles: segment starts
  unsigned *texcl;          // segment tiles + 1: exclusive scan of tflags
  double *head_sum, *tail_sum;          // segment tiles x d
  unsigned *head_cnt, *tail_cnt, *tail_vox, *tinfo;   // tinfo bit 0: the tile owns a voxel spanning tiles; bit 1: its row 0 starts a voxel
  size_t bytes;
};

inline size_t vx_align(size_t x) { return (x + 255) & ~(size_t)255; }

VxLayout vx_layout(void *base, int batch, long long total, int d) {
  VxLayout L{};
  const size_t T = (size_t)total, B = (size_t)batch;
  const size_t nrt = (T + RADIX_TILE - 1) / RADIX_TILE;
  const size_t mt = (T + SEG_TILE - 1) / SEG_TILE + B;
  char *p = static_cast<char *>(base);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char *q = p ? p + o : nullptr;
    o += vx_align(bytes);
    return q;
  };
  L.plan = (VxPlan *)take(sizeof(VxPlan));
  L.soff = (long long *)take((B + 1) * 8);
  L.mm = (long long *)take(B * 6 * 8);
  L.cloud = (VxCloud *)take(B * sizeof(VxCloud));
  L.tile_start = (int *)take((B + 1) * 4);
  L.mcount = (unsigned *)take(B * 4);
  L.keys[0] = (unsigned long long *)take(T * 8);
  L.keys[1] = (unsigned long long *)take(T * 8);
  L.idx[0] = (unsigned *)take(T * 4);
  L.idx[1] = (unsigned *)take(T * 4);
  L.counts = (unsigned *)take(256 * nrt * 4);
  L.dtot = (unsigned *)take(256 * 4);
  L.tflags = (unsigned *)take(mt * 4);
  L.texcl = (unsigned *)take((mt + 1) * 4);
  L.head_sum = (double *)take(mt * (size_t)d * 8);
  L.tail_sum = (double *)take(mt * (size_t)d * 8);
  L.head_cnt = (unsigned *)take(mt * 4);
  L.tail_cnt = (unsigned *)take(mt * 4);
  L.tail_vox = (unsigned *)take(mt * 4);
  L.tinfo = (unsigned *)take(mt * 4);
  L.bytes = o;
  return L;
}

// largest b in [0, n) with a[b] <= x (a ascending, a[0] <= x): the cloud of a point / row, or of a tile
template <typename T>
__device__ __forceinline__ int vx_upper(const T *a, int n, long long x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)a[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ long long vx_coord(float p, float leaf) { return (long long)floorf(p / leaf); }

// Block-wide exclusive scan of one value per thread (256 threads); returns the exclusive prefix, *total the sum.
template <typename T>
__device__ T vx_block_excl(T v, T *lds, T *total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < VX_THREADS; off <<= 1) {
    const T left = t >= off ? lds[t - off] : T(0);
    __syncthreads();
    lds[t] += left;
    __syncthreads();
  }
  const T incl = lds[t];
  *total = lds[VX_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// ---- init: offsets[b] clamped into [offsets[b-1], total] (a running maximum), offsets[B] = total; min / max slots
__global__ __launch_bounds__(VX_THREADS) void vx_init_kernel(const long long *__restrict__ offsets, int batch, long long total,
                                                               VxLayout L) {
  __shared__ long long lds[VX_THREADS];
  long long carry = 0;
  for (int base = 0; base <= batch; base += VX_THREADS) {
    const int b = base + threadIdx.x;
    long long v = b <= batch ? offsets[b] : 0;
    v = v < 0 ? 0 : (v > total ? total : v);
    if (b == 0) v = 0;
    if (b == batch) v = total;
    // inclusive running max over the block
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < VX_THREADS; off <<= 1) {
      const long long left = threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
      __syncthreads();
      if (left > lds[threadIdx.x]) lds[threadIdx.x] = left;
      __syncthreads();
    }
    long long m = lds[threadIdx.x];
    if (carry > m) m = carry;
    if (b <= batch) L.soff[b] = m;
    const long long last = lds[VX_THREADS - 1];
    __syncthreads();
    if (last > carry) carry = last;
  }
  for (int b = threadIdx.x; b < batch; b += VX_THREADS) {
    long long *s = L.mm + (size_t)b * 6;
    s[0] = s[1] = s[2] = INT64_MAX;
    s[3] = s[4] = s[5] = INT64_MIN;
  }
}

// ---- minmax: each wave takes 64 x 16 consecutive points; a wave inside one cloud reduces first (6 atomics per wave)
constexpr int MM_PER_LANE = 16;
__global__ __launch_bounds__(VX_THREADS) void vx_minmax_kernel(const float *__restrict__ pts, int batch, int total, int d,
                                                                 const float *__restrict__ leaf, VxLayout L) {
  const int lane = threadIdx.x & 63;
  const long long w0 = ((long long)blockIdx.x * (VX_THREADS / 64) + (threadIdx.x >> 6)) * (64 * MM_PER_LANE);
  if (w0 >= total) return;
  const long long w1 = w0 + 64 * MM_PER_LANE < total ? w0 + 64 * MM_PER_LANE : total;
  const int b0 = vx_upper(L.soff, batch, w0), b1 = vx_upper(L.soff, batch, w1 - 1);
  if (b0 == b1) {
    const float lf = leaf[b0];
    long long mn[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, mx[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    for (long long i = w0 + lane; i < w1; i += 64) {
      const float *p = pts + i * d;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long v = vx_coord(p[c], lf);
        mn[c] = v < mn[c] ? v : mn[c];
        mx[c] = v > mx[c] ? v : mx[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_xor(mn[c], o, 64), z = __shfl_xor(mx[c], o, 64);
        mn[c] = a < mn[c] ? a : mn[c];
        mx[c] = z > mx[c] ? z : mx[c];
      }
    }
    if (lane == 0) {
      long long *s = L.mm + (size_t)b0 * 6;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        atomicMin(s + c, mn[c]);
        atomicMax(s + 3 + c, mx[c]);
      }
    }
  } else {        // a wave across cloud boundaries (rare unless clouds are tiny): per point
    for (long long i = w0 + lane; i < w1; i += 64) {
      const int b = vx_upper(L.soff, batch, i);
      const float lf = leaf[b];
      const float *p = pts + i * d;
      long long *s = L.mm + (size_t)b * 6;
      for (int c = 0; c < 3; ++c) {
        const long long v = vx_coord(p[c], lf);
        atomicMin(s + c, v);
        atomicMax(s + 3 + c, v);
      }
    }
  }
}

// ---- plan: extents d_j = max_j - min_j + 1; key bits of a cloud = bits of d0*d1*d2 - 1 when that product fits int64,
// else 64 (the reference's int64 key wraps and is sorted as signed: such keys are sign-flipped so that unsigned order is
// signed order, and then every key of the batch is); tiles of SEG_TILE rows per cloud
__global__ __launch_bounds__(VX_THREADS) void vx_plan_kernel(int batch, VxLayout L) {
  __shared__ int lds[VX_THREADS];
  __shared__ int s_bits, s_flip;
  if (threadIdx.x == 0) s_bits = 0, s_flip = 0;
  __syncthreads();
  int carry = 0;
  for (int base = 0; base < batch; base += VX_THREADS) {
    const int b = base + threadIdx.x;
    int ntiles = 0;
    if (b < batch) {
      const long long n = L.soff[b + 1] - L.soff[b];
      const long long *s = L.mm + (size_t)b * 6;
      VxCloud c{};
      if (n > 0) {
        unsigned long long dd[3];
        for (int j = 0; j < 3; ++j) {
          c.mn[j] = s[j];
          dd[j] = (unsigned long long)s[3 + j] - (unsigned long long)s[j] + 1ull;
        }
        c.d1 = dd[1];
        c.d2 = dd[2];
        unsigned long long p12, p;
        const bool ovf = __builtin_umulll_overflow(dd[1], dd[2], &p12) || __builtin_umulll_overflow(dd[0], p12, &p) ||
                         p == 0 || p - 1ull > (unsigned long long)INT64_MAX;
        int bits = 64;
        if (!ovf) bits = (p - 1ull) == 0 ? 0 : 64 - __clzll((long long)(p - 1ull));
        else atomicOr(&s_flip, 1);
        atomicMax(&s_bits, bits);
        ntiles = (int)((n + SEG_TILE - 1) / SEG_TILE);
      } else {
        c.mn[0] = c.mn[1] = c.mn[2] = 0;
        c.d1 = c.d2 = 1;
      }
      L.cloud[b] = c;
    }
    int tot;
    const int ex = vx_block_excl(ntiles, lds, &tot);
    if (b < batch) L.tile_start[b] = carry + ex;
    carry += tot;
  }
  __syncthreads();
  const unsigned long long flip = s_flip ? (1ull << 63) : 0ull;
  for (int b = threadIdx.x; b < batch; b += VX_THREADS) L.cloud[b].flip = flip;
  if (threadIdx.x == 0) {
    L.tile_start[batch] = carry;
    L.plan->nbits = s_flip ? 64 : s_bits;
    L.plan->ntiles = carry;
  }
}

// ---- keys: c0*d1*d2 + c1*d2 + c2 on the shifted coordinates, wrapping (the reference's int64 arithmetic bit for bit)
__global__ __launch_bounds__(VX_THREADS) void vx_keys_kernel(const float *__restrict__ pts, int batch, int total, int d,
                                                               const float *__restrict__ leaf, VxLayout L) {
  const int i = blockIdx.x * VX_THREADS + threadIdx.x;
  if (i >= total) return;
  const int b = vx_upper(L.soff, batch, i);
  const VxCloud c = L.cloud[b];
  const float lf = leaf[b];
  const float *p = pts + (size_t)i * d;
  const unsigned long long k0 = (unsigned long long)vx_coord(p[0], lf) - (unsigned long long)c.mn[0];
  const unsigned long long k1 = (unsigned long long)vx_coord(p[1], lf) - (unsigned long long)c.mn[1];
  const unsigned long long k2 = (unsigned long long)vx_coord(p[2], lf) - (unsigned long long)c.mn[2];
  L.keys[0][i] = (k0 * c.d1 * c.d2 + k1 * c.d2 + k2) ^ c.flip;
  L.idx[0][i] = (unsigned)i;
}

// ---- radix passes.  pass < KEY_PASSES: key digit `pass`; pass >= KEY_PASSES: cloud-id digit pass - KEY_PASSES.
// Returns -1 for an inactive pass, else the index of the buffer the pass reads.
__device__ __forceinline__ int vx_pass_src(const VxPlan *plan, int pass) {
  const int nbits = plan->nbits;
  const int kp = (nbits + 7) >> 3;
  if (pass < KEY_PASSES) return 8 * pass >= nbits ? -1 : (pass & 1);
  return (kp + pass - KEY_PASSES) & 1;
}
__device__ __forceinline__ unsigned vx_digit(unsigned long long key, unsigned idx, int pass, const long long *soff, int batch) {
  if (pass < KEY_PASSES) return (unsigned)(key >> (8 * pass)) & 255u;
  return ((unsigned)vx_upper(soff, batch, idx) >> (8 * (pass - KEY_PASSES))) & 255u;
}

__global__ __launch_bounds__(VX_THREADS) void vx_hist_kernel(int batch, int total, int pass, VxLayout L) {
  __shared__ unsigned hist[256];
  const int src = vx_pass_src(L.plan, pass);
  if (src < 0) return;
  const int nrt = (total + RADIX_TILE - 1) / RADIX_TILE;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long *keys = L.keys[src];
  const unsigned *idx = L.idx[src];
  const long long base = (long long)blockIdx.x * RADIX_TILE + (threadIdx.x >> 6) * (RADIX_TILE / 4) + (threadIdx.x & 63);
#pragma unroll 4
  for (int r = 0; r < RADIX_ITEMS; ++r) {
    const long long i = base + r * 64;
    if (i < total) atomicAdd(&hist[vx_digit(keys[i], pass < KEY_PASSES ? 0u : idx[i], pass, L.soff, batch)], 1u);
  }
  __syncthreads();
  L.counts[(size_t)threadIdx.x * nrt + blockIdx.x] = hist[threadIdx.x];
}

// one block per digit: exclusive scan of that digit's tile counts in place, the digit's total to dtot
__global__ __launch_bounds__(VX_THREADS) void vx_rowscan_kernel(int total, int pass, VxLayout L) {
  __shared__ unsigned lds[VX_THREADS];
  if (vx_pass_src(L.plan, pass) < 0) return;
  const int nrt = (total + RADIX_TILE - 1) / RADIX_TILE;
  unsigned *row = L.counts + (size_t)blockIdx.x * nrt;
  unsigned carry = 0;
  for (int base = 0; base < nrt; base += VX_THREADS) {
    const int t = base + threadIdx.x;
    const unsigned v = t < nrt ? row[t] : 0u;
    unsigned tot;
    const unsigned ex = vx_block_excl(v, lds, &tot);
    if (t < nrt) row[t] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) L.dtot[blockIdx.x] = carry;
}

// stable scatter: wave w of the tile ranks its 1024 keys in order (16 rounds of 64; lanes with equal digits found with
// eight 64-bit ballots), then destination = digit base + tile offset + keys of that digit in earlier waves + rank
__global__ __launch_bounds__(VX_THREADS) void vx_scatter_kernel(int batch, int total, int pass, VxLayout L) {
  __shared__ unsigned wc[4][256];
  __shared__ unsigned gbase[256];
  __shared__ unsigned lds[VX_THREADS];
  const int src = vx_pass_src(L.plan, pass);
  if (src < 0) return;
  const int nrt = (total + RADIX_TILE - 1) / RADIX_TILE;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  {
    unsigned tot;
    const unsigned ex = vx_block_excl(L.dtot[t], lds, &tot);
    gbase[t] = ex + L.counts[(size_t)t * nrt + blockIdx.x];
    for (int k = 0; k < 4; ++k) wc[k][t] = 0;
  }
  __syncthreads();
  const unsigned long long *keys = L.keys[src];
  const unsigned *idx = L.idx[src];
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long long base = (long long)blockIdx.x * RADIX_TILE + w * (RADIX_TILE / 4) + lane;
  unsigned long long k[RADIX_ITEMS];
  unsigned id[RADIX_ITEMS], rank[RADIX_ITEMS];
#pragma unroll
  for (int r = 0; r < RADIX_ITEMS; ++r) {
    const long long i = base + r * 64;
    const bool valid = i < total;
    k[r] = valid ? keys[i] : 0ull;
    id[r] = valid ? idx[i] : 0u;
  }
#pragma unroll
  for (int r = 0; r < RADIX_ITEMS; ++r) {
    const bool valid = base + r * 64 < total;
    const unsigned dg = vx_digit(k[r], id[r], pass, L.soff, batch);
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (dg >> bit) & 1u;
      const unsigned long long m = __ballot(on);
      peers &= on ? m : ~m;
    }
    const unsigned before = wc[w][dg];
    rank[r] = (before + (unsigned)__popcll(peers & lt)) | (dg << 24);   // rank < 1024
    if (valid && (peers & lt) == 0ull) wc[w][dg] = before + (unsigned)__popcll(peers);
  }
  __syncthreads();
  {
    unsigned pref = 0;
    for (int q = 0; q < 4; ++q) {
      const unsigned c = wc[q][t];
      wc[q][t] = pref + gbase[t];
      pref += c;
    }
  }
  __syncthreads();
  unsigned long long *okeys = L.keys[src ^ 1];
  unsigned *oidx = L.idx[src ^ 1];
#pragma unroll
  for (int r = 0; r < RADIX_ITEMS; ++r) {
    if (base + r * 64 >= total) continue;
    const unsigned dg = rank[r] >> 24;
    const unsigned dst = wc[w][dg] + (rank[r] & 0xFFFFFFu);
    if (dst < (unsigned)total) {
      okeys[dst] = k[r];
      oidx[dst] = id[r];
    }
  }
}

// ---- segments.  Sorted row r (cloud b, local row l = r - off_b) starts a voxel iff l == 0 or key[r] != key[r-1].
struct VxTile {
  int b;
  long long off, rows;     // cloud's first row and length
  long long l0;            // tile's first local row
  int nrows;               // rows of this tile
};
__device__ __forceinline__ bool vx_tile(const VxLayout &L, int batch, int t, VxTile *T) {
  if (t >= L.plan->ntiles) return false;
  const int b = vx_upper(L.tile_start, batch, t);
  T->b = b;
  T->off = L.soff[b];
  T->rows = L.soff[b + 1] - T->off;
  T->l0 = (long long)(t - L.tile_start[b]) * SEG_TILE;
  const long long left = T->rows - T->l0;
  T->nrows = left < SEG_TILE ? (int)left : SEG_TILE;
  return true;
}
__device__ __forceinline__ const unsigned long long *vx_sorted_keys(const VxLayout &L, int cpasses) {
  const int kp = (L.plan->nbits + 7) >> 3;
  return L.keys[(kp + cpasses) & 1];
}
__device__ __forceinline__ const unsigned *vx_sorted_idx(const VxLayout &L, int cpasses) {
  const int kp = (L.plan->nbits + 7) >> 3;
  return L.idx[(kp + cpasses) & 1];
}

__global__ __launch_bounds__(VX_THREADS) void vx_seg_count_kernel(int batch, int cpasses, VxLayout L) {
  VxTile T;
  if (!vx_tile(L, batch, blockIdx.x, &T)) return;
  const unsigned long long *keys = vx_sorted_keys(L, cpasses);
  const long long l = T.l0 + threadIdx.x, r = T.off + l;
  const bool start = threadIdx.x < T.nrows && (l == 0 || keys[r] != keys[r - 1]);
  const int n = __syncthreads_count(start);
  if (threadIdx.x == 0) L.tflags[blockIdx.x] = (unsigned)n;
}

// voxel numbering: texcl = exclusive scan of tflags over all tiles; M_b = starts in cloud b's tiles
__global__ __launch_bounds__(VX_THREADS) void vx_seg_scan_kernel(int batch, VxLayout L, long long *__restrict__ out_counts) {
  __shared__ unsigned lds[VX_THREADS];
  const int nt = L.plan->ntiles;
  unsigned carry = 0;
  for (int base = 0; base < nt; base += VX_THREADS) {
    const int t = base + threadIdx.x;
    unsigned tot;
    const unsigned ex = vx_block_excl(t < nt ? L.tflags[t] : 0u, lds, &tot);
    if (t < nt) L.texcl[t] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) L.texcl[nt] = carry;
  __syncthreads();
  for (int b = threadIdx.x; b < batch; b += VX_THREADS) {
    const unsigned m = L.texcl[L.tile_start[b + 1]] - L.texcl[L.tile_start[b]];
    L.mcount[b] = m;
    out_counts[b] = m;
  }
}

// fp64 segmented inclusive scan over the tile's rows (Hillis-Steele: the same tree for every tile, so a voxel's sum
// depends only on its rows' positions relative to the cloud), DC columns per round; voxels that start and end in the
// tile are finished here.  Also the tile's share of the padding rows and of the mask.
template <int DC>
__global__ __launch_bounds__(VX_THREADS) void vx_seg_sum_kernel(const float *__restrict__ pts, int batch, int d, int cpasses,
                                                                  VxLayout L, float *__restrict__ out, uint8_t *__restrict__ mask) {
  __shared__ double sv[2][DC][VX_THREADS];
  __shared__ unsigned char sf[2][VX_THREADS];
  __shared__ int wlast[4];
  __shared__ unsigned wcnt[4];
  VxTile T;
  if (!vx_tile(L, batch, blockIdx.x, &T)) return;
  const int t = blockIdx.x, i = threadIdx.x, w = i >> 6, lane = i & 63;
  const unsigned long long *keys = vx_sorted_keys(L, cpasses);
  const unsigned *idx = vx_sorted_idx(L, cpasses);
  const bool in = i < T.nrows;
  const long long l = T.l0 + i, r = T.off + l;
  const unsigned long long key = in ? keys[r] : 0ull;
  const bool start = !in || l == 0 || key != keys[r - 1];      // rows past the tile: isolated, never written
  // does the voxel of row i end at row i?  (next row starts a voxel, or the cloud ends)
  bool end;
  if (!in) end = true;
  else if (l + 1 == T.rows) end = true;
  else end = keys[r + 1] != key;
  const unsigned src = in ? idx[r] : 0u;
  // head: last start at or before row i in the tile (-1: the voxel began in an earlier tile); fi: starts up to row i
  const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  const unsigned long long sm = __ballot(start && in);
  if (lane == 0) {
    wcnt[w] = (unsigned)__popcll(sm);
    wlast[w] = sm ? w * 64 + 63 - __clzll((long long)sm) : -1;
  }
  __syncthreads();
  int head = -1;
  unsigned fi = (unsigned)__popcll(sm & le);
  for (int q = 0; q < w; ++q) {
    fi += wcnt[q];
    head = wlast[q] > head ? wlast[q] : head;
  }
  const unsigned long long mine = sm & le;
  if (mine) head = w * 64 + 63 - __clzll((long long)mine);
  const unsigned mb = L.mcount[T.b];
  const unsigned vbase = L.texcl[t] - L.texcl[L.tile_start[T.b]];
  // voxel of row i, numbered within the cloud (a continuing first voxel is the previous tile's last)
  const unsigned vox = vbase + fi - 1u;
  const unsigned cnt = head >= 0 ? (unsigned)(i - head + 1) : (unsigned)(i + 1);
  const bool last_row = i == T.nrows - 1;
  // pieces: head piece = the first voxel's rows in this tile when it began earlier; tail piece = the last voxel's rows
  // when it goes on into the next tile
  const bool head_piece = in && head < 0 && (end || last_row);
  const bool tail_piece = in && last_row && !end;
  const bool done = in && head >= 0 && end;
  for (int c0 = 0; c0 < d; c0 += DC) {
    double v[DC];
    bool f = start;
#pragma unroll
    for (int c = 0; c < DC; ++c) v[c] = (in && c0 + c < d) ? (double)pts[(size_t)src * d + c0 + c] : 0.0;
    int buf = 0;
#pragma unroll
    for (int off = 1; off < VX_THREADS; off <<= 1) {
#pragma unroll
      for (int c = 0; c < DC; ++c) sv[buf][c][i] = v[c];
      sf[buf][i] = f;
      __syncthreads();
      if (i >= off && !f) {
#pragma unroll
        for (int c = 0; c < DC; ++c) v[c] = sv[buf][c][i - off] + v[c];
        f = sf[buf][i - off];
      }
      buf ^= 1;
    }
    if (done) {
      float *o = out + (size_t)(T.off + vox) * d + c0;
#pragma unroll
      for (int c = 0; c < DC; ++c)
        if (c0 + c < d) o[c] = (float)(v[c] / (double)cnt);
    }
    if (head_piece) {
#pragma unroll
      for (int c = 0; c < DC; ++c)
        if (c0 + c < d) L.head_sum[(size_t)t * d + c0 + c] = v[c];
    }
    if (tail_piece) {
#pragma unroll
      for (int c = 0; c < DC; ++c)
        if (c0 + c < d) L.tail_sum[(size_t)t * d + c0 + c] = v[c];
    }
    __syncthreads();          // the next round's first LDS writes
  }
  if (head_piece) L.head_cnt[t] = cnt;
  if (tail_piece) {
    L.tail_cnt[t] = cnt;
    L.tail_vox[t] = vox;
  }
  if (i == 0) {
    // bit 0: this tile owns a voxel that starts in it and goes on past it (seg_fixup finishes it); bit 1: the tile's
    // first row starts a voxel (the voxel of the previous tile's last row, if any, ended there)
    bool owns = false;
    if (T.nrows > 0) {
      const long long lr = T.l0 + T.nrows - 1, rr = T.off + lr;
      const bool open = lr + 1 < T.rows && keys[rr + 1] == keys[rr];
      owns = open && (wlast[0] >= 0 || wlast[1] >= 0 || wlast[2] >= 0 || wlast[3] >= 0);
    }
    L.tinfo[t] = (owns ? 1u : 0u) | (start ? 2u : 0u);
  }
  // padding and mask for the tile's own row range of the output block
  if (in) {
    mask[r] = l < (long long)mb ? 1 : 0;
    if (l >= (long long)mb)
      for (int c = 0; c < d; ++c) out[(size_t)r * d + c] = 0.0f;
  }
}

// voxels spanning tiles t0 < ... <= t1: tail piece of t0 then the head pieces of t0+1 .. t1, summed in a fixed tree
__global__ __launch_bounds__(VX_THREADS) void vx_seg_fixup_kernel(int batch, int d, VxLayout L, float *__restrict__ out) {
  __shared__ int s_end;
  __shared__ double red[VX_THREADS];
  __shared__ unsigned long long redc[VX_THREADS];
  VxTile T;
  const int t0 = blockIdx.x;
  if (!vx_tile(L, batch, t0, &T)) return;
  if (!(L.tinfo[t0] & 1u)) return;
  const int tend = L.tile_start[T.b + 1];       // cloud's tiles end
  if (threadIdx.x == 0) s_end = tend;
  __syncthreads();
  // the voxel runs on through the following tiles that have no voxel start, and ends at the first tile tt with one:
  // just before tt when tt's row 0 starts a voxel (t1 = tt - 1, s_end = tt), inside tt otherwise (t1 = tt, s_end =
  // tt + 1); or in the cloud's last tile.  Only tiles t0+1 .. t1 hold a head piece of this voxel.
  for (int base = t0 + 1; base < tend; base += VX_THREADS) {
    const int tt = base + threadIdx.x;
    if (tt < tend) {
      const unsigned info = L.tinfo[tt];
      if (info & 2u) atomicMin(&s_end, tt);
      else if (L.tflags[tt] != 0u) atomicMin(&s_end, tt + 1);
    }
    __syncthreads();
    const int e = s_end;
    __syncthreads();          // every thread has read s_end before any thread's next atomicMin
    if (e < tend) break;
  }
  const int npieces = s_end - t0;      // piece 0 = tail of t0, piece k = head of t0 + k
  unsigned long long cnt = 0;
  for (int k = threadIdx.x; k < npieces; k += VX_THREADS) cnt += k == 0 ? L.tail_cnt[t0] : L.head_cnt[t0 + k];
  redc[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = VX_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) redc[threadIdx.x] += redc[threadIdx.x + s];
    __syncthreads();
  }
  const double n = (double)redc[0];
  const size_t row = (size_t)(T.off + L.tail_vox[t0]);
  for (int c = 0; c < d; ++c) {
    double acc = 0.0;
    for (int k = threadIdx.x; k < npieces; k += VX_THREADS)
      acc += k == 0 ? L.tail_sum[(size_t)t0 * d + c] : L.head_sum[(size_t)(t0 + k) * d + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = VX_THREADS / 2; s > 0; s >>= 1) {
      if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[row * d + c] = (float)(red[0] / n);
    __syncthreads();
  }
}

int vx_cloud_passes(int batch) {
  int bits = 0;
  while (bits < 31 && (1 << bits) < batch) ++bits;
  return (bits + 7) / 8;
}

bool vx_args_ok(int batch, long long total, int d) { return batch >= 1 && d >= 3 && total >= 0 && total < (1ll << 31); }

}  // namespace

extern "C" size_t mi_voxel_downsample_workspace_bytes(int batch, int64_t total, int d) {
  if (!vx_args_ok(batch, total, d)) return 0;
  return vx_layout(nullptr, batch, total, d).bytes;
}

extern "C" int mi_voxel_downsample(const float *points, const int64_t *offsets, int batch, int64_t total, int d,
                                   const float *leaf, float *out_points, uint8_t *out_mask, int64_t *out_counts,
                                   void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!offsets || !leaf || !out_counts || !workspace) return MI_E_NULL;
  if (total > 0 && (!points || !out_points || !out_mask)) return MI_E_NULL;     // an all-empty batch has no rows
  if (!vx_args_ok(batch, total, d)) return MI_E_SHAPE;
  if ((uintptr_t)workspace % 16 != 0 || (uintptr_t)offsets % 8 != 0 || (uintptr_t)out_counts % 8 != 0 ||
      (uintptr_t)points % 4 != 0 || (uintptr_t)leaf % 4 != 0 || (uintptr_t)out_points % 4 != 0)
    return MI_E_ALIGN;
  const VxLayout L = vx_layout(workspace, batch, total, d);
  if (workspace_bytes < L.bytes) return MI_E_CAPACITY;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int T = (int)total;
  const int nrt = (T + RADIX_TILE - 1) / RADIX_TILE;
  const int mt = (T + SEG_TILE - 1) / SEG_TILE + batch;
  const int cpasses = vx_cloud_passes(batch);
  const long long *soff = reinterpret_cast<const long long *>(offsets);
  hipLaunchKernelGGL(vx_init_kernel, dim3(1), dim3(VX_THREADS), 0, s, soff, batch, (long long)T, L);
  if (T > 0) {
    const int waves = (T + 64 * MM_PER_LANE - 1) / (64 * MM_PER_LANE);
    hipLaunchKernelGGL(vx_minmax_kernel, dim3((waves + 3) / 4), dim3(VX_THREADS), 0, s, points, batch, T, d, leaf, L);
  }
  hipLaunchKernelGGL(vx_plan_kernel, dim3(1), dim3(VX_THREADS), 0, s, batch, L);
  if (T > 0) {
    hipLaunchKernelGGL(vx_keys_kernel, dim3((T + VX_THREADS - 1) / VX_THREADS), dim3(VX_THREADS), 0, s, points, batch, T, d,
                       leaf, L);
    for (int pass = 0; pass < KEY_PASSES + cpasses; ++pass) {
      hipLaunchKernelGGL(vx_hist_kernel, dim3(nrt), dim3(VX_THREADS), 0, s, batch, T, pass, L);
      hipLaunchKernelGGL(vx_rowscan_kernel, dim3(256), dim3(VX_THREADS), 0, s, T, pass, L);
      hipLaunchKernelGGL(vx_scatter_kernel, dim3(nrt), dim3(VX_THREADS), 0, s, batch, T, pass, L);
    }
    hipLaunchKernelGGL(vx_seg_count_kernel, dim3(mt), dim3(VX_THREADS), 0, s, batch, cpasses, L);
  }
  hipLaunchKernelGGL(vx_seg_scan_kernel, dim3(1), dim3(VX_THREADS), 0, s, batch, L, reinterpret_cast<long long *>(out_counts));
  if (T > 0) {
    if (d == 3)
      hipLaunchKernelGGL(vx_seg_sum_kernel<3>, dim3(mt), dim3(VX_THREADS), 0, s, points, batch, d, cpasses, L, out_points, out_mask);
    else if (d == 4)
      hipLaunchKernelGGL(vx_seg_sum_kernel<4>, dim3(mt), dim3(VX_THREADS), 0, s, points, batch, d, cpasses, L, out_points, out_mask);
    else if (d == 6)
      hipLaunchKernelGGL(vx_seg_sum_kernel<6>, dim3(mt), dim3(VX_THREADS), 0, s, points, batch, d, cpasses, L, out_points, out_mask);
    else
      hipLaunchKernelGGL(vx_seg_sum_kernel<4>, dim3(mt), dim3(VX_THREADS), 0, s, points, batch, d, cpasses, L, out_points, out_mask);
    hipLaunchKernelGGL(vx_seg_fixup_kernel, dim3(mt), dim3(VX_THREADS), 0, s, batch, d, L, out_points);
  }
  return mi_launch_status();
}
