// K16 frame ingest (mi_ingest_frames): interleaved colour uint8 camera frames of any size -> (B,1,H,W) gray model frames,
// uint8 or float32, in one bandwidth-bound kernel.  The arithmetic is ingest_math.h (OpenCV's 8-bit gray + bilinear path
// restated in integers); DESIGN.md K16 has the structure and the measurements.
//
// One workgroup of 256 lanes produces a tile of IG_ROWS output rows x `tile_w` output columns of one frame:
//   1. the source rows the tile's taps touch -- a contiguous range when it is at most 2 * IG_ROWS rows (upscale .. 2x
//      downscale: consecutive output rows share source rows and each is read once), otherwise the two tap rows of every
//      output row (rows no tap touches are never read) -- are read over the tile's column span with 16-byte loads of
//      ALIGNED spans (a row of 3-byte pixels starts at any byte offset; the lane shifts its 16 * C + 4 bytes by the
//      row's phase with v_alignbyte), converted to gray in registers and staged in LDS as 1 byte per pixel;
//   2. every lane blends 4 neighbouring output pixels from the staged gray rows and stores them as one 4-byte (uint8)
//      or 16-byte (float32) vector; widths that are no multiple of 4, or a misaligned `dst`, take scalar stores.
// Equal source and destination sizes (SAME) skip the taps and the blend: the formula is the identity there.
#include "common.h"
#include "ingest_math.h"

#define IG_THREADS 256
#define IG_ROWS 8                       // output rows per workgroup
#define IG_SLOTS (2 * IG_ROWS)          // staged source rows per workgroup
#define IG_TILE_W 256                   // most output columns per workgroup (one x tap per lane)
#define IG_STRIDE 1024                  // LDS bytes per staged row
// most source columns a tile may span: a staged row holds the span, up to 15 pixels in front of it (the aligned start)
// and up to 16 behind it (the last lane's whole group of 16)
#define IG_SPAN_MAX (IG_STRIDE - 32)
#define IG_MAX_PITCH (1LL << 40)

struct IgXTap {
  unsigned short m0, m1;                // the taps' columns relative to the tile's first source column
  short a0, a1;
};
struct IgYTap {
  int slot0, slot1, b0, b1;
};

struct IgArgs {
  const uint8_t *src;
  void *dst;
  long long row_pitch, frame_pitch;
  double scale_x, scale_y;
  int src_h, src_w, h, w;
  int tile_w, rgb, dst_f32, vec_ok;
};

template <int C, bool SAME>
__global__ __launch_bounds__(IG_THREADS) void ingest_kernel(const IgArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t gray[IG_SLOTS * IG_STRIDE];
  __shared__ IgXTap xtap[IG_TILE_W];
  __shared__ IgYTap ytap[IG_ROWS];
  __shared__ int shift[IG_SLOTS];       // staged row: pixel k of the span sits at byte k + shift

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * a.tile_w, y0 = blockIdx.y * IG_ROWS, frame = blockIdx.z;
  const int tw = min(a.tile_w, a.w - x0), th = min(IG_ROWS, a.h - y0);

  // the tile's source window (every lane computes the same four numbers)
  int cs, ce, ylo, nslots;
  bool contiguous = true;
  if (SAME) {
    cs = x0;
    ce = x0 + tw - 1;
    ylo = y0;
    nslots = th;
  } else {
    cs = mi_ingest_tap(x0, a.src_w, a.scale_x).s0;
    ce = mi_ingest_tap(x0 + tw - 1, a.src_w, a.scale_x).s1;
    ylo = mi_ingest_tap(y0, a.src_h, a.scale_y).s0;
    const int yhi = mi_ingest_tap(y0 + th - 1, a.src_h, a.scale_y).s1;
    contiguous = yhi - ylo + 1 <= IG_SLOTS;
    nslots = contiguous ? yhi - ylo + 1 : 2 * th;
    if (tid < tw) {
      const MiIngestTap t = mi_ingest_tap(x0 + tid, a.src_w, a.scale_x);
      xtap[tid] = IgXTap{(unsigned short)(t.s0 - cs), (unsigned short)(t.s1 - cs), (short)t.w0, (short)t.w1};
    }
    if (tid < th) {
      const MiIngestTap t = mi_ingest_tap(y0 + tid, a.src_h, a.scale_y);
      ytap[tid] = contiguous ? IgYTap{t.s0 - ylo, t.s1 - ylo, t.w0, t.w1} : IgYTap{2 * tid, 2 * tid + 1, t.w0, t.w1};
    }
  }
  const int span = ce - cs + 1;                                  // <= IG_SPAN_MAX: the host chose tile_w for that

  // ---- 1. stage the source rows as gray bytes ------------------------------------------------------------------------
  constexpr int GROUP = 16 * C;                                  // bytes of 16 pixels: what one lane converts
  const int groups = (15 + span * C + GROUP - 1) / GROUP;        // per row, for the worst alignment
  const uint8_t *const frame_base = a.src + (long long)frame * a.frame_pitch + (long long)cs * C;
  for (int item = tid; item < nslots * groups; item += IG_THREADS) {
    const int slot = item / groups, li = item - slot * groups;
    int row = ylo + slot;
    if (!SAME && !contiguous) {
      const MiIngestTap t = mi_ingest_tap(y0 + (slot >> 1), a.src_h, a.scale_y);
      row = (slot & 1) ? t.s1 : t.s0;
    }
    const uint8_t *const base = frame_base + (long long)row * a.row_pitch;
    const unsigned off = (unsigned)((uintptr_t)base & 15);       // 0..15: the span starts this far into its aligned block
    const unsigned len = (off + (unsigned)span * C + 15u) & ~15u; // bytes of the aligned blocks that hold the span
    if (li == 0) shift[slot] = off / C;
    const unsigned q0 = (unsigned)li * GROUP;
    if (q0 >= len) continue;                                     // past the row's last aligned block
    // the lane's GROUP bytes and the 4 that follow; only aligned blocks that hold a byte of the span are touched
    const uint8_t *const p = base - off + q0;
    unsigned d[4 * C + 1];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (q0 + 16 * j < len) v = *reinterpret_cast<const uint4 *>(p + 16 * j);
      d[4 * j] = v.x, d[4 * j + 1] = v.y, d[4 * j + 2] = v.z, d[4 * j + 3] = v.w;
    }
    d[4 * C] = q0 + GROUP < len ? *reinterpret_cast<const unsigned *>(p + GROUP) : 0u;
    // the first pixel that STARTS in this lane's group starts at byte `phase` of it (the same for every group of the row:
    // GROUP is a multiple of C); shifting by it puts pixel j at bytes C*j .. C*j + C - 1
    const unsigned phase = off % C;
    unsigned g4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned packed = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 4 * q + i;                                 // pixel of the group
        unsigned g;
        if (C == 1) {
          g = (d[j >> 2] >> (8 * (j & 3))) & 0xffu;
        } else {
          unsigned px[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int byte = C * j + c;
            const unsigned word = __builtin_amdgcn_alignbyte(d[byte / 4 + 1], d[byte / 4], phase);
            px[c] = (word >> (8 * (byte & 3))) & 0xffu;
          }
          g = (unsigned)mi_ingest_gray((int)(a.rgb ? px[2] : px[0]), (int)px[1], (int)(a.rgb ? px[0] : px[2]));
        }
        packed |= g << (8 * i);
      }
      g4[q] = packed;
    }
    *reinterpret_cast<uint4 *>(&gray[slot * IG_STRIDE + 16 * li]) = make_uint4(g4[0], g4[1], g4[2], g4[3]);
  }
  __syncthreads();

  // ---- 2. blend and store: 4 output pixels per lane ---------------------------------------------------------------------
  const int quads = (tw + 3) >> 2;
  for (int item = tid; item < th * quads; item += IG_THREADS) {
    const int r = item / quads, xq = (item - r * quads) * 4;
    int out[4];
    if (SAME) {
      const uint8_t *row = &gray[r * IG_STRIDE + shift[r] + xq];
#pragma unroll
      for (int i = 0; i < 4; ++i) out[i] = xq + i < tw ? row[i] : 0;
    } else {
      const IgYTap yt = ytap[r];
      const uint8_t *top = &gray[yt.slot0 * IG_STRIDE + shift[yt.slot0]];
      const uint8_t *bot = &gray[yt.slot1 * IG_STRIDE + shift[yt.slot1]];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        out[i] = 0;
        if (xq + i < tw) {
          const IgXTap xt = xtap[xq + i];
          const int r_top = mi_ingest_hblend(top[xt.m0], top[xt.m1], xt.a0, xt.a1);
          const int r_bot = mi_ingest_hblend(bot[xt.m0], bot[xt.m1], xt.a0, xt.a1);
          out[i] = mi_ingest_vblend(r_top, r_bot, yt.b0, yt.b1);
        }
      }
    }
    const size_t o = ((size_t)frame * a.h + (y0 + r)) * (size_t)a.w + (size_t)(x0 + xq);
    if (a.vec_ok && xq + 3 < tw) {                               // w % 4 == 0 and tile_w % 4 == 0: o is a multiple of 4
      if (a.dst_f32)
        *reinterpret_cast<float4 *>(static_cast<float *>(a.dst) + o) = make_float4((float)out[0], (float)out[1], (float)out[2], (float)out[3]);
      else
        *reinterpret_cast<unsigned *>(static_cast<uint8_t *>(a.dst) + o) =
            (unsigned)out[0] | ((unsigned)out[1] << 8) | ((unsigned)out[2] << 16) | ((unsigned)out[3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (xq + i >= tw) break;
        if (a.dst_f32)
          static_cast<float *>(a.dst)[o + i] = (float)out[i];
        else
          static_cast<uint8_t *>(a.dst)[o + i] = (uint8_t)out[i];
      }
    }
  }
}

// Output columns per workgroup: as many as IG_TILE_W, fewer when the tile's source span would not fit a staged row
// (span <= (tile_w - 1) * scale + 3, plus float32 rounding of the tap position: < 0.01 at 16384 columns), then evened
// out over the tiles.  A multiple of 4 whenever it is at least 4, so that vector stores stay aligned.
static int ig_tile_w(int src_w, int w) {
  const double scale = (double)src_w / (double)w;
  int tw = IG_TILE_W;
  if ((tw - 1) * scale + 4.0 > IG_SPAN_MAX) tw = (int)((IG_SPAN_MAX - 4.0) / scale) + 1;
  if (tw < 1) tw = 1;
  const int tiles = ceil_div(w, tw);
  tw = min(tw, ceil_div(ceil_div(w, tiles), 4) * 4);
  if (tw >= 4) tw &= ~3;
  return tw;
}

extern "C" int mi_ingest_frames(const uint8_t *src, int batch, int src_h, int src_w, int channels, long long row_pitch,
                                long long frame_pitch, int channel_order, void *dst, int dst_is_f32, int h, int w,
                                mi_stream_t stream) {
  if (!src || !dst) return MI_E_NULL;
  if (batch < 1 || src_h < 1 || src_w < 1 || h < 1 || w < 1) return MI_E_SHAPE;
  if (channels != 1 && channels != 3 && channels != 4) return MI_E_PARAM;
  if (channel_order != MI_INGEST_BGR && channel_order != MI_INGEST_RGB) return MI_E_PARAM;
  if (batch > MI_INGEST_MAX_DIM || src_h > MI_INGEST_MAX_DIM || src_w > MI_INGEST_MAX_DIM || h > MI_INGEST_MAX_DIM || w > MI_INGEST_MAX_DIM) return MI_E_PARAM;
  if (row_pitch < (long long)src_w * channels || row_pitch > IG_MAX_PITCH) return MI_E_PARAM;
  if (frame_pitch < row_pitch * src_h || frame_pitch > IG_MAX_PITCH * 256) return MI_E_PARAM;
  MI_ENTER();
  IgArgs a;
  a.src = src, a.dst = dst, a.row_pitch = row_pitch, a.frame_pitch = frame_pitch;
  a.scale_x = (double)src_w / (double)w, a.scale_y = (double)src_h / (double)h;
  a.src_h = src_h, a.src_w = src_w, a.h = h, a.w = w;
  const bool same = src_h == h && src_w == w;
  a.tile_w = same ? IG_TILE_W : ig_tile_w(src_w, w);
  a.rgb = channel_order == MI_INGEST_RGB, a.dst_f32 = dst_is_f32 != 0;
  a.vec_ok = w % 4 == 0 && a.tile_w % 4 == 0 && (uintptr_t)dst % (dst_is_f32 ? 16 : 4) == 0;
  const dim3 grid(ceil_div(w, a.tile_w), ceil_div(h, IG_ROWS), batch);
  hipStream_t s = (hipStream_t)stream;
#define IG_LAUNCH(C, SAME) hipLaunchKernelGGL((ingest_kernel<C, SAME>), grid, dim3(IG_THREADS), 0, s, a)
  if (same) {
    if (channels == 1) IG_LAUNCH(1, true);
    else if (channels == 3) IG_LAUNCH(3, true);
    else IG_LAUNCH(4, true);
  } else {
    if (channels == 1) IG_LAUNCH(1, false);
    else if (channels == 3) IG_LAUNCH(3, false);
    else IG_LAUNCH(4, false);
  }
#undef IG_LAUNCH
  return mi_launch_status();
}
