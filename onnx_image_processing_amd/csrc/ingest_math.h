// K16 frame ingest: the per-pixel arithmetic of mi_ingest_frames (include/mi355x_match.h states it), as
// __host__ __device__ inlines so that the kernel (ingest.hip) and the host harness (tests/native/ingest_host.cpp) run the
// same code.  Integers throughout, except the tap position: one double multiply-subtract rounded to float32, a float32
// subtraction and two float32 products rounded to nearest even.  Built with -ffp-contract=off: nothing here may be fused.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define MI_INGEST_HD __host__ __device__ __forceinline__

// gray weights of B, G, R in 1/32768 and the weight scale of the bilinear taps
#define MI_INGEST_CB 3735
#define MI_INGEST_CG 19235
#define MI_INGEST_CR 9798
#define MI_INGEST_ONE 2048

// the two taps of destination index d along one axis: source indices s0 <= s1 and their weights in 1/2048
struct MiIngestTap {
  int s0, s1, w0, w1;
};

// scale = (double)src / (double)dst, computed once on the host and handed to the kernel
MI_INGEST_HD MiIngestTap mi_ingest_tap(int d, int src, double scale) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    s = 0;
    f = 0.0f;
  }
  if (s >= src - 1) {
    s = src - 1;
    f = 0.0f;
  }
  MiIngestTap t;
  t.s0 = s;
  t.s1 = s + 1 < src ? s + 1 : src - 1;
  t.w1 = (int)rintf(f * 2048.0f);
  t.w0 = (int)rintf((1.0f - f) * 2048.0f);
  return t;
}

MI_INGEST_HD int mi_ingest_gray(int b, int g, int r) {
  return (MI_INGEST_CB * b + MI_INGEST_CG * g + MI_INGEST_CR * r + 16384) >> 15;
}

// horizontal pass: gray at the two taps of one source row -> an 19-bit intermediate
MI_INGEST_HD int mi_ingest_hblend(int g0, int g1, int a0, int a1) { return g0 * a0 + g1 * a1; }

// vertical pass on two horizontal results
MI_INGEST_HD int mi_ingest_vblend(int r_top, int r_bot, int b0, int b1) {
  return (((b0 * (r_top >> 4)) >> 16) + ((b1 * (r_bot >> 4)) >> 16) + 2) >> 2;
}
