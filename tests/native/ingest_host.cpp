// Host harness for csrc/ingest_math.h (no GPU is touched: nothing is launched): frames are ingested on the host with the
// per-pixel functions the K16 kernel runs -- tap positions and weights, gray, the two blend passes.
// tests/test_ingest_host.py compiles it with hipcc and compares its output bit for bit with tests/ingest_oracle.py.
//   ingest_host < request      request: one text line "batch src_h src_w channels rgb h w\n", then batch * src_h * src_w *
//                              channels bytes (contiguous HWC frames); output: batch * h * w gray bytes
#include "../../onnx_image_processing_amd/csrc/ingest_math.h"

#include <cstdio>
#include <vector>

int main() {
  int batch, src_h, src_w, channels, rgb, h, w;
  char line[128];
  if (!fgets(line, sizeof line, stdin)) return 2;
  if (sscanf(line, "%d %d %d %d %d %d %d", &batch, &src_h, &src_w, &channels, &rgb, &h, &w) != 7) return 2;
  std::vector<unsigned char> src((size_t)batch * src_h * src_w * channels), dst((size_t)batch * h * w);
  if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 3;
  const double scale_x = (double)src_w / (double)w, scale_y = (double)src_h / (double)h;
  auto gray_at = [&](int b, int y, int x) {
    const unsigned char *p = &src[(((size_t)b * src_h + y) * src_w + x) * channels];
    if (channels == 1) return (int)p[0];
    return rgb ? mi_ingest_gray(p[2], p[1], p[0]) : mi_ingest_gray(p[0], p[1], p[2]);
  };
  for (int b = 0; b < batch; ++b)
    for (int y = 0; y < h; ++y) {
      const MiIngestTap ty = mi_ingest_tap(y, src_h, scale_y);
      for (int x = 0; x < w; ++x) {
        const MiIngestTap tx = mi_ingest_tap(x, src_w, scale_x);
        const int r_top = mi_ingest_hblend(gray_at(b, ty.s0, tx.s0), gray_at(b, ty.s0, tx.s1), tx.w0, tx.w1);
        const int r_bot = mi_ingest_hblend(gray_at(b, ty.s1, tx.s0), gray_at(b, ty.s1, tx.s1), tx.w0, tx.w1);
        dst[((size_t)b * h + y) * w + x] = (unsigned char)mi_ingest_vblend(r_top, r_bot, ty.w0, ty.w1);
      }
    }
  return fwrite(dst.data(), 1, dst.size(), stdout) == dst.size() ? 0 : 4;
}
