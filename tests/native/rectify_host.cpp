// Host harness for the arithmetic of csrc/rectify.hip (no GPU is touched: nothing is launched): csrc/rectify_math.h -- the
// section's atan and tan, the forward models, the map element and mask byte of a destination pixel, one remapped pixel in
// every element type and interpolation, one undistorted point, the stereo rig -- driven as the kernels drive it, one call
// per output element.  tests/test_rectify_host.py compiles it with hipcc, plain and under the host sanitizers, and compares
// its output with tests/rectify_oracle.py.  Raw little-endian values on both standard streams; the camera is 35 numbers on the
// command line: k (9), dist (8), r (9), k_new (9), each printed with 17 significant digits.
//   rectify_host trig N < x                                       N doubles -> atan(x) (N doubles), tan(x) (N doubles)
//   rectify_host map MODEL SRC_H SRC_W H W CAMERA                 -> map (H*W*2 int32), mask (H*W bytes)
//   rectify_host remap TYPE INTERPOLATION BATCH SRC_H SRC_W H W BORDER < map src
//                                                                 map (H*W*2 int32), src (BATCH*SRC_H*SRC_W elements) -> dst
//   rectify_host points MODEL COUNT ITERATIONS MAX_RESIDUAL HAS_NEW CAMERA < pts
//                                                                 COUNT*2 float32 -> out (COUNT*2 float32), ok (COUNT bytes)
//   rectify_host rig H W K1 (9) K2 (9) R (9) T (3)                -> status (one int32), r1, r2, k_new (9 doubles each),
//                                                                 baseline, fb (doubles)
#include "../../onnx_image_processing_amd/csrc/rectify_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <typename T>
static bool read_all(std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, stdin) == n;
}
template <typename T>
static void write_all(const std::vector<T> &v) {
  fwrite(v.data(), sizeof(T), v.size(), stdout);
}

static void numbers(char **argv, int n, double *out) {
  for (int i = 0; i < n; ++i) out[i] = strtod(argv[i], nullptr);
}

// the 35 numbers of a camera; has_new = 0 drops k_new as a NULL does
static int camera_of(char **argv, int model, int has_new, RcCamera *cam) {
  double v[35];
  numbers(argv, 35, v);
  return rc_camera(model, v, v + 9, v + 17, has_new ? v + 26 : nullptr, cam);
}

template <typename T>
static int remap(int batch, int sh, int sw, int h, int w, bool linear, double border, const std::vector<int32_t> &map) {
  std::vector<T> src;
  if (!read_all(src, (size_t)batch * sh * sw)) return 2;
  std::vector<T> dst((size_t)batch * h * w);
  memset(dst.data(), 0xA5, dst.size() * sizeof(T));                          // garbage on entry, as a caller's buffer
  for (int f = 0; f < batch; ++f)
    for (size_t p = 0; p < (size_t)h * w; ++p)
      dst[(size_t)f * h * w + p] = rc_remap_pixel(src.data() + (size_t)f * sh * sw, sh, sw, map[2 * p], map[2 * p + 1], linear, (T)border);
  write_all(dst);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 1;
  const char *mode = argv[1];
  if (!strcmp(mode, "trig") && argc == 3) {
    std::vector<double> x;
    if (!read_all(x, (size_t)atoll(argv[2]))) return 2;
    std::vector<double> a(x.size()), t(x.size());
    for (size_t i = 0; i < x.size(); ++i) {
      a[i] = rc_atan(x[i]);
      t[i] = rc_tan(x[i]);
    }
    write_all(a);
    write_all(t);
    return 0;
  }
  if (!strcmp(mode, "map") && argc == 7 + 35) {
    const int model = atoi(argv[2]), sh = atoi(argv[3]), sw = atoi(argv[4]), h = atoi(argv[5]), w = atoi(argv[6]);
    RcCamera cam;
    if (sh < 1 || sw < 1 || h < 1 || w < 1 || sh > 4096 || sw > 4096 || h > 4096 || w > 4096 || camera_of(argv + 7, model, 1, &cam)) return 2;
    std::vector<int32_t> map((size_t)h * w * 2, 0x5a5a5a5a);
    std::vector<uint8_t> mask((size_t)h * w, (uint8_t)0xA5);
    for (int v = 0; v < h; ++v)
      for (int u = 0; u < w; ++u) {
        const size_t p = (size_t)v * w + u;
        rc_map_pixel(cam, sh, sw, v, u, &map[2 * p], &map[2 * p + 1], &mask[p]);
      }
    write_all(map);
    write_all(mask);
    return 0;
  }
  if (!strcmp(mode, "remap") && argc == 10) {
    const int type = atoi(argv[2]), interpolation = atoi(argv[3]), batch = atoi(argv[4]), sh = atoi(argv[5]), sw = atoi(argv[6]);
    const int h = atoi(argv[7]), w = atoi(argv[8]);
    const double border = strtod(argv[9], nullptr);
    if (batch < 1 || sh < 1 || sw < 1 || h < 1 || w < 1 || batch > 64 || sh > 4096 || sw > 4096 || h > 4096 || w > 4096) return 2;
    if (type == MI_RECTIFY_U16 && interpolation == MI_RECTIFY_LINEAR) return 2;
    std::vector<int32_t> map;
    if (!read_all(map, (size_t)h * w * 2)) return 2;
    const bool linear = interpolation == MI_RECTIFY_LINEAR;
    if (type == MI_RECTIFY_U8) return remap<uint8_t>(batch, sh, sw, h, w, linear, border, map);
    if (type == MI_RECTIFY_U16) return remap<uint16_t>(batch, sh, sw, h, w, linear, border, map);
    if (type == MI_RECTIFY_F32) return remap<float>(batch, sh, sw, h, w, linear, border, map);
    return 2;
  }
  if (!strcmp(mode, "points") && argc == 7 + 35) {
    const int model = atoi(argv[2]), count = atoi(argv[3]), iterations = atoi(argv[4]), has_new = atoi(argv[6]);
    const double max_residual = strtod(argv[5], nullptr);
    RcCamera cam;
    if (count < 1 || count > (1 << 20) || iterations < 1 || iterations > MI_RECTIFY_MAX_ITERATIONS || camera_of(argv + 7, model, has_new, &cam))
      return 2;
    std::vector<float> pts;
    if (!read_all(pts, (size_t)count * 2)) return 2;
    std::vector<float> out((size_t)count * 2, -7.0f);
    std::vector<uint8_t> ok((size_t)count, (uint8_t)0xA5);
    for (int i = 0; i < count; ++i)
      ok[(size_t)i] = (uint8_t)rc_undistort_point(cam, pts[2 * (size_t)i], pts[2 * (size_t)i + 1], iterations, max_residual, &out[2 * (size_t)i],
                                                  &out[2 * (size_t)i + 1]);
    write_all(out);
    write_all(ok);
    return 0;
  }
  if (!strcmp(mode, "rig") && argc == 4 + 30) {
    const int h = atoi(argv[2]), w = atoi(argv[3]);
    double v[30];
    numbers(argv + 4, 30, v);
    std::vector<double> out(29, 0.0);
    const int32_t status = rc_stereo_rig(v, v + 9, v + 18, v + 27, h, w, out.data(), out.data() + 9, out.data() + 18, out.data() + 27, out.data() + 28);
    fwrite(&status, sizeof(status), 1, stdout);
    write_all(out);
    return 0;
  }
  fprintf(stderr, "usage: rectify_host trig | map | remap | points | rig ...\n");
  return 1;
}
