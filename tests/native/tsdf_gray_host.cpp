// Host harness for the arithmetic of csrc/tsdf_gray.hip (plain C++: csrc/tsdf_gray_math.h needs no HIP header and nothing is
// launched): a voxel's projection, its joint update by one depth and one gray sample in the kernel's own sequence, and the
// gather of the intensity volume at a point, exactly the code the kernels run.  tests/test_tsdf_gray_host.py compiles it and
// compares its output with tests/tsdf_gray_oracle.py.  Every mode reads records from stdin until it ends and prints one line
// per record (%.9g floats):
//   tsdf_gray_host project  i j k voxel_size origin(3) R(9) t(3) fx fy cx cy w h                       -> ok px py qz
//   tsdf_gray_host fuse     d z_scale min max qz truncation max_weight tsdf weight g gray gweight      -> fused updated tsdf weight gray gweight
//   tsdf_gray_host sample FILE nx ny nz      posed x y z f origin(3) voxel_size R(9) t(3)              -> ok I
// FILE holds the intensity volume's nz * ny * nx records of (gray, gweight) as raw float32.
#include "../../onnx_image_processing_amd/csrc/tsdf_gray_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool rf(float *p, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%f", &p[i]) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2 && argc != 6) {
    fprintf(stderr, "usage: tsdf_gray_host project | fuse | sample FILE nx ny nz  (records on stdin)\n");
    return 1;
  }
  const char *mode = argv[1];
  if (!strcmp(mode, "project")) {
    float a[25];
    while (rf(a, 25)) {
      const float p[3] = {tsdf_centre((int)a[0], a[3], a[4]), tsdf_centre((int)a[1], a[3], a[5]), tsdf_centre((int)a[2], a[3], a[6])};
      float q[3], px, py;
      icp_rotate(a + 7, p, q);
      for (int j = 0; j < 3; ++j) q[j] += a[16 + j];
      const bool ok = icp_project(q, a[19], a[20], a[21], a[22], (int)a[23], (int)a[24], &px, &py);
      printf("%d %.9g %.9g %.9g\n", ok ? 1 : 0, ok ? px : 0.0f, ok ? py : 0.0f, q[2]);
    }
    return 0;
  }
  if (!strcmp(mode, "fuse")) {
    float a[12];
    while (rf(a, 12)) {
      const bool fused = tsdf_fuse(a[0], a[1], a[2], a[3], a[4], a[5], a[6], &a[7], &a[8]);
      bool updated = false;
      if (tsdf_gray_band(fused, a[0], a[1], a[4], a[5])) updated = tsdf_gray_fuse(a[9], a[6], &a[10], &a[11]);
      printf("%d %d %.9g %.9g %.9g %.9g\n", fused ? 1 : 0, updated ? 1 : 0, a[7], a[8], a[10], a[11]);
    }
    return 0;
  }
  if (!strcmp(mode, "sample") && argc == 6) {
    const int nx = atoi(argv[3]), ny = atoi(argv[4]), nz = atoi(argv[5]);
    if (nx < 2 || ny < 2 || nz < 2) return 1;
    std::vector<float> vol((size_t)nx * ny * nz * 2);
    FILE *fp = fopen(argv[2], "rb");
    if (!fp || fread(vol.data(), sizeof(float), vol.size(), fp) != vol.size()) {
      fprintf(stderr, "cannot read %s\n", argv[2]);
      return 1;
    }
    fclose(fp);
    float a[21];
    while (rf(a, 21)) {
      float I = 0.0f;
      bool ok = false;
      if (a[4] != 0.0f && fabsf(a[1]) < INFINITY && fabsf(a[2]) < INFINITY && fabsf(a[3]) < INFINITY) {     // the kernel's gate
        float xw[3] = {a[1], a[2], a[3]};
        if (a[0] != 0.0f) tsdf_gray_world(a + 1, a + 9, a + 18, xw);
        ok = tsdf_gray_sample(vol.data(), nx, ny, nz, xw, a + 5, a[8], &I);
      }
      printf("%d %.9g\n", ok ? 1 : 0, I);
    }
    return 0;
  }
  fprintf(stderr, "unknown mode %s\n", mode);
  return 1;
}
