// Host harness for the arithmetic of csrc/tsdf.hip (plain C++: csrc/tsdf_math.h needs no HIP header and nothing is launched):
// a voxel's centre, projection and update, the ray's grid coordinate, the trilinear sample, the hit interpolation, the normal
// and the composition of poses, exactly the code the kernels run.  tests/test_tsdf_host.py compiles it and compares its output
// with tests/tsdf_oracle.py.  Every mode reads records from stdin until it ends and prints one line per record (%.9g floats):
//   tsdf_host project  i j k voxel_size origin(3) R(9) t(3) fx fy cx cy w h             -> ok px py qz
//   tsdf_host fuse     d z_scale min max qz truncation max_weight tsdf weight           -> ok tsdf weight
//   tsdf_host point    xn yn s R(9) t(3) origin(3) voxel_size                           -> g(3)
//   tsdf_host hit      s_prev step f_prev f                                             -> s
//   tsdf_host compose  ra(9) ta(3) rb(9) tb(3)                                          -> r(9) t(3)
//   tsdf_host sample FILE nx ny nz      g(3)                                            -> ok f
//   tsdf_host normal FILE nx ny nz      g(3) R(9) v(3)                                  -> ok n(3)
// FILE holds the volume's nz * ny * nx records of (tsdf, weight) as raw float32.
#include "../../onnx_image_processing_amd/csrc/tsdf_math.h"

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
    fprintf(stderr, "usage: tsdf_host project | fuse | point | hit | compose | (sample | normal) FILE nx ny nz  (records on stdin)\n");
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
    float a[9];
    while (rf(a, 9)) {
      const bool ok = tsdf_fuse(a[0], a[1], a[2], a[3], a[4], a[5], a[6], &a[7], &a[8]);
      printf("%d %.9g %.9g\n", ok ? 1 : 0, a[7], a[8]);
    }
    return 0;
  }
  if (!strcmp(mode, "point")) {
    float a[19], g[3];
    while (rf(a, 19)) {
      tsdf_grid_point(a[0], a[1], a[2], a + 3, a + 12, a + 15, a[18], g);
      printf("%.9g %.9g %.9g\n", g[0], g[1], g[2]);
    }
    return 0;
  }
  if (!strcmp(mode, "hit")) {
    float a[4];
    while (rf(a, 4)) printf("%.9g\n", tsdf_hit(a[0], a[1], a[2], a[3]));
    return 0;
  }
  if (!strcmp(mode, "compose")) {
    float a[24], r[9], t[3];
    while (rf(a, 24)) {
      tsdf_compose(a, a + 9, a + 12, a + 21, r, t);
      for (int j = 0; j < 9; ++j) printf("%.9g ", r[j]);
      printf("%.9g %.9g %.9g\n", t[0], t[1], t[2]);
    }
    return 0;
  }
  if ((!strcmp(mode, "sample") || !strcmp(mode, "normal")) && argc == 6) {
    const int nx = atoi(argv[3]), ny = atoi(argv[4]), nz = atoi(argv[5]);
    if (nx < 2 || ny < 2 || nz < 2) return 1;
    std::vector<float> vol((size_t)nx * ny * nz * 2);
    FILE *fp = fopen(argv[2], "rb");
    if (!fp || fread(vol.data(), sizeof(float), vol.size(), fp) != vol.size()) {
      fprintf(stderr, "cannot read %s\n", argv[2]);
      return 1;
    }
    fclose(fp);
    if (!strcmp(mode, "sample")) {
      float g[3], f;
      while (rf(g, 3)) {
        const bool ok = tsdf_sample(vol.data(), nx, ny, nz, g, &f);
        printf("%d %.9g\n", ok ? 1 : 0, f);
      }
    } else {
      float a[15], n[3];
      while (rf(a, 15)) {
        const bool ok = tsdf_normal(vol.data(), nx, ny, nz, a, a + 3, a + 12, n);
        printf("%d %.9g %.9g %.9g\n", ok ? 1 : 0, n[0], n[1], n[2]);
      }
    }
    return 0;
  }
  fprintf(stderr, "unknown mode %s\n", mode);
  return 1;
}
