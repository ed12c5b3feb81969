// What the TSDF family shares on the host: K19 (tsdf.hip), K22 (tsdf_gray.hip) and, for the volume checks, K20 (surface.hip).
// The grid and camera structs, the predicates, and the checks of a volume, a grid, a depth range, the frames of an
// integration and its camera.  The kernels share no device code: K22i carries the lazily loaded intensity record through
// K19i's loop, and K19i's row addressing and per-frame projection written as helpers were longer than the two copies
// they replace and moved both kernels' registers.
#pragma once
#include "common.h"

#include <math.h>

namespace {

struct TsdfGrid {
  int nx, ny, nz;
  float origin[3], voxel_size, truncation;
};
struct TsdfCam {
  float fx, fy, cx, cy, z_scale, min_depth, max_depth;
};

inline bool tsdf_positive(float v) { return v > 0.0f && v < INFINITY; }
inline bool tsdf_finite(float v) { return fabsf(v) < INFINITY; }

inline int tsdf_volume_status(int batch, int nz, int ny, int nx) {
  if (batch < 1 || nz < 2 || ny < 2 || nx < 2) return MI_E_SHAPE;
  if ((double)batch * (double)nz * (double)ny * (double)nx >= 2147483648.0) return MI_E_SHAPE;
  if (batch > 65535) return MI_E_PARAM;
  return MI_OK;
}
inline int tsdf_origin_status(float ox, float oy, float oz, float voxel_size) {
  return tsdf_finite(ox) && tsdf_finite(oy) && tsdf_finite(oz) && tsdf_positive(voxel_size) ? MI_OK : MI_E_PARAM;
}
inline int tsdf_grid_status(float ox, float oy, float oz, float voxel_size, float truncation) {
  return tsdf_origin_status(ox, oy, oz, voxel_size) == MI_OK && tsdf_positive(truncation) ? MI_OK : MI_E_PARAM;
}
inline bool tsdf_depth_range_ok(float min_depth, float max_depth) {
  return min_depth > 0.0f && max_depth >= min_depth && max_depth < INFINITY;
}
// the (batch, frames, h, w) frames of an integration
inline int tsdf_frames_status(int batch, int frames, int h, int w) {
  if (frames < 1 || h < 3 || w < 3) return MI_E_SHAPE;
  if ((double)batch * (double)frames * (double)h * (double)w >= 2147483648.0) return MI_E_SHAPE;
  return MI_OK;
}
// max_weight and the camera of an integration
inline int tsdf_fusion_status(float max_weight, const TsdfCam &cam) {
  if (!tsdf_positive(max_weight) || !tsdf_positive(cam.fx) || !tsdf_positive(cam.fy) || !tsdf_finite(cam.cx) ||
      !tsdf_finite(cam.cy) || !tsdf_positive(cam.z_scale) || !tsdf_depth_range_ok(cam.min_depth, cam.max_depth))
    return MI_E_PARAM;
  return MI_OK;
}

}  // namespace
