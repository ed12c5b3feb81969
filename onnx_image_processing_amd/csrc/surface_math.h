// The arithmetic of K20 (surface.hip; include/mi355x_match.h, "TSDF surface extraction"): a voxel's observed / inside bits, a
// cell's owned-edge mask and triangle count, the 6 x 16 triangle table of the Kuhn split generated from the header's
// orientation rule, the interpolation along an edge, the vertex and its normal.  float32 with nothing fused.  Like
// tsdf_math.h it needs no HIP header: a plain C++ compiler builds it for the host (tests/native/surface_host.cpp).
#pragma once
#include "tsdf_math.h"

#include <stdint.h>

namespace {

// the six tetrahedra of a cell around the diagonal 0-7: corners in path order; corner m is the voxel offset
// (m & 1, (m >> 1) & 1, (m >> 2) & 1), so an edge p < q has q = p | e with e = q - p its class
constexpr int SURFACE_TETS[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// the six edges of a tetrahedron as pairs of path positions a < b, and the edge of a pair
constexpr int SURFACE_EDGE_POS[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
constexpr int surface_edge_of(int a, int b) { return a > b ? surface_edge_of(b, a) : (a == 0 ? b - 1 : a + b); }

// One table entry: the triangle count in bits 0-1, then the triangles' edges (indices into SURFACE_EDGE_POS), 3 bits each:
// triangle n, vertex v at bit 2 + 3 * (3 * n + v).
struct SurfaceTable {
  uint32_t entry[6][16];
};

// twice the midpoint of edge `edge` of tetrahedron t in the unit cell, along `axis`
constexpr int surface_mid2(int t, int edge, int axis) {
  return ((SURFACE_TETS[t][SURFACE_EDGE_POS[edge][0]] >> axis) & 1) + ((SURFACE_TETS[t][SURFACE_EDGE_POS[edge][1]] >> axis) & 1);
}

// the triangle (e0, e1, e2) of tetrahedron t in case `mask` (bit s: path position s is inside), its last two vertices swapped
// unless (v1 - v0) x (v2 - v0) points from the inside corners' mean towards the outside corners' mean
constexpr uint32_t surface_oriented(int t, int mask, int e0, int e1, int e2) {
  int in[3] = {0, 0, 0}, out[3] = {0, 0, 0}, n_in = 0, n_out = 0;
  for (int s = 0; s < 4; ++s)
    for (int a = 0; a < 3; ++a) {
      const int c = (SURFACE_TETS[t][s] >> a) & 1;
      if ((mask >> s) & 1) in[a] += c; else out[a] += c;
    }
  for (int s = 0; s < 4; ++s) ((mask >> s) & 1) ? ++n_in : ++n_out;
  int u[3] = {0, 0, 0}, v[3] = {0, 0, 0};
  for (int a = 0; a < 3; ++a) {
    u[a] = surface_mid2(t, e1, a) - surface_mid2(t, e0, a);
    v[a] = surface_mid2(t, e2, a) - surface_mid2(t, e0, a);
  }
  const int n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  int dot = 0;
  for (int a = 0; a < 3; ++a) dot += n[a] * (out[a] * n_in - in[a] * n_out);      // the means' difference times n_in n_out
  return dot > 0 ? (uint32_t)(e0 | (e1 << 3) | (e2 << 6)) : (uint32_t)(e0 | (e2 << 3) | (e1 << 6));
}

constexpr SurfaceTable surface_make_table() {
  SurfaceTable T{};
  for (int t = 0; t < 6; ++t)
    for (int mask = 0; mask < 16; ++mask) {
      int pos_in[4] = {0, 0, 0, 0}, pos_out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
      for (int s = 0; s < 4; ++s) {
        if ((mask >> s) & 1) pos_in[n_in++] = s; else pos_out[n_out++] = s;
      }
      uint32_t e = 0;
      if (n_in == 1 || n_in == 3) {                         // one corner on its own side: the edges to the three others
        const int s = n_in == 1 ? pos_in[0] : pos_out[0];
        const int *o = n_in == 1 ? pos_out : pos_in;
        e = 1u | (surface_oriented(t, mask, surface_edge_of(s, o[0]), surface_edge_of(s, o[1]), surface_edge_of(s, o[2])) << 2);
      } else if (n_in == 2) {                               // A < B inside, C < D outside: (AC, AD, BD) then (AC, BD, BC)
        const int A = pos_in[0], B = pos_in[1], C = pos_out[0], D = pos_out[1];
        const int ac = surface_edge_of(A, C), ad = surface_edge_of(A, D), bd = surface_edge_of(B, D), bc = surface_edge_of(B, C);
        e = 2u | (surface_oriented(t, mask, ac, ad, bd) << 2) | (surface_oriented(t, mask, ac, bd, bc) << 11);
      }
      T.entry[t][mask] = e;
    }
  return T;
}

ICP_HD uint32_t surface_table_entry(int t, int mask) {
  static constexpr SurfaceTable T = surface_make_table();
  return T.entry[t][mask];
}

// a voxel's bits: 1 = observed (weight >= min_weight), 2 = inside (observed and not tsdf > 0: NaN counts as inside)
ICP_HD unsigned surface_voxel_bits(float tsdf, float weight, float min_weight) {
  const bool obs = weight >= min_weight;
  return (obs ? 1u : 0u) | ((obs && !(tsdf > 0.0f)) ? 2u : 0u);
}

// One cell from its corners' bits (bit m of `obs` / `inside`: corner m; a corner outside the volume is not observed):
// *edges has bit e set iff the edge of class e owned by corner 0 carries a vertex (both ends observed, one of them inside);
// the return value is the number of triangles of the six tetrahedra (all four corners observed; 1 or 3 inside: 1, 2 inside: 2).
ICP_HD int surface_cell(unsigned obs, unsigned inside, unsigned *edges) {
  *edges = (obs & 1u) ? (obs & (inside ^ ((inside & 1u) ? 0xFFu : 0u)) & 0xFEu) : 0u;
  int triangles = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const unsigned corners = (1u << SURFACE_TETS[t][0]) | (1u << SURFACE_TETS[t][1]) | (1u << SURFACE_TETS[t][2]) | (1u << SURFACE_TETS[t][3]);
    if ((obs & corners) == corners) {
      const int n_in = __builtin_popcount(inside & corners);
      triangles += (n_in == 0 || n_in == 4) ? 0 : (n_in == 2 ? 2 : 1);
    }
  }
  return triangles;
}

// the case of tetrahedron t: bit s set iff its path position s is inside
ICP_HD int surface_tet_case(unsigned inside, int t) {
  return (int)(((inside >> SURFACE_TETS[t][0]) & 1u) | (((inside >> SURFACE_TETS[t][1]) & 1u) << 1) |
               (((inside >> SURFACE_TETS[t][2]) & 1u) << 2) | (((inside >> SURFACE_TETS[t][3]) & 1u) << 3));
}

// where the field crosses zero between the edge's ends p and q, as a fraction of the edge from p
ICP_HD float surface_alpha(float f_p, float f_q) { return f_p / (f_p - f_q); }

// the vertex on the edge of class e owned by voxel (i, j, k): its world position and its grid coordinate
ICP_HD void surface_vertex(int i, int j, int k, int e, float a, const float *origin, float voxel_size, float *pos, float *g) {
  const int idx[3] = {i, j, k};
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float c = tsdf_centre(idx[ax], voxel_size, origin[ax]);
    const bool moves = (e >> ax) & 1;
    pos[ax] = moves ? c + a * voxel_size : c;
    g[ax] = moves ? (float)idx[ax] + a : (float)idx[ax];
  }
}

// the normal at grid coordinate g: the central difference of the trilinear field over +- one voxel per axis (all six samples
// valid), normalised; it points to the positive (free) side.  false and zeros otherwise.
ICP_HD bool surface_normal(const float *vol, int nx, int ny, int nz, const float *g, float *n) {
  n[0] = n[1] = n[2] = 0.0f;
  float grad[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float hi[3] = {g[0], g[1], g[2]}, lo[3] = {g[0], g[1], g[2]}, fh, fl;
    hi[a] = g[a] + 1.0f;
    lo[a] = g[a] - 1.0f;
    ok = tsdf_sample(vol, nx, ny, nz, hi, &fh) && ok;
    ok = tsdf_sample(vol, nx, ny, nz, lo, &fl) && ok;
    grad[a] = fh - fl;
  }
  if (!ok) return false;
  const float len = sqrtf((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
  if (!(len > 0.0f) || !(len < INFINITY)) return false;
  n[0] = grad[0] / len;
  n[1] = grad[1] / len;
  n[2] = grad[2] / len;
  return true;
}

}  // namespace
