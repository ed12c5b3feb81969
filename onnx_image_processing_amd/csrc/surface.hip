// K20 TSDF surface extraction (include/mi355x_match.h, "TSDF surface extraction"): the zero level set of a K19 volume as an
// indexed triangle mesh by marching tetrahedra over the Kuhn split of every cell, with per-vertex normals, batched over
// volumes under K19's contract.  The arithmetic is surface_math.h's.
//
// Workspace, per call: one byte per voxel (its owned-edge mask, bit e = class e), then per x-row of a volume the pair
// (vertices, triangles) it owns and the pair of its exclusive prefixes.  A row (j, k) owns the vertices of its voxels' edges
// and the triangles of the cells whose corner 0 lies in it, so that vertex ids and triangle ordinals both follow the rows.
//
// K20c  surface_classify_kernel  grid (ceil(nz ny / 4), batch), 256 threads: a wave owns one x-row as in K19i, lane l its
//       voxels l, l + 64, ...  A lane loads its voxel's column of the four rows (j, k), (j+1, k), (j, k+1), (j+1, k+1) (8 bytes
//       each; the three neighbour rows come from cache, every row being the first row of one wave), turns it into observed /
//       inside bits and takes the column of i + 1 from the next lane; lane 63 loads it.  It writes the mask byte and the
//       row's totals.
// K20s  surface_scan_kernel      grid (batch), 1024 threads: an exclusive scan of a volume's row totals (a contiguous run of
//       rows per thread, the threads' sums scanned in LDS), and the counts from the same scan.
// K20e  surface_emit_kernel      the grid of K20c plus up to SURFACE_TAIL_BLOCKS workgroups per volume that write the rows
//       past the counts.  A row whose totals are zero leaves at once.  Otherwise the wave walks the row in chunks of 64 with
//       the running vertex counts of its four rows as carries: a voxel's first vertex id is its row's prefix + the carry + the
//       count of the lanes below (a wave scan of the masks' popcounts); the id of edge (p, e) is that base + popcount(mask[p]
//       & ((1 << e) - 1)).  Vertices and normals are written by the edge's owner, triangles by the cell.  Nothing a workgroup
//       reads is written by another workgroup of the same launch.
// No atomics, no memset, nothing allocated, integer sums only: the same bits alone or in a batch, from run to run and under
// graph replay; every output element is written.  Built with -ffp-contract=off.
#include "common.h"
#include "surface_math.h"
#include "tsdf_shared.h"

#include <math.h>

namespace {

constexpr int SURFACE_SCAN_THREADS = 1024;
constexpr int SURFACE_TAIL_BLOCKS = 64;

struct SurfaceGrid {
  int nx, ny, nz;
  float origin[3], voxel_size, min_weight;
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ int wave_scan_int(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// bits of the voxels (i, j + dy, k + dz), dy + 2 dz = r = 0..3: observed at bit r, inside at bit 4 + r; 0 where there is no voxel.
// line points at voxel 0 of row (j, k).
__device__ __forceinline__ unsigned surface_column(const float2 *__restrict__ line, const SurfaceGrid &g, int i, bool has_y, bool has_z) {
  if (i >= g.nx) return 0u;
  const size_t row = (size_t)g.nx, slice = (size_t)g.nx * (size_t)g.ny;
  const float2 r0 = line[i];
  unsigned b = surface_voxel_bits(r0.x, r0.y, g.min_weight), c = (b & 1u) | ((b >> 1) << 4);
  if (has_y) {
    const float2 r1 = line[row + i];
    b = surface_voxel_bits(r1.x, r1.y, g.min_weight);
    c |= ((b & 1u) << 1) | ((b >> 1) << 5);
  }
  if (has_z) {
    const float2 r2 = line[slice + i];
    b = surface_voxel_bits(r2.x, r2.y, g.min_weight);
    c |= ((b & 1u) << 2) | ((b >> 1) << 6);
    if (has_y) {
      const float2 r3 = line[slice + row + i];
      b = surface_voxel_bits(r3.x, r3.y, g.min_weight);
      c |= ((b & 1u) << 3) | ((b >> 1) << 7);
    }
  }
  return c;
}

// the cell's corner bits (bit m: corner m = dx + 2 r) from the columns of i (c0) and i + 1 (c1)
__device__ __forceinline__ void surface_corners(unsigned c0, unsigned c1, unsigned *obs, unsigned *inside) {
  unsigned o = 0, n = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    o |= (((c0 >> r) & 1u) << (2 * r)) | (((c1 >> r) & 1u) << (2 * r + 1));
    n |= (((c0 >> (4 + r)) & 1u) << (2 * r)) | (((c1 >> (4 + r)) & 1u) << (2 * r + 1));
  }
  *obs = o;
  *inside = n;
}

// the columns of voxel i (this lane's) and of i + 1: the next lane's, which lane 63 loads itself
__device__ __forceinline__ void surface_columns(const float2 *__restrict__ line, const SurfaceGrid &g, int i, int lane, bool has_y,
                                                bool has_z, unsigned *c0, unsigned *c1) {
  *c0 = surface_column(line, g, i, has_y, has_z);
  *c1 = (unsigned)__shfl_down((int)*c0, 1, 64);
  if (lane == 63) *c1 = surface_column(line, g, i + 1, has_y, has_z);
}

// ---- K20c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surface_classify_kernel(const float2 *__restrict__ vol, SurfaceGrid g,
                                                               uint8_t *__restrict__ mask, int2 *__restrict__ totals) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, rows = g.nz * g.ny;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);       // over nz * ny, wave-uniform
  if (row >= rows) return;
  const int k = row / g.ny, j = row - k * g.ny;
  const bool has_y = j + 1 < g.ny, has_z = k + 1 < g.nz;
  const size_t first = ((size_t)b * (size_t)rows + (size_t)row) * (size_t)g.nx;
  const float2 *line = vol + first;
  int nv = 0, nt = 0;
  for (int i0 = 0; i0 < g.nx; i0 += 64) {
    const int i = i0 + lane;
    unsigned c0, c1, obs, inside, edges;
    surface_columns(line, g, i, lane, has_y, has_z, &c0, &c1);
    surface_corners(c0, c1, &obs, &inside);
    nt += surface_cell(obs, inside, &edges);
    nv += __builtin_popcount(edges);
    if (mask && i < g.nx) mask[first + i] = (uint8_t)edges;
  }
  nv = wave_sum_int(nv);
  nt = wave_sum_int(nt);
  if (lane == 0) totals[(size_t)b * (size_t)rows + (size_t)row] = make_int2(nv, nt);
}

// ---- K20s ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SURFACE_SCAN_THREADS) void surface_scan_kernel(const int2 *__restrict__ totals, int rows,
                                                                            int2 *__restrict__ prefix, int32_t *__restrict__ counts) {
  __shared__ int2 part[SURFACE_SCAN_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const int2 *in = totals + (size_t)b * (size_t)rows;
  int2 *out = prefix + (size_t)b * (size_t)rows;
  const int per = (rows + SURFACE_SCAN_THREADS - 1) / SURFACE_SCAN_THREADS;
  const int r0 = min(rows, t * per), r1 = min(rows, r0 + per);
  int2 s = make_int2(0, 0);
  for (int r = r0; r < r1; ++r) {
    const int2 v = in[r];
    s.x += v.x;
    s.y += v.y;
  }
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < SURFACE_SCAN_THREADS; o <<= 1) {       // Hillis-Steele, inclusive
    int2 u = make_int2(0, 0);
    if (t >= o) u = part[t - o];
    __syncthreads();
    if (t >= o) {
      part[t].x += u.x;
      part[t].y += u.y;
    }
    __syncthreads();
  }
  int2 run = t > 0 ? part[t - 1] : make_int2(0, 0);
  for (int r = r0; r < r1; ++r) {
    const int2 v = in[r];
    out[r] = run;
    run.x += v.x;
    run.y += v.y;
  }
  if (t == SURFACE_SCAN_THREADS - 1) {
    counts[2 * b] = part[t].x;
    counts[2 * b + 1] = part[t].y;
  }
}

// ---- K20e ------------------------------------------------------------------------------------------------------------------
struct SurfaceOut {
  float4 *vertex, *normal;
  int32_t *triangle;
  int max_vertices, max_triangles;
};

__device__ __forceinline__ int surface_pick6(const int *v, int n) {      // v[n] without indexing registers by a variable
  return n == 0 ? v[0] : n == 1 ? v[1] : n == 2 ? v[2] : n == 3 ? v[3] : n == 4 ? v[4] : v[5];
}

template <bool TRIANGLES>
__global__ __launch_bounds__(256) void surface_emit_kernel(const float2 *__restrict__ vol, SurfaceGrid g,
                                                           const uint8_t *__restrict__ mask, const int2 *__restrict__ totals,
                                                           const int2 *__restrict__ prefix, const int32_t *__restrict__ counts,
                                                           int row_blocks, int tail_blocks, SurfaceOut out) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, rows = g.nz * g.ny;
  float4 *vertex = out.vertex ? out.vertex + (size_t)b * (size_t)out.max_vertices : nullptr;
  float4 *normal = out.normal ? out.normal + (size_t)b * (size_t)out.max_vertices : nullptr;
  int32_t *triangle = out.triangle ? out.triangle + (size_t)b * (size_t)out.max_triangles * 3 : nullptr;
  if ((int)blockIdx.x >= row_blocks) {                       // the rows past the counts: zeros and (-1, -1, -1)
    const int first = ((int)blockIdx.x - row_blocks) * 256 + (int)threadIdx.x, stride = tail_blocks * 256;
    const int nv = counts[2 * b], nt = counts[2 * b + 1];
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (long long r = (long long)nv + first; r < out.max_vertices; r += stride) {
      if (vertex) vertex[r] = zero;
      if (normal) normal[r] = zero;
    }
    if (TRIANGLES)
      for (long long r = (long long)nt + first; r < out.max_triangles; r += stride) {
        triangle[3 * r] = -1;
        triangle[3 * r + 1] = -1;
        triangle[3 * r + 2] = -1;
      }
    return;
  }
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
  if (row >= rows) return;
  const size_t brow = (size_t)b * (size_t)rows + (size_t)row;
  const int2 tot = totals[brow];
  const bool cells = TRIANGLES && tot.y > 0;
  if (!(cells || ((vertex || normal) && tot.x > 0))) return;
  const int k = row / g.ny, j = row - k * g.ny;
  const bool has_y = j + 1 < g.ny, has_z = k + 1 < g.nz;     // both true where the row has cells
  const size_t first = brow * (size_t)g.nx, srow = (size_t)g.nx, sslice = (size_t)g.nx * (size_t)g.ny;
  const float2 *line = vol + first;
  const float *volume = reinterpret_cast<const float *>(vol + (size_t)b * (size_t)rows * (size_t)g.nx);
  const uint8_t *mline = mask + first;
  const int2 pre = prefix[brow];
  // running first vertex id of the chunk in the rows (j, k), (j+1, k), (j, k+1), (j+1, k+1), and triangle ordinal
  int carry0 = pre.x, carry1 = 0, carry2 = 0, carry3 = 0, tcarry = pre.y;
  if (cells) {
    carry1 = prefix[brow + 1].x;
    carry2 = prefix[brow + (size_t)g.ny].x;
    carry3 = prefix[brow + (size_t)g.ny + 1].x;
  }
  for (int i0 = 0; i0 < g.nx; i0 += 64) {
    const int i = i0 + lane;
    const bool here = i < g.nx;
    const unsigned m0 = here ? mline[i] : 0u;
    const int own = __builtin_popcount(m0);
    const int incl0 = wave_scan_int(own, lane);
    const int base0 = carry0 + incl0 - own;
    const int next0 = carry0 + __shfl(incl0, 63, 64);
    if ((vertex || normal) && m0 != 0u && base0 < out.max_vertices) {
      const float f_p = line[i].x;
      int id = base0;
#pragma unroll
      for (int e = 1; e < 8; ++e) {
        if (!((m0 >> e) & 1u)) continue;
        if (id < out.max_vertices) {
          const float f_q = line[(size_t)i + (e & 1) + ((e >> 1) & 1) * srow + ((e >> 2) & 1) * sslice].x;
          const float a = surface_alpha(f_p, f_q);
          float pos[3], gc[3], n[3];
          surface_vertex(i, j, k, e, a, g.origin, g.voxel_size, pos, gc);
          if (vertex) vertex[id] = make_float4(pos[0], pos[1], pos[2], 1.0f);
          if (normal) {
            const bool ok = surface_normal(volume, g.nx, g.ny, g.nz, gc, n);
            normal[id] = make_float4(n[0], n[1], n[2], ok ? 1.0f : 0.0f);
          }
        }
        ++id;
      }
    }
    carry0 = next0;
    if (!cells) continue;
    // ---- triangles of the cells (i, j, k) ----
    const unsigned m1 = here ? mline[srow + i] : 0u, m2 = here ? mline[sslice + i] : 0u, m3 = here ? mline[sslice + srow + i] : 0u;
    const int c1 = __builtin_popcount(m1), c2 = __builtin_popcount(m2), c3 = __builtin_popcount(m3);
    const int incl1 = wave_scan_int(c1, lane), incl2 = wave_scan_int(c2, lane), incl3 = wave_scan_int(c3, lane);
    const int next1 = carry1 + __shfl(incl1, 63, 64), next2 = carry2 + __shfl(incl2, 63, 64), next3 = carry3 + __shfl(incl3, 63, 64);
    // masks and first ids of the eight corners: corner m = dx + 2 r; dx = 1 is the next lane's voxel, for lane 63 the first
    // voxel of the next chunk, whose first id is the running count after this chunk
    const int bs0 = base0, bs2 = carry1 + incl1 - c1, bs4 = carry2 + incl2 - c2, bs6 = carry3 + incl3 - c3;
    int bs1 = __shfl_down(bs0, 1, 64), bs3 = __shfl_down(bs2, 1, 64), bs5 = __shfl_down(bs4, 1, 64), bs7 = __shfl_down(bs6, 1, 64);
    unsigned k1 = (unsigned)__shfl_down((int)m0, 1, 64), k3 = (unsigned)__shfl_down((int)m1, 1, 64);
    unsigned k5 = (unsigned)__shfl_down((int)m2, 1, 64), k7 = (unsigned)__shfl_down((int)m3, 1, 64);
    if (lane == 63) {
      const bool more = i + 1 < g.nx;
      bs1 = next0; bs3 = next1; bs5 = next2; bs7 = next3;
      k1 = more ? mline[i + 1] : 0u;
      k3 = more ? mline[srow + i + 1] : 0u;
      k5 = more ? mline[sslice + i + 1] : 0u;
      k7 = more ? mline[sslice + srow + i + 1] : 0u;
    }
    carry1 = next1; carry2 = next2; carry3 = next3;
    unsigned col0, col1, obs, inside, edges;
    surface_columns(line, g, i, lane, has_y, has_z, &col0, &col1);
    surface_corners(col0, col1, &obs, &inside);
    const int nt = surface_cell(obs, inside, &edges);
    const int tincl = wave_scan_int(nt, lane);
    int ord = tcarry + tincl - nt;
    tcarry += __shfl(tincl, 63, 64);
    if (nt == 0 || ord >= out.max_triangles) continue;       // after the chunk's last cross-lane operation
    const int cb[8] = {bs0, bs1, bs2, bs3, bs4, bs5, bs6, bs7};
    const unsigned cm[8] = {m0, k1, m1, k3, m2, k5, m3, k7};
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const unsigned corners = (1u << SURFACE_TETS[t][0]) | (1u << SURFACE_TETS[t][1]) | (1u << SURFACE_TETS[t][2]) | (1u << SURFACE_TETS[t][3]);
      if ((obs & corners) != corners) continue;
      const uint32_t entry = surface_table_entry(t, surface_tet_case(inside, t));
      const int n = (int)(entry & 3u);
      if (n == 0) continue;
      int ids[6];                                            // the ids on the tetrahedron's six edges; t is a constant here
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const int p = SURFACE_TETS[t][SURFACE_EDGE_POS[e][0]], q = SURFACE_TETS[t][SURFACE_EDGE_POS[e][1]];
        ids[e] = cb[p] + __builtin_popcount(cm[p] & ((1u << (q - p)) - 1u));
      }
      for (int tri = 0; tri < n; ++tri) {
        if (ord < out.max_triangles) {
          const uint32_t ev = entry >> (2 + 9 * tri);
          int32_t *o = triangle + 3 * (size_t)ord;
          o[0] = surface_pick6(ids, (int)(ev & 7u));
          o[1] = surface_pick6(ids, (int)((ev >> 3) & 7u));
          o[2] = surface_pick6(ids, (int)((ev >> 6) & 7u));
        }
        ++ord;
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
size_t surface_align16(size_t n) { return (n + 15) & ~(size_t)15; }

// K19's volume checks (tsdf_shared.h), and ids that fit int32: 12 * voxels of one volume < 2^31.  The id bound comes after
// K19's batch bound here and still wins over it: a batch above 65535 of volumes that large fails K19's element bound first.
int surface_volume_status(int batch, int nz, int ny, int nx) {
  if (const int s = tsdf_volume_status(batch, nz, ny, nx)) return s;
  if (12.0 * (double)nz * (double)ny * (double)nx >= 2147483648.0) return MI_E_SHAPE;
  return MI_OK;
}

}  // namespace

extern "C" size_t mi_tsdf_surface_workspace_bytes(int batch, int nz, int ny, int nx) {
  if (surface_volume_status(batch, nz, ny, nx) != MI_OK) return 0;
  const size_t rows = (size_t)batch * (size_t)nz * (size_t)ny;
  return surface_align16(rows * (size_t)nx) + 2 * rows * sizeof(int2);
}

extern "C" int mi_tsdf_surface(const float *volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y,
                               float origin_z, float voxel_size, float min_weight, int max_vertices, int max_triangles,
                               float *vertex_out, float *normal_out, int32_t *triangle_out, int32_t *counts_out, void *workspace,
                               size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!volume || !counts_out || !workspace) return MI_E_NULL;
  if ((!vertex_out && max_vertices != 0) || (!triangle_out && max_triangles != 0)) return MI_E_NULL;
  if (const int s = surface_volume_status(batch, nz, ny, nx)) return s;
  if ((double)batch * (double)max_vertices >= 2147483648.0 || (double)batch * (double)max_triangles >= 2147483648.0) return MI_E_SHAPE;
  if (tsdf_origin_status(origin_x, origin_y, origin_z, voxel_size) != MI_OK || !tsdf_positive(min_weight) || max_vertices < 0 ||
      max_triangles < 0)
    return MI_E_PARAM;
  if (!mi_aligned16({volume, vertex_out, normal_out, workspace}) || ((uintptr_t)triangle_out % 4) != 0 ||
      ((uintptr_t)counts_out % 4) != 0)
    return MI_E_ALIGN;
  if (workspace_bytes < mi_tsdf_surface_workspace_bytes(batch, nz, ny, nx)) return MI_E_CAPACITY;

  const size_t rows = (size_t)batch * (size_t)nz * (size_t)ny;
  uint8_t *mask = static_cast<uint8_t *>(workspace);
  int2 *totals = reinterpret_cast<int2 *>(mask + surface_align16(rows * (size_t)nx));
  int2 *prefix = totals + rows;
  const bool sizing = max_vertices == 0 && max_triangles == 0;           // nothing to write but the counts: no mask is kept
  const SurfaceGrid g{nx, ny, nz, {origin_x, origin_y, origin_z}, voxel_size, min_weight};
  const float2 *vol = reinterpret_cast<const float2 *>(volume);
  const int row_blocks = ceil_div(nz * ny, 4);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(surface_classify_kernel, dim3((unsigned)row_blocks, (unsigned)batch), dim3(256), 0, s, vol, g,
                     sizing ? nullptr : mask, totals);
  MI_CHECK_LAUNCH();
  hipLaunchKernelGGL(surface_scan_kernel, dim3((unsigned)batch), dim3(SURFACE_SCAN_THREADS), 0, s, totals, nz * ny, prefix, counts_out);
  if (sizing) return mi_launch_status();
  MI_CHECK_LAUNCH();
  const int longest = max_vertices > max_triangles ? max_vertices : max_triangles;
  const int tail_blocks = longest == 0 ? 0 : (ceil_div(longest, 256) < SURFACE_TAIL_BLOCKS ? ceil_div(longest, 256) : SURFACE_TAIL_BLOCKS);
  const SurfaceOut out{reinterpret_cast<float4 *>(vertex_out), reinterpret_cast<float4 *>(normal_out), triangle_out, max_vertices,
                       max_triangles};
  const dim3 grid((unsigned)(row_blocks + tail_blocks), (unsigned)batch);
  if (triangle_out)
    hipLaunchKernelGGL(surface_emit_kernel<true>, grid, dim3(256), 0, s, vol, g, mask, totals, prefix, counts_out, row_blocks,
                       tail_blocks, out);
  else
    hipLaunchKernelGGL(surface_emit_kernel<false>, grid, dim3(256), 0, s, vol, g, mask, totals, prefix, counts_out, row_blocks,
                       tail_blocks, out);
  return mi_launch_status();
}
