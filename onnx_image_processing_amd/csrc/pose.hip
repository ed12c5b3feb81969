// K15 relative pose (include/mi355x_match.h, "relative pose"): RANSAC essential matrix, pose recovery, two-view DLT.
// Replaces the host step of reference pytorch_model/vo/pose_estimation.py:53-162 (cv2.findEssentialMat(RANSAC),
// cv2.recoverPose, cv2.triangulatePoints), one pair at a time there, batched over pairs here.
//
// The RANSAC skeleton -- staging, the hypothesis kernel, the first minimum, the mask write-back, the host checks -- is
// ransac_wave.h's; PoModel below is what K15 supplies to it.
// K15a  rw_hyp_kernel<PoModel>.  Each lane builds the 8x9 epipolar system of its sample on Hartley-normalised
//       points in LDS -- element (r, c) of lane l at word (r * 9 + c) * 64 + l, so every access of the wave is one bank row,
//       conflict-free, and the elimination indexes rows and columns at run time without scratch -- and reduces it by
//       Gauss-Jordan with complete pivoting (the column permutation is nine nibbles of one 64-bit register).  Null vector,
//       denormalisation, manifold projection (essential_math.h).
// K15b  po_ransac_kernel   one wave per pair: the best hypothesis, then refine_rounds x {inliers of the best E at k_r *
//       threshold -> normal equations (45 sums per lane, lanes stride over the correspondences, wave_sum_dpp) -> minimum
//       eigenvector by shifted inverse iteration on a Cholesky factor, every lane redundantly -> denormalise, project ->
//       rescore: the float32 truncated sum over all rows, compared in float32}; inlier bytes of the best E at `threshold`.
// K15c  po_refit_kernel    the refit alone on a caller's mask.
// K15d  po_pose_kernel     one wave per pair: t from the largest cross product of E's columns, the two rotations
//       cof(E) -+ [t]x E, four candidates, per-correspondence depths from the two-view linear equations, ballot counts.
// K15e  po_triangulate_kernel   one thread per point: 4x4 DLT rows conditioned to unit norm, one-sided Jacobi SVD.
// fp32 throughout; built with -ffp-contract=off; no atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "essential_math.h"
#include "ransac_wave.h"       // the skeleton; pose_sampler.h: po_mix, po_draw, po_sample_ranks (header: "Sampling")

#include <math.h>

namespace {

constexpr int PO_MAXN = MI_POSE_MAX_N;
constexpr float PO_RANK_TOL = 1e-5f;      // a pivot at or below this fraction of the first pivot: rank-deficient sample
constexpr int PO_SQUARINGS = 14;          // manifold projection: B^(2^14) in place of 16384 power-iteration steps
constexpr int PO_JACOBI_SWEEPS = 6;       // triangulate: one-sided Jacobi sweeps over the 6 column pairs

// po_sampson, the squared Sampson distance of one correspondence (header: "Scoring"), is essential_math.h's

// Hartley parameters -> E = T2^T E_hat T1, then the projection onto singular values (s, s, 0).  v: the null vector
// (row-major E_hat), h1 / h2: (cx, cy, s) of image 1 / 2.  Returns false when the result is not finite.
__host__ __device__ __forceinline__ bool po_finish_e(const float *v, const float *h1, const float *h2, float *e_out) {
  const float t1[3][3] = {{h1[2], 0.0f, -h1[2] * h1[0]}, {0.0f, h1[2], -h1[2] * h1[1]}, {0.0f, 0.0f, 1.0f}};
  const float t2[3][3] = {{h2[2], 0.0f, -h2[2] * h2[0]}, {0.0f, h2[2], -h2[2] * h2[1]}, {0.0f, 0.0f, 1.0f}};
  float tmp[3][3], e[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) tmp[r][c] = (t2[0][r] * v[0 * 3 + c] + t2[1][r] * v[1 * 3 + c]) + t2[2][r] * v[2 * 3 + c];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) e[r][c] = (tmp[r][0] * t1[0][c] + tmp[r][1] * t1[1][c]) + tmp[r][2] * t1[2][c];
  float bm[3][3], bs[3][3];
  em_manifold_gram(e, bm, bs);
  // dominant eigenvector of bm (va) and of bs (vc): square the matrix PO_SQUARINGS times (scaled by its trace, which
  // bounds its largest eigenvalue from above and from below by a third: no overflow, no underflow; a minimal sample's E_hat
  // has no small third singular value, so the eigenvalues of bs can be within a percent of each other: 6 squarings left
  // errors of 0.5, 14 leave 3e-6 in a float32 emulation over random matrices), then take the column of largest norm -- every
  // column of B^(2^k) is the dominant eigenvector times its own component, so no start vector can be orthogonal to it
  float vv[2][3];
  for (int which = 0; which < 2; ++which) {
    float m[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) m[r][c] = which ? bs[r][c] : bm[r][c];
    for (int it = 0; it < PO_SQUARINGS; ++it) {
      const float inv_tr = 1.0f / ((m[0][0] + m[1][1]) + m[2][2]);
      float sq[3][3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m[r][c] = m[r][c] * inv_tr;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sq[r][c] = (m[r][0] * m[0][c] + m[r][1] * m[1][c]) + m[r][2] * m[2][c];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m[r][c] = sq[r][c];
    }
    float best = -1.0f;
    for (int c = 0; c < 3; ++c) {
      const float nn = (m[0][c] * m[0][c] + m[1][c] * m[1][c]) + m[2][c] * m[2][c];
      if (nn > best) {
        best = nn;
        vv[which][0] = m[0][c];
        vv[which][1] = m[1][c];
        vv[which][2] = m[2][c];
      }
    }
    unit3(vv[which]);
  }
  // Rayleigh-Ritz in the plane orthogonal to vc: rotate (va, vc x va) onto the eigenvectors of the 2x2 restriction of
  // E^T E, so that E va and E vb are orthogonal even when the two leading singular values are close
  float va[3] = {vv[0][0], vv[0][1], vv[0][2]}, vb[3], w[3];
  const float *vc = vv[1];
  const float dac = (va[0] * vc[0] + va[1] * vc[1]) + va[2] * vc[2];
  for (int r = 0; r < 3; ++r) va[r] = va[r] - dac * vc[r];
  unit3(va);
  cross3(vc, va, vb);
  unit3(vb);
  matvec3(bm, va, w);
  const float gaa = (va[0] * w[0] + va[1] * w[1]) + va[2] * w[2], gab = (vb[0] * w[0] + vb[1] * w[1]) + vb[2] * w[2];
  matvec3(bm, vb, w);
  const float gbb = (vb[0] * w[0] + vb[1] * w[1]) + vb[2] * w[2];
  const float th = 0.5f * atan2f(2.0f * gab, gaa - gbb);
  const float cs = cosf(th), sn = sinf(th);
  float v1[3];
  for (int r = 0; r < 3; ++r) v1[r] = cs * va[r] + sn * vb[r];
  float proj[3][3];
  em_manifold_from_vectors(e, v1, vc, proj);
  float chk = 0.0f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      e_out[r * 3 + c] = proj[r][c];
      chk += fabsf(proj[r][c]);
    }
  return chk < INFINITY && chk > 0.0f;       // false for NaN, infinities and the zero matrix
}

// E from one 8-sample (header: "Solve").  A: the lane's 81-word work area, word w at A[w * 64] (K15a: LDS, lanes
// interleaved; a host harness passes any buffer of 81 * 64 floats).  False: rank-deficient sample or no finite result.
__host__ __device__ __forceinline__ int po_col(unsigned long long perm, int c) { return (int)((perm >> (4 * c)) & 15ull); }
__host__ __device__ inline bool po_solve_minimal(const float4 *q, float *A, float *e) {
  bool ok = true;
  // Hartley normalisation of the sample: centroid, then sqrt(2) over the RMS distance to it
  float h1[3], h2[3];
  {
    float sx1 = 0.0f, sy1 = 0.0f, sx2 = 0.0f, sy2 = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s) { sx1 += q[s].x; sy1 += q[s].y; sx2 += q[s].z; sy2 += q[s].w; }
    h1[0] = sx1 / 8.0f; h1[1] = sy1 / 8.0f; h2[0] = sx2 / 8.0f; h2[1] = sy2 / 8.0f;
    float d1 = 0.0f, d2 = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float ax = q[s].x - h1[0], ay = q[s].y - h1[1], bx = q[s].z - h2[0], by = q[s].w - h2[1];
      d1 += ax * ax + ay * ay;
      d2 += bx * bx + by * by;
    }
    ok = d1 > 0.0f && d2 > 0.0f;
    h1[2] = sqrtf(2.0f) / sqrtf(d1 / 8.0f);
    h2[2] = sqrtf(2.0f) / sqrtf(d2 / 8.0f);
  }
#define PO_A(r, c) A[((r) * 9 + (c)) * 64]
  if (ok) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float x1 = (q[s].x - h1[0]) * h1[2], y1 = (q[s].y - h1[1]) * h1[2];
      const float x2 = (q[s].z - h2[0]) * h2[2], y2 = (q[s].w - h2[1]) * h2[2];
      PO_A(s, 0) = x2 * x1; PO_A(s, 1) = x2 * y1; PO_A(s, 2) = x2;
      PO_A(s, 3) = y2 * x1; PO_A(s, 4) = y2 * y1; PO_A(s, 5) = y2;
      PO_A(s, 6) = x1;      PO_A(s, 7) = y1;      PO_A(s, 8) = 1.0f;
    }
    unsigned long long perm = 0x876543210ull;
    float first = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 8 && ok; ++k) {
      float best = -1.0f;
      int br = k, bc = k;
      for (int r = k; r < 8; ++r)
        for (int c = k; c < 9; ++c) {
          const float m = fabsf(PO_A(r, po_col(perm, c)));
          if (m > best) { best = m; br = r; bc = c; }               // strict: the first maximum in (row, column) order
        }
      if (k == 0) first = best;
      if (!(best > PO_RANK_TOL * first)) { ok = false; break; }
      if (br != k)
        for (int c = 0; c < 9; ++c) { const float t = PO_A(k, c); PO_A(k, c) = PO_A(br, c); PO_A(br, c) = t; }
      {
        const unsigned long long ck = (perm >> (4 * k)) & 15ull, cb = (perm >> (4 * bc)) & 15ull;
        perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * bc)))) | (cb << (4 * k));
        if (bc != k) perm |= ck << (4 * bc);
      }
      const int pk = po_col(perm, k);
      const float piv = PO_A(k, pk);
      for (int c = k + 1; c < 9; ++c) { const int cc = po_col(perm, c); PO_A(k, cc) = PO_A(k, cc) / piv; }
      for (int r = 0; r < 8; ++r) {
        if (r == k) continue;
        const float f = PO_A(r, pk);
        for (int c = k + 1; c < 9; ++c) { const int cc = po_col(perm, c); PO_A(r, cc) = PO_A(r, cc) - f * PO_A(k, cc); }
      }
    }
    if (ok) {
      const int fc = po_col(perm, 8);
      PO_A(8, fc) = 1.0f;
      for (int k = 0; k < 8; ++k) PO_A(8, po_col(perm, k)) = -PO_A(k, fc);
      float v[9], nn = 0.0f;
#pragma unroll
      for (int c = 0; c < 9; ++c) { v[c] = PO_A(8, c); nn += v[c] * v[c]; }
      nn = sqrtf(nn);
#pragma unroll
      for (int c = 0; c < 9; ++c) v[c] = v[c] / nn;
      ok = po_finish_e(v, h1, h2, e);
    }
  }
#undef PO_A
  return ok;
}

// ---- K15's model (ransac_wave.h) ----------------------------------------------------------------------------------------------
struct PoModel {
  using Row = float4;                         // x1, y1, x2, y2
  static constexpr int MAX_N = PO_MAXN, SAMPLE = 8, MIN_ROWS = 8, FLOATS = 9, STRIDE1 = 2, STRIDE2 = 2;
  struct HypScratch {
    float a[81 * 64];                         // rows 0..7 of the system, row 8: the null vector
  };
  static __device__ __forceinline__ Row load(const float *__restrict__ p1, const float *__restrict__ p2, int i) {
    return make_float4(p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
  }
  static __device__ __forceinline__ float *lane_scratch(HypScratch &x) { return x.a + threadIdx.x; }
  static constexpr auto solve_minimal = po_solve_minimal;      // called as it stands: a wrapper changes K15a's code
  static __host__ __device__ __forceinline__ float dist2(const float *e, Row q) { return po_sampson(e, q); }
};
using PoStage = RwStage<PoModel>;
using PoPairShared = RwPairShared<PoModel>;

// ---- wave-wide pieces of K15b / K15c ----------------------------------------------------------------------------------------
// MSAC cost and inlier count of E over the staged correspondences, lanes striding, fixed reduction order
__device__ __forceinline__ void po_score_wave(const float *e, const PoStage &S, int nv, float thr2, float &cost, int &count) {
  const int lane = threadIdx.x & 63;
  float c = 0.0f;
  int k = 0;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const float d2 = i < nv ? po_sampson(e, S.p[i]) : INFINITY;
    k += wave_count(i < nv && d2 <= thr2);
    c += i < nv ? fminf(d2, thr2) : 0.0f;
  }
  cost = wave_sum_dpp(c);
  count = k;
}

// E from the staged correspondences with sel[i] != 0 (sel == nullptr: all of them): Hartley-normalised normal equations,
// minimum eigenvector, denormalisation, projection.  Every lane returns the same E; false: fewer than 8 rows or no
// finite result.
__device__ bool po_refit_wave(const PoStage &S, int nv, const uint8_t *sel, float *e_out) {
  const int lane = threadIdx.x & 63;
  int m = 0;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    const bool on = i < nv && (sel ? sel[i] != 0 : true);
    m += wave_count(on);
    if (on) { const float4 q = S.p[i]; s[0] += q.x; s[1] += q.y; s[2] += q.z; s[3] += q.w; }
  }
  if (m < 8) return false;
  wave_sum4(s);
  float h1[3], h2[3];
  h1[0] = s[0] / (float)m; h1[1] = s[1] / (float)m; h2[0] = s[2] / (float)m; h2[1] = s[3] / (float)m;
  float d1 = 0.0f, d2 = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv && (sel ? sel[i] != 0 : true)) {
      const float4 q = S.p[i];
      const float ax = q.x - h1[0], ay = q.y - h1[1], bx = q.z - h2[0], by = q.w - h2[1];
      d1 += ax * ax + ay * ay;
      d2 += bx * bx + by * by;
    }
  }
  d1 = wave_sum_dpp(d1);
  d2 = wave_sum_dpp(d2);
  if (!(d1 > 0.0f && d2 > 0.0f)) return false;
  h1[2] = sqrtf(2.0f) / sqrtf(d1 / (float)m);
  h2[2] = sqrtf(2.0f) / sqrtf(d2 / (float)m);
  // upper triangle of A^T A, entry (r, c >= r) at r * 9 - r * (r - 1) / 2 + (c - r)
  float acc[45];
#pragma unroll
  for (int k = 0; k < 45; ++k) acc[k] = 0.0f;
  for (int i0 = 0; i0 < nv; i0 += 64) {
    const int i = i0 + lane;
    if (i < nv && (sel ? sel[i] != 0 : true)) {
      const float4 q = S.p[i];
      const float x1 = (q.x - h1[0]) * h1[2], y1 = (q.y - h1[1]) * h1[2], x2 = (q.z - h2[0]) * h2[2], y2 = (q.w - h2[1]) * h2[2];
      const float a[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0f};
      int k = 0;
#pragma unroll
      for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = r; c < 9; ++c) acc[k++] += a[r] * a[c];
    }
  }
  float mm[9][9];
  {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c) {
        const float t = wave_sum_dpp(acc[k++]);
        mm[r][c] = t;
        mm[c][r] = t;
      }
  }
  // the eigenvector of M's smallest eigenvalue: shifted inverse iteration (essential_math.h, shared with K24's refit)
  float v[9];
  em_min_eigenvector9(mm, v);
  return po_finish_e(v, h1, h2, e_out);
}

// ---- K15b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void po_ransac_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                       const uint8_t *__restrict__ valid, int n, int num_hyp, float thr,
                                                       int rounds, const float *__restrict__ e_h,
                                                       const float *__restrict__ cost_h, float *__restrict__ e_out,
                                                       uint8_t *__restrict__ inlier, int *__restrict__ best_h_out,
                                                       int *__restrict__ count_out) {
  __shared__ PoPairShared S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S.st, pts1 + (size_t)b * n * 2, pts2 + (size_t)b * n * 2, valid ? valid + (size_t)b * n : nullptr, n);
  float e[9];
  int bh;
  const bool usable = rw_best_hypothesis<PoModel>(e_h, cost_h, b, num_hyp, e, bh);
  const float thr2 = thr * thr;
  if (usable && rounds > 0) {
    float cur;
    int cnt;
    po_score_wave(e, S.st, nv, thr2, cur, cnt);                       // the hypothesis' cost in THIS kernel's summation order
    for (int r = 0; r < rounds; ++r) {
      const float kr = 1.0f + 0.5f * (float)(rounds - 1 - r);
      rw_flag_inliers(S, nv, e, (kr * thr) * (kr * thr), true);
      float e2[9], c2;
      int k2;
      const bool ok = po_refit_wave(S.st, nv, S.sel, e2);
      __syncthreads();
      if (!ok) continue;
      po_score_wave(e2, S.st, nv, thr2, c2, k2);
      if (c2 < cur) {
        cur = c2;
#pragma unroll
        for (int c = 0; c < 9; ++c) e[c] = e2[c];
      }
    }
  }
  rw_flag_inliers(S, nv, e, thr2, usable);
  int cnt = 0;
  for (int i0 = 0; i0 < nv; i0 += 64) cnt += wave_count(i0 + lane < nv && S.sel[i0 + lane] != 0);
  rw_write_mask(S, nv, n, inlier + (size_t)b * n);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 9; ++c) e_out[(size_t)b * 9 + c] = e[c];
    best_h_out[b] = bh;
    count_out[b] = cnt;
  }
}

// ---- K15c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void po_refit_kernel(const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                      const uint8_t *__restrict__ mask, int n, float *__restrict__ e_out,
                                                      uint8_t *__restrict__ ok_out) {
  __shared__ PoStage S;
  const int b = blockIdx.x;
  const int nv = rw_stage(S, pts1 + (size_t)b * n * 2, pts2 + (size_t)b * n * 2, mask + (size_t)b * n, n);
  float e[9];
  const bool ok = po_refit_wave(S, nv, nullptr, e);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 9; ++c) e_out[(size_t)b * 9 + c] = ok ? e[c] : 0.0f;
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K15d ------------------------------------------------------------------------------------------------------------------
// depths of one correspondence under x2 ~ R x1 + t: z1 minimises |x2 x (z1 R x1 + t)|, z2 = (z1 R x1 + t).z
__host__ __device__ __forceinline__ bool po_in_front(const float (*rm)[3], const float *t, float4 q, float dist) {
  const float x1[3] = {q.x, q.y, 1.0f}, x2[3] = {q.z, q.w, 1.0f};
  float rx[3], a[3], c[3];
  matvec3(rm, x1, rx);
  cross3(x2, rx, a);
  cross3(x2, t, c);
  const float den = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
  const float z1 = -((a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]) / den;
  const float z2 = z1 * rx[2] + t[2];
  return den > 0.0f && z1 > 0.0f && z2 > 0.0f && z1 < dist && z2 < dist;
}

// t and the two rotations of one essential matrix (header: mi_recover_pose); false for a zero or non-finite matrix
__host__ __device__ inline bool po_decompose(const float *e_in, float *t, float (*rot)[3][3]) {
  float e[3][3], fro = 0.0f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) { e[r][c] = e_in[r * 3 + c]; fro += e[r][c] * e[r][c]; }
  const bool usable = fro > 0.0f && fro < INFINITY;                   // false for NaN
  const float sc = sqrtf(2.0f) / sqrtf(fro);                          // |E|_F = sqrt(2)  <=>  |t| = 1
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) e[r][c] = usable ? e[r][c] * sc : 0.0f;
  // t: the left null vector, from the largest cross product of two columns (the first on ties)
  t[0] = t[1] = t[2] = 0.0f;
  {
    const float c0[3] = {e[0][0], e[1][0], e[2][0]}, c1[3] = {e[0][1], e[1][1], e[2][1]}, c2[3] = {e[0][2], e[1][2], e[2][2]};
    float x[3][3];
    cross3(c0, c1, x[0]);
    cross3(c0, c2, x[1]);
    cross3(c1, c2, x[2]);
    float best = -1.0f;
    for (int k = 0; k < 3; ++k) {
      const float nn = (x[k][0] * x[k][0] + x[k][1] * x[k][1]) + x[k][2] * x[k][2];
      if (nn > best) { best = nn; t[0] = x[k][0]; t[1] = x[k][1]; t[2] = x[k][2]; }
    }
    const float nn = sqrtf(best);
    for (int k = 0; k < 3; ++k) t[k] = nn > 0.0f ? t[k] / nn : 0.0f;
  }
  // the two rotations: cof(E) - [t]x E and cof(E) + [t]x E, each followed by one Newton step towards the nearest
  // orthogonal matrix, R (3 I - R^T R) / 2 (E is on the manifold only to rounding)
  {
    float cof[3][3], te[3][3];
    cross3(e[1], e[2], cof[0]);
    cross3(e[2], e[0], cof[1]);
    cross3(e[0], e[1], cof[2]);
    for (int c = 0; c < 3; ++c) {
      const float col[3] = {e[0][c], e[1][c], e[2][c]};
      float x[3];
      cross3(t, col, x);
      te[0][c] = x[0]; te[1][c] = x[1]; te[2][c] = x[2];
    }
    for (int w = 0; w < 2; ++w) {
      float r0[3][3], g[3][3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) r0[r][c] = w ? cof[r][c] + te[r][c] : cof[r][c] - te[r][c];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
          g[r][c] = (r == c ? 3.0f : 0.0f) - ((r0[0][r] * r0[0][c] + r0[1][r] * r0[1][c]) + r0[2][r] * r0[2][c]);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) rot[w][r][c] = 0.5f * ((r0[r][0] * g[0][c] + r0[r][1] * g[1][c]) + r0[r][2] * g[2][c]);
    }
  }
  return usable;
}

__global__ __launch_bounds__(64) void po_pose_kernel(const float *__restrict__ e_in, const float *__restrict__ pts1,
                                                     const float *__restrict__ pts2, const uint8_t *__restrict__ mask, int n,
                                                     float dist, float *__restrict__ r_out, float *__restrict__ t_out,
                                                     uint8_t *__restrict__ pose_mask, int *__restrict__ count_out,
                                                     uint8_t *__restrict__ ok_out) {
  __shared__ PoPairShared S;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = rw_stage(S.st, pts1 + (size_t)b * n * 2, pts2 + (size_t)b * n * 2, mask ? mask + (size_t)b * n : nullptr, n);
  float t[3], rot[2][3][3];
  const bool usable = po_decompose(e_in + (size_t)b * 9, t, rot);   // wave-uniform
  // candidates 0: (Ra, +t)  1: (Rb, +t)  2: (Ra, -t)  3: (Rb, -t); most points in front of both cameras, the first on ties
  int best_cnt = -1, best_k = 0;
  for (int k = 0; k < 4; ++k) {
    const float sg = k < 2 ? 1.0f : -1.0f;
    const float tk[3] = {sg * t[0], sg * t[1], sg * t[2]};
    int cnt = 0;
    for (int i0 = 0; i0 < nv; i0 += 64) {
      const int i = i0 + lane;
      cnt += wave_count(usable && i < nv && po_in_front(rot[k & 1], tk, S.st.p[min(i, PO_MAXN - 1)], dist));
    }
    if (cnt > best_cnt) { best_cnt = cnt; best_k = k; }
  }
  const float sg = best_k < 2 ? 1.0f : -1.0f;
  const float tk[3] = {sg * t[0], sg * t[1], sg * t[2]};
  float rk[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) rk[r][c] = (best_k & 1) ? rot[1][r][c] : rot[0][r][c];
  for (int i = lane; i < nv; i += 64) S.sel[i] = (usable && po_in_front(rk, tk, S.st.p[i], dist)) ? 1 : 0;
  __syncthreads();
  rw_write_mask(S, nv, n, pose_mask + (size_t)b * n);
  if (lane == 0) {
    const bool ok = best_cnt >= 5;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) r_out[(size_t)b * 9 + r * 3 + c] = ok ? rk[r][c] : (r == c ? 1.0f : 0.0f);
      t_out[(size_t)b * 3 + r] = ok ? tk[r] : 0.0f;
    }
    count_out[b] = best_cnt;
    ok_out[b] = ok ? 1 : 0;
  }
}

// ---- K15e ------------------------------------------------------------------------------------------------------------------
// one point of mi_triangulate: X / w into out[3] (zeros when not finite); returns the finite flag
__host__ __device__ inline bool po_triangulate_point(const float *p1, const float *p2, float x1, float y1, float x2, float y2,
                                                     float *out) {
  float a[4][4], v[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    a[0][c] = x1 * p1[8 + c] - p1[c];
    a[1][c] = y1 * p1[8 + c] - p1[4 + c];
    a[2][c] = x2 * p2[8 + c] - p2[c];
    a[3][c] = y2 * p2[8 + c] - p2[4 + c];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float nn = sqrtf(((a[r][0] * a[r][0] + a[r][1] * a[r][1]) + a[r][2] * a[r][2]) + a[r][3] * a[r][3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a[r][c] = nn > 0.0f ? a[r][c] / nn : 0.0f;
      v[r][c] = r == c ? 1.0f : 0.0f;
    }
  }
  // one-sided Jacobi: rotate column pairs of A (and of V) until the columns are orthogonal; A = U S V^T then has
  // S_c = |column c| and the right singular vectors in the columns of V
  for (int sweep = 0; sweep < PO_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        float al = 0.0f, be = 0.0f, ga = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { al += a[r][p] * a[r][p]; be += a[r][q] * a[r][q]; ga += a[r][p] * a[r][q]; }
        if (fabsf(ga) > 1e-12f * sqrtf(al * be)) {
          const float zeta = (be - al) / (2.0f * ga);
          const float tt = (zeta >= 0.0f ? 1.0f : -1.0f) / (fabsf(zeta) + sqrtf(1.0f + zeta * zeta));
          const float cs = 1.0f / sqrtf(1.0f + tt * tt), sn = cs * tt;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float ap = a[r][p], aq = a[r][q], vp = v[r][p], vq = v[r][q];
            a[r][p] = cs * ap - sn * aq;
            a[r][q] = sn * ap + cs * aq;
            v[r][p] = cs * vp - sn * vq;
            v[r][q] = sn * vp + cs * vq;
          }
        }
      }
  }
  // the smallest, second smallest and largest squared singular value; a system of rank < 3 (the second smallest not above
  // 1e-5 times the largest: identical rays under identical cameras) has no unique solution
  float best = INFINITY, second = INFINITY, largest = 0.0f, x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float nn = ((a[0][c] * a[0][c] + a[1][c] * a[1][c]) + a[2][c] * a[2][c]) + a[3][c] * a[3][c];
    largest = fmaxf(largest, nn);
    if (nn < best) {
      second = best;
      best = nn;
      x[0] = v[0][c]; x[1] = v[1][c]; x[2] = v[2][c]; x[3] = v[3][c];
    } else if (nn < second) {
      second = nn;
    }
  }
  const float w = x[3];
  const bool ok = second > 1e-10f * largest && fabsf(w) > 1e-9f && fabsf(x[0] / w) < INFINITY && fabsf(x[1] / w) < INFINITY &&
                  fabsf(x[2] / w) < INFINITY;
  out[0] = ok ? x[0] / w : 0.0f;
  out[1] = ok ? x[1] / w : 0.0f;
  out[2] = ok ? x[2] / w : 0.0f;
  return ok;
}

__global__ __launch_bounds__(256) void po_triangulate_kernel(const float *__restrict__ proj1, const float *__restrict__ proj2,
                                                             const float *__restrict__ pts1, const float *__restrict__ pts2,
                                                             int n, long long total, float *__restrict__ out,
                                                             uint8_t *__restrict__ finite) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const long long b = gid / n;
  const float *p1 = proj1 + b * 12, *p2 = proj2 + b * 12;
  const float x1 = pts1[2 * gid], y1 = pts1[2 * gid + 1], x2 = pts2[2 * gid], y2 = pts2[2 * gid + 1];
  float x[3];
  const bool ok = po_triangulate_point(p1, p2, x1, y1, x2, y2, x);
  out[3 * gid + 0] = x[0];
  out[3 * gid + 1] = x[1];
  out[3 * gid + 2] = x[2];
  finite[gid] = ok ? 1 : 0;
}

int po_shape_status(int batch, int n) { return rw_shape_status(batch, n, PO_MAXN); }

}  // namespace

extern "C" int mi_essential_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                       int num_hypotheses, float threshold, uint32_t seed, float *e_h, float *cost,
                                       int32_t *count, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !e_h || !cost || !count) return MI_E_NULL;
  if (const int s = rw_hyp_params(batch, n, PO_MAXN, num_hypotheses, threshold)) return s;
  return rw_launch_hyp<PoModel>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, e_h, cost, count,
                                (hipStream_t)stream);
}

extern "C" int mi_essential_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *e,
                                  uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !mask || !e || !ok) return MI_E_NULL;
  if (const int s = po_shape_status(batch, n)) return s;
  hipLaunchKernelGGL(po_refit_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, pts1, pts2, mask, n, e, ok);
  return mi_launch_status();
}

extern "C" size_t mi_essential_ransac_workspace_bytes(int batch, int n, int num_hypotheses) {
  return rw_workspace_bytes(batch, n, PO_MAXN, num_hypotheses, 9);
}

extern "C" int mi_essential_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                   int num_hypotheses, float threshold, int refine_rounds, uint32_t seed, float *e,
                                   uint8_t *inlier, int32_t *best_h, int32_t *count, void *workspace,
                                   size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!pts1 || !pts2 || !e || !inlier || !best_h || !count || !workspace) return MI_E_NULL;
  if (const int s = rw_ransac_params(batch, n, PO_MAXN, num_hypotheses, threshold, refine_rounds, 9, workspace, workspace_bytes))
    return s;
  const RwWork w = rw_carve(workspace, batch, num_hypotheses, 9);
  hipStream_t s = (hipStream_t)stream;
  if (const int st = rw_launch_hyp<PoModel>(pts1, pts2, valid, batch, n, num_hypotheses, threshold, seed, w.model_h,
                                            w.cost, w.count, s))
    return st;
  hipLaunchKernelGGL(po_ransac_kernel, dim3((unsigned)batch), dim3(64), 0, s, pts1, pts2, valid, n, num_hypotheses, threshold,
                     refine_rounds, w.model_h, w.cost, e, inlier, best_h, count);
  return mi_launch_status();
}

extern "C" int mi_recover_pose(const float *e, const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n,
                               float distance_threshold, float *r, float *t, uint8_t *pose_mask, int32_t *count,
                               uint8_t *ok, mi_stream_t stream) {
  MI_ENTER();
  if (!e || !pts1 || !pts2 || !r || !t || !pose_mask || !count || !ok) return MI_E_NULL;
  if (const int s = po_shape_status(batch, n)) return s;
  if (!(distance_threshold > 0.0f)) return MI_E_PARAM;
  hipLaunchKernelGGL(po_pose_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, e, pts1, pts2, mask, n,
                     distance_threshold, r, t, pose_mask, count, ok);
  return mi_launch_status();
}

extern "C" int mi_triangulate(const float *proj1, const float *proj2, const float *pts1, const float *pts2, int batch, int n,
                              float *points, uint8_t *finite, mi_stream_t stream) {
  MI_ENTER();
  if (!proj1 || !proj2 || !pts1 || !pts2 || !points || !finite) return MI_E_NULL;
  if (batch < 1 || n < 1) return MI_E_SHAPE;
  const long long total = (long long)batch * n;
  if (total > 0x7fffffffLL * 256LL) return MI_E_SHAPE;
  hipLaunchKernelGGL(po_triangulate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, proj1,
                     proj2, pts1, pts2, n, total, points, finite);
  return mi_launch_status();
}
