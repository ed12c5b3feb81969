// The arithmetic of K23 (pnp.hip; include/mi355x_match.h, "absolute pose"): the P3P minimal solver (a Lambda-twist
// structure: one real root of a cubic by Newton, the eigen-decomposition of a singular symmetric 3x3 form by rg_jacobi<3>,
// two quadratics, a Gauss-Newton polish of the three depths, rotation and translation by Horn's rg_solve_minimal), the
// reprojection score and one row's two lines of the reprojection Gauss-Newton system.  float32 throughout (but for what
// rigid_math.h does in float64); only + - * / and sqrtf, fixed iteration counts: the host and the device return the same
// bits (tests/native/pnp_host.cpp runs it without a GPU).  Needs nothing of HIP but the __host__ __device__ markers of
// rigid_math.h, which it includes.
#pragma once
#include "rigid_math.h"

#include <math.h>

namespace {

// Newton steps on the monic cubic.  The start lies beyond a stationary point on the side of the root, so the iteration is
// monotone; it is quadratic near the root, but where the two stationary points nearly coincide the start lies far out and
// every step only takes a third off.  Measured on the CPU with the float32 restatement (tests/pnp_oracle.py) on 10 x 64
// planted samples (1262 candidates): candidates further than 1e-3 m from the float64 oracle's: 28 after 8 steps, 18
// after 12, 14 after 16, 13 after 24, 12 to 13 after 32, 48 and 64 (what is left is float32 conditioning, not the root).
constexpr int PNP_CUBIC_NEWTON = 24;
// Gauss-Newton steps on the three law-of-cosines equations, per candidate.  Measured the same way on the same samples, as
// the largest depth difference between a float32 candidate and the float64 oracle's (metres; depths 3 to 9 m).  The
// median is 5.3e-6 whatever the count: the float32 floor, at which a step moves the median candidate by 4.8e-6 (step 1:
// by 1.6e-5).  The ill-conditioned tail sets the count: the 99th percentile is 3.9e-3 after one step, 1.0e-3 after two,
// 8.2e-4 after three, 5.7e-4 after four.  The count is the smallest k after which two more steps take less off that
// percentile than they leave of it, d99(k) - d99(k + 2) <= d99(k + 2): two (tests/test_pnp_host.py re-measures it).
constexpr int PNP_POLISH = 2;
// Gauss-Newton iterations of the reprojection refit.  Measured with the float64 oracle on the 15 refit cases of
// tests/test_gpu_pnp.py (n = 64, 97 and 4, with and without 0.5 px of noise, the start 2 deg and 6 cm off the truth),
// against 20 iterations: 1 iteration leaves 6.3e-2 deg and 4.4e-3 m, 2 leave 3.3e-5 deg and 3.4e-6 m, 3 leave 5.0e-8 deg
// and 5.0e-9 m, 4 leave 7.6e-11 deg.  The refit tolerance of that test (the float32 oracle's deviation with its margins) is
// 3.8e-5 deg and 8.1e-6 m: 2 iterations are inside it by a hair for this start, and would not be for a start further
// off; 3 are inside a hundredth of it.  Three iterations.
constexpr int PNP_GN_ITERS = 3;

// one staged correspondence: the model point and the normalised image point (20 bytes)
struct alignas(4) PnpRow {
  float X[3], u, v;
};

// what the (up to) four candidates of one sample share
struct PnpSetup {
  float f[3][3];                         // unit bearings
  float c12, c13, c23, a12, a13, a23;    // cosines between bearings, squared distances between model points
  float np[3], nq[3];                    // sqrt(sigma_p) e_p and sqrt(-sigma_q) e_q of the singular form D0
};

// cofactors of the symmetric m = (m00 m01 m02 m11 m12 m22), same order
__host__ __device__ __forceinline__ void pnp_cof(const float *m, float *c) {
  c[0] = m[3] * m[5] - m[4] * m[4];
  c[1] = m[2] * m[4] - m[1] * m[5];
  c[2] = m[1] * m[4] - m[2] * m[3];
  c[3] = m[0] * m[5] - m[2] * m[2];
  c[4] = m[1] * m[2] - m[0] * m[4];
  c[5] = m[0] * m[3] - m[1] * m[1];
}
// sum over i, j of c_ij b_ij for symmetric c, b
__host__ __device__ __forceinline__ float pnp_sdot(const float *c, const float *b) {
  return ((c[0] * b[0] + c[3] * b[3]) + c[5] * b[5]) + 2.0f * ((c[1] * b[1] + c[2] * b[2]) + c[4] * b[4]);
}

// (header: "Solve", steps 1-4).  q: the three rows of the minimal sample.  False: a degenerate sample, no real
// factorisation of D0, or a non-finite value on the way.
__host__ __device__ inline bool pnp_setup(const PnpRow *q, PnpSetup &S) {
  if (rg_degenerate3(q[0].X, q[1].X, q[2].X)) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float nn = sqrtf((q[k].u * q[k].u + q[k].v * q[k].v) + 1.0f);
    S.f[k][0] = q[k].u / nn;
    S.f[k][1] = q[k].v / nn;
    S.f[k][2] = 1.0f / nn;
  }
  if (rg_degenerate3(S.f[0], S.f[1], S.f[2])) return false;
  S.c12 = (S.f[0][0] * S.f[1][0] + S.f[0][1] * S.f[1][1]) + S.f[0][2] * S.f[1][2];
  S.c13 = (S.f[0][0] * S.f[2][0] + S.f[0][1] * S.f[2][1]) + S.f[0][2] * S.f[2][2];
  S.c23 = (S.f[1][0] * S.f[2][0] + S.f[1][1] * S.f[2][1]) + S.f[1][2] * S.f[2][2];
  {
    const float d0 = q[0].X[0] - q[1].X[0], d1 = q[0].X[1] - q[1].X[1], d2 = q[0].X[2] - q[1].X[2];
    S.a12 = (d0 * d0 + d1 * d1) + d2 * d2;
  }
  {
    const float d0 = q[0].X[0] - q[2].X[0], d1 = q[0].X[1] - q[2].X[1], d2 = q[0].X[2] - q[2].X[2];
    S.a13 = (d0 * d0 + d1 * d1) + d2 * d2;
  }
  {
    const float d0 = q[1].X[0] - q[2].X[0], d1 = q[1].X[1] - q[2].X[1], d2 = q[1].X[2] - q[2].X[2];
    S.a23 = (d0 * d0 + d1 * d1) + d2 * d2;
  }
  // D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23 (M_ij: the form of l_i^2 + l_j^2 - 2 c_ij l_i l_j)
  const float d1[6] = {S.a23, -(S.a23 * S.c12), 0.0f, S.a23 - S.a12, S.a12 * S.c23, -S.a12};
  const float d2[6] = {S.a23, 0.0f, -(S.a23 * S.c13), -S.a13, S.a13 * S.c23, S.a23 - S.a13};
  float k1[6], k2[6];
  pnp_cof(d1, k1);
  pnp_cof(d2, k2);
  const float c0 = (d1[0] * k1[0] + d1[1] * k1[1]) + d1[2] * k1[2];         // det D1
  const float c3 = (d2[0] * k2[0] + d2[1] * k2[1]) + d2[2] * k2[2];         // det D2
  const float c1 = pnp_sdot(k1, d2), c2 = pnp_sdot(k2, d1);
  const float b = c2 / c3, c = c1 / c3, d = c0 / c3;                        // g^3 + b g^2 + c g + d = det(D1 + g D2) / det D2
  float g;
  const float bb = b * b - 3.0f * c;
  if (bb >= 0.0f) {                                                         // two stationary points t1 <= t2
    const float v = sqrtf(bb);
    const float t1 = (-b - v) / 3.0f;
    const float f1 = ((t1 + b) * t1 + c) * t1 + d;
    if (f1 > 0.0f) {
      g = t1 - sqrtf(-f1 / (3.0f * t1 + b));
    } else {
      const float t2 = (-b + v) / 3.0f;
      const float f2 = ((t2 + b) * t2 + c) * t2 + d;
      g = t2 + sqrtf(-f2 / (3.0f * t2 + b));
    }
  } else {
    g = -b / 3.0f;
  }
#pragma unroll 1
  for (int it = 0; it < PNP_CUBIC_NEWTON; ++it) {
    const float fv = ((g + b) * g + c) * g + d, fp = (3.0f * g + 2.0f * b) * g + c;
    if (fp != 0.0f) g = g - fv / fp;
  }
  float a[3][3], e[3][3];
  a[0][0] = d1[0] + g * d2[0];
  a[0][1] = d1[1] + g * d2[1];
  a[0][2] = d1[2] + g * d2[2];
  a[1][1] = d1[3] + g * d2[3];
  a[1][2] = d1[4] + g * d2[4];
  a[2][2] = d1[5] + g * d2[5];
  a[1][0] = a[0][1];
  a[2][0] = a[0][2];
  a[2][1] = a[1][2];
  rg_jacobi<3>(a, e);
  const float l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
  int iz = 0;                                                               // the eigenvalue nearest 0, the first among equals
  float lo = fabsf(l0);
  if (fabsf(l1) < lo) { iz = 1; lo = fabsf(l1); }
  if (fabsf(l2) < lo) { iz = 2; }
  float lp = iz == 0 ? l1 : l0, lq = iz == 2 ? l1 : l2;
  float ep[3], eq[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ep[k] = iz == 0 ? e[k][1] : e[k][0];
    eq[k] = iz == 2 ? e[k][1] : e[k][2];
  }
  if (!(lp * lq < 0.0f)) return false;                                      // also NaN
  const bool swap = lp < 0.0f;
  const float sp = sqrtf(swap ? lq : lp), sq = sqrtf(swap ? -lp : -lq);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    S.np[k] = sp * (swap ? eq[k] : ep[k]);
    S.nq[k] = sq * (swap ? ep[k] : eq[k]);
  }
  return true;
}

// Candidate c = 0 .. 3 (header: "Solve", steps 5-8): plane np + nq for c < 2 and np - nq for c >= 2, root c & 1 of the
// quadratic.  l: the three depths after the polish; rt = (R row-major, t).  False: no such candidate.
__host__ __device__ inline bool pnp_candidate(const PnpRow *q, const PnpSetup &S, int c, float *l, float *rt) {
  const float sg = (c & 2) ? -1.0f : 1.0f;
  const float n0 = S.np[0] + sg * S.nq[0], n1 = S.np[1] + sg * S.nq[1], n2 = S.np[2] + sg * S.nq[2];
  const float w0 = -n1 / n0, w1 = -n2 / n0;                                 // l1 = w0 l2 + w1 l3
  const float qa = ((S.a13 - S.a12) * w1 * w1 + 2.0f * S.a12 * S.c13 * w1) - S.a12;
  const float qb = (2.0f * S.a12 * S.c13 * w0 - 2.0f * S.a13 * S.c12 * w1) - 2.0f * w0 * w1 * (S.a12 - S.a13);
  const float qc = ((S.a13 - S.a12) * w0 * w0 - 2.0f * S.a13 * S.c12 * w0) + S.a13;
  const float disc = qb * qb - 4.0f * qa * qc;
  if (!(disc >= 0.0f)) return false;
  const float sd = sqrtf(disc);
  const float qq = -0.5f * (qb + (qb >= 0.0f ? sd : -sd));
  const float tau = (c & 1) ? qc / qq : qq / qa;                            // l3 / l2
  if (!(tau > 0.0f)) return false;
  float l2 = sqrtf(S.a23 / (tau * (tau - 2.0f * S.c23) + 1.0f));
  float l3 = tau * l2;
  float l1 = w0 * l2 + w1 * l3;
  if (!(l1 > 0.0f && l2 > 0.0f && l3 > 0.0f) || !(l1 < INFINITY && l2 < INFINITY && l3 < INFINITY)) return false;
#pragma unroll 1
  for (int it = 0; it < PNP_POLISH; ++it) {
    const float r0 = ((l1 * l1 + l2 * l2) - 2.0f * S.c12 * l1 * l2) - S.a12;
    const float r1 = ((l1 * l1 + l3 * l3) - 2.0f * S.c13 * l1 * l3) - S.a13;
    const float r2 = ((l2 * l2 + l3 * l3) - 2.0f * S.c23 * l2 * l3) - S.a23;
    const float j00 = 2.0f * (l1 - S.c12 * l2), j01 = 2.0f * (l2 - S.c12 * l1);
    const float j10 = 2.0f * (l1 - S.c13 * l3), j12 = 2.0f * (l3 - S.c13 * l1);
    const float j21 = 2.0f * (l2 - S.c23 * l3), j22 = 2.0f * (l3 - S.c23 * l2);
    const float det = -(j00 * j12 * j21) - j01 * j10 * j22;
    if (det != 0.0f) {
      l1 = l1 - ((-(j12 * j21) * r0 - j01 * j22 * r1) + j01 * j12 * r2) / det;
      l2 = l2 - ((-(j10 * j22) * r0 + j00 * j22 * r1) - j00 * j12 * r2) / det;
      l3 = l3 - ((j10 * j21 * r0 - j00 * j21 * r1) - j01 * j10 * r2) / det;
    }
  }
  if (!(l1 > 0.0f && l2 > 0.0f && l3 > 0.0f) || !(l1 < INFINITY && l2 < INFINITY && l3 < INFINITY)) return false;
  l[0] = l1;
  l[1] = l2;
  l[2] = l3;
  RgRow p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      p[k].a[j] = q[k].X[j];
      p[k].b[j] = l[k] * S.f[k][j];
    }
  return rg_solve_minimal(p, rt);
}

// squared reprojection distance of one row under (R, t) (header: "Score"); +inf for z <= 0 or a non-finite value
__host__ __device__ __forceinline__ float pnp_dist2(const float *rt, const PnpRow &q) {
  const float x = ((rt[0] * q.X[0] + rt[1] * q.X[1]) + rt[2] * q.X[2]) + rt[9];
  const float y = ((rt[3] * q.X[0] + rt[4] * q.X[1]) + rt[5] * q.X[2]) + rt[10];
  const float z = ((rt[6] * q.X[0] + rt[7] * q.X[1]) + rt[8] * q.X[2]) + rt[11];
  const float du = x / z - q.u, dv = y / z - q.v;
  const float d2 = du * du + dv * dv;
  return (z > 0.0f && d2 < INFINITY) ? d2 : INFINITY;
}

// (R, t) from a 4-sample: rows 0 .. 2 solve, row 3 picks the candidate (the smallest pnp_dist2, the first among equals).
// False: no candidate.
__host__ __device__ inline bool pnp_solve_minimal(const PnpRow *q, float *rt) {
  PnpSetup S;
  if (!pnp_setup(q, S)) return false;
  bool found = false;
  float best = INFINITY;
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {
    float l[3], cand[12];
    if (!pnp_candidate(q, S, c, l, cand)) continue;
    const float d2 = pnp_dist2(cand, q[3]);
    if (!found || d2 < best) {
      found = true;
      best = d2;
#pragma unroll
      for (int k = 0; k < 12; ++k) rt[k] = cand[k];
    }
  }
  return found;
}

// one row's two lines of the reprojection system under the left perturbation (omega, tau) (header: "Refit"); false (and
// zeros) for z <= 0
__host__ __device__ __forceinline__ bool pnp_lines(const float *rt, const PnpRow &q, float *ju, float *jv, float *ru, float *rv) {
  const float x = ((rt[0] * q.X[0] + rt[1] * q.X[1]) + rt[2] * q.X[2]) + rt[9];
  const float y = ((rt[3] * q.X[0] + rt[4] * q.X[1]) + rt[5] * q.X[2]) + rt[10];
  const float z = ((rt[6] * q.X[0] + rt[7] * q.X[1]) + rt[8] * q.X[2]) + rt[11];
  const bool ok = z > 0.0f;
  const float xn = x / z, yn = y / z, iz = 1.0f / z;
  ju[0] = ok ? -(xn * yn) : 0.0f;
  ju[1] = ok ? 1.0f + xn * xn : 0.0f;
  ju[2] = ok ? -yn : 0.0f;
  ju[3] = ok ? iz : 0.0f;
  ju[4] = 0.0f;
  ju[5] = ok ? -(xn * iz) : 0.0f;
  jv[0] = ok ? -(1.0f + yn * yn) : 0.0f;
  jv[1] = ok ? xn * yn : 0.0f;
  jv[2] = ok ? xn : 0.0f;
  jv[3] = 0.0f;
  jv[4] = ok ? iz : 0.0f;
  jv[5] = ok ? -(yn * iz) : 0.0f;
  *ru = ok ? xn - q.u : 0.0f;
  *rv = ok ? yn - q.v : 0.0f;
  return ok;
}

}  // namespace
