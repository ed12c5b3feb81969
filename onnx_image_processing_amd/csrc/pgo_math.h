// The arithmetic of K27 (pgo.hip; include/mi355x_match.h): Log of a rotation, the inverse left
// Jacobian of SO(3), one edge's residual and its two 6x6 lines, the products a linearisation collects from them and the
// solve with a node's factored preconditioner block.  Per-edge work is float32.  Like icp_math.h it needs no HIP header:
// a plain C++ compiler builds everything except pgo_block_factor, which takes ba_math.h's LDL^T and so exists under hipcc
// only.  tests/native/pgo_host.cpp runs it without a GPU against tests/pgo_oracle.py.
#pragma once
#if defined(__HIPCC__)
#include "ba_math.h"      // first: it brings the HIP markers icp_math.h uses under hipcc
#endif
#include "icp_math.h"

#include <math.h>

namespace {

constexpr float PGO_LOG_SMALL = 1e-4f;        // sin(theta) below this (and cos(theta) > 0): theta / sin(theta) = 1 + sin^2 / 6
constexpr float PGO_LOG_NEAR_PI = -0.9f;      // cos(theta) below this: the axis comes from the symmetric part of R
constexpr float PGO_JL_SERIES = 0.0625f;      // theta^2 below this: the coefficient of [phi]x^2 by its series

// phi = Log(R), R row-major.  v = vee(R - R^T) / 2 = sin(theta) a, c = (trace R - 1) / 2 = cos(theta), theta = atan2(|v|, c).
// c >= PGO_LOG_NEAR_PI: phi = (theta / |v|) v, and (1 + |v|^2 / 6) v where |v| < PGO_LOG_SMALL.  Below -- theta above 154
// degrees, where |v| -> 0 loses the axis --: a a^T = (R + R^T - 2 c I) / (2 (1 - c)), so with m the largest diagonal
// element a_m = sqrt((R_mm - c) / (1 - c)), a_n = (R_mn + R_nm) / (2 (1 - c) a_m), the sign that of a . v (+ at v = 0, where
// theta = pi and -phi is the same rotation), phi = theta a.
ICP_HD void pgo_log(const float *R, float *phi) {
  const float v[3] = {0.5f * (R[7] - R[5]), 0.5f * (R[2] - R[6]), 0.5f * (R[3] - R[1])};
  const float s2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], s = sqrtf(s2);
  const float c = 0.5f * (((R[0] + R[4]) + R[8]) - 1.0f);
  const float theta = atan2f(s, c);
  if (c >= PGO_LOG_NEAR_PI || !(c >= -2.0f)) {            // (NaN goes this way and stays NaN)
    const float k = s < PGO_LOG_SMALL ? 1.0f + s2 / 6.0f : theta / s;
    phi[0] = k * v[0]; phi[1] = k * v[1]; phi[2] = k * v[2];
    return;
  }
  const float d = 1.0f - c, s01 = R[1] + R[3], s02 = R[2] + R[6], s12 = R[5] + R[7];
  float a[3];
  if (R[0] >= R[4] && R[0] >= R[8]) {
    const float q = (R[0] - c) / d, am = sqrtf(q > 0.0f ? q : 0.0f), den = (2.0f * d) * am;
    a[0] = am; a[1] = s01 / den; a[2] = s02 / den;
  } else if (R[4] >= R[8]) {
    const float q = (R[4] - c) / d, am = sqrtf(q > 0.0f ? q : 0.0f), den = (2.0f * d) * am;
    a[0] = s01 / den; a[1] = am; a[2] = s12 / den;
  } else {
    const float q = (R[8] - c) / d, am = sqrtf(q > 0.0f ? q : 0.0f), den = (2.0f * d) * am;
    a[0] = s02 / den; a[1] = s12 / den; a[2] = am;
  }
  const float dot = (a[0] * v[0] + a[1] * v[1]) + a[2] * v[2];
  const float sg = dot < 0.0f ? -theta : theta;
  phi[0] = sg * a[0]; phi[1] = sg * a[1]; phi[2] = sg * a[2];
}

// J = J_l^-1(phi) = I - [phi]x / 2 + k [phi]x^2, row-major, with [phi]x^2 = phi phi^T - theta^2 I and
// k = (1 - (theta / 2) cos(theta / 2) / sin(theta / 2)) / theta^2; theta^2 < PGO_JL_SERIES: k = 1/12 + theta^2 / 720 + theta^4 / 30240.
ICP_HD void pgo_jl_inv(const float *phi, float *J) {
  const float th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
  float k;
  if (th2 < PGO_JL_SERIES) {
    k = (1.0f / 12.0f + th2 / 720.0f) + (th2 * th2) / 30240.0f;
  } else {
    const float h = 0.5f * sqrtf(th2);
    k = (1.0f - (h * cosf(h)) / sinf(h)) / th2;
  }
  const float kx[9] = {0.0f, -phi[2], phi[1], phi[2], 0.0f, -phi[0], -phi[1], phi[0], 0.0f};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const float sq = phi[a] * phi[b] - (a == b ? th2 : 0.0f);
      J[a * 3 + b] = ((a == b ? 1.0f : 0.0f) - 0.5f * kx[a * 3 + b]) + k * sq;
    }
}

// one edge at the float32 poses (R_i, t_i), (R_j, t_j) with the measurement (R_z, t_z)
struct PgoEdge {
  float e[6];      // (Log R_d, t_d)
  float rp[9];     // R_p = R_j R_i^T
  float u[3];      // R_d t_z
};

// out = A B^T for row-major 3x3: out_ab = (A_a0 B_b0 + A_a1 B_b1) + A_a2 B_b2
ICP_HD void pgo_mul_abt(const float *A, const float *B, float *out) {
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) out[a * 3 + b] = (A[a * 3] * B[b * 3] + A[a * 3 + 1] * B[b * 3 + 1]) + A[a * 3 + 2] * B[b * 3 + 2];
}

// header "Residual": R_p = R_j R_i^T, t_p = t_j - R_p t_i, R_d = R_p R_z^T, u = R_d t_z, t_d = t_p - u, e = (Log R_d, t_d)
ICP_HD void pgo_residual(const float *ri, const float *ti, const float *rj, const float *tj, const float *rz, const float *tz,
                         PgoEdge &o) {
  float rd[9], w[3];
  pgo_mul_abt(rj, ri, o.rp);
  pgo_mul_abt(o.rp, rz, rd);
  icp_rotate(o.rp, ti, w);
  icp_rotate(rd, tz, o.u);
  pgo_log(rd, o.e);
  for (int a = 0; a < 3; ++a) o.e[3 + a] = (tj[a] - w[a]) - o.u[a];
}

// the symmetric information matrix from the upper triangle of info (6, 6)
ICP_HD void pgo_omega(const float *info, float *O) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) O[r * 6 + c] = r <= c ? info[r * 6 + c] : info[c * 6 + r];
}

// left to right: ((((a0 b0 + a1 b1) + a2 b2) + a3 b3) + a4 b4) + a5 b5 with strides sa, sb
ICP_HD float pgo_dot6(const float *a, int sa, const float *b, int sb) {
  float s = a[0] * b[0];
  for (int k = 1; k < 6; ++k) s = s + a[k * sa] * b[k * sb];
  return s;
}

// oe = Omega e and chi2 = e . oe
ICP_HD float pgo_chi2(const float *O, const float *e, float *oe) {
  for (int r = 0; r < 6; ++r) oe[r] = pgo_dot6(O + r * 6, 1, e, 1);
  return pgo_dot6(e, 1, oe, 1);
}

// K25's Huber term on chi = sqrt(chi2).  false (rho = +inf, w = 0): chi2 is not finite.
ICP_HD bool pgo_rho(float chi2, float huber, float *w, float *rho) {
  *w = 1.0f;
  *rho = chi2;
  if (!(fabsf(chi2) < INFINITY)) { *w = 0.0f; *rho = INFINITY; return false; }
  if (huber > 0.0f) {
    const float chi = sqrtf(chi2);
    if (chi > huber) {
      *w = huber / chi;
      *rho = (2.0f * huber) * chi - huber * huber;
    }
  }
  return true;
}

// the lines (header "Jacobians"), row-major 6x6, of e with respect to the left perturbations of node i and node j:
//   J_j = [[J_l^-1, 0], [-[t_d]x, I]],   J_i = [[-J_l^-1 R_p, 0], [-[u]x R_p, -R_p]]
ICP_HD void pgo_lines(const PgoEdge &o, float *Ji, float *Jj) {
  float jl[9];
  pgo_jl_inv(o.e, jl);
  const float *td = o.e + 3;
  const float tx[9] = {0.0f, -td[2], td[1], td[2], 0.0f, -td[0], -td[1], td[0], 0.0f};
  const float ux[9] = {0.0f, -o.u[2], o.u[1], o.u[2], 0.0f, -o.u[0], -o.u[1], o.u[0], 0.0f};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const float jr = (jl[a * 3] * o.rp[b] + jl[a * 3 + 1] * o.rp[3 + b]) + jl[a * 3 + 2] * o.rp[6 + b];
      const float ur = (ux[a * 3] * o.rp[b] + ux[a * 3 + 1] * o.rp[3 + b]) + ux[a * 3 + 2] * o.rp[6 + b];
      Jj[a * 6 + b] = jl[a * 3 + b];
      Jj[a * 6 + 3 + b] = 0.0f;
      Jj[(3 + a) * 6 + b] = -tx[a * 3 + b];
      Jj[(3 + a) * 6 + 3 + b] = a == b ? 1.0f : 0.0f;
      Ji[a * 6 + b] = -jr;
      Ji[a * 6 + 3 + b] = 0.0f;
      Ji[(3 + a) * 6 + b] = -ur;
      Ji[(3 + a) * 6 + 3 + b] = -o.rp[a * 3 + b];
    }
}

// A = Omega J: A_rc = dot6 over k of Omega_rk J_kc
ICP_HD void pgo_omega_j(const float *O, const float *J, float *A) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) A[r * 6 + c] = pgo_dot6(O + r * 6, 1, J + c, 6);
}

// out = w J^T A: out_rc = w (dot6 over k of J_kr A_kc).  sym: the upper triangle is computed and mirrored.
ICP_HD void pgo_jt_a(const float *J, const float *A, float w, bool sym, float *out) {
  for (int r = 0; r < 6; ++r)
    for (int c = sym ? r : 0; c < 6; ++c) {
      const float v = w * pgo_dot6(J + r, 6, A + c, 6);
      out[r * 6 + c] = v;
      if (sym) out[c * 6 + r] = v;
    }
}

// g = w J^T oe
ICP_HD void pgo_jt_v(const float *J, const float *oe, float w, float *g) {
  for (int r = 0; r < 6; ++r) g[r] = w * pgo_dot6(J + r, 6, oe, 1);
}

// index of (r, c), r <= c, in the packed upper triangle of a 6x6 matrix (ba_tri(6, r, c))
ICP_HD int pgo_tri6(int r, int c) { return r * 6 - (r * (r - 1)) / 2 + (c - r); }

// z = M^-1 r from the factors of M = L D L^T (fac: d_j at (j, j), l_ij at (j, i), packed upper triangle, float32):
// y = r, y_k -= l_ki y_i for i ascending; z_k = y_k / d_k, z_k -= l_ik z_i for i descending
ICP_HD void pgo_ldlt_apply(const float *fac, const float *r, float *z) {
  float y[6];
  for (int i = 0; i < 6; ++i) y[i] = r[i];
  for (int i = 0; i < 6; ++i)
    for (int k = i + 1; k < 6; ++k) y[k] = y[k] - fac[pgo_tri6(i, k)] * y[i];
  for (int i = 0; i < 6; ++i) z[i] = y[i] / fac[pgo_tri6(i, i)];
  for (int i = 5; i >= 0; --i)
    for (int k = 0; k < i; ++k) z[k] = z[k] - fac[pgo_tri6(k, i)] * z[i];
}

#if defined(__HIPCC__)
// fac = the LDL^T factors of M = D + lambda diag D (float64 by ba_ldlt_solve, rounded to float32) for a node's block D
// (6x6 row-major, float32).  false -- the node is FROZEN for this step, fac = 0 --: K18's pivot rule fails, or a factor is
// not finite.  work: 27 doubles of the caller's (the block being factored and ba_ldlt_solve's right-hand side).
ICP_HD bool pgo_block_factor(const float *D, float lambda, float *fac, double *work) {
  double *a = work, *x = work + 21;
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      const double d = (double)D[r * 6 + c];
      a[k++] = r == c ? d + (double)lambda * d : d;
    }
  bool ok = ba_ldlt_solve(a, x, 6, 0, 1, [] {});
  for (k = 0; k < 21; ++k) {
    fac[k] = (float)a[k];
    ok = ok && fabsf(fac[k]) < INFINITY;
  }
  if (!ok)
    for (k = 0; k < 21; ++k) fac[k] = 0.0f;
  return ok;
}
#endif

}  // namespace
