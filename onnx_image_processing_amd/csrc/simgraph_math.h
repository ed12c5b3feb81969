// The arithmetic of K31 (simgraph.hip; include/mi355x_match_simgraph.h): one Sim(3) edge's residual and its two 7x7 lines, the
// products a linearisation collects from them, the solve with a node's factored 7x7 preconditioner block, the update of a
// node's float64 state and the map correction.  K27's pgo_math.h with a scale per node: Log, J_l^-1, the 3x3 product and the
// Huber term are taken from it as they are.  Per-edge work is float32.  A plain C++ compiler builds everything except
// sg_block_factor, which takes ba_math.h's LDL^T and so exists under hipcc only.  tests/native/simgraph_host.cpp runs it
// without a GPU against tests/simgraph_oracle.py.
#pragma once
#include "pgo_math.h"

#include <math.h>

namespace {

// one edge at the float32 states (s_i, R_i, t_i), (s_j, R_j, t_j) with the measurement (s_z, R_z, t_z)
struct SgEdge {
  float e[7];      // (Log R_d, t_d, log s_d)
  float rp[9];     // R_p = R_j R_i^T
  float u[3];      // s_d (R_d t_z)
  float sp;        // s_p = s_j / s_i
};

// header "Residual"
ICP_HD void sg_residual(float si, const float *ri, const float *ti, float sj, const float *rj, const float *tj, float sz,
                        const float *rz, const float *tz, SgEdge &o) {
  float rd[9], w[3], v[3];
  pgo_mul_abt(rj, ri, o.rp);
  pgo_mul_abt(o.rp, rz, rd);
  o.sp = sj / si;
  const float sd = o.sp / sz;
  icp_rotate(o.rp, ti, w);
  icp_rotate(rd, tz, v);
  pgo_log(rd, o.e);
  for (int a = 0; a < 3; ++a) {
    o.u[a] = sd * v[a];
    o.e[3 + a] = (tj[a] - o.sp * w[a]) - o.u[a];
  }
  o.e[6] = logf(sd);
}

// the symmetric information matrix from the upper triangle of info (7, 7)
ICP_HD void sg_omega(const float *info, float *O) {
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) O[r * 7 + c] = r <= c ? info[r * 7 + c] : info[c * 7 + r];
}

// left to right: (((((a0 b0 + a1 b1) + a2 b2) + a3 b3) + a4 b4) + a5 b5) + a6 b6 with strides sa, sb
ICP_HD float sg_dot7(const float *a, int sa, const float *b, int sb) {
  float s = a[0] * b[0];
  for (int k = 1; k < 7; ++k) s = s + a[k * sa] * b[k * sb];
  return s;
}

// oe = Omega e and chi2 = e . oe
ICP_HD float sg_chi2(const float *O, const float *e, float *oe) {
  for (int r = 0; r < 7; ++r) oe[r] = sg_dot7(O + r * 7, 1, e, 1);
  return sg_dot7(e, 1, oe, 1);
}

// the lines (header "Jacobians"), row-major 7x7, of e with respect to the left perturbations (w, tau, sigma) of node i and j
ICP_HD void sg_lines(const SgEdge &o, float *Ji, float *Jj) {
  float jl[9];
  pgo_jl_inv(o.e, jl);
  const float *td = o.e + 3;
  const float tx[9] = {0.0f, -td[2], td[1], td[2], 0.0f, -td[0], -td[1], td[0], 0.0f};
  const float ux[9] = {0.0f, -o.u[2], o.u[1], o.u[2], 0.0f, -o.u[0], -o.u[1], o.u[0], 0.0f};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) {
      const float jr = (jl[a * 3] * o.rp[b] + jl[a * 3 + 1] * o.rp[3 + b]) + jl[a * 3 + 2] * o.rp[6 + b];
      const float ur = (ux[a * 3] * o.rp[b] + ux[a * 3 + 1] * o.rp[3 + b]) + ux[a * 3 + 2] * o.rp[6 + b];
      Jj[a * 7 + b] = jl[a * 3 + b];
      Jj[a * 7 + 3 + b] = 0.0f;
      Jj[(3 + a) * 7 + b] = -tx[a * 3 + b];
      Jj[(3 + a) * 7 + 3 + b] = a == b ? 1.0f : 0.0f;
      Ji[a * 7 + b] = -jr;
      Ji[a * 7 + 3 + b] = 0.0f;
      Ji[(3 + a) * 7 + b] = -ur;
      Ji[(3 + a) * 7 + 3 + b] = -(o.sp * o.rp[a * 3 + b]);
    }
    Jj[a * 7 + 6] = 0.0f;
    Ji[a * 7 + 6] = 0.0f;
    Jj[(3 + a) * 7 + 6] = td[a];
    Ji[(3 + a) * 7 + 6] = o.u[a];
  }
  for (int b = 0; b < 6; ++b) { Jj[42 + b] = 0.0f; Ji[42 + b] = 0.0f; }
  Jj[48] = 1.0f;
  Ji[48] = -1.0f;
}

// A = Omega J: A_rc = dot7 over k of Omega_rk J_kc
ICP_HD void sg_omega_j(const float *O, const float *J, float *A) {
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) A[r * 7 + c] = sg_dot7(O + r * 7, 1, J + c, 7);
}

// out = w J^T A: out_rc = w (dot7 over k of J_kr A_kc).  sym: the upper triangle is computed and mirrored.
ICP_HD void sg_jt_a(const float *J, const float *A, float w, bool sym, float *out) {
  for (int r = 0; r < 7; ++r)
    for (int c = sym ? r : 0; c < 7; ++c) {
      const float v = w * sg_dot7(J + r, 7, A + c, 7);
      out[r * 7 + c] = v;
      if (sym) out[c * 7 + r] = v;
    }
}

// g = w J^T oe
ICP_HD void sg_jt_v(const float *J, const float *oe, float w, float *g) {
  for (int r = 0; r < 7; ++r) g[r] = w * sg_dot7(J + r, 7, oe, 1);
}

// index of (r, c), r <= c, in the packed upper triangle of a 7x7 matrix (ba_tri(7, r, c))
ICP_HD int sg_tri7(int r, int c) { return r * 7 - (r * (r - 1)) / 2 + (c - r); }

// z = M^-1 r from the factors of M = L D L^T (fac: d_j at (j, j), l_ij at (j, i), packed upper triangle, float32): K27's
// pgo_ldlt_apply for 7 unknowns
ICP_HD void sg_ldlt_apply(const float *fac, const float *r, float *z) {
  float y[7];
  for (int i = 0; i < 7; ++i) y[i] = r[i];
  for (int i = 0; i < 7; ++i)
    for (int k = i + 1; k < 7; ++k) y[k] = y[k] - fac[sg_tri7(i, k)] * y[i];
  for (int i = 0; i < 7; ++i) z[i] = y[i] / fac[sg_tri7(i, i)];
  for (int i = 6; i >= 0; --i)
    for (int k = 0; k < i; ++k) z[k] = z[k] - fac[sg_tri7(k, i)] * z[i];
}

// header "Update": state = (R row-major, t, s), 13 doubles; x = (w, tau, sigma)
ICP_HD void sg_update(double *state, const double *x) {
  double e[9], o[13];
  icp_exp(x, e);
  const double k = exp(x[6]);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = (e[i * 3] * state[j] + e[i * 3 + 1] * state[3 + j]) + e[i * 3 + 2] * state[6 + j];
    o[9 + i] = k * ((e[i * 3] * state[9] + e[i * 3 + 1] * state[10]) + e[i * 3 + 2] * state[11]) + x[3 + i];
  }
  o[12] = k * state[12];
  for (int i = 0; i < 13; ++i) state[i] = o[i];
}

// header, mi_simgraph_correct: a node's metric pose from its optimised state (s', R', t'), float64 rounded once
ICP_HD void sg_correct_pose(float s, const float *r, const float *t, float *r_out, float *t_out) {
  for (int k = 0; k < 9; ++k) r_out[k] = r[k];
  for (int a = 0; a < 3; ++a) t_out[a] = (float)((double)t[a] / (double)s);
}

// ... and a landmark attached to that node, whose pose was (R_old, t_old) before
ICP_HD void sg_correct_point(const float *r_old, const float *t_old, float s, const float *r, const float *t, const float *x,
                             float *x_out) {
  double d[3];
  for (int a = 0; a < 3; ++a) {
    const double y = (((double)r_old[3 * a] * (double)x[0] + (double)r_old[3 * a + 1] * (double)x[1]) +
                      (double)r_old[3 * a + 2] * (double)x[2]) + (double)t_old[a];
    d[a] = y - (double)t[a];
  }
  for (int c = 0; c < 3; ++c)
    x_out[c] = (float)((((double)r[c] * d[0] + (double)r[3 + c] * d[1]) + (double)r[6 + c] * d[2]) / (double)s);
}

#if defined(__HIPCC__)
// fac = the LDL^T factors of M = D + lambda diag D (float64 by ba_ldlt_solve, rounded to float32) for a node's block D
// (7x7 row-major, float32).  false -- the node is FROZEN for this step, fac = 0 --: K18's pivot rule fails, or a factor is
// not finite.  work: 35 doubles of the caller's (the block being factored and ba_ldlt_solve's right-hand side).
ICP_HD bool sg_block_factor(const float *D, float lambda, float *fac, double *work) {
  double *a = work, *x = work + 28;
  for (int i = 0; i < 7; ++i) x[i] = 0.0;
  int k = 0;
  for (int r = 0; r < 7; ++r)
    for (int c = r; c < 7; ++c) {
      const double d = (double)D[r * 7 + c];
      a[k++] = r == c ? d + (double)lambda * d : d;
    }
  bool ok = ba_ldlt_solve(a, x, 7, 0, 1, [] {});
  for (k = 0; k < 28; ++k) {
    fac[k] = (float)a[k];
    ok = ok && fabsf(fac[k]) < INFINITY;
  }
  if (!ok)
    for (k = 0; k < 28; ++k) fac[k] = 0.0f;
  return ok;
}
#endif

}  // namespace
