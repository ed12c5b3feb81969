// K31 Sim(3) pose-graph optimisation (include/mi355x_match_simgraph.h): K27's Levenberg-Marquardt with block-Jacobi
// preconditioned conjugate gradients (pgo.hip) on nodes that carry a scale -- 7 degrees of freedom per node, 7x7 blocks -- and
// the map correction that follows it.  The per-edge arithmetic, the preconditioner solve, the update and the correction are
// simgraph_math.h's (on pgo_math.h, K18's icp_exp and K25's LDL^T).  pgo.hip and this file share a skeleton and no code: K27's
// bits stay what they are.
//
// One workgroup of 256 threads per graph; no workgroup ever waits for another.
//   plan       the active edges (eij), per node its incident (edge, side) list in ascending edge index: a count per node,
//              a workgroup prefix sum, a stable fill.  Once per launch.
//   linearise  edges strided over the threads: e, w, Omega J_i, Omega J_j, the three 7x7 blocks and the two gradient
//              parts -> workspace (161 floats per edge); then per node element D_i, g_i over the node's list.
//   factor     one thread per live node: LDL^T of D_i + lambda diag D_i
//   pcg        x, r, p, q (A p, then z) in dynamic LDS, 4 x 7N floats; one thread per scalar row for A p and the vector
//              updates, one per node for z = M^-1 r; every dot product by sg_block_sum into float64
//   step       the candidate states (float64), their float32 rounding, the candidate's cost; accepted -> the state
// K31a sg_cost_kernel, K31b sg_linearise_kernel, K31c sg_refine_kernel, K31d sg_correct_kernel.  Built with
// -ffp-contract=off; no atomics; every reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "simgraph_math.h"

#include "mi355x_match_simgraph.h"

#include <math.h>

namespace {

constexpr int SG_THREADS = 256, SG_WAVES = SG_THREADS / 64;
constexpr int SG_EB = 161;           // workspace floats per edge: H_ii (49), H_jj (49), H_ij (49), g_i (7), g_j (7)
constexpr int SG_HIJ = 98, SG_GI = 147;
constexpr int SG_STATE = 13;         // doubles per node: R (9), t (3), s

struct SgShared {
  double red[2];
  float part[SG_WAVES][2];
  int scan[SG_THREADS];
};
constexpr size_t SG_SHARED_BYTES = (sizeof(SgShared) + 15) & ~(size_t)15;

// byte offsets of a graph's workspace arrays, each a multiple of 16
struct SgLayout {
  size_t state, cand, r, t, s, cr, ct, cs, diag, g, fac, eb, start, list, eij, live, frozen, total;
};
__host__ __device__ inline SgLayout sg_layout(int N, int E) {
  SgLayout l;
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
  l.state = take((size_t)N * SG_STATE * 8);    // float64 state and candidate
  l.cand = take((size_t)N * SG_STATE * 8);
  l.r = take((size_t)N * 9 * 4);               // their float32 roundings, the states every line is formed at
  l.t = take((size_t)N * 3 * 4);
  l.s = take((size_t)N * 4);
  l.cr = take((size_t)N * 9 * 4);
  l.ct = take((size_t)N * 3 * 4);
  l.cs = take((size_t)N * 4);
  l.diag = take((size_t)N * 49 * 4);
  l.g = take((size_t)N * 7 * 4);
  l.fac = take((size_t)N * 28 * 4);
  l.eb = take((size_t)E * SG_EB * 4);
  l.start = take((size_t)(N + 1) * 4);
  l.list = take((size_t)E * 2 * 4);
  l.eij = take((size_t)E * 2 * 4);
  l.live = take((size_t)N * 4);
  l.frozen = take((size_t)N * 4);
  l.total = o;
  return l;
}

struct SgGraph {
  const int32_t *ei;
  const float *zs, *zr, *zt, *info;
  const uint8_t *ev, *fixed;
  int N, E;
  float huber;
  double *state, *cand;
  float *r, *t, *s, *cr, *ct, *cs, *diag, *g, *fac, *eb;
  int *start, *list, *eij, *live, *frozen;
};

__device__ __forceinline__ SgGraph sg_graph(const int32_t *ei, const float *zs, const float *zr, const float *zt, const float *info,
                                            const uint8_t *ev, const uint8_t *fixed, int N, int E, float huber, void *ws) {
  const size_t b = blockIdx.x;
  SgGraph G;
  G.N = N; G.E = E; G.huber = huber;
  G.ei = ei + b * E * 2;
  G.zs = zs + b * E;
  G.zr = zr + b * E * 9;
  G.zt = zt + b * E * 3;
  G.info = info + b * E * 49;
  G.ev = ev + b * E;
  G.fixed = fixed ? fixed + b * N : nullptr;
  if (ws) {
    const SgLayout l = sg_layout(N, E);
    char *base = (char *)ws + b * l.total;
    G.state = (double *)(base + l.state); G.cand = (double *)(base + l.cand);
    G.r = (float *)(base + l.r); G.t = (float *)(base + l.t); G.s = (float *)(base + l.s);
    G.cr = (float *)(base + l.cr); G.ct = (float *)(base + l.ct); G.cs = (float *)(base + l.cs);
    G.diag = (float *)(base + l.diag); G.g = (float *)(base + l.g); G.fac = (float *)(base + l.fac); G.eb = (float *)(base + l.eb);
    G.start = (int *)(base + l.start); G.list = (int *)(base + l.list); G.eij = (int *)(base + l.eij);
    G.live = (int *)(base + l.live); G.frozen = (int *)(base + l.frozen);
  }
  return G;
}

// red[k] = the sum of acc[k] over the workgroup: wave_sum_dpp, then the waves in order in float64 (pgo.hip's pgo_block_sum)
template <int NS>
__device__ __forceinline__ void sg_block_sum(SgShared &S, const float *acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const float v = wave_sum_dpp(acc[k]);
    if (lane == 0) S.part[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < SG_WAVES; ++w) t += (double)S.part[w][threadIdx.x];
    S.red[threadIdx.x] = t;
  }
  __syncthreads();
}

// the sum of v over the workgroup and, in *before, over the threads below this one (integers: any order gives the same)
__device__ __forceinline__ int sg_int_sum(SgShared &S, int v, int *before) {
  __syncthreads();
  S.scan[threadIdx.x] = v;
  __syncthreads();
  int total = 0, b = 0;
#pragma unroll 4
  for (int i = 0; i < SG_THREADS; ++i) {
    b = i == (int)threadIdx.x ? total : b;
    total += S.scan[i];
  }
  *before = b;
  return total;
}

// header "Edges": is edge e active, and between which nodes
__device__ __forceinline__ bool sg_edge_active(const SgGraph &G, int e, int *i, int *j) {
  *i = -1; *j = -1;
  if (G.ev[e] == 0) return false;
  const int a = G.ei[2 * e], b = G.ei[2 * e + 1];
  if (a == b || a < 0 || a >= G.N || b < 0 || b >= G.N) return false;
  const float zs = G.zs[e];
  bool finite = zs > 0.0f && zs < INFINITY;
  for (int k = 0; k < 9; ++k) finite = finite && fabsf(G.zr[(size_t)e * 9 + k]) < INFINITY;
  for (int k = 0; k < 3; ++k) finite = finite && fabsf(G.zt[(size_t)e * 3 + k]) < INFINITY;
  for (int k = 0; k < 49; ++k) finite = finite && fabsf(G.info[(size_t)e * 49 + k]) < INFINITY;
  if (!finite) return false;
  *i = a; *j = b;
  return true;
}

// plan: eij, start, list, live.  counts = (active edges, fixed nodes, live nodes), the same in every thread.
// Bounds: list holds one entry per end of an active edge, at most 2 E; `at` of a thread starts at the number of entries of the
// nodes below its chunk and ends at that of the nodes up to its chunk's end.
__device__ void sg_plan(SgShared &S, const SgGraph &G, int *counts) {
  const int t = threadIdx.x;
  int nact = 0;
  for (int e = t; e < G.E; e += SG_THREADS) {
    int i, j;
    nact += sg_edge_active(G, e, &i, &j) ? 1 : 0;
    G.eij[2 * e] = i;
    G.eij[2 * e + 1] = j;
  }
  int before;
  counts[0] = sg_int_sum(S, nact, &before);             // (its barriers publish eij)
  const int chunk = (G.N + SG_THREADS - 1) / SG_THREADS, lo = t * chunk, hi = lo + chunk < G.N ? lo + chunk : G.N;
  int mine = 0;
  for (int n = lo; n < hi; ++n)
    for (int e = 0; e < G.E; ++e) mine += (G.eij[2 * e] == n ? 1 : 0) + (G.eij[2 * e + 1] == n ? 1 : 0);
  sg_int_sum(S, mine, &before);
  int at = before, nfixed = 0, nlive = 0;
  if (t == 0) G.start[0] = 0;
  for (int n = lo; n < hi; ++n) {
    const int first = at;
    for (int e = 0; e < G.E; ++e) {
      if (G.eij[2 * e] == n) G.list[at++] = 2 * e;
      if (G.eij[2 * e + 1] == n) G.list[at++] = 2 * e + 1;
    }
    G.start[n + 1] = at;
    const bool fixed = G.fixed[n] != 0;
    G.live[n] = (!fixed && at > first) ? 1 : 0;
    G.frozen[n] = 0;
    nfixed += fixed ? 1 : 0;
    nlive += (!fixed && at > first) ? 1 : 0;
  }
  counts[1] = sg_int_sum(S, nfixed, &before);
  counts[2] = sg_int_sum(S, nlive, &before);
  __syncthreads();
}

// the residual of the active edge e = (i, j) at the float32 state (s, r, t), its Omega and chi2
__device__ __forceinline__ float sg_edge_chi2(const SgGraph &G, const float *s, const float *r, const float *t, int e, int i, int j,
                                              SgEdge &o, float *O, float *oe) {
  float ri[9], ti[3], rj[9], tj[3], rz[9], tz[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) { ri[k] = r[(size_t)i * 9 + k]; rj[k] = r[(size_t)j * 9 + k]; rz[k] = G.zr[(size_t)e * 9 + k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) { ti[k] = t[(size_t)i * 3 + k]; tj[k] = t[(size_t)j * 3 + k]; tz[k] = G.zt[(size_t)e * 3 + k]; }
  sg_residual(s[i], ri, ti, s[j], rj, tj, G.zs[e], rz, tz, o);
  sg_omega(G.info + (size_t)e * 49, O);
  return sg_chi2(O, o.e, oe);
}

// the cost at (s, r, t) (header "Cost"), the same in every thread.  eij: the plan's, or nullptr (the activity is then decided here).
template <bool WRITE>
__device__ double sg_cost_pass(SgShared &S, const SgGraph &G, const float *s, const float *r, const float *t, const int *eij,
                               float *chi2_out, uint8_t *active_out, int *nactive) {
  float acc[2] = {0.0f, 0.0f};
  for (int e = threadIdx.x; e < G.E; e += SG_THREADS) {
    int i, j;
    if (eij) { i = eij[2 * e]; j = eij[2 * e + 1]; } else sg_edge_active(G, e, &i, &j);
    float chi2 = 0.0f;
    if (i >= 0) {
      SgEdge o;
      float O[49], oe[7], w, rho;
      chi2 = sg_edge_chi2(G, s, r, t, e, i, j, o, O, oe);
      if (!pgo_rho(chi2, G.huber, &w, &rho)) chi2 = INFINITY;
      acc[0] += rho;
      acc[1] += 1.0f;
    }
    if (WRITE) {
      chi2_out[e] = chi2;
      if (active_out) active_out[e] = i >= 0 ? 1 : 0;
    }
  }
  sg_block_sum<2>(S, acc);
  *nactive = (int)S.red[1];
  return S.red[0];
}

// linearise at (G.s, G.r, G.t): the edge blocks, then D and g of every node (zero unless the node is live)
__device__ void sg_linearise(const SgGraph &G) {
  for (int e = threadIdx.x; e < G.E; e += SG_THREADS) {
    const int i = G.eij[2 * e], j = G.eij[2 * e + 1];
    if (i < 0) continue;
    float *out = G.eb + (size_t)e * SG_EB;
    SgEdge o;
    float O[49], oe[7], w, rho;
    const float chi2 = sg_edge_chi2(G, G.s, G.r, G.t, e, i, j, o, O, oe);
    if (!pgo_rho(chi2, G.huber, &w, &rho)) {
      for (int k = 0; k < SG_EB; ++k) out[k] = 0.0f;
      continue;
    }
    const bool coupled = G.fixed[i] == 0 && G.fixed[j] == 0;
    float Ji[49], Jj[49], A[49];
    sg_lines(o, Ji, Jj);
    sg_omega_j(O, Jj, A);
    sg_jt_a(Jj, A, w, true, out + 49);
    sg_jt_a(Ji, A, coupled ? w : 0.0f, false, out + SG_HIJ);
    sg_omega_j(O, Ji, A);
    sg_jt_a(Ji, A, w, true, out);
    sg_jt_v(Ji, oe, w, out + SG_GI);
    sg_jt_v(Jj, oe, w, out + SG_GI + 7);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G.N * 56; idx += SG_THREADS) {
    const int n = idx / 56, k = idx % 56;
    float s = 0.0f;
    if (G.live[n]) {
      for (int q = G.start[n]; q < G.start[n + 1]; ++q) {
        const int ent = G.list[q], side = ent & 1;
        const float *blk = G.eb + (size_t)(ent >> 1) * SG_EB;
        s += k < 49 ? blk[side * 49 + k] : blk[SG_GI + side * 7 + (k - 49)];
      }
    }
    if (k < 49) G.diag[(size_t)n * 49 + k] = s; else G.g[(size_t)n * 7 + (k - 49)] = s;
  }
  __syncthreads();
}

// row c of node n of (H + lambda diag H) p
__device__ __forceinline__ float sg_ap_row(const SgGraph &G, const float *p, int n, int c, float lambda) {
  const float *D = G.diag + (size_t)n * 49 + c * 7, *pn = p + 7 * n;
  float acc = sg_dot7(D, 1, pn, 1);
  acc = acc + (lambda * D[c]) * pn[c];
  for (int q = G.start[n]; q < G.start[n + 1]; ++q) {
    const int ent = G.list[q], e = ent >> 1, side = ent & 1;
    const float *B = G.eb + (size_t)e * SG_EB + SG_HIJ, *po = p + 7 * G.eij[2 * e + (1 - side)];
    acc = acc + (side == 0 ? sg_dot7(B + 7 * c, 1, po, 1) : sg_dot7(B + c, 7, po, 1));
  }
  return acc;
}

// the damped step (header "Solve"): x = the step of every live node (0 elsewhere) after `trips` PCG trips
__device__ void sg_pcg(SgShared &S, const SgGraph &G, float *x, float *r, float *p, float *q, float lambda, int trips) {
  const int t = threadIdx.x, rows = 7 * G.N;
  for (int n = t; n < G.N; n += SG_THREADS) {
    double work[35];
    if (G.live[n]) G.frozen[n] = sg_block_factor(G.diag + (size_t)n * 49, lambda, G.fac + (size_t)n * 28, work) ? 0 : 1;
  }
  __syncthreads();
  for (int row = t; row < rows; row += SG_THREADS) {
    const int n = row / 7;
    x[row] = 0.0f;
    p[row] = 0.0f;
    r[row] = (G.live[n] && !G.frozen[n]) ? -G.g[row] : 0.0f;
  }
  __syncthreads();
  float acc[2] = {0.0f, 0.0f};
  for (int n = t; n < G.N; n += SG_THREADS) {
    float z[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (G.live[n] && !G.frozen[n]) sg_ldlt_apply(G.fac + (size_t)n * 28, r + 7 * n, z);
#pragma unroll
    for (int k = 0; k < 7; ++k) { q[7 * n + k] = z[k]; p[7 * n + k] = z[k]; }
  }
  __syncthreads();
  for (int row = t; row < rows; row += SG_THREADS) acc[0] += r[row] * q[row];
  sg_block_sum<1>(S, acc);
  double rz = S.red[0];
  bool dead = false;
#pragma unroll 1
  for (int trip = 0; trip < trips; ++trip) {
    acc[0] = 0.0f;
    for (int row = t; row < rows; row += SG_THREADS) {
      const int n = row / 7;
      const float v = (G.live[n] && !G.frozen[n]) ? sg_ap_row(G, p, n, row - 7 * n, lambda) : 0.0f;
      q[row] = v;
      acc[0] += p[row] * v;
    }
    sg_block_sum<1>(S, acc);
    const double pap = S.red[0];                          // workgroup-uniform: read after the sum's last barrier
    dead = dead || !(pap > 0.0) || !(pap < INFINITY) || rz == 0.0;
    const float alpha = dead ? 0.0f : (float)(rz / pap);
    for (int row = t; row < rows; row += SG_THREADS) {
      x[row] = x[row] + alpha * p[row];
      r[row] = r[row] - alpha * q[row];
    }
    __syncthreads();
    for (int n = t; n < G.N; n += SG_THREADS) {
      float z[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (G.live[n] && !G.frozen[n]) sg_ldlt_apply(G.fac + (size_t)n * 28, r + 7 * n, z);
#pragma unroll
      for (int k = 0; k < 7; ++k) q[7 * n + k] = z[k];
    }
    __syncthreads();
    acc[0] = 0.0f;
    for (int row = t; row < rows; row += SG_THREADS) acc[0] += r[row] * q[row];
    sg_block_sum<1>(S, acc);
    const double rz_new = S.red[0];
    if (!dead) {
      const float beta = (float)(rz_new / rz);
      for (int row = t; row < rows; row += SG_THREADS) p[row] = q[row] + beta * p[row];
      rz = rz_new;
    }
    __syncthreads();
  }
}

// the candidate: the update of every live node's float64 state by its step, and its float32 rounding
__device__ void sg_step(const SgGraph &G, const float *x) {
  for (int n = threadIdx.x; n < G.N; n += SG_THREADS) {
    double st[SG_STATE];
#pragma unroll
    for (int c = 0; c < SG_STATE; ++c) st[c] = G.state[(size_t)n * SG_STATE + c];
    if (G.live[n] && !G.frozen[n]) {
      double d[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) d[k] = (double)x[7 * n + k];
      sg_update(st, d);
    }
#pragma unroll
    for (int c = 0; c < SG_STATE; ++c) {
      G.cand[(size_t)n * SG_STATE + c] = st[c];
      if (c < 9) G.cr[(size_t)n * 9 + c] = (float)st[c];
      else if (c < 12) G.ct[(size_t)n * 3 + (c - 9)] = (float)st[c];
      else G.cs[n] = (float)st[c];
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void sg_stage(const SgGraph &G, const float *s, const float *r, const float *t) {
  for (int idx = threadIdx.x; idx < G.N * SG_STATE; idx += SG_THREADS) {
    const int n = idx / SG_STATE, c = idx % SG_STATE;
    const float v = c < 9 ? r[(size_t)n * 9 + c] : c < 12 ? t[(size_t)n * 3 + (c - 9)] : s[n];
    G.state[idx] = (double)v;
    if (c < 9) G.r[(size_t)n * 9 + c] = v;
    else if (c < 12) G.t[(size_t)n * 3 + (c - 9)] = v;
    else G.s[n] = v;
  }
  __syncthreads();
}

extern __shared__ __attribute__((aligned(16))) char sg_lds[];

// ---- K31a ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_cost_kernel(const float *__restrict__ s, const float *__restrict__ r,
                                                             const float *__restrict__ t, const int32_t *__restrict__ ei,
                                                             const float *__restrict__ zs, const float *__restrict__ zr,
                                                             const float *__restrict__ zt, const float *__restrict__ info,
                                                             const uint8_t *__restrict__ ev, int N, int E, float huber,
                                                             float *__restrict__ chi2, float *__restrict__ cost,
                                                             uint8_t *__restrict__ active) {
  SgShared &S = *reinterpret_cast<SgShared *>(sg_lds);
  const size_t b = blockIdx.x;
  const SgGraph G = sg_graph(ei, zs, zr, zt, info, ev, nullptr, N, E, huber, nullptr);
  int nact;
  const double c = sg_cost_pass<true>(S, G, s + b * N, r + b * N * 9, t + b * N * 3, nullptr, chi2 + b * E, active + b * E, &nact);
  if (threadIdx.x == 0) cost[b] = (float)c;
}

// ---- K31b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_linearise_kernel(const float *__restrict__ s, const float *__restrict__ r,
                                                                  const float *__restrict__ t, const int32_t *__restrict__ ei,
                                                                  const float *__restrict__ zs, const float *__restrict__ zr,
                                                                  const float *__restrict__ zt, const float *__restrict__ info,
                                                                  const uint8_t *__restrict__ ev, const uint8_t *__restrict__ fixed,
                                                                  int N, int E, float huber, float *__restrict__ diag,
                                                                  float *__restrict__ off, float *__restrict__ g,
                                                                  float *__restrict__ cost, void *__restrict__ ws) {
  SgShared &S = *reinterpret_cast<SgShared *>(sg_lds);
  const size_t b = blockIdx.x;
  const SgGraph G = sg_graph(ei, zs, zr, zt, info, ev, fixed, N, E, huber, ws);
  sg_stage(G, s + b * N, r + b * N * 9, t + b * N * 3);
  int counts[3], nact;
  sg_plan(S, G, counts);
  const double c = sg_cost_pass<false>(S, G, G.s, G.r, G.t, G.eij, nullptr, nullptr, &nact);
  sg_linearise(G);
  for (int idx = threadIdx.x; idx < N * 49; idx += SG_THREADS) diag[b * N * 49 + idx] = G.diag[idx];
  for (int idx = threadIdx.x; idx < N * 7; idx += SG_THREADS) g[b * N * 7 + idx] = G.g[idx];
  for (int idx = threadIdx.x; idx < E * 49; idx += SG_THREADS) {
    const int e = idx / 49;
    off[b * E * 49 + idx] = G.eij[2 * e] >= 0 ? G.eb[(size_t)e * SG_EB + SG_HIJ + idx % 49] : 0.0f;
  }
  if (threadIdx.x == 0) cost[b] = (float)c;
}

// ---- K31c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_refine_kernel(const float *__restrict__ s0, const float *__restrict__ r0,
                                                               const float *__restrict__ t0, const int32_t *__restrict__ ei,
                                                               const float *__restrict__ zs, const float *__restrict__ zr,
                                                               const float *__restrict__ zt, const float *__restrict__ info,
                                                               const uint8_t *__restrict__ ev, const uint8_t *__restrict__ fixed,
                                                               int N, int E, int iterations, int trips, float huber,
                                                               float *__restrict__ s_out, float *__restrict__ r_out,
                                                               float *__restrict__ t_out, float *__restrict__ chi2_out,
                                                               float *__restrict__ cost0_out, float *__restrict__ cost_out,
                                                               int *__restrict__ accepted_out, float *__restrict__ info_out,
                                                               uint8_t *__restrict__ ok_out, void *__restrict__ ws) {
  SgShared &S = *reinterpret_cast<SgShared *>(sg_lds);
  float *x = reinterpret_cast<float *>(sg_lds + SG_SHARED_BYTES), *rr = x + 7 * N, *p = rr + 7 * N, *q = p + 7 * N;
  const size_t b = blockIdx.x;
  const int t = threadIdx.x;
  const SgGraph G = sg_graph(ei, zs, zr, zt, info, ev, fixed, N, E, huber, ws);
  sg_stage(G, s0 + b * N, r0 + b * N * 9, t0 + b * N * 3);
  int counts[3], nact, accepted = 0;
  sg_plan(S, G, counts);
  double cost0 = sg_cost_pass<false>(S, G, G.s, G.r, G.t, G.eij, nullptr, nullptr, &nact);
  double cost = cost0;
  const bool refused = !(cost0 < INFINITY) || counts[0] == 0 || counts[1] == 0 || counts[2] == 0;   // the same in every thread
  if (!refused) {
    double lambda = BA_LAMBDA0;
    bool stale = true;                                     // the blocks in the workspace are not those of the state
#pragma unroll 1
    for (int it = 0; it < iterations; ++it) {
      if (stale) sg_linearise(G);
      stale = false;
      sg_pcg(S, G, x, rr, p, q, (float)lambda, trips);
      sg_step(G, x);
      const double c = sg_cost_pass<false>(S, G, G.cs, G.cr, G.ct, G.eij, nullptr, nullptr, &nact);
      if (c < INFINITY && c < cost) {
        for (int idx = t; idx < N * SG_STATE; idx += SG_THREADS) G.state[idx] = G.cand[idx];
        for (int idx = t; idx < N * 9; idx += SG_THREADS) G.r[idx] = G.cr[idx];
        for (int idx = t; idx < N * 3; idx += SG_THREADS) G.t[idx] = G.ct[idx];
        for (int idx = t; idx < N; idx += SG_THREADS) G.s[idx] = G.cs[idx];
        cost = c;
        ++accepted;
        stale = true;
        lambda = lambda / BA_LAMBDA_STEP > BA_LAMBDA_MIN ? lambda / BA_LAMBDA_STEP : BA_LAMBDA_MIN;
      } else {
        lambda = lambda * BA_LAMBDA_STEP < BA_LAMBDA_MAX ? lambda * BA_LAMBDA_STEP : BA_LAMBDA_MAX;
      }
      __syncthreads();
    }
    if (stale) sg_linearise(G);
    sg_cost_pass<true>(S, G, G.s, G.r, G.t, G.eij, chi2_out + b * E, nullptr, &nact);
  } else {
    cost0 = counts[0] == 0 ? 0.0 : INFINITY;
    cost = cost0;
    for (int e = t; e < E; e += SG_THREADS) chi2_out[b * E + e] = 0.0f;
  }
  for (int idx = t; idx < N * 49; idx += SG_THREADS) info_out[b * N * 49 + idx] = refused ? 0.0f : G.diag[idx];
  for (int idx = t; idx < N * 9; idx += SG_THREADS) r_out[b * N * 9 + idx] = G.r[idx];
  for (int idx = t; idx < N * 3; idx += SG_THREADS) t_out[b * N * 3 + idx] = G.t[idx];
  for (int idx = t; idx < N; idx += SG_THREADS) s_out[b * N + idx] = G.s[idx];
  if (t == 0) {
    cost0_out[b] = (float)cost0;
    cost_out[b] = (float)cost;
    accepted_out[b] = accepted;
    ok_out[b] = refused ? 0 : 1;
  }
}

// ---- K31d ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sg_correct_kernel(const float *__restrict__ r_old, const float *__restrict__ t_old,
                                                         const float *__restrict__ s, const float *__restrict__ r,
                                                         const float *__restrict__ t, const float *__restrict__ points,
                                                         const int32_t *__restrict__ ref, int nodes, int landmarks,
                                                         float *__restrict__ r_out, float *__restrict__ t_out,
                                                         float *__restrict__ points_out) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nodes + landmarks) return;
  if (i < nodes) {
    const size_t n = (size_t)b * nodes + i;
    sg_correct_pose(s[n], r + n * 9, t + n * 3, r_out + n * 9, t_out + n * 3);
  } else {
    const size_t l = (size_t)b * landmarks + (i - nodes);
    const int k = ref[l];
    if (k < 0 || k >= nodes) {
      for (int c = 0; c < 3; ++c) points_out[l * 3 + c] = points[l * 3 + c];
    } else {
      const size_t n = (size_t)b * nodes + k;
      sg_correct_point(r_old + n * 9, t_old + n * 3, s[n], r + n * 9, t + n * 3, points + l * 3, points_out + l * 3);
    }
  }
}

int sg_shape_status(int batch, int nodes, int edges) {
  if (batch < 1 || nodes < 2 || edges < 1) return MI_E_SHAPE;
  if (batch > 65535 || nodes > MI_SIMGRAPH_MAX_NODES || edges > MI_SIMGRAPH_MAX_EDGES) return MI_E_PARAM;
  return MI_OK;
}
bool sg_huber_ok(float huber) { return huber >= 0.0f && huber < INFINITY; }
int sg_workspace_status(const void *workspace, size_t bytes, int batch, int nodes, int edges) {
  if (((uintptr_t)workspace % 16) != 0) return MI_E_ALIGN;
  if (bytes < mi_simgraph_workspace_bytes(batch, nodes, edges)) return MI_E_CAPACITY;
  return MI_OK;
}
size_t sg_lds_bytes(int nodes) { return SG_SHARED_BYTES + (size_t)4 * 7 * nodes * sizeof(float); }

}  // namespace

extern "C" size_t mi_simgraph_workspace_bytes(int batch, int nodes, int edges) {
  if (sg_shape_status(batch, nodes, edges) != MI_OK) return 0;
  return (size_t)batch * sg_layout(nodes, edges).total;
}

extern "C" int mi_simgraph_cost(const float *s, const float *r, const float *t, const int32_t *edge_index, const float *zs,
                                const float *zr, const float *zt, const float *info, const uint8_t *edge_valid, int batch,
                                int nodes, int edges, float huber, float *chi2, float *cost, uint8_t *active, mi_stream_t stream) {
  MI_ENTER();
  if (!s || !r || !t || !edge_index || !zs || !zr || !zt || !info || !edge_valid || !chi2 || !cost || !active) return MI_E_NULL;
  if (const int st = sg_shape_status(batch, nodes, edges)) return st;
  if (!sg_huber_ok(huber)) return MI_E_PARAM;
  hipLaunchKernelGGL(sg_cost_kernel, dim3((unsigned)batch), dim3(SG_THREADS), SG_SHARED_BYTES, (hipStream_t)stream, s, r, t,
                     edge_index, zs, zr, zt, info, edge_valid, nodes, edges, huber, chi2, cost, active);
  return mi_launch_status();
}

extern "C" int mi_simgraph_linearise(const float *s, const float *r, const float *t, const int32_t *edge_index, const float *zs,
                                     const float *zr, const float *zt, const float *info, const uint8_t *edge_valid,
                                     const uint8_t *fixed, int batch, int nodes, int edges, float huber, float *diag, float *off,
                                     float *g, float *cost, void *workspace, size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!s || !r || !t || !edge_index || !zs || !zr || !zt || !info || !edge_valid || !fixed || !diag || !off || !g || !cost ||
      !workspace)
    return MI_E_NULL;
  if (const int st = sg_shape_status(batch, nodes, edges)) return st;
  if (!sg_huber_ok(huber)) return MI_E_PARAM;
  if (const int st = sg_workspace_status(workspace, workspace_bytes, batch, nodes, edges)) return st;
  hipLaunchKernelGGL(sg_linearise_kernel, dim3((unsigned)batch), dim3(SG_THREADS), SG_SHARED_BYTES, (hipStream_t)stream, s, r, t,
                     edge_index, zs, zr, zt, info, edge_valid, fixed, nodes, edges, huber, diag, off, g, cost, workspace);
  return mi_launch_status();
}

extern "C" int mi_simgraph_refine(const float *s0, const float *r0, const float *t0, const int32_t *edge_index, const float *zs,
                                  const float *zr, const float *zt, const float *info, const uint8_t *edge_valid,
                                  const uint8_t *fixed, int batch, int nodes, int edges, int iterations, int pcg_iterations,
                                  float huber, float *s, float *r, float *t, float *chi2, float *cost0, float *cost,
                                  int32_t *accepted, float *info_out, uint8_t *ok, void *workspace, size_t workspace_bytes,
                                  mi_stream_t stream) {
  MI_ENTER();
  if (!s0 || !r0 || !t0 || !edge_index || !zs || !zr || !zt || !info || !edge_valid || !fixed || !s || !r || !t || !chi2 ||
      !cost0 || !cost || !accepted || !info_out || !ok || !workspace)
    return MI_E_NULL;
  if (const int st = sg_shape_status(batch, nodes, edges)) return st;
  if (iterations < 1 || iterations > MI_SIMGRAPH_MAX_ITERATIONS || pcg_iterations < 1 || pcg_iterations > MI_SIMGRAPH_MAX_PCG ||
      !sg_huber_ok(huber))
    return MI_E_PARAM;
  if (const int st = sg_workspace_status(workspace, workspace_bytes, batch, nodes, edges)) return st;
  const size_t lds = sg_lds_bytes(nodes);
  static size_t allowed = 64 * 1024;                     // raised once, to what the node cap needs (mi_pgo_refine's pattern)
  if (lds > allowed) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(sg_refine_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)sg_lds_bytes(MI_SIMGRAPH_MAX_NODES));
    if (e != hipSuccess) return (int)e;
    allowed = sg_lds_bytes(MI_SIMGRAPH_MAX_NODES);
  }
  hipLaunchKernelGGL(sg_refine_kernel, dim3((unsigned)batch), dim3(SG_THREADS), lds, (hipStream_t)stream, s0, r0, t0, edge_index,
                     zs, zr, zt, info, edge_valid, fixed, nodes, edges, iterations, pcg_iterations, huber, s, r, t, chi2, cost0,
                     cost, accepted, info_out, ok, workspace);
  return mi_launch_status();
}

extern "C" int mi_simgraph_correct(const float *r_old, const float *t_old, const float *s, const float *r, const float *t,
                                   const float *points, const int32_t *ref, int batch, int nodes, int landmarks, float *r_out,
                                   float *t_out, float *points_out, mi_stream_t stream) {
  MI_ENTER();
  if (nodes > 0 && (!r_old || !t_old || !s || !r || !t || !r_out || !t_out)) return MI_E_NULL;
  if (landmarks > 0 && (!points || !ref || !points_out)) return MI_E_NULL;
  if (batch < 1 || nodes < 0 || landmarks < 0 || (nodes == 0 && landmarks == 0)) return MI_E_SHAPE;
  if (batch > 65535 || (long long)nodes + landmarks > MI_SIMGRAPH_MAX_ROWS) return MI_E_PARAM;
  hipLaunchKernelGGL(sg_correct_kernel, dim3((unsigned)ceil_div(nodes + landmarks, 256), (unsigned)batch), dim3(256), 0,
                     (hipStream_t)stream, r_old, t_old, s, r, t, points, ref, nodes, landmarks, r_out, t_out, points_out);
  return mi_launch_status();
}
