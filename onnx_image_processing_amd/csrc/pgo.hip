// K27 pose-graph optimisation (include/mi355x_match.h): Levenberg-Marquardt on the relative-pose
// edges of a graph of keyframes, every damped step solved by a fixed number of preconditioned conjugate-gradient trips with
// the block-Jacobi preconditioner, batched over independent graphs under K25's contract.  The per-edge arithmetic and the
// preconditioner solve are pgo_math.h's (on K18's icp_update_pose and K25's LDL^T).
//
// One workgroup of 256 threads per graph; no workgroup ever waits for another.
//   plan       the active edges (eij), per node its incident (edge, side) list in ascending edge index: a count per node,
//              a workgroup prefix sum, a stable fill.  A function of edge_index, edge_valid, fixed and the finiteness of
//              the measurements: once per launch.
//   linearise  edges strided over the threads: e, w, Omega J_i, Omega J_j, the three 6x6 blocks and the two gradient
//              parts -> workspace (120 floats per edge); then per node element D_i, g_i over the node's list.
//   factor     one thread per live node: LDL^T of D_i + lambda diag D_i
//   pcg        x, r, p, q (A p, then z) in dynamic LDS, 4 x 6N floats; one thread per scalar row for A p and the vector
//              updates, one per node for z = M^-1 r; every dot product by pgo_block_sum into float64
//   step       the candidate poses (float64), their float32 rounding, the candidate's cost; accepted -> the state
// K27a pgo_cost_kernel, K27b pgo_linearise_kernel, K27c pgo_refine_kernel.  Built with -ffp-contract=off; no atomics; every
// reduction has a fixed order: bitwise reproducible.
#include "common.h"
#include "pgo_math.h"

#include <math.h>

namespace {

constexpr int PGO_THREADS = 256, PGO_WAVES = PGO_THREADS / 64;
constexpr int PGO_EB = 120;          // workspace floats per edge: H_ii (36), H_jj (36), H_ij (36), g_i (6), g_j (6)
constexpr int PGO_HIJ = 72, PGO_GI = 108;

struct PgoShared {
  double red[2];
  float part[PGO_WAVES][2];
  int scan[PGO_THREADS];
};
constexpr size_t PGO_SHARED_BYTES = (sizeof(PgoShared) + 15) & ~(size_t)15;

// byte offsets of a graph's workspace arrays, each a multiple of 16
struct PgoLayout {
  size_t pose, cand, r, t, cr, ct, diag, g, fac, eb, start, list, eij, live, frozen, total;
};
__host__ __device__ inline PgoLayout pgo_layout(int N, int E) {
  PgoLayout l;
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
  l.pose = take((size_t)N * 12 * 8);      // float64 state and candidate
  l.cand = take((size_t)N * 12 * 8);
  l.r = take((size_t)N * 9 * 4);          // their float32 roundings, the poses every line is formed at
  l.t = take((size_t)N * 3 * 4);
  l.cr = take((size_t)N * 9 * 4);
  l.ct = take((size_t)N * 3 * 4);
  l.diag = take((size_t)N * 36 * 4);
  l.g = take((size_t)N * 6 * 4);
  l.fac = take((size_t)N * 21 * 4);
  l.eb = take((size_t)E * PGO_EB * 4);
  l.start = take((size_t)(N + 1) * 4);
  l.list = take((size_t)E * 2 * 4);
  l.eij = take((size_t)E * 2 * 4);
  l.live = take((size_t)N * 4);
  l.frozen = take((size_t)N * 4);
  l.total = o;
  return l;
}

struct PgoGraph {
  const int32_t *ei;
  const float *zr, *zt, *info;
  const uint8_t *ev, *fixed;
  int N, E;
  float huber;
  double *pose, *cand;
  float *r, *t, *cr, *ct, *diag, *g, *fac, *eb;
  int *start, *list, *eij, *live, *frozen;
};

__device__ __forceinline__ PgoGraph pgo_graph(const int32_t *ei, const float *zr, const float *zt, const float *info,
                                              const uint8_t *ev, const uint8_t *fixed, int N, int E, float huber, void *ws) {
  const size_t b = blockIdx.x;
  PgoGraph G;
  G.N = N; G.E = E; G.huber = huber;
  G.ei = ei + b * E * 2;
  G.zr = zr + b * E * 9;
  G.zt = zt + b * E * 3;
  G.info = info + b * E * 36;
  G.ev = ev + b * E;
  G.fixed = fixed ? fixed + b * N : nullptr;
  if (ws) {
    const PgoLayout l = pgo_layout(N, E);
    char *base = (char *)ws + b * l.total;
    G.pose = (double *)(base + l.pose); G.cand = (double *)(base + l.cand);
    G.r = (float *)(base + l.r); G.t = (float *)(base + l.t); G.cr = (float *)(base + l.cr); G.ct = (float *)(base + l.ct);
    G.diag = (float *)(base + l.diag); G.g = (float *)(base + l.g); G.fac = (float *)(base + l.fac); G.eb = (float *)(base + l.eb);
    G.start = (int *)(base + l.start); G.list = (int *)(base + l.list); G.eij = (int *)(base + l.eij);
    G.live = (int *)(base + l.live); G.frozen = (int *)(base + l.frozen);
  }
  return G;
}

// red[k] = the sum of acc[k] over the workgroup: wave_sum_dpp, then the waves in order in float64 (ba.hip's ba_block_sum)
template <int NS>
__device__ __forceinline__ void pgo_block_sum(PgoShared &S, const float *acc) {
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
    for (int w = 0; w < PGO_WAVES; ++w) t += (double)S.part[w][threadIdx.x];
    S.red[threadIdx.x] = t;
  }
  __syncthreads();
}

// the sum of v over the workgroup and, in *before, over the threads below this one (integers: any order gives the same)
__device__ __forceinline__ int pgo_int_sum(PgoShared &S, int v, int *before) {
  __syncthreads();
  S.scan[threadIdx.x] = v;
  __syncthreads();
  int total = 0, b = 0;
#pragma unroll 4                                          // (unrolled whole, the 256 reads in flight take 256 registers)
  for (int i = 0; i < PGO_THREADS; ++i) {
    b = i == (int)threadIdx.x ? total : b;
    total += S.scan[i];
  }
  *before = b;
  return total;
}

// header "Edges": is edge e active, and between which nodes
__device__ __forceinline__ bool pgo_edge_active(const PgoGraph &G, int e, int *i, int *j) {
  *i = -1; *j = -1;
  if (G.ev[e] == 0) return false;
  const int a = G.ei[2 * e], b = G.ei[2 * e + 1];
  if (a == b || a < 0 || a >= G.N || b < 0 || b >= G.N) return false;
  bool finite = true;
  for (int k = 0; k < 9; ++k) finite = finite && fabsf(G.zr[(size_t)e * 9 + k]) < INFINITY;
  for (int k = 0; k < 3; ++k) finite = finite && fabsf(G.zt[(size_t)e * 3 + k]) < INFINITY;
  for (int k = 0; k < 36; ++k) finite = finite && fabsf(G.info[(size_t)e * 36 + k]) < INFINITY;
  if (!finite) return false;
  *i = a; *j = b;
  return true;
}

// plan: eij, start, list, live.  counts = (active edges, fixed nodes, live nodes), the same in every thread.
__device__ void pgo_plan(PgoShared &S, const PgoGraph &G, int *counts) {
  const int t = threadIdx.x;
  int nact = 0;
  for (int e = t; e < G.E; e += PGO_THREADS) {
    int i, j;
    nact += pgo_edge_active(G, e, &i, &j) ? 1 : 0;
    G.eij[2 * e] = i;
    G.eij[2 * e + 1] = j;
  }
  int before;
  counts[0] = pgo_int_sum(S, nact, &before);            // (its barriers publish eij)
  const int chunk = (G.N + PGO_THREADS - 1) / PGO_THREADS, lo = t * chunk, hi = lo + chunk < G.N ? lo + chunk : G.N;
  int mine = 0;
  for (int n = lo; n < hi; ++n)
    for (int e = 0; e < G.E; ++e) mine += (G.eij[2 * e] == n ? 1 : 0) + (G.eij[2 * e + 1] == n ? 1 : 0);
  pgo_int_sum(S, mine, &before);
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
  counts[1] = pgo_int_sum(S, nfixed, &before);
  counts[2] = pgo_int_sum(S, nlive, &before);
  __syncthreads();
}

// the residual of the active edge e = (i, j) at the float32 poses (r, t), its Omega and chi2
__device__ __forceinline__ float pgo_edge_chi2(const PgoGraph &G, const float *r, const float *t, int e, int i, int j, PgoEdge &o,
                                               float *O, float *oe) {
  float ri[9], ti[3], rj[9], tj[3], rz[9], tz[3], info[36];
#pragma unroll
  for (int k = 0; k < 9; ++k) { ri[k] = r[(size_t)i * 9 + k]; rj[k] = r[(size_t)j * 9 + k]; rz[k] = G.zr[(size_t)e * 9 + k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) { ti[k] = t[(size_t)i * 3 + k]; tj[k] = t[(size_t)j * 3 + k]; tz[k] = G.zt[(size_t)e * 3 + k]; }
#pragma unroll
  for (int k = 0; k < 36; ++k) info[k] = G.info[(size_t)e * 36 + k];
  pgo_residual(ri, ti, rj, tj, rz, tz, o);
  pgo_omega(info, O);
  return pgo_chi2(O, o.e, oe);
}

// the cost at (r, t) (header "Cost"), the same in every thread.  eij: the plan's, or nullptr (the activity is then decided here).
template <bool WRITE>
__device__ double pgo_cost_pass(PgoShared &S, const PgoGraph &G, const float *r, const float *t, const int *eij, float *chi2_out,
                                uint8_t *active_out, int *nactive) {
  float acc[2] = {0.0f, 0.0f};
  for (int e = threadIdx.x; e < G.E; e += PGO_THREADS) {
    int i, j;
    if (eij) { i = eij[2 * e]; j = eij[2 * e + 1]; } else pgo_edge_active(G, e, &i, &j);
    float chi2 = 0.0f;
    if (i >= 0) {
      PgoEdge o;
      float O[36], oe[6], w, rho;
      chi2 = pgo_edge_chi2(G, r, t, e, i, j, o, O, oe);
      if (!pgo_rho(chi2, G.huber, &w, &rho)) chi2 = INFINITY;
      acc[0] += rho;
      acc[1] += 1.0f;
    }
    if (WRITE) {
      chi2_out[e] = chi2;
      if (active_out) active_out[e] = i >= 0 ? 1 : 0;
    }
  }
  pgo_block_sum<2>(S, acc);
  *nactive = (int)S.red[1];
  return S.red[0];
}

// linearise at (G.r, G.t): the edge blocks, then D and g of every node (zero unless the node is live)
__device__ void pgo_linearise(const PgoGraph &G) {
  for (int e = threadIdx.x; e < G.E; e += PGO_THREADS) {
    const int i = G.eij[2 * e], j = G.eij[2 * e + 1];
    if (i < 0) continue;
    float *out = G.eb + (size_t)e * PGO_EB;
    PgoEdge o;
    float O[36], oe[6], w, rho;
    const float chi2 = pgo_edge_chi2(G, G.r, G.t, e, i, j, o, O, oe);
    if (!pgo_rho(chi2, G.huber, &w, &rho)) {
      for (int k = 0; k < PGO_EB; ++k) out[k] = 0.0f;
      continue;
    }
    const bool coupled = G.fixed[i] == 0 && G.fixed[j] == 0;
    float Ji[36], Jj[36], A[36];
    pgo_lines(o, Ji, Jj);
    pgo_omega_j(O, Jj, A);
    pgo_jt_a(Jj, A, w, true, out + 36);
    pgo_jt_a(Ji, A, coupled ? w : 0.0f, false, out + PGO_HIJ);
    pgo_omega_j(O, Ji, A);
    pgo_jt_a(Ji, A, w, true, out);
    pgo_jt_v(Ji, oe, w, out + PGO_GI);
    pgo_jt_v(Jj, oe, w, out + PGO_GI + 6);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G.N * 42; idx += PGO_THREADS) {
    const int n = idx / 42, k = idx % 42;
    float s = 0.0f;
    if (G.live[n]) {
      for (int q = G.start[n]; q < G.start[n + 1]; ++q) {
        const int ent = G.list[q], side = ent & 1;
        const float *blk = G.eb + (size_t)(ent >> 1) * PGO_EB;
        s += k < 36 ? blk[side * 36 + k] : blk[PGO_GI + side * 6 + (k - 36)];
      }
    }
    if (k < 36) G.diag[(size_t)n * 36 + k] = s; else G.g[(size_t)n * 6 + (k - 36)] = s;
  }
  __syncthreads();
}

// row c of node n of (H + lambda diag H) p
__device__ __forceinline__ float pgo_ap_row(const PgoGraph &G, const float *p, int n, int c, float lambda) {
  const float *D = G.diag + (size_t)n * 36 + c * 6, *pn = p + 6 * n;
  float acc = pgo_dot6(D, 1, pn, 1);
  acc = acc + (lambda * D[c]) * pn[c];
  for (int q = G.start[n]; q < G.start[n + 1]; ++q) {
    const int ent = G.list[q], e = ent >> 1, side = ent & 1;
    const float *B = G.eb + (size_t)e * PGO_EB + PGO_HIJ, *po = p + 6 * G.eij[2 * e + (1 - side)];
    acc = acc + (side == 0 ? pgo_dot6(B + 6 * c, 1, po, 1) : pgo_dot6(B + c, 6, po, 1));
  }
  return acc;
}

// the damped step (header "Solve"): x = the step of every live node (0 elsewhere) after `trips` PCG trips
__device__ void pgo_pcg(PgoShared &S, const PgoGraph &G, float *x, float *r, float *p, float *q, float lambda, int trips) {
  const int t = threadIdx.x, rows = 6 * G.N;
  for (int n = t; n < G.N; n += PGO_THREADS) {
    double work[27];                                       // (registers: the 6x6 factorisation unrolls whole)
    if (G.live[n]) G.frozen[n] = pgo_block_factor(G.diag + (size_t)n * 36, lambda, G.fac + (size_t)n * 21, work) ? 0 : 1;
  }
  __syncthreads();
  for (int row = t; row < rows; row += PGO_THREADS) {
    const int n = row / 6;
    x[row] = 0.0f;
    p[row] = 0.0f;
    r[row] = (G.live[n] && !G.frozen[n]) ? -G.g[row] : 0.0f;
  }
  __syncthreads();
  float acc[2] = {0.0f, 0.0f};
  for (int n = t; n < G.N; n += PGO_THREADS) {
    float z[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (G.live[n] && !G.frozen[n]) pgo_ldlt_apply(G.fac + (size_t)n * 21, r + 6 * n, z);
#pragma unroll
    for (int k = 0; k < 6; ++k) { q[6 * n + k] = z[k]; p[6 * n + k] = z[k]; }
  }
  __syncthreads();
  for (int row = t; row < rows; row += PGO_THREADS) acc[0] += r[row] * q[row];
  pgo_block_sum<1>(S, acc);
  double rz = S.red[0];
  bool dead = false;
#pragma unroll 1
  for (int trip = 0; trip < trips; ++trip) {
    acc[0] = 0.0f;
    for (int row = t; row < rows; row += PGO_THREADS) {
      const int n = row / 6;
      const float v = (G.live[n] && !G.frozen[n]) ? pgo_ap_row(G, p, n, row - 6 * n, lambda) : 0.0f;
      q[row] = v;
      acc[0] += p[row] * v;
    }
    pgo_block_sum<1>(S, acc);
    const double pap = S.red[0];                          // workgroup-uniform: read after the sum's last barrier
    dead = dead || !(pap > 0.0) || !(pap < INFINITY) || rz == 0.0;
    const float alpha = dead ? 0.0f : (float)(rz / pap);
    for (int row = t; row < rows; row += PGO_THREADS) {
      x[row] = x[row] + alpha * p[row];
      r[row] = r[row] - alpha * q[row];
    }
    __syncthreads();
    for (int n = t; n < G.N; n += PGO_THREADS) {
      float z[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (G.live[n] && !G.frozen[n]) pgo_ldlt_apply(G.fac + (size_t)n * 21, r + 6 * n, z);
#pragma unroll
      for (int k = 0; k < 6; ++k) q[6 * n + k] = z[k];
    }
    __syncthreads();
    acc[0] = 0.0f;
    for (int row = t; row < rows; row += PGO_THREADS) acc[0] += r[row] * q[row];
    pgo_block_sum<1>(S, acc);
    const double rz_new = S.red[0];
    if (!dead) {
      const float beta = (float)(rz_new / rz);
      for (int row = t; row < rows; row += PGO_THREADS) p[row] = q[row] + beta * p[row];
      rz = rz_new;
    }
    __syncthreads();
  }
}

// the candidate: K18's update of every live node's float64 pose by its step, and its float32 rounding
__device__ void pgo_step(const PgoGraph &G, const float *x) {
  for (int n = threadIdx.x; n < G.N; n += PGO_THREADS) {
    double pose[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) pose[c] = G.pose[(size_t)n * 12 + c];
    if (G.live[n] && !G.frozen[n]) {
      double d[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) d[k] = (double)x[6 * n + k];
      icp_update_pose(pose, d);
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      G.cand[(size_t)n * 12 + c] = pose[c];
      if (c < 9) G.cr[(size_t)n * 9 + c] = (float)pose[c]; else G.ct[(size_t)n * 3 + (c - 9)] = (float)pose[c];
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void pgo_stage(const PgoGraph &G, const float *r, const float *t) {
  for (int idx = threadIdx.x; idx < G.N * 12; idx += PGO_THREADS) {
    const int n = idx / 12, c = idx % 12;
    const float v = c < 9 ? r[(size_t)n * 9 + c] : t[(size_t)n * 3 + (c - 9)];
    G.pose[idx] = (double)v;
    if (c < 9) G.r[(size_t)n * 9 + c] = v; else G.t[(size_t)n * 3 + (c - 9)] = v;
  }
  __syncthreads();
}

extern __shared__ __attribute__((aligned(16))) char pgo_lds[];

// ---- K27a ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PGO_THREADS) void pgo_cost_kernel(const float *__restrict__ r, const float *__restrict__ t,
                                                               const int32_t *__restrict__ ei, const float *__restrict__ zr,
                                                               const float *__restrict__ zt, const float *__restrict__ info,
                                                               const uint8_t *__restrict__ ev, int N, int E, float huber,
                                                               float *__restrict__ chi2, float *__restrict__ cost,
                                                               uint8_t *__restrict__ active) {
  PgoShared &S = *reinterpret_cast<PgoShared *>(pgo_lds);
  const size_t b = blockIdx.x;
  const PgoGraph G = pgo_graph(ei, zr, zt, info, ev, nullptr, N, E, huber, nullptr);
  int nact;
  const double c = pgo_cost_pass<true>(S, G, r + b * N * 9, t + b * N * 3, nullptr, chi2 + b * E, active + b * E, &nact);
  if (threadIdx.x == 0) cost[b] = (float)c;
}

// ---- K27b ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PGO_THREADS) void pgo_linearise_kernel(const float *__restrict__ r, const float *__restrict__ t,
                                                                    const int32_t *__restrict__ ei, const float *__restrict__ zr,
                                                                    const float *__restrict__ zt, const float *__restrict__ info,
                                                                    const uint8_t *__restrict__ ev, const uint8_t *__restrict__ fixed,
                                                                    int N, int E, float huber, float *__restrict__ diag,
                                                                    float *__restrict__ off, float *__restrict__ g,
                                                                    float *__restrict__ cost, void *__restrict__ ws) {
  PgoShared &S = *reinterpret_cast<PgoShared *>(pgo_lds);
  const size_t b = blockIdx.x;
  const PgoGraph G = pgo_graph(ei, zr, zt, info, ev, fixed, N, E, huber, ws);
  pgo_stage(G, r + b * N * 9, t + b * N * 3);
  int counts[3], nact;
  pgo_plan(S, G, counts);
  const double c = pgo_cost_pass<false>(S, G, G.r, G.t, G.eij, nullptr, nullptr, &nact);
  pgo_linearise(G);
  for (int idx = threadIdx.x; idx < N * 36; idx += PGO_THREADS) diag[b * N * 36 + idx] = G.diag[idx];
  for (int idx = threadIdx.x; idx < N * 6; idx += PGO_THREADS) g[b * N * 6 + idx] = G.g[idx];
  for (int idx = threadIdx.x; idx < E * 36; idx += PGO_THREADS) {
    const int e = idx / 36;
    off[b * E * 36 + idx] = G.eij[2 * e] >= 0 ? G.eb[(size_t)e * PGO_EB + PGO_HIJ + idx % 36] : 0.0f;
  }
  if (threadIdx.x == 0) cost[b] = (float)c;
}

// ---- K27c ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PGO_THREADS) void pgo_refine_kernel(const float *__restrict__ r0, const float *__restrict__ t0,
                                                                 const int32_t *__restrict__ ei, const float *__restrict__ zr,
                                                                 const float *__restrict__ zt, const float *__restrict__ info,
                                                                 const uint8_t *__restrict__ ev, const uint8_t *__restrict__ fixed,
                                                                 int N, int E, int iterations, int trips, float huber,
                                                                 float *__restrict__ r_out, float *__restrict__ t_out,
                                                                 float *__restrict__ chi2_out, float *__restrict__ cost0_out,
                                                                 float *__restrict__ cost_out, int *__restrict__ accepted_out,
                                                                 float *__restrict__ info_out, uint8_t *__restrict__ ok_out,
                                                                 void *__restrict__ ws) {
  PgoShared &S = *reinterpret_cast<PgoShared *>(pgo_lds);
  float *x = reinterpret_cast<float *>(pgo_lds + PGO_SHARED_BYTES), *rr = x + 6 * N, *p = rr + 6 * N, *q = p + 6 * N;
  const size_t b = blockIdx.x;
  const int t = threadIdx.x;
  const PgoGraph G = pgo_graph(ei, zr, zt, info, ev, fixed, N, E, huber, ws);
  pgo_stage(G, r0 + b * N * 9, t0 + b * N * 3);
  int counts[3], nact, accepted = 0;
  pgo_plan(S, G, counts);
  double cost0 = pgo_cost_pass<false>(S, G, G.r, G.t, G.eij, nullptr, nullptr, &nact);
  double cost = cost0;
  const bool refused = !(cost0 < INFINITY) || counts[0] == 0 || counts[1] == 0 || counts[2] == 0;   // the same in every thread
  if (!refused) {
    double lambda = BA_LAMBDA0;
    bool stale = true;                                     // the blocks in the workspace are not those of the state
#pragma unroll 1
    for (int it = 0; it < iterations; ++it) {
      if (stale) pgo_linearise(G);
      stale = false;
      pgo_pcg(S, G, x, rr, p, q, (float)lambda, trips);
      pgo_step(G, x);
      const double c = pgo_cost_pass<false>(S, G, G.cr, G.ct, G.eij, nullptr, nullptr, &nact);
      if (c < INFINITY && c < cost) {
        for (int idx = t; idx < N * 12; idx += PGO_THREADS) G.pose[idx] = G.cand[idx];
        for (int idx = t; idx < N * 9; idx += PGO_THREADS) G.r[idx] = G.cr[idx];
        for (int idx = t; idx < N * 3; idx += PGO_THREADS) G.t[idx] = G.ct[idx];
        cost = c;
        ++accepted;
        stale = true;
        lambda = lambda / BA_LAMBDA_STEP > BA_LAMBDA_MIN ? lambda / BA_LAMBDA_STEP : BA_LAMBDA_MIN;
      } else {
        lambda = lambda * BA_LAMBDA_STEP < BA_LAMBDA_MAX ? lambda * BA_LAMBDA_STEP : BA_LAMBDA_MAX;
      }
      __syncthreads();
    }
    if (stale) pgo_linearise(G);
    pgo_cost_pass<true>(S, G, G.r, G.t, G.eij, chi2_out + b * E, nullptr, &nact);
  } else {
    cost0 = counts[0] == 0 ? 0.0 : INFINITY;
    cost = cost0;
    for (int e = t; e < E; e += PGO_THREADS) chi2_out[b * E + e] = 0.0f;
  }
  for (int idx = t; idx < N * 36; idx += PGO_THREADS) info_out[b * N * 36 + idx] = refused ? 0.0f : G.diag[idx];
  for (int idx = t; idx < N * 9; idx += PGO_THREADS) r_out[b * N * 9 + idx] = G.r[idx];
  for (int idx = t; idx < N * 3; idx += PGO_THREADS) t_out[b * N * 3 + idx] = G.t[idx];
  if (t == 0) {
    cost0_out[b] = (float)cost0;
    cost_out[b] = (float)cost;
    accepted_out[b] = accepted;
    ok_out[b] = refused ? 0 : 1;
  }
}

int pgo_shape_status(int batch, int nodes, int edges) {
  if (batch < 1 || nodes < 2 || edges < 1) return MI_E_SHAPE;
  if (batch > 65535 || nodes > MI_PGO_MAX_NODES || edges > MI_PGO_MAX_EDGES) return MI_E_PARAM;
  return MI_OK;
}
bool pgo_huber_ok(float huber) { return huber >= 0.0f && huber < INFINITY; }
int pgo_workspace_status(const void *workspace, size_t bytes, int batch, int nodes, int edges) {
  if (((uintptr_t)workspace % 16) != 0) return MI_E_ALIGN;
  if (bytes < mi_pgo_workspace_bytes(batch, nodes, edges)) return MI_E_CAPACITY;
  return MI_OK;
}
size_t pgo_lds_bytes(int nodes) { return PGO_SHARED_BYTES + (size_t)4 * 6 * nodes * sizeof(float); }

}  // namespace

extern "C" size_t mi_pgo_workspace_bytes(int batch, int nodes, int edges) {
  if (pgo_shape_status(batch, nodes, edges) != MI_OK) return 0;
  return (size_t)batch * pgo_layout(nodes, edges).total;
}

extern "C" int mi_pgo_cost(const float *r, const float *t, const int32_t *edge_index, const float *zr, const float *zt,
                           const float *info, const uint8_t *edge_valid, int batch, int nodes, int edges, float huber, float *chi2,
                           float *cost, uint8_t *active, mi_stream_t stream) {
  MI_ENTER();
  if (!r || !t || !edge_index || !zr || !zt || !info || !edge_valid || !chi2 || !cost || !active) return MI_E_NULL;
  if (const int s = pgo_shape_status(batch, nodes, edges)) return s;
  if (!pgo_huber_ok(huber)) return MI_E_PARAM;
  hipLaunchKernelGGL(pgo_cost_kernel, dim3((unsigned)batch), dim3(PGO_THREADS), PGO_SHARED_BYTES, (hipStream_t)stream, r, t,
                     edge_index, zr, zt, info, edge_valid, nodes, edges, huber, chi2, cost, active);
  return mi_launch_status();
}

extern "C" int mi_pgo_linearise(const float *r, const float *t, const int32_t *edge_index, const float *zr, const float *zt,
                                const float *info, const uint8_t *edge_valid, const uint8_t *fixed, int batch, int nodes, int edges,
                                float huber, float *diag, float *off, float *g, float *cost, void *workspace,
                                size_t workspace_bytes, mi_stream_t stream) {
  MI_ENTER();
  if (!r || !t || !edge_index || !zr || !zt || !info || !edge_valid || !fixed || !diag || !off || !g || !cost || !workspace)
    return MI_E_NULL;
  if (const int s = pgo_shape_status(batch, nodes, edges)) return s;
  if (!pgo_huber_ok(huber)) return MI_E_PARAM;
  if (const int s = pgo_workspace_status(workspace, workspace_bytes, batch, nodes, edges)) return s;
  hipLaunchKernelGGL(pgo_linearise_kernel, dim3((unsigned)batch), dim3(PGO_THREADS), PGO_SHARED_BYTES, (hipStream_t)stream, r, t,
                     edge_index, zr, zt, info, edge_valid, fixed, nodes, edges, huber, diag, off, g, cost, workspace);
  return mi_launch_status();
}

extern "C" int mi_pgo_refine(const float *r0, const float *t0, const int32_t *edge_index, const float *zr, const float *zt,
                             const float *info, const uint8_t *edge_valid, const uint8_t *fixed, int batch, int nodes, int edges,
                             int iterations, int pcg_iterations, float huber, float *r, float *t, float *chi2, float *cost0,
                             float *cost, int32_t *accepted, float *info_out, uint8_t *ok, void *workspace, size_t workspace_bytes,
                             mi_stream_t stream) {
  MI_ENTER();
  if (!r0 || !t0 || !edge_index || !zr || !zt || !info || !edge_valid || !fixed || !r || !t || !chi2 || !cost0 || !cost ||
      !accepted || !info_out || !ok || !workspace)
    return MI_E_NULL;
  if (const int s = pgo_shape_status(batch, nodes, edges)) return s;
  if (iterations < 1 || iterations > MI_PGO_MAX_ITERATIONS || pcg_iterations < 1 || pcg_iterations > MI_PGO_MAX_PCG ||
      !pgo_huber_ok(huber))
    return MI_E_PARAM;
  if (const int s = pgo_workspace_status(workspace, workspace_bytes, batch, nodes, edges)) return s;
  const size_t lds = pgo_lds_bytes(nodes);
  static size_t allowed = 64 * 1024;                     // raised once, to what the node cap needs (place.hip's pattern)
  if (lds > allowed) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pgo_refine_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)pgo_lds_bytes(MI_PGO_MAX_NODES));
    if (e != hipSuccess) return (int)e;
    allowed = pgo_lds_bytes(MI_PGO_MAX_NODES);
  }
  hipLaunchKernelGGL(pgo_refine_kernel, dim3((unsigned)batch), dim3(PGO_THREADS), lds, (hipStream_t)stream, r0, t0, edge_index, zr,
                     zt, info, edge_valid, fixed, nodes, edges, iterations, pcg_iterations, huber, r, t, chi2, cost0, cost, accepted,
                     info_out, ok, workspace);
  return mi_launch_status();
}
