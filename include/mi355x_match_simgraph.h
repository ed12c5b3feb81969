/* mi355x_match_simgraph.h -- the similarity pose-graph section (K31) of the C ABI, with a header and a library of its own, as
 * K30's: libmi355x_match_simgraph.so exports exactly the MI_API declarations below, under the conventions (return values,
 * MI_E_*, mi_stream_t, ABI version) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the export
 * of that header and nothing else.  The Python binding reads it next to the others (onnx_image_processing_amd/_native.py,
 * SIMGRAPH_SIGNATURES, SIMGRAPH_CONSTANTS, load_simgraph()). */
#ifndef MI355X_MATCH_SIMGRAPH_H
#define MI355X_MATCH_SIMGRAPH_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Sim(3) pose-graph optimisation (K31): a 7-DoF loop constraint moves and RESCALES the whole trajectory -------------------
 * K26 finds the old keyframe a new frame shows and K30 turns the landmarks round the two into a similarity X2 = s R X1 + t.
 * In a monocular map that s is not 1: the unit has drifted round the loop.  K27's nodes carry no scale and can only tear the
 * trajectory to fit the rotation and translation; this section is K27 with a scale per node -- ORB-SLAM's
 * OptimizeEssentialGraph, g2o's VertexSim3Expmap / EdgeSim3 on the host -- and the map correction that follows it.  The
 * algorithm is K27's ("pose-graph optimisation" in include/mi355x_match.h) with 6 -> 7 wherever a node's degrees of freedom
 * appear; what is stated here is what differs, and every rule not restated is K27's, word for word: Threads (256 per graph,
 * the fixed-order sums: each thread's float32 partial sum over e = tid, tid + 256, ..., wave_sum_dpp over each wave, the four
 * waves added in wave order in float64), Log, Cost and Huber on chi = sqrt(chi2), System (per-node sums in ascending edge
 * index), Solve (block-Jacobi PCG, exactly pcg_iterations trips, the workgroup-uniform `dead` flag, every barrier reached by
 * every thread on every trip), Loop (K25's lambda schedule, no early stop) and Refusal.  Entries under K27's contract: pure
 * functions of their arguments, no allocation, no synchronisation, no memset, one stream, no atomics, every sum in a fixed
 * order (the same inputs give the same bits, alone or inside a batch), capturable into a hipGraph; outputs and workspace may
 * hold anything on entry, every output element is written and outputs alias nothing; MI_E_* before any launch, in the order
 * NULL, shape, parameters, alignment, capacity.
 *
 * State.  N nodes with s (batch, N), r (batch, N, 3, 3), t (batch, N, 3) float32: X_c = s R X + t, s the node's unit relative
 *   to the world's (1 for a metric pose: then this is K27's node).  fixed (batch, N) bytes: non-zero = all 7 degrees of
 *   freedom of the node are held.  2 <= N <= MI_SIMGRAPH_MAX_NODES, 1 <= E <= MI_SIMGRAPH_MAX_EDGES (below: MI_E_SHAPE, as
 *   batch < 1; above: MI_E_PARAM, as batch > 65535).  huber < 0 or not finite: MI_E_PARAM.
 * Edges.  edge_index (batch, E, 2) int32 (i, j); zs (batch, E), zr (batch, E, 3, 3), zt (batch, E, 3) float32: the measured
 *   similarity X_j = s_z R_z X_i + t_z -- what mi_sim3_ransac returns for (frame 1 = i, frame 2 = j), and what two current
 *   poses give for an odometry or covisibility edge (scale 1 for metric poses); info (batch, E, 7, 7) float32 in (rotation,
 *   translation, log-scale) order: Omega_rc = info[min(r, c), max(r, c)], only the upper triangle enters the arithmetic;
 *   edge_valid (batch, E) bytes.  An edge is INACTIVE when its byte is 0, i == j, an index lies outside [0, N), one of the
 *   1 + 9 + 3 + 49 numbers of zs, zr, zt, info is not finite, or zs is not above 0.  An inactive edge is read no further, adds
 *   nothing and reports chi2 = 0.  A node is LIVE when it is not fixed and has an active edge.
 * dot7(a, b) = (((((a0 b0 + a1 b1) + a2 b2) + a3 b3) + a4 b4) + a5 b5) + a6 b6.
 * Residual (float32, at the float32 state).  R_p = R_j R_i^T, s_p = s_j / s_i, w = R_p t_i, t_p = t_j - s_p w;
 *   R_d = R_p R_z^T, s_d = s_p / s_z, u = s_d (R_d t_z), t_d = t_p - u (3x3 products and R x as ((a0 b0 + a1 b1) + a2 b2));
 *   e = (Log R_d, t_d, log s_d) with K27's Log and logf.  These are the coordinates of the update below.  A node scale that
 *   is not positive makes log s_d not finite (or NaN): the edge's chi2 is +inf, the initial cost is not finite and the graph
 *   is refused -- there is no separate rule.  (Two NEGATIVE scales at the two ends of every edge they touch would cancel in
 *   s_p; the entries do not look for that.)
 * Update (left, 7-vector (w, tau, sigma)): R <- Exp(w) R, s <- exp(sigma) s, t <- exp(sigma) (Exp(w) t) + tau; formed in
 *   float64 on the float64 state (Exp is K18's, each row of Exp(w) R and Exp(w) t as ((a0 b0 + a1 b1) + a2 b2)).
 * Jacobians (float32).  Exact to first order in the left perturbation of node i and of node j, 7x7, with J_l^-1 at
 *   phi = Log R_d (K27's):
 *       J_j = [[ J_l^-1,     0,         0   ],        J_i = [[ -J_l^-1 R_p,   0,          0  ],
 *              [ -[t_d]x,    I,         t_d ],               [ -[u]x R_p,     -s_p R_p,   u  ],
 *              [ 0,          0,         1   ]]               [ 0,             0,          -1 ]]
 *   At s = 1 everywhere the upper-left 6x6 blocks are K27's lines.  tests/test_simgraph_host.py holds them against central
 *   differences of the residual on both sides, over all 7 coordinates, at scales from 0.2 to 5.
 * Blocks, per active edge with a finite chi2 (an edge with chi2 = +inf adds zeros): A_i = Omega J_i, A_j = Omega J_j
 *   (A_rc = dot7 over k of Omega_rk J_kc);  H_ii = w J_i^T A_i, H_jj = w J_j^T A_j, H_ij = w J_i^T A_j (each element w times
 *   dot7 over k; the upper triangles of H_ii and H_jj are computed and mirrored);  g_i = w J_i^T oe, g_j = w J_j^T oe.
 *   H_ij = 0 when i or j is fixed.  3 x 49 + 14 = 161 workspace floats per edge.
 * Solve.  K27's with 7x7 blocks: M_n = D_n with the diagonal D_rr + lambda D_rr in float64, factored L D L^T by K25's column
 *   algorithm under K18's pivot rule, the 28 factors rounded to float32; a node that fails is FROZEN for the step.  The PCG
 *   vectors x, r, p, q are 4 x 7N floats of dynamic LDS: 112 KB at the node cap.
 * Refusal.  K27's: the initial cost is not finite, there is no active edge, no fixed node, or no live node.
 * A long chain with few closures needs pcg_iterations of the order of its length, as K27's. */
#define MI_SIMGRAPH_MAX_NODES 1024
#define MI_SIMGRAPH_MAX_EDGES 4096
#define MI_SIMGRAPH_MAX_ITERATIONS 32
#define MI_SIMGRAPH_MAX_PCG 256
#define MI_SIMGRAPH_MAX_ROWS 16777216

/* Cost alone, the outlier test between rounds: chi2 (batch, E) float32, the unweighted chi2 of every active edge (+inf where
 * it is not finite) and 0 for an inactive one; cost (batch) float32; active (batch, E) bytes.  One launch. */
MI_API int mi_simgraph_cost(const float *s, const float *r, const float *t, const int32_t *edge_index, const float *zs,
                            const float *zr, const float *zt, const float *info, const uint8_t *edge_valid, int batch, int nodes,
                            int edges, float huber, float *chi2, float *cost, uint8_t *active, mi_stream_t stream);

/* Workspace of mi_simgraph_linearise and mi_simgraph_refine: per graph the float64 state and candidate (13 doubles per node),
 * their float32 roundings, the plan (edge ends, list offsets, lists), D, g and the factors per node and 161 floats per edge,
 * every array rounded up to 16 bytes; 0 for an unsupported shape.  16-byte aligned (MI_E_ALIGN), any content; shorter:
 * MI_E_CAPACITY. */
MI_API size_t mi_simgraph_workspace_bytes(int batch, int nodes, int edges);

/* One undamped linearisation at the given state: diag (batch, N, 7, 7) float32, D_n, zero for a fixed or edgeless node; off
 * (batch, E, 7, 7), H_ij, zero for an inactive edge and an edge that touches a fixed node; g (batch, N, 7); cost (batch).
 * One launch. */
MI_API int mi_simgraph_linearise(const float *s, const float *r, const float *t, const int32_t *edge_index, const float *zs,
                                 const float *zr, const float *zt, const float *info, const uint8_t *edge_valid,
                                 const uint8_t *fixed, int batch, int nodes, int edges, float huber, float *diag, float *off,
                                 float *g, float *cost, void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* The whole loop in one launch.  1 <= iterations <= MI_SIMGRAPH_MAX_ITERATIONS, 1 <= pcg_iterations <= MI_SIMGRAPH_MAX_PCG
 * (MI_E_PARAM).  s (batch, N), r (batch, N, 3, 3), t (batch, N, 3): the final state (a node that is not live is its input's
 * bits); chi2 (batch, E): the unweighted chi2 of mi_simgraph_cost at the result; cost0, cost (batch) float32: the cost at the
 * input and at the result; accepted (batch) int32: the number of accepted steps; info_out (batch, N, 7, 7): diag of
 * mi_simgraph_linearise at the result, bit for bit -- the CONDITIONAL information of each node given its neighbours, not the
 * marginal; ok (batch) bytes.  A refused graph: ok = 0, the state equals the inputs, chi2 = 0, accepted = 0, info_out = 0,
 * cost0 = cost = +inf (0 when no edge is active). */
MI_API int mi_simgraph_refine(const float *s0, const float *r0, const float *t0, const int32_t *edge_index, const float *zs,
                              const float *zr, const float *zt, const float *info, const uint8_t *edge_valid, const uint8_t *fixed,
                              int batch, int nodes, int edges, int iterations, int pcg_iterations, float huber, float *s, float *r,
                              float *t, float *chi2, float *cost0, float *cost, int32_t *accepted, float *info_out, uint8_t *ok,
                              void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* The map correction after the optimisation (ORB-SLAM's CorrectLoop tail): the keyframes were metric poses r_old (batch, N, 3,
 * 3), t_old (batch, N, 3) (X_c = R_old X + t_old) before; (s, r, t) (batch, N ...) is the optimised state (s', R', t'); points
 * (batch, L, 3) are landmarks of the old map and ref (batch, L) int32 the keyframe each one is attached to.  Poses come back
 * metric: r_out = R', t_out = t' / s'.  A landmark keeps its place in its reference keyframe's camera, in the new unit:
 * points_out = R'^T ((R_old X + t_old) - t') / s' with the reference node's poses, so that r_out X' + t_out = (R_old X +
 * t_old) / s': the camera sees the same ray, the depth scaled by 1 / s'.  A landmark whose ref lies outside [0, N) is copied
 * unchanged, bit for bit.  Every element is formed in float64 from the float32 inputs, widened exactly, and rounded to float32
 * once:  t_out_a = t'_a / s';  Y_a = ((R_old,a0 X_0 + R_old,a1 X_1) + R_old,a2 X_2) + t_old,a;  d_a = Y_a - t'_a;
 * X'_c = ((R'_0c d_0 + R'_1c d_1) + R'_2c d_2) / s'.  s' is not examined.  N or L may be 0 (then its arrays may be NULL), not
 * both; batch < 1, a negative count or both 0: MI_E_SHAPE; batch > 65535 or N + L > MI_SIMGRAPH_MAX_ROWS: MI_E_PARAM.  With
 * N = 0 no pose array is read and every landmark is copied.  Outputs alias no input.  One thread per node or landmark, one
 * launch. */
MI_API int mi_simgraph_correct(const float *r_old, const float *t_old, const float *s, const float *r, const float *t,
                               const float *points, const int32_t *ref, int batch, int nodes, int landmarks, float *r_out,
                               float *t_out, float *points_out, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_SIMGRAPH_H */
