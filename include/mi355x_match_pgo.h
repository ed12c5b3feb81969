/* mi355x_match_pgo.h -- the pose-graph section (K27) of the C ABI, with a header and a library of its own:
 * libmi355x_match_pgo.so exports exactly the MI_API declarations below, under the conventions (return values, MI_E_*,
 * mi_stream_t, ABI version 3) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the export of
 * that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * EXTRA_SIGNATURES, load_pgo()). */
#ifndef MI355X_MATCH_PGO_H
#define MI355X_MATCH_PGO_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pose-graph optimisation (K27): odometry edges and loop edges move the whole trajectory so that the loop closes -----------
 * K26 finds the old keyframe a new frame shows, K15 / K17 / K18 / K21 / K23 / K24 turn the pair into a relative pose with a
 * 6x6 information matrix, K25 refines a window.  This section takes those edges and optimises every pose of the graph:
 * Levenberg-Marquardt, each damped step solved by a fixed number of preconditioned conjugate-gradient trips with the
 * block-Jacobi preconditioner, `batch` independent graphs per call (one per loop candidate of K26, say), one workgroup
 * each.  The host calls users would reach for are g2o or GTSAM.  Four entries under the contract of the K15 / K23 / K25
 * sections: pure functions of their arguments, no allocation, no synchronisation, no memset, one stream, no atomics, every
 * sum in a fixed order (the same inputs give the same bits, alone or inside a batch), capturable into a hipGraph; outputs
 * and workspace may hold anything on entry, every output element is written and outputs alias nothing; MI_E_* before any
 * launch.
 *
 * State.  N nodes with poses r (batch, N, 3, 3), t (batch, N, 3) float32, X_c = R X + t (K23's convention).  fixed (batch, N)
 *   bytes: non-zero = the node is held (the gauge; a map's keyframes in relocalisation).  2 <= N <= MI_PGO_MAX_NODES,
 *   1 <= E <= MI_PGO_MAX_EDGES (below: MI_E_SHAPE, as batch < 1; above: MI_E_PARAM, as batch > 65535).  huber < 0 or not
 *   finite: MI_E_PARAM.
 * Edges.  edge_index (batch, E, 2) int32 (i, j); zr (batch, E, 3, 3), zt (batch, E, 3) float32: the measured motion X_j =
 *   R_z X_i + t_z, what RgbdPoseEstimator, DenseRgbdRefiner, DirectRgbdRefiner and AbsolutePoseEstimator.forward_rgbd return
 *   for (frame 1 = i, frame 2 = j); info (batch, E, 6, 6) float32 in (rotation, translation) order: Omega_rc = info[min(r, c),
 *   max(r, c)], only the upper triangle enters the arithmetic; edge_valid (batch, E) bytes.  An edge is INACTIVE when its
 *   byte is 0, i == j, an index lies outside [0, N), or one of the 9 + 3 + 36 numbers of zr, zt, info is not finite.  An
 *   inactive edge is read no further, adds nothing and reports chi2 = 0: the padding of a ragged batch.  A node is LIVE
 *   when it is not fixed and has an active edge.
 * Threads.  256 per graph.  A sum "over the edges" (or over the 6N rows of a vector) is: each thread's float32 partial sum
 *   over e = tid, tid + 256, ... in that order, wave_sum_dpp over the 64 lanes of each wave, then the four waves' sums added
 *   in wave order in float64 starting from 0.  dot6(a, b) = ((((a0 b0 + a1 b1) + a2 b2) + a3 b3) + a4 b4) + a5 b5.
 * Residual (float32, at the float32 poses).  R_p = R_j R_i^T, t_p = t_j - R_p t_i; R_d = R_p R_z^T, u = R_d t_z, t_d = t_p - u
 *   (3x3 products and R x as ((a0 b0 + a1 b1) + a2 b2)); e = (Log R_d, t_d): the coordinates of K18's update (R <- Exp(w) R,
 *   t <- Exp(w) t + tau), in which K18 / K21 / K23 express their information matrices.
 * Log.  v = vee(R - R^T) / 2, s = |v|, c = (trace R - 1) / 2, theta = atan2(s, c).  c >= -0.9: phi = (theta / s) v, and
 *   (1 + s^2 / 6) v where s < 1e-4.  c < -0.9 (theta above 154 degrees, where s -> 0 loses the axis): the axis from the
 *   symmetric part -- m the largest diagonal element of R, a_m = sqrt((R_mm - c) / (1 - c)), a_n = (R_mn + R_nm) /
 *   (2 (1 - c) a_m) -- with the sign of a . v, phi = theta a.  The branch is continuous up to pi; AT pi, v = 0 decides no
 *   sign and phi = +pi a (the rotation by -pi a is the same one).  The linearisation of Log has no limit at pi (J_l^-1
 *   stays finite there, k -> 1 / pi^2, but the residual jumps from pi a to -pi a): an edge does not converge across it.
 * Cost.  oe = Omega e (oe_r = dot6(Omega_r, e)), chi2 = dot6(e, oe).  chi = sqrt(chi2); with huber > 0 and chi > huber:
 *   rho = (2 huber) chi - huber huber and w = huber / chi; otherwise rho = chi2, w = 1.  An edge whose chi2 is not finite has
 *   chi2 = rho = +inf.  cost = the sum of rho over the edges (above; inactive edges add 0), a float64, returned rounded to
 *   float32.  Nothing active: 0.
 * Jacobians (float32).  Exact to first order in the left perturbation of node i and of node j:
 *       J_j = [[J_l^-1, 0], [-[t_d]x, I]],   J_i = [[-J_l^-1 R_p, 0], [-[u]x R_p, -R_p]]
 *   with J_l^-1 = I - [phi]x / 2 + k ([phi] [phi]^T - theta^2 I) at phi = Log R_d, k = (1 - (theta / 2) cos(theta / 2) /
 *   sin(theta / 2)) / theta^2, and k = (1/12 + theta^2 / 720) + theta^4 / 30240 where theta^2 < 1/16.
 * Blocks, per active edge with a finite chi2 (an edge with chi2 = +inf adds zeros).  A_i = Omega J_i, A_j = Omega J_j
 *   (A_rc = dot6 over k of Omega_rk J_kc);  H_ii = w J_i^T A_i, H_jj = w J_j^T A_j, H_ij = w J_i^T A_j (each element w times
 *   dot6 over k; the upper triangles of H_ii and H_jj are computed and mirrored);  g_i = w J_i^T oe, g_j = w J_j^T oe.
 *   H_ij = 0 when i or j is fixed.
 * System.  Per live node n: D_n and g_n = the float32 sums of H_ii or H_jj (g_i or g_j) over the node's active edges IN
 *   ASCENDING EDGE INDEX, starting from 0; every other node has D = 0, g = 0.
 * Solve, of (H + lambda diag H) dx = -g with lambda rounded to float32.  Per live node M_n = D_n with the diagonal D_rr +
 *   lambda D_rr in float64, factored L D L^T by K25's column algorithm under K18's pivot rule (max diag M_n > 0, every pivot
 *   above 1e-6 max diag M_n and finite), the factors rounded to float32; a node that fails is FROZEN for this step (dx_n =
 *   0, it acts as fixed).  z = M^-1 r per node, float32: y = r, y_k -= l_ki y_i for i ascending, z_k = y_k / d_k, z_k -=
 *   l_ik z_i for i descending.  Vectors are float32 and 0 outside the live, unfrozen nodes.  x = 0, r = -g, z = M^-1 r,
 *   p = z, rz = r . z.  Exactly pcg_iterations trips, no residual test:
 *       (A p)_row = dot6(D_row, p_n), + (lambda D_rr) p_r, then + dot6 of the row of H_ij (of H_ij^T on side j) with p of
 *       the other end, over the node's edges in ascending edge index;
 *       pAp = p . A p;  dead <- dead or not (pAp > 0) or pAp not finite or rz == 0;  alpha = dead ? 0 : (float)(rz / pAp);
 *       x += alpha p, r -= alpha A p, z = M^-1 r, rz' = r . z;  unless dead: p = z + (float)(rz' / rz) p, rz = rz'.
 *   Every dot product is a sum over the 6N rows (above) into float64.  `dead` is a workgroup-uniform value read after a
 *   barrier, and every barrier is reached by every thread on every trip; once dead every later trip changes nothing.
 * Step.  K18's update of the float64 pose of every live, unfrozen node with dx_n, rounded to float32 for every line.
 * Loop.  K25's: lambda = 1e-4 (float64).  `iterations` times: linearise at the state, solve with lambda, step to a candidate,
 *   evaluate its cost; when that is finite and strictly lower (float64 sums compared), the candidate becomes the state and
 *   lambda <- max(lambda / 10, 1e-9); otherwise lambda <- min(10 lambda, 1e6).  Never stops early.
 * Refusal.  The initial cost is not finite, there is no active edge, no fixed node, or no live node.
 * A long chain with few closures needs pcg_iterations of the order of its length: block-Jacobi PCG moves information one
 * edge per trip and does not shorten a chain's diameter. */
#define MI_PGO_MAX_NODES 1024
#define MI_PGO_MAX_EDGES 4096
#define MI_PGO_MAX_ITERATIONS 32
#define MI_PGO_MAX_PCG 256

/* Cost alone, the outlier test between rounds: chi2 (batch, E) float32, the unweighted chi2 of every active edge (+inf
 * where it is not finite) and 0 for an inactive one; cost (batch) float32; active (batch, E) bytes.  One launch. */
MI_API int mi_pgo_cost(const float *r, const float *t, const int32_t *edge_index, const float *zr, const float *zt,
                       const float *info, const uint8_t *edge_valid, int batch, int nodes, int edges, float huber, float *chi2,
                       float *cost, uint8_t *active, mi_stream_t stream);

/* Workspace of mi_pgo_linearise and mi_pgo_refine: per graph the float64 state and candidate, their float32 roundings, the
 * plan (edge ends, list offsets, lists), D, g and the factors per node and 120 floats per edge, every array rounded up to
 * 16 bytes; 0 for an unsupported shape.  16-byte aligned (MI_E_ALIGN), any content; shorter: MI_E_CAPACITY. */
MI_API size_t mi_pgo_workspace_bytes(int batch, int nodes, int edges);

/* One undamped linearisation at the given state: diag (batch, N, 6, 6) float32, D_n, zero for a fixed or edgeless node;
 * off (batch, E, 6, 6), H_ij, the (i, j) block, zero for an inactive edge and an edge that touches a fixed node; g
 * (batch, N, 6); cost (batch).  One launch. */
MI_API int mi_pgo_linearise(const float *r, const float *t, const int32_t *edge_index, const float *zr, const float *zt,
                            const float *info, const uint8_t *edge_valid, const uint8_t *fixed, int batch, int nodes, int edges,
                            float huber, float *diag, float *off, float *g, float *cost, void *workspace, size_t workspace_bytes,
                            mi_stream_t stream);

/* The whole loop in one launch.  1 <= iterations <= MI_PGO_MAX_ITERATIONS, 1 <= pcg_iterations <= MI_PGO_MAX_PCG
 * (MI_E_PARAM).  r (batch, N, 3, 3), t (batch, N, 3): the final state (a node that is not live is its input's bits);
 * chi2 (batch, E): the unweighted chi2 of mi_pgo_cost at the result; cost0, cost (batch) float32: the cost at the input and
 * at the result; accepted (batch) int32: the number of accepted steps; info_out (batch, N, 6, 6): diag of mi_pgo_linearise at
 * the result, bit for bit -- the CONDITIONAL information of each node given its neighbours, not the marginal; ok (batch)
 * bytes.  A refused graph: ok = 0, the poses equal the inputs, chi2 = 0, accepted = 0, info_out = 0, cost0 = cost = +inf
 * (0 when no edge is active). */
MI_API int mi_pgo_refine(const float *r0, const float *t0, const int32_t *edge_index, const float *zr, const float *zt,
                         const float *info, const uint8_t *edge_valid, const uint8_t *fixed, int batch, int nodes, int edges,
                         int iterations, int pcg_iterations, float huber, float *r, float *t, float *chi2, float *cost0,
                         float *cost, int32_t *accepted, float *info_out, uint8_t *ok, void *workspace, size_t workspace_bytes,
                         mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_PGO_H */
