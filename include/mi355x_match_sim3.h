/* mi355x_match_sim3.h -- the similarity-alignment section (K30) of the C ABI, with a header and a library of its own:
 * libmi355x_match_sim3.so exports exactly the MI_API declarations below, under the conventions (return values, MI_E_*,
 * mi_stream_t, ABI version) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the export of
 * that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * SIM3_SIGNATURES, SIM3_CONSTANTS, load_sim3()). */
#ifndef MI355X_MATCH_SIM3_H
#define MI355X_MATCH_SIM3_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- similarity alignment (K30): 3-D to 3-D landmark correspondences -> the similarity between two maps ---------------------
 * K15 returns a translation of unit length and K25 / K28 work on windows that each end in a gauge and a SCALE of their own;
 * K17 solves X2 = R X1 + t, "no scale".  This section relates two maps whose units differ -- two bundle-adjustment windows of
 * a monocular sequence, the landmarks round a loop candidate against those round the current keyframe, two sessions, an
 * estimated trajectory against a reference one -- by X2 = s R X1 + t from 3-point RANSAC (ORB-SLAM's Sim3Solver).  Entries
 * under the contract of the K15 / K17 sections of include/mi355x_match.h: pure functions of their arguments, no allocation,
 * no synchronisation, no memset, one stream, no atomics, every sum in a fixed order (the same inputs and seed give the same
 * bits, alone or inside a batch), capturable into a hipGraph; outputs and workspace may hold anything on entry and every
 * output element is written; MI_E_* before any launch.
 * Row i of pair b is pts1[b][i] <-> pts2[b][i], (batch, n, 3) float32; `valid` / `mask` (batch, n) bytes select rows
 * (non-zero = use; valid may be NULL: every row).  Rows that are not selected are never read for their coordinates.
 * 1 <= n <= MI_SIM3_MAX_N (a staged row is K17's, 24 bytes: 48 KB of rows and 4 KB of indices in LDS; the second kernel of
 * mi_sim3_ransac adds 4 KB of flags), batch <= 65535 (MI_E_PARAM beyond; < 1: MI_E_SHAPE).  Order of the checks: NULL, shape,
 * parameters (the metric after the threshold, before refine_rounds), alignment, capacity.
 *
 * Divergences from ORB-SLAM's Sim3Solver, all deliberate:
 *   - NO NON-LINEAR REFINEMENT follows (ORB-SLAM runs OptimizeSim3 on the result): refinement is refine_rounds rounds of
 *     closed-form refit on the inliers, as K17's;
 *   - the best hypothesis is the one of minimum truncated cost (MSAC), not of maximum inlier count; a fixed number of
 *     hypotheses, no adaptive stop; the sampler is K15's stateless counter-based hash;
 *   - the scale is Umeyama's one-sided form num / den below (ORB-SLAM's, with its fixed-scale switch left out), refused
 *     outside [MI_SIM3_MIN_SCALE, MI_SIM3_MAX_SCALE];
 *   - the reprojection test is on normalised coordinates with ONE threshold for both frames (ORB-SLAM: pixels, a threshold per
 *     point from its octave's sigma).
 *
 * Model.  X2 = s R X1 + t, stored as 13 floats: R row-major, then t, then s.
 * Sampling.  K17's ("metric RGB-D pose": Sampling), unchanged: three distinct ranks.
 * Rotation.  K17's solve from the sample ("metric RGB-D pose": Solve): centroids ca, cb, S, Horn's N, 6 cyclic Jacobi sweeps,
 *   the one correction.  R is, bit for bit, what mi_rigid_hypotheses gives for the same rows and seed.
 * Scale.  a'_k = a_k - ca, b'_k = b_k - cb, r_k = R a'_k with r_kj = (R_j0 a'_k0 + R_j1 a'_k1) + R_j2 a'_k2;
 *   num = the sum over k in order of ((b'_k0 r_k0 + b'_k1 r_k1) + b'_k2 r_k2); den = the sum over k in order of
 *   ((a'_k0^2 + a'_k1^2) + a'_k2^2); s = num / den; t_j = cb_j - s ((R_j0 ca_0 + R_j1 ca_1) + R_j2 ca_2).  float32.
 * Degenerate sample.  K17's test in either frame (it is free of scale); also refused: a result that is not finite, s <
 *   MI_SIM3_MIN_SCALE or s > MI_SIM3_MAX_SCALE.  A refused hypothesis, or fewer than 3 valid rows: cost = +inf, count = 0 and
 *   zeros in the model.
 * Metric MI_SIM3_POINT.  u_j = (s ((R_j0 x + R_j1 y) + R_j2 z) + t_j) - X2_j for X1 = (x, y, z); d^2 = (u_0^2 + u_1^2) + u_2^2.
 *   The threshold is in the units of frame 2.  For maps in world frames and for trajectories.
 * Metric MI_SIM3_REPROJ.  The points are in the two keyframes' CAMERA frames (z forward).  Y_j = s ((R_j0 x + R_j1 y) + R_j2 z)
 *   + t_j; with v = X2 - t, W_j = ((R_0j v_0 + R_1j v_1) + R_2j v_2) * inv_s, inv_s = 1.0f / s formed once per model;
 *   e2 = (Y_x / Y_z - X2_x / X2_z)^2 + (Y_y / Y_z - X2_y / X2_z)^2; e1 the same with W against X1; d^2 = e1 + e2: the
 *   symmetric form, as K24's transfer error.  The threshold is in normalised units (pixels / focal length).  A row whose
 *   X1_z, X2_z, Y_z or W_z is not above 0 has d^2 = +inf: it is never an inlier and adds thr^2 to the cost.  ORB-SLAM's test
 *   on projected map points: the depth error of a triangulated point, large and along its ray, does not decide the inliers.
 * Cost, selection, rounds, acceptance.  K17's: count = number of rows with d^2 <= thr^2, cost = the sum over the valid rows
 *   in index order of min(d^2, thr^2), float32; the lowest h among equal costs; k_r = 1 + (R - 1 - r) / 2; a refit replaces
 *   the best model only on a strictly lower cost, costs held as (rows beyond the threshold, float32 sum of the inliers' d^2)
 *   and compared as k thr^2 + sum in float64. */
#define MI_SIM3_MAX_N 2048
#define MI_SIM3_MIN_SCALE 1e-3f
#define MI_SIM3_MAX_SCALE 1e3f
#define MI_SIM3_MAX_ROWS 16777216
enum { MI_SIM3_POINT = 0, MI_SIM3_REPROJ = 1 };

/* H = num_hypotheses hypotheses per pair, generated and scored: srt_h (batch, H, 13); cost (batch, H) float32, count
 * (batch, H) int32.  H < 1: MI_E_SHAPE; H > MI_POSE_MAX_HYPOTHESES, threshold <= 0 or not finite, metric not one of the two:
 * MI_E_PARAM.  One launch: ceil(H / 64) x batch waves, a lane per hypothesis. */
MI_API int mi_sim3_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                              float threshold, int metric, uint32_t seed, float *srt_h, float *cost, int32_t *count,
                              mi_stream_t stream);

/* s (batch), r (batch, 3, 3), t (batch, 3) from the rows with mask != 0 (mask is required), the same for both metrics: K17's
 * refit (mi_rigid_refit: centroids, then the centred products S, Ca, Cb, two passes of lanes-strided sums; the set is
 * degenerate when Ca or Cb is, by K17's eigenvalue test), the rotation as above from S, then in a third pass num = the sum of
 * ((b'_0 r_0 + b'_1 r_1) + b'_2 r_2) over the rows, lanes-strided then folded across the wave, den = (Ca_xx + Ca_yy) + Ca_zz,
 * s = num / den and t as above.  ok (batch) bytes: 0 with s = 1, r = identity and t = 0 for fewer than 3 rows, a degenerate
 * set, a result that is not finite or a scale outside the range, else 1.  One wave per pair. */
MI_API int mi_sim3_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *s, float *r,
                         float *t, uint8_t *ok, mi_stream_t stream);

/* The whole estimator, mi_rigid_ransac's steps and output rules with the model and metric above: mi_sim3_hypotheses into the
 * workspace, the hypothesis of minimum cost, refine_rounds rounds of {inliers at k_r * threshold, refit as mi_sim3_refit,
 * score at `threshold`, accept on a strictly lower cost}.  s (batch), r (batch, 3, 3), t (batch, 3); inlier (batch, n) bytes:
 * d^2 <= threshold^2 under the result, 0 for rows that are not valid; best_h (batch); count (batch) = number of inlier bytes
 * set; rmse (batch) float32 = sqrt of the mean d^2 over the inliers, in the metric's units; ok (batch) bytes = 1 when a usable
 * hypothesis exists and count >= 3.  Where ok = 0: s = 1, r = identity, t = 0, no inliers, count = 0, rmse = 0.  With
 * refine_rounds = 0 and ok = 1, s / r / t / count are exactly srt_h[best_h] / count[best_h] of mi_sim3_hypotheses.
 * 0 <= refine_rounds <= MI_POSE_MAX_REFINE_ROUNDS (MI_E_PARAM).  workspace: mi_sim3_ransac_workspace_bytes(batch, n, H) bytes
 * (0 for an unsupported request), 16-byte aligned (MI_E_ALIGN), any content; shorter: MI_E_CAPACITY.  Two launches. */
MI_API size_t mi_sim3_ransac_workspace_bytes(int batch, int n, int num_hypotheses);
MI_API int mi_sim3_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                          float threshold, int metric, int refine_rounds, uint32_t seed, float *s, float *r, float *t,
                          uint8_t *inlier, int32_t *best_h, int32_t *count, float *rmse, uint8_t *ok, void *workspace,
                          size_t workspace_bytes, mi_stream_t stream);

/* Map 1 moved into map 2's frame and units by (s (batch), r (batch, 3, 3), t (batch, 3)): its landmarks points (batch,
 * landmarks, 3) -> points_out, X' = s R X + t; its frame poses r_k (batch, frames, 3, 3), t_k (batch, frames, 3) with
 * X_c = R_k X + t_k -> r_out, t_out with R_k' = R_k R^T and t_k' = s t_k - R_k' t, so that R_k' X' + t_k' = s (R_k X + t_k):
 * the camera sees the same rays, its depths in map 2's units.  Every element is formed in float64 from the float32 inputs,
 * widened exactly, and rounded to float32 once:  X'_j = s ((R_j0 X_0 + R_j1 X_1) + R_j2 X_2) + t_j;
 * R_k'_ij = (R_k,i0 R_j0 + R_k,i1 R_j1) + R_k,i2 R_j2;  t_k'_i = s t_k,i - ((R_k'_i0 t_0 + R_k'_i1 t_1) + R_k'_i2 t_2) with the
 * float64 R_k'.  frames or landmarks may be 0 (then its arrays may be NULL), not both; batch < 1, a negative count or both 0:
 * MI_E_SHAPE; batch > 65535 or frames + landmarks > MI_SIM3_MAX_ROWS: MI_E_PARAM.  Outputs alias no input.  One thread per
 * frame or landmark, one launch. */
MI_API int mi_sim3_apply(const float *s, const float *r, const float *t, int batch, int frames, int landmarks, const float *r_k,
                         const float *t_k, const float *points, float *r_out, float *t_out, float *points_out,
                         mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_SIM3_H */
