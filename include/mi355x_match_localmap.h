/* mi355x_match_localmap.h -- the local-map tracking section (K29) of the C ABI, with a header and a library of its own, as
 * K27 and K28 have: libmi355x_match_localmap.so exports exactly the MI_API declarations below, under the conventions (return
 * values, MI_E_*, mi_stream_t, ABI version 3) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays
 * the export of that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * LOCALMAP_SIGNATURES, load_localmap()). */
#ifndef MI355X_MATCH_LOCALMAP_H
#define MI355X_MATCH_LOCALMAP_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- local-map tracking (K29): a descriptor per landmark, and landmarks projected into a frame and matched in a window ----
 * K28 produces triangulated landmarks, K23 wants 3-D to 2-D matches of a new frame.  This section is the join: a tracker that
 * has a predicted pose projects its landmarks and searches a small window around each projection (ORB-SLAM's
 * SearchByProjection in TrackLocalMap).  mi_localmap_descriptors gives every landmark slot the descriptor of one of its
 * observations; mi_localmap_match matches one frame per batch item against that item's landmarks.  Entries under the contract
 * of the K25 .. K28 sections: pure functions of their arguments, no allocation, no synchronisation, no memset, one stream,
 * capturable into a hipGraph; outputs may hold anything on entry, every output element is written and outputs alias nothing;
 * MI_E_* before any launch; the same inputs give the same bits, alone or inside a batch.
 * Atomics.  No global atomics.  mi_localmap_match uses INTEGER atomics on LDS: atomicMin on a keypoint's claim word and
 *   atomicAdd on the five state counters.  Every result below is defined by the inputs alone -- a keypoint's claim is the
 *   smallest claim made on it, a count is a count -- so the order in which they land changes no output bit.  No
 *   floating-point value is ever combined atomically.
 *
 * Descriptors.  The packed hard bits of mi_sparse_bad / mi_sparse_bad_oriented: num_bits is 256 or 512 (anything else:
 *   MI_E_PARAM), W = num_bits / 32 words of 32 bits.  hamming(a, b) = popcount(a xor b) over the W words.  ABSENT = num_bits + 1.
 * Shapes.  1 <= F <= MI_LOCALMAP_MAX_FRAMES, 1 <= K <= MI_LOCALMAP_MAX_KEYPOINTS, 1 <= L <= MI_LOCALMAP_MAX_LANDMARKS
 *   (= MI_BA_MAX_LANDMARKS), 1 <= batch <= 65535 (below: MI_E_SHAPE; above: MI_E_PARAM).  Order of the checks: NULL, shape,
 *   parameters. */
#define MI_LOCALMAP_MAX_LANDMARKS 2048
#define MI_LOCALMAP_MAX_KEYPOINTS 1024
#define MI_LOCALMAP_MAX_FRAMES 16

/* A representative descriptor per landmark slot.  bits (batch, F, K, W) uint32; track_kp (batch, F, L) int32 as
 * mi_tracks_build writes it.  The VIEWS of slot l are the frames f, ascending, with 0 <= track_kp[f, l] < K; any other value
 * means "not seen".  With n views, for view a: the n distances hamming(a, b) over all views b, a itself included (distance
 * 0), sorted ascending; med_a is element (n - 1) / 2 (integer division) of that list.  The representative is the view with
 * the smallest key med_a << 8 | f_a: the medoid under the median distance, the lowest frame on a tie (ORB-SLAM's
 * ComputeDistinctiveDescriptors).  rep_bits (batch, L, W) uint32: that view's words, bit for bit; rep_frame (batch, L) int32:
 * its frame; rep_median (batch, L) int32: its med.  n = 0: zeros, -1 and ABSENT.  16 lanes per slot, one launch. */
MI_API int mi_localmap_descriptors(const uint32_t *bits, const int32_t *track_kp, int batch, int frames, int keypoints,
                                   int landmarks, int num_bits, uint32_t *rep_bits, int32_t *rep_frame, int32_t *rep_median,
                                   mi_stream_t stream);

/* One frame per batch item against that item's landmarks.  One workgroup per item, one launch, no workspace.
 * points (batch, L, 3) float32; point_valid (batch, L) bytes or NULL (every point); rep_bits (batch, L, W); r (batch, 3, 3),
 * t (batch, 3) float32: the predicted pose, X_c = R X + t; cam (batch, 4) float32: fx, fy, cx, cy; kp (batch, K, 2) float32 in
 * pixel (y, x) order; kp_valid (batch, K) bytes or NULL (every keypoint); kp_bits (batch, K, W).
 * Parameters (MI_E_PARAM otherwise, NaN included): 0 < min_depth < max_depth, both finite; radius > 0 and finite;
 *   0 <= max_distance <= num_bits; 0 < ratio <= 1; height, width >= 1.
 * All geometry is float64; the float32 inputs are widened exactly and every operation is the one written here, in this order,
 * unfused.
 * 1. Projection.  q_i = ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i; z = q_2; u = fx (q_0 / z) + cx; v = fy (q_1 / z) + cy.  The
 *    landmark is IN VIEW iff its point_valid byte is set, q_0, q_1, q_2 are finite, min_depth <= z <= max_depth,
 *    0 <= u <= width - 1 and 0 <= v <= height - 1.  proj (batch, L, 2) float32: (v, u) rounded, (-1, -1) when not in view.
 * 2. Window.  A valid keypoint j = (ky, kx) is in the window iff du du + dv dv <= radius radius with du = kx - u, dv = ky - v
 *    (radius radius is the float64 product of the widened radius).
 * 3. Nearest two (K26's rule, over the keypoints in the window).  The key of keypoint j is hamming(rep_l, kp_bits_j) << 16 | j;
 *    key1 is the smallest key, key2 the smallest among the others; d1 = key1 >> 16, j1 = key1 & 0xffff, d2 = key2 >> 16.  An
 *    empty window: d1 = ABSENT, j1 = -1; a window of one: d2 = ABSENT.
 * 4. Candidate.  l is a CANDIDATE iff d1 <= max_distance and (float)d1 < ratio * (float)d2: one float32 multiply and one
 *    compare, K26's vote.
 * 5. One landmark per keypoint.  The claim of candidate l on j1 has the key d1 << 16 | l.  kp_lm (batch, K) int32: the l of the
 *    smallest claim on j, or -1.  l is KEPT iff kp_lm[j1] == l.  A loser is not given its second choice.
 * 6. Outputs.  lm_state (batch, L) bytes: 0 not in view, 1 in view with an empty window, 2 failed the distance or the ratio
 *    test, 3 lost its keypoint to another landmark, 4 kept.  lm_kp (batch, L) int32: j1 if kept, else -1.  lm_distance
 *    (batch, L) int32: d1 for the states 2 .. 4, else ABSENT.  match_keypoints (batch, L, 2) float32: the kept keypoint's two
 *    floats bit for bit, else (-1, -1).  counts (batch, 5) int32: the number of landmarks in each state.
 * points, match_keypoints and lm_state == 4 are the points3d, keypoints2d and valid of K23 (mi_pnp_ransac after
 * mi_normalise_keypoints); kp_lm == -1 marks the keypoints left over for new landmarks. */
MI_API int mi_localmap_match(const float *points, const uint8_t *point_valid, const uint32_t *rep_bits, const float *r,
                             const float *t, const float *cam, const float *kp, const uint8_t *kp_valid, const uint32_t *kp_bits,
                             int batch, int landmarks, int keypoints, int num_bits, int height, int width, float min_depth,
                             float max_depth, float radius, int max_distance, float ratio, float *proj, uint8_t *lm_state,
                             int32_t *lm_kp, int32_t *lm_distance, float *match_keypoints, int32_t *kp_lm, int32_t *counts,
                             mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_LOCALMAP_H */
