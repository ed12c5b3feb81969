/* mi355x_match_tracks.h -- the landmark-track section (K28) of the C ABI, with a header and a library of its own, as K27
 * has: libmi355x_match_tracks.so exports exactly the MI_API declarations below, under the conventions (return values,
 * MI_E_*, mi_stream_t, ABI version 3) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the
 * export of that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * TRACKS_SIGNATURES, load_tracks()). */
#ifndef MI355X_MATCH_TRACKS_H
#define MI355X_MATCH_TRACKS_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- landmark tracks (K28): pairwise matches over a window of frames -> the track form K25 reads, and N-view triangulation ----
 * The matcher's output is pairwise: keypoint indices (i, j) per frame pair (mi_match_pairs' match_ij, mi_mnn_extract's
 * indices).  K25 wants a window in track form: one column per landmark, one row per frame.  This section is the join:
 * mi_tracks_build labels the connected components of the match graph, rejects the ambiguous ones and orders the rest
 * into landmark slots; mi_tracks_triangulate gives every slot a point from all the frames that see it.  The host code it
 * replaces is a union-find, a gather and a per-landmark least-squares loop.  Entries under the contract of the K25 / K27
 * sections: pure functions of their arguments, no allocation, no synchronisation, no memset, one stream, capturable into
 * a hipGraph; outputs and workspace may hold anything on entry, every output element is written and outputs alias
 * nothing; MI_E_* before any launch; the same inputs give the same bits, alone or inside a batch.
 * Atomics.  No global atomics.  The labelling uses INTEGER atomics on LDS (atomicMin on a label, atomicOr / atomicAdd on a
 *   root's frame mask and node count, atomicAdd on the four counters): every result below is defined by the inputs alone
 *   -- a component's label is its smallest node, whatever order the hooks land in -- so the order in which they land
 *   changes no output bit.  No floating-point value is ever combined atomically.
 *
 * Shapes.  2 <= F <= MI_TRACKS_MAX_FRAMES frames, 1 <= K <= MI_TRACKS_MAX_KEYPOINTS keypoints per frame, 1 <= P <=
 *   MI_TRACKS_MAX_PAIRS listed pairs, 1 <= M <= MI_TRACKS_MAX_MATCHES match records per pair, 1 <= L <= MI_BA_MAX_LANDMARKS
 *   slots (below: MI_E_SHAPE, as batch < 1; above: MI_E_PARAM, as batch > 65535).  min_views outside 2 .. F: MI_E_PARAM.
 * Matches.  pair_frames (batch, P, 2) int32 (a, b); match_ij (batch, P, M, 2) int32 (i in a, j in b); match_valid
 *   (batch, P, M) bytes; kp_valid (batch, F, K) bytes or NULL (every keypoint).  A match is ACTIVE when its byte is not 0,
 *   0 <= a, b < F and a != b, 0 <= i, j < K, and both ends' kp_valid bytes are set.  Anything else is padding and is read
 *   no further: the index fields of an invalid record may hold anything.  Reversed pairs (b, a), repeated pairs and
 *   repeated matches are legal and change nothing.
 * Components.  Node n = f K + k.  A COMPONENT is a connected component of the graph of the active matches; its LABEL is its
 *   smallest node, its LENGTH its number of nodes.  It CONFLICTS when it holds two nodes of one frame; it is ELIGIBLE when
 *   it does not and its length is at least min_views.  The eligible components ordered by (length descending, label
 *   ascending) fill the slots 0, 1, ...; those beyond L are dropped.
 * Triangulation (float64 throughout; the float32 inputs are widened exactly).  Over the frames f that see the landmark, in
 *   ascending f: with the observation (x, y), n = sqrt((x x + y y) + 1),
 *       d_k = ((R_0k x + R_1k y) + R_2k) / n      (d = R^T m / |m|, m = (x, y, 1): the ray in the world frame)
 *       c_k = -((R_0k t_0 + R_1k t_1) + R_2k t_2) (the camera centre)
 *       P_ij = [i == j] - d_i d_j;   A_ij += P_ij (i <= j);   b_i += (P_i0 c_0 + P_i1 c_1) + P_i2 c_2
 *   from A = 0, b = 0.  Solve A X = b by the symmetric cofactor inverse: C_00 = A_11 A_22 - A_12 A_12, C_01 = A_02 A_12 - A_01
 *   A_22, C_02 = A_01 A_12 - A_02 A_11, C_11 = A_00 A_22 - A_02 A_02, C_12 = A_01 A_02 - A_00 A_12, C_22 = A_00 A_11 - A_01 A_01, det =
 *   (A_00 C_00 + A_01 C_01) + A_02 C_02, X_i = ((C_i0 b_0 + C_i1 b_1) + C_i2 b_2) / det.  USABLE (K25's pivot rule): with the
 *   pivots p_0 = A_00, p_1 = C_22 / A_00, p_2 = det / C_22 and dmax the largest diagonal element of A: dmax > 0, every pivot
 *   above 1e-6 dmax, every X_i finite.  Parallel rays fail it (so does a landmark nobody sees).
 *   Per seeing frame: q_i = ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i; z = q_2; with z > 0, u = q_0 / z - x, v = q_1 / z - y, e2 =
 *   u u + v v.  e2max = the largest e2 (+inf when a z is not positive or the solve is unusable).  cos_par = the smallest
 *   (d_a0 d_b0 + d_a1 d_b1) + d_a2 d_b2 over the pairs a < b of seeing frames (1 with fewer than two).
 *   point_ok: seen count >= min_views, usable, every z > 0, e2max <= max_e2 and cos_par <= max_cos (float64 comparisons). */
#define MI_TRACKS_MAX_FRAMES 16
#define MI_TRACKS_MAX_KEYPOINTS 1024
#define MI_TRACKS_MAX_PAIRS 120
#define MI_TRACKS_MAX_MATCHES 1024

/* Workspace of mi_tracks_build: per window one int32 per match record (the two nodes of an active match, packed),
 * rounded up to 16 bytes; 0 for an unsupported shape.  16-byte aligned (MI_E_ALIGN), any content; shorter: MI_E_CAPACITY. */
MI_API size_t mi_tracks_workspace_bytes(int batch, int frames, int keypoints, int pairs, int matches, int landmarks);

/* Matches to tracks.  One workgroup per window, one launch.  keypoints (batch, F, K, 2) float32 are copied and never
 * interpreted.  track_kp (batch, F, L) int32: the keypoint index of slot l in frame f, or -1; vis (batch, F, L) bytes: 1
 * where track_kp >= 0; track_keypoints (batch, F, L, 2) float32: that keypoint's two floats bit for bit, 0 where not seen;
 * track_len (batch, L) int32; kp_track (batch, F, K) int32: the slot of the keypoint's component, -2 for a node of a
 * conflicting component, -1 otherwise; counts (batch, 4) int32: components of >= 2 nodes, conflicting, eligible, kept =
 * min(eligible, L).  An empty slot: -1 / 0 / 0 / 0. */
MI_API int mi_tracks_build(const int32_t *pair_frames, const int32_t *match_ij, const uint8_t *match_valid,
                           const uint8_t *kp_valid, const float *keypoints, int batch, int frames, int keypoints_per_frame,
                           int pairs, int matches, int min_views, int landmarks, int32_t *track_kp, uint8_t *vis,
                           float *track_keypoints, int32_t *track_len, int32_t *kp_track, int32_t *counts, void *workspace,
                           size_t workspace_bytes, mi_stream_t stream);

/* N-view triangulation of every slot.  One thread per landmark, one launch, no workspace.  r (batch, F, 3, 3), t (batch, F, 3)
 * float32 with X_c = R X + t; obs (batch, F, L, 2) float32 normalised (x, y) as mi_normalise_keypoints writes them, read
 * only where vis (batch, F, L) is not 0.  max_e2 (a normalised squared distance) must be > 0 and finite, max_cos (the cosine
 * of the smallest accepted parallax angle) in (-1, 1] (MI_E_PARAM).  points (batch, L, 3) float32: X rounded, zeros when the
 * solve is unusable; point_ok (batch, L) bytes; vis_out (batch, F, L) bytes: 1 where vis is set and point_ok, else 0 -- K25
 * derives "active" from vis alone, so a failed landmark takes no part; e2max, cos_par (batch, L) float32, rounded. */
MI_API int mi_tracks_triangulate(const float *r, const float *t, const float *obs, const uint8_t *vis, int batch, int frames,
                                 int landmarks, int min_views, float max_e2, float max_cos, float *points, uint8_t *point_ok,
                                 uint8_t *vis_out, float *e2max, float *cos_par, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_TRACKS_H */
