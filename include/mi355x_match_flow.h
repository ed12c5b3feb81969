/* mi355x_match_flow.h -- the feature-tracking section (K32) of the C ABI, with a header and a library of its own:
 * libmi355x_match_flow.so exports exactly the MI_API declarations below, under the conventions (return values, MI_E_*,
 * mi_stream_t, ABI version) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the export of
 * that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * FLOW_SIGNATURES, FLOW_CONSTANTS, load_flow()). */
#ifndef MI355X_MATCH_FLOW_H
#define MI355X_MATCH_FLOW_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- feature tracking (K32): two gray frames and the keypoints of the first -> their sub-pixel positions in the second --------
 * Every other stage of the library associates two frames by descriptor matching.  This section is the KLT front end of a
 * visual-odometry loop: pyramidal Lucas-Kanade in the inverse (template-gradient) form of cv2.calcOpticalFlowPyrLK, the
 * forward-backward test and the refill of lost slots with fresh corners.  Entries under the contract of the K30 section
 * (include/mi355x_match_sim3.h): pure functions of their arguments, no allocation, no synchronisation, no memset, one
 * stream, no floating-point atomics, every sum in a fixed order (the same inputs give the same bits, alone or inside a
 * batch), capturable into a hipGraph; outputs may hold anything on entry and every output element is written; MI_E_* before
 * any launch.  Order of the checks: NULL, shape, parameters, alignment, capacity.
 * Keypoints are (batch, k, 2) float32 (y, x) pixel coordinates; (-1, -1) marks padding, as mi_topk_keypoints writes it.
 * batch < 1, k < 1, h < 1, w < 1: MI_E_SHAPE; batch > 65535, k > MI_FLOW_MAX_K: MI_E_PARAM.
 *
 * Pyramid.  h_0 = h, w_0 = w; h_{l+1} = (h_l + 1) / 2, w_{l+1} = (w_l + 1) / 2 (integer division).  Level l is a contiguous
 *   (batch, h_l, w_l) float32 block at byte offset o_l of the pyramid: o_0 = 0, o_{l+1} = o_l + batch h_l w_l 4 rounded up
 *   to a multiple of 256; mi_flow_pyramid_bytes is o_levels.  Level 0 is the frame widened to float32.  Level l+1 is
 *   cv2.pyrDown of level l: with S the level below, R(i) the reflect-101 index (R(i) = -i below 0, 2 n - 2 - i from n on) and
 *   tap(a, b, c, d, e) = ((a + e) + 4.0f * (b + d)) + 6.0f * c in float32, not contracted,
 *     row_j(x) = tap(S[R(2y+j)][R(2x-2)], S[R(2y+j)][R(2x-1)], S[R(2y+j)][2x], S[R(2y+j)][R(2x+1)], S[R(2y+j)][R(2x+2)]),
 *     out(y, x) = tap(row_-2(x), row_-1(x), row_0(x), row_1(x), row_2(x)) * (1.0f / 256.0f).
 *   For a uint8 frame levels 0 to 2 are exact (multiples of 2^-16 below 256).
 *   1 <= levels <= MI_FLOW_MAX_LEVELS and min(h_l, w_l) >= 2 r + 3 at every level, else MI_E_PARAM: a coarser level cannot
 *   hold a window.  r is mi_flow_track's radius; the pyramid entries, which know no radius, apply the rule with r = 1 (5
 *   pixels; mi_flow_pyramid_bytes: 0), so a pyramid can be too coarse for a large window and fine for a small one.
 *   h, w <= 32768 and batch h w <= MI_FLOW_MAX_PIXELS (2^32: 16 GB of level 0), else MI_E_PARAM.
 *
 * Sampling.  Every read of a frame is the bilinear sample B(F, x, y) of level F at float32 (x, y), clamped to the frame IN
 *   FLOAT before any conversion to an integer (replicate border; fmaxf / fminf, so that NaN clamps to 0):
 *     x = fminf(fmaxf(x, 0), w_l - 1), x0 = floorf(x), fx = x - x0, i0 = (int)x0, i1 = min(i0 + 1, w_l - 1); y likewise;
 *     top = F[j0][i0] + fx * (F[j0][i1] - F[j0][i0]); bot = F[j1][i0] + fx * (F[j1][i1] - F[j1][i0]);
 *     B = top + fy * (bot - top).
 *   No keypoint, guess or step, whatever its value, produces an index outside the level.
 *
 * Tracking, per keypoint p = (p_y, p_x), levels l = levels - 1 .. 0, radius r, n = (2r + 1)^2 window pixels q = (dy + r)
 *   (2r + 1) + (dx + r) for dy, dx in -r .. r, all float32, not contracted:
 *     c = p * 2^-l;  T(dx, dy) = B(level l of frame 1, c_x + (float)dx, c_y + (float)dy);
 *     gx = 0.5f * (T(dx + 1, dy) - T(dx - 1, dy)), gy = 0.5f * (T(dx, dy + 1) - T(dx, dy - 1));
 *     G = [gxx gxy; gxy gyy] = sum of [gx gx, gx gy; gx gy, gy gy];
 *     min_eig = ((gyy + gxx) - sqrtf((gxx - gyy) (gxx - gyy) + 4.0f * (gxy gxy))) / (2.0f * (float)n);
 *     min_eig < min_eigen (or not a number): the point is lost, MI_FLOW_FLAT.  Else det = gxx gyy - gxy gxy, and up to
 *     max_iterations times:  e = T(dx, dy) - B(level l of frame 2, (c_x + d_x) + (float)dx, (c_y + d_y) + (float)dy);
 *       b_x = sum e gx, b_y = sum e gy, a = sum |e|;
 *       delta_x = (gyy b_x - gxy b_y) / det, delta_y = (gxx b_y - gxy b_x) / det;  d += delta;
 *       stop when delta_x delta_x + delta_y delta_y < epsilon epsilon.
 *     After the level: (c_x + d_x, c_y + d_y) not finite or outside [0, w_l - 1] x [0, h_l - 1]: lost, MI_FLOW_LEFT.
 *     Else, above level 0, d = 2 d.  At the top level d starts from guess * 2^-(levels-1) (guess: (batch, k, 2) (dy, dx) in
 *     level-0 pixels) or from 0 when guess is NULL.
 *   Sum order: lane t of the 64 serves the pixels q = t, t + 64, t + 128, ... and adds its terms in that order starting
 *     from 0; the 64 partial sums p[0..63] fold as a binary tree over neighbours, the total being that of the butterfly
 *     for s = 1, 2, 4, .., 32: p[t] += p[t ^ s].  The kernel does not run that butterfly: it folds with two quad permutes, two
 *     row mirrors and two masked row broadcasts into lane 63 and reads that lane back into every lane; the pairs added at each
 *     step are the butterfly's and float addition commutes, so the bits are the same.
 *   Outputs: keypoints2 = p + d (the level-0 c + d); status = 1; code = MI_FLOW_OK; residual = a / (float)n of the last
 *     iteration at level 0; iterations = the total over all levels.  Running out of iterations is NOT a loss (as OpenCV).
 *   Loss: a keypoint that is padding, not finite or outside [0, w - 1] x [0, h - 1], or whose guess is not finite:
 *     MI_FLOW_PADDING; MI_FLOW_FLAT and MI_FLOW_LEFT as above.  A lost point has status 0, keypoints2 = (-1, -1), residual 0,
 *     iterations 0 and its code.
 *   Because every sample is clamped into the frame, a track that drifts onto foreign texture is NOT lost by itself:
 *     mi_flow_check is the test for that. */
#define MI_FLOW_MAX_LEVELS 8
#define MI_FLOW_MAX_RADIUS 10
#define MI_FLOW_MAX_K 4096
#define MI_FLOW_MAX_ITERATIONS 64
#define MI_FLOW_MAX_CELLS 16384
#define MI_FLOW_MAX_CANDIDATES 65536
#define MI_FLOW_MAX_PIXELS 4294967296
enum { MI_FLOW_OK = 0, MI_FLOW_PADDING = 1, MI_FLOW_FLAT = 2, MI_FLOW_LEFT = 3 };

/* gray (batch, h, w): uint8 (gray_is_u8 != 0) or float32, the two outputs of mi_ingest_frames.  pyramid: pyramid_bytes >=
 * mi_flow_pyramid_bytes(batch, h, w, levels) bytes (MI_E_CAPACITY), 16-byte aligned, as a float32 gray must be 4-byte
 * aligned (MI_E_ALIGN).  `levels` launches, one thread per output pixel. */
MI_API size_t mi_flow_pyramid_bytes(int batch, int h, int w, int levels);
MI_API int mi_flow_pyramid(const void *gray, int gray_is_u8, int batch, int h, int w, int levels, float *pyramid,
                           size_t pyramid_bytes, mi_stream_t stream);

/* pyr1, pyr2: pyramids of (batch, h, w, levels) as mi_flow_pyramid writes them (16-byte aligned: MI_E_ALIGN).  guess may be
 * NULL.  keypoints2 (batch, k, 2) float32; status, code (batch, k) bytes; residual (batch, k) float32; iterations (batch, k)
 * int32.  1 <= radius <= MI_FLOW_MAX_RADIUS, 1 <= max_iterations <= MI_FLOW_MAX_ITERATIONS, epsilon > 0 and finite,
 * min_eigen >= 0 and finite, levels as for the pyramid: MI_E_PARAM.  Every float32 / int32 array 4-byte aligned, inputs and
 * outputs (MI_E_ALIGN).  One launch for all levels: one wave per keypoint, four
 * waves to a workgroup; the template and both gradients stay in registers; the iteration loop is wave-uniform and a wave
 * whose point converges or is lost leaves at once. */
MI_API int mi_flow_track(const float *pyr1, const float *pyr2, const float *keypoints1, const float *guess, int batch, int h,
                         int w, int levels, int k, int radius, int max_iterations, float epsilon, float min_eigen,
                         float *keypoints2, uint8_t *status, uint8_t *code, float *residual, int32_t *iterations,
                         mi_stream_t stream);

/* The forward-backward test: keypoints_back is keypoints1 tracked to frame 2 and back.  dist = sqrtf(dy dy + dx dx) of
 * keypoints_back - keypoints1 in float32; status (batch, k) bytes = 1 where status_fwd and status_bwd are non-zero and
 * dist <= max_distance; fb_distance (batch, k) float32 = dist where both statuses are non-zero, else +inf.  max_distance
 * >= 0 and finite (MI_E_PARAM); the float32 arrays 4-byte aligned (MI_E_ALIGN).  One thread per keypoint. */
MI_API int mi_flow_check(const float *keypoints1, const float *keypoints_back, const uint8_t *status_fwd,
                         const uint8_t *status_bwd, int batch, int k, float max_distance, uint8_t *status, float *fb_distance,
                         mi_stream_t stream);

/* Refill of lost slots with new corners that do not sit on live tracks: the goodFeaturesToTrack(mask=...) step of a KLT
 * loop, defined so that it is deterministic.  The frame is cut into cells of cell x cell pixels, ceil(h / cell) x
 * ceil(w / cell) of them (more than MI_FLOW_MAX_CELLS, or cell < 1: MI_E_PARAM); a point (y, x) lies in cell
 * ((int)y / cell, (int)x / cell) after the float clamp of "Sampling".  keypoints (batch, k, 2) with status (batch, k)
 * bytes: slot i is live when status != 0, and a live slot occupies its cell.  candidates (batch, n_cand, 2) score-descending
 * (y, x) as mi_topk_keypoints writes them, the first min(max(cand_count[b], 0), n_cand) of image b real (cand_count (batch)
 * int32; 1 <= n_cand <= MI_FLOW_MAX_CANDIDATES); a real candidate that is not finite or has a negative coordinate is
 * skipped.  A candidate is accepted when no live keypoint lies in its cell and it is the lowest-indexed candidate there.
 * Accepted candidates in index order fill the lost slots in ascending slot order until either runs out.  keypoints_out
 * (batch, k, 2): the live keypoints, the fills, (-1, -1) in slots still lost; is_new (batch, k) bytes: 1 in filled slots;
 * counts (batch, 3) int32: live, accepted, filled.  The float32 / int32 arrays 4-byte aligned (MI_E_ALIGN).  A request whose
 * cells + k + 4 ints of LDS exceed 64 KB raises a function attribute on its first call on each device (kept per device, safe
 * between host threads); that call is not a stream operation: make it outside a hipGraph capture.  One workgroup per image; the cell winners are found with integer LDS
 * atomicMin, whose result does not depend on the order of arrival. */
MI_API int mi_flow_replenish(const float *keypoints, const uint8_t *status, const float *candidates, const int32_t *cand_count,
                             int batch, int k, int n_cand, int h, int w, int cell, float *keypoints_out, uint8_t *is_new,
                             int32_t *counts, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_FLOW_H */
