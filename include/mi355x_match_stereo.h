/* mi355x_match_stereo.h -- the stereo-depth section (K33) of the C ABI, with a header and a library of its own:
 * libmi355x_match_stereo.so exports exactly the MI_API declarations below, under the conventions (return values, MI_E_*,
 * mi_stream_t, ABI version) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the export of
 * that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * STEREO_SIGNATURES, STEREO_CONSTANTS, load_stereo()). */
#ifndef MI355X_MATCH_STEREO_H
#define MI355X_MATCH_STEREO_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- stereo depth (K33): a rectified stereo pair -> a disparity map and a depth frame ---------------------------------------------
 * Every depth consumer of the library (mi_depth_to_points, mi_tsdf_integrate, the RGB-D estimators) takes a depth frame that a
 * sensor delivered.  This section is the third sensor set-up, a calibrated stereo rig: census transform, Hamming matching
 * cost, semi-global aggregation over 4 or 8 paths, winner-take-all with a uniqueness test and a left-right check, a parabola
 * sub-pixel step and depth = f b / d; what a host otherwise does with cv2.StereoSGBM on the CPU.  The arithmetic is integer
 * from the census bits to the aggregated volume, float32 for the sub-pixel step and the division.  Entries under the contract
 * of the K30 and K32 sections (include/mi355x_match_sim3.h, include/mi355x_match_flow.h): pure functions of their arguments, no
 * allocation, no synchronisation, no memset, one stream, no floating-point atomics (no atomics at all), the same bits alone or
 * inside a batch, capturable into a hipGraph; outputs may hold anything on entry and every output element is written; MI_E_*
 * before any launch.  Order of the checks: NULL, shape, parameters, alignment, capacity.
 * batch < 1, h < 1, w < 1: MI_E_SHAPE.  batch h w >= 2^26 (MI_STEREO_MAX_PIXELS; the volume limit below at D = 64): MI_E_PARAM.
 *
 * The inputs are RECTIFIED: a scene point lies on the same row of both views, at x_right = x_left - d with d >= 0.
 * Undistortion and rectification are the K34 section's (include/mi355x_match_rectify.h: mi_rectify_stereo_rig, mi_rectify_map,
 * mi_rectify_remap); the speckle and median post-filters are the K35 section's (include/mi355x_match_filter.h: mi_filter_speckle,
 * mi_filter_median), applied to the disparity this section writes.
 *
 * Census.  gray is (batch, h, w), uint8 or float32 (the two outputs of mi_ingest_frames); census is (batch, h, w) uint64.
 *   The window is 9 wide and 7 high.  Bit k of pixel (y, x) belongs to the k-th offset (dy, dx), dy = -3 .. 3 outer,
 *   dx = -4 .. 4 inner, the centre skipped: k = 0 .. 61, bits 62 and 63 are 0.  The bit is 1 when
 *   G[clamp(y + dy, 0, h - 1)][clamp(x + dx, 0, w - 1)] < G[y][x] (replicate border; for float32 a float compare, so a NaN on
 *   either side gives 0).  No index leaves the frame.
 *
 * Cost.  C(y, x, d) = popcount(census_left(y, x) ^ census_right(y, x - d)) for x - d >= 0, and MI_STEREO_COST_OUTSIDE = 64
 *   otherwise (above any real cost, which is at most 62).  d = 0 .. D - 1 with D one of 64, 128, 256 (else MI_E_PARAM).
 *
 * Paths.  The directions r = (dy, dx) are, in this order, (0,1), (0,-1), (1,0), (-1,0), (1,1), (-1,-1), (1,-1), (-1,1);
 *   paths = 4 takes the first four, paths = 8 all (anything else: MI_E_PARAM).  For a pixel p whose predecessor p - r is
 *   outside the frame L_r(p, d) = C(p, d); otherwise, with m = min_k L_r(p - r, k),
 *     L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + P1, L_r(p - r, d + 1) + P1, m + P2) - m,
 *   the d - 1 term absent at d = 0 and the d + 1 term at d = D - 1.  0 <= P1 <= P2 <= 255, else MI_E_PARAM.
 *   L_r <= C + P2 <= 319, so S = the sum of L_r over the paths fits uint16 (8 * 319 = 2552).  volume is (batch, h, w, D)
 *   uint16 and holds exactly S.  batch h w D >= 2^32: MI_E_PARAM.  w < D is legal.
 *
 * Selection.  d* = argmin_d S(y, x, d), the lowest d on ties.  The right view's disparity is computed from the same volume:
 *   dR(y, xr) = argmin over d with xr + d <= w - 1 of S(y, xr + d, d), the lowest d on ties; int16 (batch, h, w).
 *   The tests, in this order:
 *   - uniqueness, 0 <= uniqueness <= 100 (else MI_E_PARAM; 0 turns it off): MI_STEREO_NOT_UNIQUE when some d with
 *     |d - d*| > 1 has S(d) * (100 - uniqueness) < S(d*) * 100 (integers; cv2.StereoSGBM's rule);
 *   - left-right, lr_max_diff >= 0 (negative turns it off, and disparity_right may then be NULL: nothing is computed for
 *     the right view): MI_STEREO_LR when x - d* < MI_STEREO_BORDER or |dR(y, x - d*) - d*| > lr_max_diff.  The border rule
 *     covers x - d* < 0, where the right view has no pixel, and the first MI_STEREO_BORDER = 8 columns of the right view, where
 *     dR cannot vouch for a match: in the first 4 the census window of the right pixel is replicated border, and the path sums
 *     need about as many pixels again to recover from the costs of 64 left of them.  Without it a left pixel whose scene point
 *     lies outside the right view (x < its true disparity) is often accepted: at x = 0 only d = 0 has a real cost, wins by a
 *     wide margin, and dR(y, 0) -- a minimum over S(y, d, d) that includes this same forced winner -- frequently agrees;
 *   - otherwise MI_STEREO_OK.
 *   Sub-pixel step: at 0 < d* < D - 1, den = S(d* - 1) + S(d* + 1) - 2 S(d*) (>= 0, d* being the minimum) and
 *   offset = (float)(S(d* - 1) - S(d* + 1)) / (float)(2 * den) in float32 when den > 0, else 0; offset = 0 at d* = 0 and at
 *   d* = D - 1.  |offset| <= 0.5.
 *   disparity (batch, h, w) float32 = (float)d* + offset, or -1.0f on a rejected pixel; code (batch, h, w) bytes.
 *
 * Depth.  depth = fb / disparity, one IEEE float32 division, where disparity >= min_disparity; 0.0f elsewhere (rejected
 *   pixels, NaN): the value every depth consumer of the library rejects, since they all require min_depth > 0.
 *   min_disparity > 0 and finite, fb > 0 and finite (MI_E_PARAM), fb = fx * baseline in the unit the depth is wanted in. */
#define MI_STEREO_COST_OUTSIDE 64
#define MI_STEREO_MAX_DISPARITIES 256
#define MI_STEREO_BORDER 8
#define MI_STEREO_MAX_PIXELS 67108864
#define MI_STEREO_MAX_VOLUME 4294967296
enum { MI_STEREO_OK = 0, MI_STEREO_NOT_UNIQUE = 1, MI_STEREO_LR = 2 };

/* gray: uint8 (gray_is_u8 != 0) or float32, then 4-byte aligned; census 8-byte aligned (MI_E_ALIGN).  One thread per pixel;
 * the 62 neighbours come through the L1. */
MI_API int mi_stereo_census(const void *gray, int gray_is_u8, int batch, int h, int w, uint64_t *census, mi_stream_t stream);

/* The workspace mi_stereo_aggregate wants for a request, in bytes: 0 today for every request (the path kernels keep a line's
 * state in registers and the matching cost is never materialised), also for one mi_stereo_aggregate refuses.  A workspace of
 * fewer bytes than this is MI_E_CAPACITY; with 0 wanted, workspace may be NULL. */
MI_API size_t mi_stereo_workspace_bytes(int batch, int h, int w, int D, int paths);

/* census_left, census_right as mi_stereo_census writes them (8-byte aligned), volume (batch, h, w, D) uint16, 16-byte aligned
 * (MI_E_ALIGN).  `paths` launches, one per direction in the order above: the first writes the volume, the later ones add to
 * it; every element has one owner thread per launch.  A wave walks one path line with the disparities in its lanes (D / 64
 * consecutive ones per lane); the previous pixel's L_r stays in registers. */
MI_API int mi_stereo_aggregate(const uint64_t *census_left, const uint64_t *census_right, int batch, int h, int w, int D,
                               int paths, int p1, int p2, uint16_t *volume, void *workspace, size_t workspace_bytes,
                               mi_stream_t stream);

/* volume as mi_stereo_aggregate writes it (16-byte aligned); disparity float32 4-byte aligned, disparity_right int16 2-byte
 * aligned (MI_E_ALIGN), code bytes.  disparity_right may be NULL only when lr_max_diff < 0 (else MI_E_NULL); when it is given
 * it is written, whatever lr_max_diff is.  Two launches: the right view's disparities (one wave per row, the running minima
 * move one lane per pixel), then the left view's with the tests (one wave per pixel, 16 pixels one after the other). */
MI_API int mi_stereo_select(const uint16_t *volume, int batch, int h, int w, int D, int uniqueness, int lr_max_diff,
                            float *disparity, int16_t *disparity_right, uint8_t *code, mi_stream_t stream);

/* disparity, depth (batch, h, w) float32, 4-byte aligned (MI_E_ALIGN).  One thread per pixel. */
MI_API int mi_stereo_depth(const float *disparity, int batch, int h, int w, float fb, float min_disparity, float *depth,
                           mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_STEREO_H */
