/* mi355x_match_filter.h -- the disparity post-filter section (K35) of the C ABI, with a header and a library of its own:
 * libmi355x_match_filter.so exports exactly the MI_API declarations below, under the conventions (return values, MI_E_*,
 * mi_stream_t, ABI version) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the export of
 * that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * FILTER_SIGNATURES, FILTER_CONSTANTS, load_filter()). */
#ifndef MI355X_MATCH_FILTER_H
#define MI355X_MATCH_FILTER_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- disparity post-filters (K35): connected components of a frame, the speckle filter, the median ------------------------------------
 * What a cv2.StereoSGBM user sets with speckleWindowSize / speckleRange, and cv2.medianBlur on the float disparities, between
 * mi_stereo_select and mi_stereo_depth / mi_depth_to_points / mi_tsdf_integrate; the labelling by itself is
 * cv2.connectedComponentsWithStats (4-connectivity) for a class map of the threshold package.  Entries under the contract of the
 * K33 section (include/mi355x_match_stereo.h): pure functions of their arguments, no allocation, no synchronisation, no memset,
 * no device value read on the host, one stream, a number of launches that is fixed and independent of the data, capturable into
 * a hipGraph; outputs may hold anything on entry and every output element is written; MI_E_* before any launch.  Order of the
 * checks: NULL, shape, parameters, alignment, capacity.  Two points differ from K33:
 *   - integer atomics (atomicMin, atomicAdd on int32) are used, on results that do not depend on the order of arrival (a
 *     minimum, a count); no floating-point atomics.  The same bits alone or inside a batch, and from run to run.
 *   - the workspace may hold anything on entry: every word that is read was written by an earlier launch of the same call.
 * batch < 1, h < 1, w < 1: MI_E_SHAPE.  batch h w >= 2^26 (MI_FILTER_MAX_PIXELS, K33's pixel limit): MI_E_PARAM.
 *
 * Validity and adjacency.  A float32 pixel is VALID iff value >= min_valid as a float32 compare, so a NaN is invalid.  Two
 *   4-neighbours (left / right / up / down, inside one frame) are JOINED iff both are valid and fabsf(a - b) <= max_diff: one
 *   float32 subtraction, so inf - inf (a NaN) does not join, and 1e30 - (-1e30) (inf) does not either.  For uint8 values
 *   (MI_FILTER_U8): value >= min_valid_u8 and |a - b| <= max_diff_u8 in integers, where min_valid_u8 = (int)min_valid and
 *   max_diff_u8 = (int)max_diff and both arguments must be whole numbers, 0 <= min_valid <= 256, 0 <= max_diff <= 255
 *   (MI_E_PARAM).  A COMPONENT is a connected component of the joined graph within one frame.
 *   max_diff negative or not finite, min_valid NaN: MI_E_PARAM (min_valid = -inf is legal: every non-NaN pixel is valid).
 *
 * Components.  labels (batch, h, w) int32: the smallest y * w + x of the pixel's component, MI_FILTER_NO_LABEL = -1 on an invalid
 *   pixel.  sizes (batch, h, w) int32: the number of pixels of its component, 0 on an invalid pixel; sizes may be NULL.  The
 *   definition makes the output unique, whatever the algorithm.
 *
 * Speckle (float32).  out = in's bits where the pixel is valid and its component has MORE than max_size pixels, invalid_value
 *   elsewhere: invalid inputs (NaN among them) are canonicalised too.  removed (batch, h, w) bytes, may be NULL: 1 where a VALID
 *   pixel was dropped, 0 elsewhere.  out may be in (exactly; a partial overlap is undefined).  max_size >= 0 (0 keeps every valid
 *   pixel), and invalid_value must be invalid itself: invalid_value >= min_valid is MI_E_PARAM; a NaN is fine.
 *   cv2.filterSpeckles on float disparities with maxSpeckleSize = max_size, maxDiff = max_diff.
 *
 * Median (float32).  k is 3 or 5 (else MI_E_PARAM); the window is k x k with a replicate border (taps are read at
 *   clamp(y + dy, 0, h - 1), clamp(x + dx, 0, w - 1): a replicated tap counts as often as it is read).  An invalid centre gives
 *   invalid_value.  Otherwise the result is the element of rank (n - 1) / 2 (from 0) among the window's n VALID taps, ordered by
 *   the monotone uint32 key of the float (key = ~bits for a set sign bit, bits | 0x80000000 otherwise), so -0.0 precedes +0.0
 *   and the result is one of the taps, bit for bit.  It does not fill holes.  out == in is MI_E_PARAM.  No workspace.
 *
 * Out of scope: a minimum disparity other than what min_valid expresses (disparities are those of d >= 0), hole filling,
 *   bilateral smoothing, 8-connectivity, uint16 frames. */
#define MI_FILTER_MAX_PIXELS 67108864
#define MI_FILTER_NO_LABEL -1
#define MI_FILTER_TILE_W 64
#define MI_FILTER_TILE_H 16
enum { MI_FILTER_U8 = 0, MI_FILTER_F32 = 1 };
/* the code byte a caller (pytorch_model.stereo.StereoMatcher) writes on a pixel the speckle filter dropped, next to
 * MI_STEREO_OK = 0, MI_STEREO_NOT_UNIQUE = 1, MI_STEREO_LR = 2 */
enum { MI_FILTER_SPECKLE = 3 };

/* The workspace mi_filter_components and mi_filter_speckle want for a request, in bytes: two int32 per pixel (the parent of the
 * union-find forest and the component counts) rounded up to 16, or 0 for a request they refuse by shape or pixel count.  A
 * workspace of fewer bytes is MI_E_CAPACITY. */
MI_API size_t mi_filter_workspace_bytes(int batch, int h, int w);

/* values (batch, h, w) uint8 (type MI_FILTER_U8) or float32 (MI_FILTER_F32, 4-byte aligned); labels, sizes int32, 4-byte aligned;
 * workspace 16-byte aligned (MI_E_ALIGN).  Four launches: a 64 x 16 tile labelled in LDS by one workgroup (row runs by a wave
 * ballot, unions between rows, the local counts); unions across the tile borders; one count per local component added to its
 * root; the labels and sizes. */
MI_API int mi_filter_components(const void *values, int type, int batch, int h, int w, float min_valid, float max_diff,
                                int32_t *labels, int32_t *sizes, void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* in, out (batch, h, w) float32, 4-byte aligned; removed bytes or NULL; workspace 16-byte aligned.  The first three launches of
 * mi_filter_components, then one thread per pixel. */
MI_API int mi_filter_speckle(const float *in, int batch, int h, int w, float min_valid, float max_diff, int max_size,
                             float invalid_value, float *out, uint8_t *removed, void *workspace, size_t workspace_bytes,
                             mi_stream_t stream);

/* in, out (batch, h, w) float32, 4-byte aligned.  One launch, one thread per pixel: a sorting network over the keys in
 * registers, 0xFFFFFFFF standing for an invalid tap. */
MI_API int mi_filter_median(const float *in, int batch, int h, int w, int k, float min_valid, float invalid_value, float *out,
                            mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_FILTER_H */
