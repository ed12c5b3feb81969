/* mi355x_match_rectify.h -- the camera-rectification section (K34) of the C ABI, with a header and a library of its own:
 * libmi355x_match_rectify.so exports exactly the MI_API declarations below, under the conventions (return values, MI_E_*,
 * mi_stream_t, ABI version) of include/mi355x_match.h, which this header includes; libmi355x_match.so stays the export of
 * that header and nothing else.  The Python binding reads it next to it (onnx_image_processing_amd/_native.py,
 * RECTIFY_SIGNATURES, RECTIFY_CONSTANTS, load_rectify()). */
#ifndef MI355X_MATCH_RECTIFY_H
#define MI355X_MATCH_RECTIFY_H

#include "mi355x_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- camera rectification (K34): a real lens -> the ideal pinhole camera every other section assumes --------------------------------
 * The pose entries take normalised, undistorted image points and mi_stereo_* takes rectified views; this section produces
 * both on the device: a sampling map per camera (cv2.initUndistortRectifyMap), the remap of a batch of frames through it
 * (cv2.remap), the undistortion of keypoints (cv2.undistortPoints) and, on the host, the rectifying rotations of a stereo rig
 * (cv2.stereoRectify).  Entries under the contract of the K30 to K33 sections: pure functions of their arguments, no
 * allocation, no synchronisation, no memset, one stream, no atomics, the same bits alone or inside a batch, capturable into a
 * hipGraph (the camera arrays are read on the host during the call and travel as kernel arguments); outputs may hold
 * anything on entry and every output element is written; MI_E_* before any launch.  Order of the checks: NULL, shape,
 * parameters, alignment, capacity.  An extent < 1: MI_E_SHAPE; an image extent above MI_RECTIFY_MAX_DIM, a batch above
 * MI_RECTIFY_MAX_BATCH, batch * n above MI_RECTIFY_MAX_POINTS: MI_E_PARAM.
 *
 * The formulas are OpenCV's camera models restated AS REMEMBERED: no cv2 build was available to compare against, so agreement
 * with cv2 is UNMEASURED.  The contract is the arithmetic stated here, operation by operation (nothing is fused), not cv2.
 *
 * Camera.  HOST arrays of doubles.  k, k_new: 3 x 3 row-major, fx = k[0], fy = k[4], cx = k[2], cy = k[5]; k[1] (skew) and
 *   k[3] must be 0, the last row 0 0 1, fx, fy > 0, everything finite, else MI_E_PARAM.  dist: MI_RECTIFY_COEFFS = 8 finite
 *   doubles; MI_RECTIFY_PINHOLE: k1 k2 p1 p2 k3 k4 k5 k6 (radial-tangential with the rational denominator);
 *   MI_RECTIFY_FISHEYE: Kannala-Brandt k1 .. k4, and dist[4 .. 7] must be 0 (MI_E_PARAM).  r: 3 x 3 row-major, finite, the
 *   rectifying rotation (camera frame -> rectified frame); NULL is the identity.  It is not tested for orthonormality.
 *
 * Forward model D(x, y) of a normalised point, float64:  r2 = x x + y y.
 *   pinhole: num = 1 + r2 (k1 + r2 (k2 + r2 k3)), den = 1 + r2 (k4 + r2 (k5 + r2 k6)); no image unless den > 0;
 *     radial = num / den, a = (2 x) y, xd = x radial + (p1 a + p2 (r2 + (2 x) x)), yd = y radial + (p1 (r2 + (2 y) y) + p2 a).
 *     The model is NOT guarded against folding over at large radii (where d|D|/dr turns negative, far points land inside
 *     the frame again); OpenCV does not guard against it either.
 *   fisheye: rr = sqrt(r2), th = atan(rr), t2 = th th, thd = th (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))), s = thd / rr, or 1
 *     at rr = 0; xd = x s, yd = y s.
 *   Source pixel: sx = fx xd + cx, sy = fy yd + cy.
 *
 * atan and tan are the section's own (csrc/rectify_math.h), from + - * / sqrt only, so that host, device and the numpy
 *   oracle agree bit for bit.  atan(x): sign and |x| apart; above 1 the reciprocal (pi/2 - atan(1/x)); two half-angle
 *   reductions x <- x / (1 + sqrt(1 + x x)) (then |x| <= tan(pi/16)); the odd Taylor polynomial through x^23 by Horner in x x;
 *   times 4.  Against numpy.arctan on 200001 points of [-50, 50] and 20001 logarithmic ones up to 1e12: at most 4.5e-16
 *   absolute, 4 ulp.  tan(t), 0 <= t <= MI_RECTIFY_MAX_THETA = 1.5 rad (85.9 degrees from the axis; no reduction, the domain
 *   is the limit): sin and cos by their Taylor series through t^23 and t^22, nested as 1 - z / (m (m + 1)) (...), one
 *   division.  Against numpy.tan on 150001 points of [0, 1.5]: at most 20 ulp (relative 2.6e-15; tan is ill-conditioned
 *   near the limit, condition number 21).
 *
 * Map (mi_rectify_map).  map is (h, w, 2) int32: the source x and y of destination pixel (v, u) in units of 1/32 pixel
 *   (MI_RECTIFY_SUBPIXEL_BITS = 5), or MI_RECTIFY_OUTSIDE in both components where there is no source pixel.  float64:
 *   x' = (u - cx_n) / fx_n, y' = (v - cy_n) / fy_n;  X = R^T (x', y', 1), X_i = (r[i] x' + r[3 + i] y') + r[6 + i];  outside
 *   unless X_z > 0;  x = X_x / X_z, y = X_y / X_z;  (sx, sy) as above (outside where the pinhole model has no image);
 *   t = floor(s 32 + 0.5) per axis;  outside unless -64 <= t_x < 32 (src_w + 1) and -64 <= t_y < 32 (src_h + 1) (a NaN or an
 *   infinity fails this);  q = (int)t, X = q >> 5;  outside unless -1 <= X_x < src_w and -1 <= X_y < src_h, i.e. when no tap
 *   of the 2 x 2 footprint {X, X + 1} can lie in the frame.  mask (h, w) bytes, may be NULL: 1 where every tap with a non-zero
 *   weight lies inside the source (X >= 0, and X <= extent - 1 at a = q & 31 = 0 or X + 1 <= extent - 1 otherwise, both
 *   axes), else 0.
 *
 * Remap (mi_rectify_remap).  src (batch, src_h, src_w), dst (batch, h, w) of one element type: MI_RECTIFY_U8,
 *   MI_RECTIFY_U16, MI_RECTIFY_F32.  One map serves the batch.  interpolation MI_RECTIFY_NEAREST for all three types,
 *   MI_RECTIFY_LINEAR for U8 and F32 (U16 with LINEAR is MI_E_PARAM: depth must not be blended across edges).  The border
 *   is the constant border_value, per tap: a tap outside the frame reads it; for U8 / U16 it must be an integer in
 *   0 .. 255 / 0 .. 65535 (MI_E_PARAM), for F32 it is converted to float32 (a NaN is legal).  A map element whose x or y is
 *   MI_RECTIFY_OUTSIDE gives border_value.  Else, per axis, X = q >> 5 and a = q & 31 (arithmetic shift), taps
 *   p00 = S[Y][X], p01 = S[Y][X + 1], p10 = S[Y + 1][X], p11 = S[Y + 1][X + 1]:
 *   U8 linear: (p00 (32 - ax)(32 - ay) + p01 ax (32 - ay) + p10 (32 - ax) ay + p11 ax ay + 512) >> 10, in integers.
 *   F32 linear: top = p00 + (p01 - p00) * (ax / 32.0f), bot = p10 + (p11 - p10) * (ax / 32.0f),
 *     out = top + (bot - top) * (ay / 32.0f); a tap whose weight is zero is not used: at ax = 0 top = p00 and bot = p10, at
 *     ay = 0 out = top, so ax = ay = 0 gives p00 exactly (its bits), even beside a NaN or the border.  Any other result that
 *     is a NaN is written as the quiet NaN 0x7FC00000: which NaN an operation returns differs between processors.
 *   Nearest: S[(qy + 16) >> 5][(qx + 16) >> 5], or border_value when that is outside the frame.
 *   No index leaves the frame.  Any int32 is a legal map element.
 *
 * Points (mi_rectify_points).  pts (batch, n, 2) float32 raw pixels (u, v); out (batch, n, 2) float32; ok (batch, n) bytes.
 *   float64 inside: xd = (u - cx) / fx, yd = (v - cy) / fy.
 *   pinhole: x = xd, y = yd, then `iterations` times (1 .. MI_RECTIFY_MAX_ITERATIONS, else MI_E_PARAM) with r2, num, den, a
 *     of the forward model at (x, y):  x = (xd - (p1 a + p2 (r2 + (2 x) x))) * (den / num),
 *     y = (yd - (p1 (r2 + (2 y) y) + p2 a)) * (den / num), both from the old (x, y).
 *   fisheye: thd = sqrt(xd xd + yd yd), th = thd, then `iterations` times Newton on the polynomial:
 *     th = th - (th (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))) - thd) / (1 + t2 (3 k1 + t2 (5 k2 + t2 (7 k3 + t2 (9 k4)))));
 *     fails unless 0 <= th <= MI_RECTIFY_MAX_THETA; s = tan(th) / thd, or 1 at thd = 0; x = xd s, y = yd s.
 *   The result is pushed through the forward model: fails when the model has no image or when the pixel it gives lies more
 *     than max_residual_px (> 0 and finite, else MI_E_PARAM) from (u, v): unless ex ex + ey ey <= max_residual_px^2.
 *   X = R (x, y, 1), X_i = (r[3 i] x + r[3 i + 1] y) + r[3 i + 2]; fails unless X_z > 0.  out = (X_x / X_z, X_y / X_z), normalised
 *     coordinates of the rectified camera, when k_new is NULL (what the pose estimators take); otherwise
 *     (fx_n (X_x / X_z) + cx_n, fy_n (X_y / X_z) + cy_n).  Fails when a float32 result is not finite.
 *   ok = 1 and the result, or ok = 0 and out = (0, 0).
 *
 * Stereo rig (mi_rectify_stereo_rig).  Host only: no stream, no GPU call; every array is a host address.  k1, k2 cameras as
 *   above; r (3 x 3) and t (3) with X2 = R X1 + t, camera 1 on the left; h, w the output size.  Only + - * / sqrt:
 *   b = sqrt((t0 t0 + t1 t1) + t2 t2);  c = -R^T t (camera 2's centre in camera 1's frame), c_i = -((r[i] t0 + r[3 + i] t1) +
 *   r[6 + i] t2);  new x = c / b;  z_mean = (r[6], r[7], 1 + r[8]) (the sum of both optical axes in camera 1's frame);
 *   y' = z_mean x X (cross product), new y = y' / |y'|;  new z = x X y.  r1 has x, y, z as rows; r2 = r1 R^T,
 *   r2[i][j] = (r1[i][0] r[3 j] + r1[i][1] r[3 j + 1]) + r1[i][2] r[3 j + 2].  k_new: f = (fy1 + fy2) / 2 on both axes,
 *   the principal point ((w - 1) / 2, (h - 1) / 2).  baseline = b, fb = f b: the value mi_stereo_depth wants.
 *   MI_E_PARAM: an input that is not finite or a bad camera; b = 0; |y'| <= 1e-6 |z_mean| (the mean optical axis is parallel to
 *   the baseline, or the axes are opposite); new x does not point to +x of camera 1 (unless x_0 > 0 and x_0 >= |x_1|: a swapped
 *   or vertical rig).  No alpha / valid-ROI optimisation: the mask of mi_rectify_map says what is valid.  Map the left
 *   camera with (k1, dist1, r1, k_new) and the right one with (k2, dist2, r2, k_new). */
#define MI_RECTIFY_COEFFS 8
#define MI_RECTIFY_SUBPIXEL_BITS 5
#define MI_RECTIFY_OUTSIDE -2147483648
#define MI_RECTIFY_MAX_DIM 16384
#define MI_RECTIFY_MAX_BATCH 65536
#define MI_RECTIFY_MAX_POINTS 16777216
#define MI_RECTIFY_MAX_ITERATIONS 64
#define MI_RECTIFY_MAX_THETA 1.5
enum { MI_RECTIFY_PINHOLE = 0, MI_RECTIFY_FISHEYE = 1 };
enum { MI_RECTIFY_U8 = 0, MI_RECTIFY_U16 = 1, MI_RECTIFY_F32 = 2 };
enum { MI_RECTIFY_NEAREST = 0, MI_RECTIFY_LINEAR = 1 };

/* map 8-byte aligned (MI_E_ALIGN); mask may be NULL.  One thread per destination pixel. */
MI_API int mi_rectify_map(int model, const double *k, const double *dist, const double *r, const double *k_new, int src_h,
                          int src_w, int h, int w, int32_t *map, uint8_t *mask, mi_stream_t stream);

/* src, dst aligned to their element (MI_E_ALIGN), map 8-byte aligned.  A lane takes four consecutive destination pixels of
 * a row and a workgroup a 64 x 16 tile of the destination, for eight frames one after the other with the map elements in
 * registers; with w a multiple of 4, map 16-byte and dst 16-byte aligned the map comes in 16-byte loads and the four results
 * leave in one store, otherwise element by element, with the same results. */
MI_API int mi_rectify_remap(const void *src, int type, int batch, int src_h, int src_w, const int32_t *map, int h, int w,
                            int interpolation, double border_value, void *dst, mi_stream_t stream);

/* pts, out 4-byte aligned (MI_E_ALIGN).  r and k_new may be NULL.  One thread per point. */
MI_API int mi_rectify_points(const float *pts, int batch, int n, int model, const double *k, const double *dist, const double *r,
                             const double *k_new, int iterations, double max_residual_px, float *out, uint8_t *ok,
                             mi_stream_t stream);

/* Host only.  r1, r2, k_new: 9 doubles each; baseline, fb: one double each; all host addresses, all required. */
MI_API int mi_rectify_stereo_rig(const double *k1, const double *k2, const double *r, const double *t, int h, int w, double *r1,
                                 double *r2, double *k_new, double *baseline, double *fb);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_MATCH_RECTIFY_H */
