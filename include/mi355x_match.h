/*
 * mi355x_match.h -- C ABI of the MI355X-native image-matching hot path.
 *
 * The reference (fateshelled/onnx_image_processing) has no FFI: its boundary for this
 * path is the Python nn.Module.forward() signatures under pytorch_model/{detector,utils,
 * descriptor,matching,pointcloud,depth,threshold,vo}.  Each entry point below is what a binding for one of those
 * forward()s calls; the reference interface it replaces is cited per function
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch.Tensor.data_ptr() on ROCm);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued
 *     asynchronously and is ordered as if it ran on `stream` (after earlier work on it, before later
 *     work), nothing synchronises, nothing allocates device memory.  mi_sinkhorn_dots (and
 *     mi_match_pairs through it; mi_sinkhorn with a workspace likewise) overlaps the halves of a batch of >= 64 pairs on helper streams
 *     joined back into `stream` by events; those helpers belong to the calling (device, stream) and
 *     are created on its first such call (mi_release_stream_resources frees them).  WHICH streams the
 *     halves run on is tuned per calling stream and per shape (batch, n, m, iterations): the first
 *     9 such calls of a shape try three schedules -- halves on {stream, helper}, on {helper, helper},
 *     unsplit -- three times each, every trial call bracketed by two hipEventRecord on `stream`; later
 *     calls read the elapsed times without waiting (hipEventQuery) and use the fastest schedule; the
 *     decision is re-measured every 8192 calls.  Same results bit for bit whatever the schedule.  Inside
 *     a stream capture nothing is tried, recorded or queried: the capture takes the decision in force,
 *     or the unsplit schedule when there is none.  mi_sinkhorn_dots_schedule reports the schedule in
 *     force, mi_sinkhorn_dots_set_schedule pins one, and the flag MI_SOLVER_NO_FORK keeps every kernel
 *     of the call on `stream` (no helper stream, no event, no tuning);
 *   - threads and devices: the device of `stream` must be the calling thread's current device.  Calls
 *     on DIFFERENT streams may run concurrently from different host threads; calls on the SAME
 *     stream must be serialised by the caller (as for any HIP stream).  Mutable state of the library:
 *     (a) per calling (device, stream): the helper streams / events above and the schedule tuner's
 *     trial times and decisions (mutex-guarded); (b) per device: one cached occupancy query (the
 *     single-launch Sinkhorn form) and the compute-unit count.  No process-wide switches (the
 *     kernel-variant test hooks of include/mi355x_match_debug.h exist only in the separate
 *     libmi355x_match_debug.so);
 *   - co-residency: ONE kernel of this library needs its whole grid resident on the device at the same
 *     time -- the single-launch Sinkhorn form mi_sinkhorn_dots / mi_match_pairs use for <= 8 pairs
 *     (<= 128 workgroups of 512 threads whose bands hand column sums to each other inside the launch).
 *     The library checks on the host that the grid fits the device it sees (occupancy x compute units;
 *     a CU-masked or partitioned device takes the multi-launch form instead), and work on other streams
 *     only delays it: its workgroups become resident as that work drains.  A band that still has not
 *     arrived after ~1 s of polling is a failure, and a loud one: the call's status word
 *     (mi_sinkhorn_dots_status_word) becomes non-zero, the pair's duals are NaN (so is P), and
 *     mi_mnn_from_duals_dots / mi_match_pairs return valid = 0 for every match of the call.  A caller
 *     that cannot accept that risk (a GPU shared with long-running foreign kernels) passes
 *     MI_SOLVER_MULTI_LAUNCH and gets the form with no cross-workgroup dependency;
 *   - tensors are dense row-major float32 unless stated; images are (n, 1, h, w);
 *   - return value: 0 = launched; > 0 = hipError_t of the failed launch; < 0 = MI_E_*
 *     argument error detected on the host before any launch.
 */
#ifndef MI355X_MATCH_H
#define MI355X_MATCH_H

#include <stddef.h>
#include <stdint.h>

/* the exported symbols: the library is built with -fvisibility=hidden, only these declarations are visible */
#define MI_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mi_stream_t;

enum {
  MI_OK = 0,
  MI_E_NULL = -1,     /* required pointer is NULL */
  MI_E_SHAPE = -2,    /* non-positive or inconsistent extent */
  MI_E_PARAM = -3,    /* parameter outside the supported set */
  MI_E_CAPACITY = -4, /* workspace / capacity too small for the request */
  MI_E_ALIGN = -5     /* pointer or pitch not aligned as documented */
};

/* descriptor output modes of mi_sparse_bad (reference descriptor/bad.py:561-567) */
enum { MI_BAD_RAW = 0, MI_BAD_SOFT = 1, MI_BAD_HARD = 2 };
/* distance types (reference matching/sinkhorn.py:95-108) */
enum { MI_DIST_L2 = 0, MI_DIST_L1 = 1 };
/* smallest epsilon of the packed (uint16 dot product) Sinkhorn form, see mi_sinkhorn_dots */
#define MI_DOTS_MIN_EPSILON 0.005
/* flags of mi_sinkhorn_dots / mi_match_params (see "co-residency" above) */
enum {
  MI_SOLVER_DEFAULT = 0,
  MI_SOLVER_MULTI_LAUNCH = 1, /* never the single-launch Sinkhorn form */
  MI_SOLVER_NO_FORK = 2,      /* never fork onto helper streams: every kernel of the call on `stream` (e.g. for a
                                 capture that must not contain cross-stream branches, or a device with one hardware
                                 queue); bit-identical results, the >= 64-pair Sinkhorn runs ~8 % slower */
  MI_SOLVER_DOTS_BELOW_1024 = 4 /* mi_sinkhorn_dots only: the caller vouches that every dot product is < 1024 (descriptors
                                 of at most 1023 bits -- mi_match_pairs sets it by itself from num_bits).  The row
                                 kernel of the batched form then reads a uint16 as the fp16 denormal dot * 2^-24 and
                                 multiplies in one mixed-precision instruction instead of converting first; the same
                                 duals bit for bit.  A value >= 1024 under this flag reads as some other fp16: wrong
                                 duals, no fault.  The row padding (columns m..pitch) may hold anything, as without the
                                 flag. */
};
/* stream schedules of mi_sinkhorn_dots for >= 64 pairs (see the conventions above) */
enum {
  MI_SCHEDULE_UNDECIDED = -1,  /* nothing decided or pinned yet for this stream / shape */
  MI_SCHEDULE_CALLER_HELPER = 0, /* halves on {caller's stream, helper 0} */
  MI_SCHEDULE_TWO_HELPERS = 1, /* halves on {helper 0, helper 1} */
  MI_SCHEDULE_UNSPLIT = 2      /* one part on the caller's stream */
};

MI_API int mi_abi_version(void);
MI_API const char *mi_error_string(int code);
/* Frees the helper streams / events held for (current device, stream), see the conventions above.  Call it
 * before destroying a stream that was passed to mi_sinkhorn_dots / mi_sinkhorn / mi_match_pairs with >= 64 pairs; the
 * stream's helper work must have completed (synchronise the stream first). */
MI_API int mi_release_stream_resources(mi_stream_t stream);
/* The stream schedule in force for mi_sinkhorn_dots calls of this shape on (current device, stream): the pinned
 * schedule, the tuner's decision, or MI_SCHEDULE_UNDECIDED.  Never blocks (finished trials are collected with
 * hipEventQuery).  Hosts log it next to their timings; a capture taken while it is undecided records the unsplit
 * schedule. */
MI_API int mi_sinkhorn_dots_schedule(mi_stream_t stream, int batch, int n, int m, int iterations);
/* Pin `schedule` (MI_SCHEDULE_CALLER_HELPER .. MI_SCHEDULE_UNSPLIT) for every shape on (current device, stream) --
 * nothing is tried or timed while pinned --, or MI_SCHEDULE_UNDECIDED to unpin and forget every decision (tuning starts
 * over).  Creates the stream's helper resources if they do not exist yet (MI_E_CAPACITY when the library already serves
 * 64 caller streams). */
MI_API int mi_sinkhorn_dots_set_schedule(mi_stream_t stream, int schedule);

/* ---- detector/shi_tomasi.py:66-112  ShiTomasiScore.forward ---------------------------------
 * score[n,1,h,w] = max(0, (a+c)/2 - sqrt(((a-c)/2)^2 + b^2 + 1e-10)) of the Sobel structure
 * tensor summed over block_size^2 (replicate padding of image and of the product maps).
 * block_size: positive odd.  Bit-exact vs the reference for uint8-valued input, block 3. */
MI_API int mi_corner_response(const float *image, int n, int h, int w, int block_size, float *score,
                       mi_stream_t stream);
/* ---- u8 ingest (sample/visual_odometry.py:65-92 load_image_from_array, sample/image_matching.py:42-46: a uint8 gray
 * frame is converted to float32 (1,1,H,W) on the host before the model sees it).  The _u8 entry points take the
 * uint8 frame itself: the same results as the float32 entry point on the converted frame, bit for bit, with 1 instead
 * of 4 bytes per pixel read (corner response: 5 instead of 8 B/px of HBM traffic; a pair costs 0.6 instead of
 * 2.5 MB of PCIe when frames are streamed from the host).  mi_convert_u8_f32 is that conversion on the device, for
 * the entry points that have no uint8 form.  The first two thirds of that host function -- colour to gray, resize to
 * the model's resolution -- are mi_ingest_frames at the end of this header. */
MI_API int mi_corner_response_u8(const uint8_t *image, int n, int h, int w, int block_size, float *score,
                          mi_stream_t stream);
MI_API int mi_convert_u8_f32(const uint8_t *src, long long count, float *dst, mi_stream_t stream);
/* mi_corner_response / _u8 (pixels_are_u8 = 0 / 1) with dynamic tile scheduling for large batches: tile_counter =
 * MI_TILE_COUNTER_BYTES of device memory, 4-byte aligned, of ANY content: the call clears the block on `stream`
 * (with a small kernel -- no entry point of this library issues hipMemsetAsync, whose captured form does not survive
 * hipGraph replays on ROCm 7.2) ahead of the kernel that draws tickets from it, so a block left dirty by a launch that died cannot
 * make a later call skip tiles.  A block must not be shared by calls that may run concurrently (different streams
 * need different blocks).  NULL = the static schedule of the two entry points above.  Same scores; equally sized
 * static shares do not finish together because the SIMDs issue oldest-first, tickets make them. */
#define MI_TILE_COUNTER_BYTES 16640
MI_API int mi_corner_response_balanced(const void *image, int pixels_are_u8, int n, int h, int w, int block_size, float *score,
                                uint32_t *tile_counter, mi_stream_t stream);
/* image1 / image2 of a matcher (two equally shaped batches of per_set images) behind ONE launch, like mi_match_pairs
 * does inside: score is (2 * per_set, h, w), batch a first; NMS and top-k then run on one batch of twice the size.
 * The same per-image results as two calls; half the launches and one tail instead of two (the _pair entries below:
 * mi_sparse_bad_pair, mi_angle_at_keypoints_pair, mi_sparse_bad_oriented_pair; AKAZE: mi_akaze_scale_sets). */
MI_API int mi_corner_response_pair(const void *image_a, const void *image_b, int pixels_are_u8, int per_set, int h, int w,
                            int block_size, float *score, uint32_t *tile_counter, mi_stream_t stream);

/* ---- utils/keypoint_utils.py:12-44  apply_nms_maxpool ---------------------------------------
 * mask = 1.0f where score >= max over the (2r+1)^2 window (outside image = -inf) - 1e-7. */
MI_API int mi_nms_mask(const float *score, int n, int h, int w, int radius, float *mask, mi_stream_t stream);

/* ---- utils/keypoint_utils.py:71-92 (candidate stage of select_topk_keypoints) ---------------
 * Emits one 64-bit key per surviving pixel:
 *     m = score * mask * border ; survive iff m > max(score_threshold, 0)
 *     key = (float_bits(m) << 32) | (0xFFFFFFFF - (y*w + x))
 * The candidate buffer is segmented: mi_candidate_layout(h, w) gives S segments (one per
 * 128x32 image tile) of C slots each; cand is uint64[n][S][C], count is uint32[n][S].  Every
 * count entry is written (no pre-zeroing), a segment holds at most its tile's pixels (cannot
 * overflow), and no global atomics are used; the order inside a segment is unspecified.
 * mi_nms_candidates fuses the NMS of mi_nms_mask (mask never materialised);
 * mi_select_candidates takes an explicit mask (the reference's two-call form). */
MI_API int mi_candidate_layout(int h, int w, int *segments, int *segment_capacity);
MI_API int mi_nms_candidates(const float *score, int n, int h, int w, int radius, float score_threshold,
                      int border_margin, uint64_t *cand, uint32_t *count, mi_stream_t stream);
MI_API int mi_select_candidates(const float *score, const float *mask, int n, int h, int w,
                         float score_threshold, int border_margin, uint64_t *cand, uint32_t *count,
                         mi_stream_t stream);

/* ---- utils/keypoint_utils.py:94-115 (top-k stage of select_topk_keypoints) ------------------
 * For each image: the k largest keys over all its segments, descending => (score desc, linear
 * index asc).  keypoints[n,k,2] = (y, x) as float, (-1,-1) beyond the candidate count;
 * kscores[n,k].  1 <= k <= 4096. */
MI_API int mi_topk_keypoints(const uint64_t *cand, const uint32_t *count, int segments, int segment_capacity,
                      int n, int w, int k, float *keypoints, float *kscores, mi_stream_t stream);

/* ---- descriptor/bad.py:436-576  SparseBAD.forward (non-oriented, sampling_mode="nearest") ---
 * pair_geom[p] = x1 | x2<<5 | y1<<10 | y2<<15 | r<<20 in the 32x32 patch frame (table rows of
 * descriptor/bad_params.py), pair_thr[p] the learned threshold.  num_pairs % 64 == 0, <= 1024.
 * desc (n,k,num_pairs) f32 and/or bits (n,k,num_pairs/32) u32 may be NULL (bits only for HARD).
 * Box sums are exact (fp64 summed-area table over a replicate-clamped 34x34 window).
 * plan (optional, may be NULL): device buffer of mi_bad_plan_bytes(num_pairs) bytes, 16-byte
 * aligned, filled once per pair table by mi_bad_plan_build.  With a plan, HARD-mode keypoints
 * with integer coordinates inside the image that sit on an integer-valued (uint8) patch take an
 * int32 fast path (precomputed table corners when >= 15 px from the border); results are identical.
 * status (optional, required for the fast path): n*k bytes of workspace; the fast kernel marks
 * the keypoints it handled and the general kernel visits the rest.
 * mi_bad_plan_build is the one set-up call of this ABI that synchronises: it reads the table back,
 * orders every pair's table-corner reads on the host so that the fast kernel's LDS gathers hit as few
 * banks twice as possible, and uploads the plan (two stream synchronisations; not hipGraph-capturable). */
MI_API size_t mi_bad_plan_bytes(int num_pairs);
MI_API int mi_bad_plan_build(const uint32_t *pair_geom, const float *pair_thr, int num_pairs, void *plan,
                      mi_stream_t stream);
MI_API int mi_sparse_bad(const float *image, int n, int h, int w, const float *keypoints, int k,
                  const uint32_t *pair_geom, const float *pair_thr, int num_pairs, int mode,
                  float temperature, int normalize, float *desc, uint32_t *bits, const void *plan,
                  uint8_t *status, mi_stream_t stream);

/* u8 ingest form of mi_sparse_bad (see mi_corner_response_u8): identical results from a uint8 image. */
MI_API int mi_sparse_bad_u8(const uint8_t *image, int n, int h, int w, const float *keypoints, int k,
                     const uint32_t *pair_geom, const float *pair_thr, int num_pairs, int mode,
                     float temperature, int normalize, float *desc, uint32_t *bits, const void *plan,
                     uint8_t *status, mi_stream_t stream);
/* mi_sparse_bad / _u8 for image1 / image2 behind one launch (see mi_corner_response_pair): keypoints (2 * per_set, k, 2),
 * status (2 * per_set * k) and the outputs hold batch a first. */
MI_API int mi_sparse_bad_pair(const void *image_a, const void *image_b, int pixels_are_u8, int per_set, int h, int w,
                       const float *keypoints, int k, const uint32_t *pair_geom, const float *pair_thr, int num_pairs,
                       int mode, float temperature, int normalize, float *desc, uint32_t *bits, const void *plan,
                       uint8_t *status, mi_stream_t stream);

/* ---- descriptor/bad.py:62-110,189-218  BADDescriptor.forward (dense, non-oriented) ------------
 * out (n, num_pairs, h, w): the BAD response at every pixel, raw / sigmoid(-c*T) / (c <= 0),
 * box centres clamped into the image, boxes over the replicate-padded image; exact fp64 box sums
 * (the reference's fp32 integral image is itself inexact above 2^24).
 * mi_gather_descriptors: descriptor/bad.py:221-333, (batch,d,h,w) map sampled at keypoints
 * (batch,nk,2) -> (batch,nk,d); bilinear = 0: integer truncation, 1: grid_sample bilinear/border. */
MI_API int mi_bad_dense(const float *image, int n, int h, int w, const uint32_t *pair_geom, const float *pair_thr,
                 int num_pairs, int mode, float temperature, float *out, mi_stream_t stream);
/* descriptor/bad.py:112-187 (_compute_diff_map_oriented): the same map with every pixel's pair offsets
 * rotated by orientation (n,1,h,w) there and the box means sampled bilinearly (exact box sums). */
MI_API int mi_bad_dense_oriented(const float *image, const float *orientation, int n, int h, int w,
                          const uint32_t *pair_geom, const float *pair_thr, int num_pairs, int mode,
                          float temperature, float *out, mi_stream_t stream);
MI_API int mi_gather_descriptors(const float *descriptor_map, int batch, int d, int h, int w, const float *keypoints,
                          int nk, int bilinear, float *out, mi_stream_t stream);

/* ---- orientation/angle_estimation.py:86-172  AngleEstimator.forward --------------------------
 * angle = atan2(m01, m10) of the Gaussian-weighted first moments, conv with ZERO padding.
 * moment_kernels: the module's (2,1,ps,ps) weight buffer (x*G then y*G), patch_size odd <= 31.
 * mi_angle_map writes the dense (n,1,h,w) map; mi_angle_at_keypoints writes theta (n,k) only at
 * the keypoints (what descriptor/bad.py:487-500 samples from the map, same nearest rounding). */
MI_API int mi_angle_map(const float *image, int n, int h, int w, int patch_size, const float *moment_kernels,
                 float *angle, mi_stream_t stream);
MI_API int mi_angle_at_keypoints(const float *image, int n, int h, int w, const float *keypoints, int k,
                          int patch_size, const float *moment_kernels, float *theta, mi_stream_t stream);
/* mi_angle_at_keypoints for image1 / image2 behind one launch (see mi_corner_response_pair): keypoints (2 * per_set, k, 2),
 * theta (2 * per_set, k), batch a first. */
MI_API int mi_angle_at_keypoints_pair(const float *image_a, const float *image_b, int per_set, int h, int w,
                               const float *keypoints, int k, int patch_size, const float *moment_kernels, float *theta,
                               mi_stream_t stream);

/* ---- descriptor/bad.py:487-517  SparseBAD.forward, oriented branch; and sampling_mode "bilinear" --
 * Pair offsets rotated by the keypoint's angle, which comes either from a dense orientation map
 * (n,1,h,w) sampled at the keypoint, or from a per-keypoint array (n,k): exactly one non-NULL.
 * bilinear = 0: box centre = nearest pixel (grid_sample "nearest"); 1: the box means of the four
 * neighbouring centres interpolated as grid_sample "bilinear" does (bad.py:535-549), response and
 * sign test in fp32.  The non-oriented bilinear case is angle 0 for every keypoint.
 * status (optional): n*k bytes of workspace; when given, keypoints on uint8-valued windows are done
 * with an int32 table (half the LDS, same results) and only the rest with the fp64 one.
 * max_reach: an upper bound, in pixels, of |pair offset from the patch centre| + box radius over the pair table, or 0 if
 * unknown.  0 < max_reach <= 22.5 (both reference tables: 22.22) lets the nearest mode use a 48 x 48 instead of a
 * 60 x 60 window per keypoint (same results, more keypoints in flight); a bound the table exceeds is a contract
 * violation (boxes clipped to the window). */
MI_API int mi_sparse_bad_oriented(const float *image, int n, int h, int w, const float *keypoints, int k,
                           const float *orientation_map, const float *keypoint_angles,
                           const uint32_t *pair_geom, const float *pair_thr, int num_pairs, int mode,
                           float temperature, int normalize, int bilinear, float max_reach, float *desc,
                           uint32_t *bits, uint8_t *status, mi_stream_t stream);
/* mi_sparse_bad_oriented with per-keypoint angles for image1 / image2 behind one launch (see mi_corner_response_pair):
 * keypoints (2 * per_set, k, 2), keypoint_angles (2 * per_set, k), status and the outputs hold batch a first. */
MI_API int mi_sparse_bad_oriented_pair(const float *image_a, const float *image_b, int per_set, int h, int w,
                                const float *keypoints, int k, const float *keypoint_angles, const uint32_t *pair_geom,
                                const float *pair_thr, int num_pairs, int mode, float temperature, int normalize,
                                int bilinear, float max_reach, float *desc, uint32_t *bits, uint8_t *status,
                                mi_stream_t stream);

/* ---- matching/sinkhorn.py:79-110,178  cost matrix -> core log-score matrix --------------------
 * z[b, i, j] = -cost(desc1[b,i], desc2[b,j]) / epsilon for i < n, j < m; row pitch `pitch` floats
 * (pitch % 4 == 0, pitch >= m, z 16-byte aligned).  The dustbin row/column of the reference's
 * augmented matrix (sinkhorn.py:187) is a constant and is not stored: mi_sinkhorn takes it as a
 * scalar.  epsilon is a double so that fp32(epsilon) and fp32(-unused/epsilon) round exactly as
 * the reference's Python-float arithmetic does.
 * _bits: descriptors are packed hard bits (num_bits % 32 == 0, <= 4096); `normalized` selects
 *     desc = bit/sqrt(popcount) (cost = 2 - 2 dot/sqrt(pa pb)) or desc = bit (cost = Hamming).
 *     Dot products are exact: popcount(a & b) on the matrix cores (256 / 512 bits: v_mfma_f32_32x32x64_f8f6f4 on
 *     FP4 operands, a bit = the nibble 1.0 / 0.0, fp32 sums <= 4096 exact; other lengths: v_mfma_i32_32x32x32_i8 on 0/1 bytes).
 * _f32: arbitrary float descriptors (n,d)/(m,d); L2 via v_mfma_f32_32x32x2_f32, L1 on the VALU. */
MI_API int mi_cost_logscores_bits(const uint32_t *bits1, const uint32_t *bits2, int batch, int n, int m,
                           int num_bits, int normalized, double epsilon, float *z, int pitch,
                           mi_stream_t stream);
MI_API int mi_cost_logscores_f32(const float *desc1, const float *desc2, int batch, int n, int m, int d,
                          int distance, double epsilon, float *z, int pitch, mi_stream_t stream);

/* ---- matching/sinkhorn.py:112-147,187-206  log-space Sinkhorn with dustbins ------------------
 * z: core log-scores as above.  dustbin_logscore = fp32(-unused_score/epsilon).  u (batch*(n+1))
 * and v (batch*(m+1)) are workspace and return the final duals.  p (batch, n+1, m+1) dense =
 * exp(Z + u + v) over the augmented matrix; may be NULL (duals only).  iterations >= 1.
 * workspace: mi_sinkhorn_workspace_bytes(batch, n, m) bytes, 16-byte aligned, enables the fused
 * iteration that reads Z once per iteration (per-band column partials); with workspace == NULL
 * (or m > 1024, for which the query returns 0) the two-pass form runs -- same results up to
 * fp32 summation order.
 * Streams: with a workspace and batch >= 64 the call runs as two half batches on the caller's stream and the library's
 * per-stream helper streams, like mi_sinkhorn_dots and scheduled by the same self-tuner (its shapes are kept apart
 * from that solver's: mi_sinkhorn_dots_schedule(stream, batch, n, m, iterations + (1 << 20)) reports this solver's
 * decision); same duals whatever the schedule.  mi_sinkhorn_dots_set_schedule(stream, MI_SCHEDULE_UNSPLIT) keeps
 * every launch of both solvers on the caller's stream; inside a stream capture nothing is tried (the decision in
 * force, or unsplit). */
MI_API size_t mi_sinkhorn_workspace_bytes(int batch, int n, int m);
MI_API int mi_sinkhorn(const float *z, int batch, int n, int m, int pitch, float dustbin_logscore,
                int iterations, float *u, float *v, float *p, void *workspace, size_t workspace_bytes,
                mi_stream_t stream);

/* ---- packed-descriptor form of the two calls above (hard-binarised descriptors, L2) -----------
 * mi_cost_dots_bits stores the exact integer dot products popcount(a_i & b_j) as uint16
 * (dots[b, i, j], row pitch `pitch` uint16 elements, pitch % 8 == 0, pitch >= m, 16-byte aligned)
 * and, per descriptor, the pair (scale, squared norm) = (1/sqrt(pop), pop * scale^2) if
 * `normalized` else (1, pop): row_info float[batch][n][2], col_info float[batch][m][2].
 * mi_sinkhorn_dots runs the same iterations as mi_sinkhorn but rebuilds
 *     z = -max(|a|^2 + |b|^2 - 2 * dot * s_a * s_b, 0) * (1/epsilon)
 * in registers on every pass: 2 bytes per matrix element per iteration instead of 4.
 * m <= 1024 (mi_sinkhorn_dots_workspace_bytes returns 0 otherwise: use the fp32 form).
 * epsilon >= MI_DOTS_MIN_EPSILON: the factored z drops the reference's clamp(cost, min=0) (sinkhorn.py:103),
 * which only acts on the rounding noise of identical normalised descriptors (cost = -O(3e-7)); that noise
 * enters z as +O(3e-7/epsilon), inside the 1e-4 parity bound down to epsilon = 0.005 and not below --
 * smaller epsilon is refused with MI_E_PARAM (mi_match_pairs_workspace_bytes returns 0): use the fp32-Z
 * form, which clamps.
 * sqnorm_bound: an upper bound of every squared norm in row_info / col_info (1 for `normalized`
 * descriptors, num_bits otherwise), or 0 if unknown.  With a bound small enough that
 * 2 * sqnorm_bound / epsilon < ~62 the row pass shifts every row of a pair by one analytic bound
 * instead of each row's own maximum (same result to fp32 rounding, fewer instructions); a bound the
 * data exceeds is a contract violation (exponent overflow).  0 always takes the per-row-maximum path.
 * flags: MI_SOLVER_DEFAULT, or MI_SOLVER_MULTI_LAUNCH to rule out the single-launch form (which otherwise runs for
 * batch <= 8, n, m <= 512 when its grid fits the device; same duals bit for bit either way).
 * mi_sinkhorn_dots_status_word: the device address, inside `workspace`, of the call's 32-bit status word -- written by
 * every mi_sinkhorn_dots call with these extents: 0 = solved, non-zero = a hand-off of the single-launch form timed out
 * and u, v (and p) of the affected pairs are NaN.  Read it after synchronising, or hand it to mi_mnn_from_duals_dots. */
MI_API int mi_cost_dots_bits(const uint32_t *bits1, const uint32_t *bits2, int batch, int n, int m, int num_bits,
                      int normalized, uint16_t *dots, int pitch, float *row_info, float *col_info,
                      mi_stream_t stream);
MI_API size_t mi_sinkhorn_dots_workspace_bytes(int batch, int n, int m);
MI_API int mi_sinkhorn_dots(const uint16_t *dots, const float *row_info, const float *col_info, int batch, int n,
                     int m, int pitch, double epsilon, double unused_score, double sqnorm_bound, int iterations,
                     float *u, float *v, float *p, void *workspace, size_t workspace_bytes, int flags,
                     mi_stream_t stream);
MI_API const uint32_t *mi_sinkhorn_dots_status_word(const void *workspace, int batch, int n, int m);

/* ---- matching/sinkhorn.py:317-465  SinkhornMatcherWithFilters (filter stage) -----------------
 * In place on p (batch, n+1, m+1): per row i < n, best/second-best core probability and the
 * dustbin entry decide valid[b,i] (ratio_threshold <= 0 / dustbin_margin < 0 disable a filter);
 * failing rows get core * 0 and dustbin entry 1, as the reference writes them. */
MI_API int mi_match_filters(float *p, int batch, int n, int m, float ratio_threshold, float dustbin_margin,
                     uint8_t *valid, mi_stream_t stream);
/* ---- matching/outlier_filters.py:11-116  probability_ratio_filter / dustbin_margin_filter ------
 * The same two tests as masks only (p is not modified): valid[b,i] for i < n.
 * has_dustbin = 1: p is (batch, n+1, m+1) with the dustbin column (dustbin_margin_filter's argument; both tests
 * available); 0: p is the (batch, n, m) core (probability_ratio_filter's argument; dustbin_margin must be < 0).
 * ratio_threshold <= 0 / dustbin_margin < 0 disable a test. */
MI_API int mi_match_filter_masks(const float *p, int batch, int n, int m, int has_dustbin, float ratio_threshold,
                          float dustbin_margin, uint8_t *valid, mi_stream_t stream);

/* ---- matching/match_extraction.py:72-181  MutualNearestNeighborMatcher.forward --------------
 * p (batch, n+1, m+1); kpts1 (batch,n,2); kpts2 (batch,m,2).  Workspace: row_best (batch*n) u64,
 * col_best (batch*m) u64.  Outputs mk1/mk2 (batch,max_matches,2), scores (batch,max_matches),
 * valid (batch,max_matches) u8, match_ij (batch,max_matches,2) i32 (may be NULL).
 * n <= 4096.  Ties: first index (argmax), then (score desc, row asc) for the top-max_matches.
 * m <= 1024: one pass over p (row and column winners together; col_best, 8-byte aligned, is cleared by the call and
 * filled by 64-bit atomic maxima -- exact, so the order of arrival cannot be seen); larger m: a row and a column pass.
 * Precondition: every entry of the core p[:, :n, :m] is finite and >= +0.0 (a probability; -0.0 is not).  The winners
 * are maxima of keys built from the entries' raw bits, which order non-negative floats only.  Outside the
 * precondition the two paths differ and neither is the reference: in the one-pass path (m <= 1024) a NaN entry never
 * wins a row or a column (a row of nothing but NaN has no match) and a negative entry loses to every other; the row
 * and column passes (m > 1024) compare raw bits throughout, so there a NaN or a negative entry beats every
 * probability. */
MI_API int mi_mnn_extract(const float *p, int batch, int n, int m, const float *kpts1, const float *kpts2,
                   int max_matches, float threshold, uint64_t *row_best, uint64_t *col_best,
                   float *mk1, float *mk2, float *scores, uint8_t *valid, int32_t *match_ij,
                   mi_stream_t stream);

/* ---- MutualNearestNeighborMatcher.forward straight from the Sinkhorn duals ---------------------
 * What feature_detection/match_extraction_wrapper.py:82-113 computes (matcher -> P -> mutual NN)
 * without materialising P: P_ij = expf((z_ij + u_i) + v_j) is evaluated in registers exactly as
 * mi_sinkhorn's final pass does, so the outputs are bit-identical to mi_sinkhorn(p != NULL) followed
 * by mi_mnn_extract.  z/pitch (or dots/row_info/col_info/pitch/epsilon) and u, v are what was
 * passed to / returned by mi_sinkhorn (mi_sinkhorn_dots) with p == NULL.  m <= 1024, n <= 4096.
 * workspace: mi_mnn_duals_workspace_bytes(batch, n, m) bytes (0 = unsupported size), 8-byte aligned.
 * solver_status (mi_mnn_from_duals_dots; may be NULL): the status word of the mi_sinkhorn_dots call that produced
 * u, v.  When it is non-zero on the device every match of this call comes back with score -1 / valid 0 / match_ij -1.
 * The _records forms write the same matches as ONE float32 record array (batch, max_matches, 6), 8-byte aligned, in
 * place of mk1 / mk2 / scores: per slot mk1.y, mk1.x, mk2.y, mk2.x, score, valid as 1.0f / 0.0f (every slot below
 * max_matches is written); valid (u8) and match_ij as above.  A consumer that wants the packed record (a gather of
 * matches between devices) then needs no packing kernel.
 * flags (mi_mnn_from_duals_dots_records): 0 or MI_SOLVER_DOTS_BELOW_1024, with the meaning it has for mi_sinkhorn_dots:
 * the caller vouches that every dot product is < 1024, and the kernel multiplies the uint16, read as an fp16 denormal,
 * in one mixed-precision instruction instead of converting first.  The same matches bit for bit; a value >= 1024 under
 * the flag gives wrong matches, no fault.  Any other bit: MI_E_PARAM. */
MI_API size_t mi_mnn_duals_workspace_bytes(int batch, int n, int m);
MI_API int mi_mnn_from_duals(const float *z, int batch, int n, int m, int pitch, const float *u, const float *v,
                      const float *kpts1, const float *kpts2, int max_matches, float threshold, void *workspace,
                      size_t workspace_bytes, float *mk1, float *mk2, float *scores, uint8_t *valid,
                      int32_t *match_ij, mi_stream_t stream);
MI_API int mi_mnn_from_duals_dots(const uint16_t *dots, const float *row_info, const float *col_info, int batch, int n,
                           int m, int pitch, double epsilon, const float *u, const float *v, const float *kpts1,
                           const float *kpts2, int max_matches, float threshold, void *workspace,
                           size_t workspace_bytes, const uint32_t *solver_status, float *mk1, float *mk2,
                           float *scores, uint8_t *valid, int32_t *match_ij, mi_stream_t stream);
MI_API int mi_mnn_from_duals_records(const float *z, int batch, int n, int m, int pitch, const float *u, const float *v,
                              const float *kpts1, const float *kpts2, int max_matches, float threshold,
                              void *workspace, size_t workspace_bytes, float *record, uint8_t *valid,
                              int32_t *match_ij, mi_stream_t stream);
MI_API int mi_mnn_from_duals_dots_records(const uint16_t *dots, const float *row_info, const float *col_info, int batch,
                                   int n, int m, int pitch, double epsilon, const float *u, const float *v,
                                   const float *kpts1, const float *kpts2, int max_matches, float threshold,
                                   void *workspace, size_t workspace_bytes, const uint32_t *solver_status, int flags,
                                   float *record, uint8_t *valid, int32_t *match_ij, mi_stream_t stream);

/* ---- detector/akaze.py  AKAZE (BASELINE config 4), all maps fp32 (n,1,h,w) ---------------------
 * mi_akaze_diffuse: one explicit step of NonLinearDiffusion.forward (akaze.py:98-131):
 *   g = sobel/8 gradients (zero pad), c = 1/(1+(|g|/kappa)^2) with |g| = sqrt(gx^2+gy^2+1e-8),
 *   l_out = l_in + dt * div(c*g) (sobel/8 on the zero-padded flux).  l_out must not alias l_in.
 * mi_akaze_hessian_scores: HessianDetector.forward (akaze.py:227-254): det of the 3x3-kernel
 *   Hessian, kept where it equals the nms_size^2 window maximum (-inf outside the image) and
 *   exceeds threshold, clamped >= 0.  nms_size odd <= 15.
 * mi_akaze_combine: AKAZE.forward's scale selection (akaze.py:442-451) on stacked per-scale maps
 *   (num_scales,n,h,w): scores = max over scales, orientations = mean of the orientations of the
 *   scales attaining the max (orientations/scale_orientations may both be NULL: scores only).
 * mi_akaze_orientation_at_keypoints: the same selection evaluated only at keypoints (n,k,2):
 *   scale_theta (num_scales,n,k) from mi_angle_at_keypoints per scale -> theta (n,k); equal to
 *   sampling the combined map the way descriptor/bad.py:487-500 does. */
MI_API int mi_akaze_diffuse(const float *l_in, int n, int h, int w, float kappa, float dt, float *l_out,
                     mi_stream_t stream);
/* One scale of AKAZE.forward (akaze.py:430-440) in one launch: l_out = `iterations` diffusion steps of l_in,
 * scores = mi_akaze_hessian_scores(l_out); identical maps, 12 instead of 8 * iterations + 8 bytes per pixel of HBM
 * traffic.  Fused for iterations 1..3 and nms_size 3 / 5 / 7 (mi_akaze_scale_fused returns 1) -- as a rolling window
 * that streams down the image (even w, 8-byte aligned maps, nms_size 3 / 5) or on an LDS-resident tile --; other
 * values run the per-step kernels and then need `tmp` (n*h*w floats) when iterations > 1.  l_out must not alias l_in.
 * kappa must lie in [MI_AKAZE_KAPPA_MIN, MI_AKAZE_KAPPA_MAX] (the range the fused kernels' exactly rounded division
 * helpers are verified for; MI_E_PARAM otherwise -- mi_akaze_diffuse + mi_akaze_hessian_scores take any kappa > 0). */
#define MI_AKAZE_KAPPA_MIN 1e-3f
#define MI_AKAZE_KAPPA_MAX 1e6f
MI_API int mi_akaze_scale_fused(int iterations, int nms_size);
MI_API int mi_akaze_scale(const float *l_in, int n, int h, int w, int iterations, float kappa, float dt, float threshold,
                   int nms_size, float *l_out, float *scores, float *tmp, mi_stream_t stream);
/* mi_akaze_scale for the FIRST scale of two equally shaped batches (image1 / image2 of a matcher) behind one launch:
 * l_out and scores are (2 * per_set, h, w), batch a first; every later scale then runs on one batch of twice the size.
 * tmp: per_set * h * w floats, as for mi_akaze_scale. */
MI_API int mi_akaze_scale_sets(const float *l_in_a, const float *l_in_b, int per_set, int h, int w, int iterations,
                        float kappa, float dt, float threshold, int nms_size, float *l_out, float *scores, float *tmp,
                        mi_stream_t stream);
/* The LAST scale with AKAZE.forward's selection across scales (akaze.py:436-451) folded in: l_out as mi_akaze_scale;
 * instead of this scale's score map, best (n,h,w) = max over the num_prev (<= 7) earlier scales' maps prev_scores
 * (num_prev,n,h,w) and this scale's, and attain (n,h,w) uint8: bit s set when earlier scale s reaches that maximum,
 * bit num_prev when this scale does -- what mi_akaze_combine computes from stacked maps, without the stack's last map
 * and without a pass of its own (the streaming form reads the earlier maps where it writes its output row).
 * mi_akaze_orientation_from_attain: mi_akaze_orientation_at_keypoints from `attain` instead of the stacked maps. */
MI_API int mi_akaze_scale_select(const float *l_in, int n, int h, int w, int iterations, float kappa, float dt,
                          float threshold, int nms_size, float *l_out, const float *prev_scores, int num_prev,
                          float *best, uint8_t *attain, float *tmp, mi_stream_t stream);
MI_API int mi_akaze_orientation_from_attain(const uint8_t *attain, const float *scale_theta, int num_scales, int n, int h,
                                     int w, const float *keypoints, int k, float *theta, mi_stream_t stream);
/* The same orientation in ONE launch from the diffused images themselves: scale_images = num_scales maps (n,h,w),
 * scale_stride floats apart (a stacked (S,n,h,w) tensor: n*h*w); per keypoint the patch_size^2 Gaussian moments
 * (mi_angle_at_keypoints) are evaluated only for the scales `attain` names -- typically one of three. */
MI_API int mi_akaze_orientation_select(const float *scale_images, size_t scale_stride, int num_scales,
                                const uint8_t *attain, int n, int h, int w, const float *keypoints, int k,
                                int patch_size, const float *moment_kernels, float *theta, mi_stream_t stream);
MI_API int mi_akaze_hessian_scores(const float *l, int n, int h, int w, float threshold, int nms_size, float *scores,
                            mi_stream_t stream);
MI_API int mi_akaze_combine(const float *scale_scores, const float *scale_orientations, int num_scales, int n, int h,
                     int w, float *scores, float *orientations, mi_stream_t stream);
MI_API int mi_akaze_orientation_at_keypoints(const float *scale_scores, const float *scale_theta, int num_scales,
                                      int n, int h, int w, const float *keypoints, int k, float *theta,
                                      mi_stream_t stream);

/* ---- matching/sinkhorn.py:228-259  SinkhornMatcherWithScores: maxima of P[:n,:m] per row / column */
MI_API int mi_core_maxima(const float *p, int batch, int n, int m, float *row_max, float *col_max, mi_stream_t stream);

/* ---- feature_detection/..._essential_matrix.py:334-360: `count` keypoints (y, x) in pixels -> normalised
 * image coordinates (x, y), the first two rows of k_inv (3x3 row-major, device memory) times [x, y, 1]. */
MI_API int mi_normalise_keypoints(const float *keypoints, long long count, const float *k_inv, float *points,
                           mi_stream_t stream);

/* ---- geometry/essential_matrix_estimator.py:302-431  EssentialMatrixEstimator.forward and the
 * composites' _estimate_essential_matrix (feature_detection/..._essential_matrix.py:184-271) -------
 * Weighted 8-point algorithm on the assignment matrix p (batch, n+1, m+1): bidirectional top_k mask
 * (k-th largest with multiplicity) AND p > 0.01 on the core (times valid1 x valid2 when given, both
 * (batch, n) / (batch, m) bytes or both NULL), Hartley normalisation with the weights' row / column
 * sums, Kronecker-factored normal equations, n_iter steps of shifted power iteration for the minimum
 * eigenvector, denormalisation, projection onto singular values (s, s, 0) with n_iter_manifold steps.
 * pts1 (batch, n, 2), pts2 (batch, m, 2): NORMALISED image coordinates (x, y) = K^-1 [px, py, 1].
 * e (batch, 3, 3).  n, m <= 1024, 1 <= top_k <= min(8, n, m).  Deterministic.
 * workspace (optional): mi_essential_matrix_workspace_bytes(batch, n, m, top_k) bytes, 16-byte aligned (the query returns
 * 0 for top_k > 4: no banded form).  With it the head runs in two launches -- one pass over the matrix spread over the
 * chip (bands of 32 rows: row thresholds, the rows' candidate entries, per-band column lists), then one workgroup per
 * pair on the sparse weights -- instead of one workgroup per pair streaming the matrix four times (~0.6 ms per launch
 * whatever the batch).  Same definition of every quantity; results agree with the workspace-less form to fp32 rounding
 * (a row's / column's few weights are added in a different order).  NULL: the single-launch dense form. */
MI_API size_t mi_essential_matrix_workspace_bytes(int batch, int n, int m, int top_k);
MI_API int mi_essential_matrix(const float *p, int batch, int n, int m, const float *pts1, const float *pts2,
                        const uint8_t *valid1, const uint8_t *valid2, int top_k, int n_iter,
                        int n_iter_manifold, float *e, void *workspace, size_t workspace_bytes, mi_stream_t stream);
/* The same head WITHOUT a materialised P, from the packed-descriptor Sinkhorn solution: dots / row_info / col_info /
 * pitch as written by mi_cost_dots_bits, u (batch, n+1) / v (batch, m+1) the duals of mi_sinkhorn_dots (p = NULL there).
 * Every entry P_ij = exp(z_ij + u_i + v_j) is rebuilt in registers with the solver's own final-pass expression, so E
 * equals mi_essential_matrix on the P that mi_sinkhorn_dots would have written, bit for bit; 2 instead of 4 bytes per
 * entry are read and the (n+1) x (m+1) matrix is neither written nor read back.  epsilon >= MI_DOTS_MIN_EPSILON. */
MI_API int mi_essential_matrix_dots(const uint16_t *dots, const float *row_info, const float *col_info, int pitch,
                             double epsilon, const float *u, const float *v, int batch, int n, int m,
                             const float *pts1, const float *pts2, const uint8_t *valid1, const uint8_t *valid2,
                             int top_k, int n_iter, int n_iter_manifold, float *e, void *workspace,
                             size_t workspace_bytes, mi_stream_t stream);

/* ---- detector/fast.py:198-239  FASTScore.forward (use_nms = False) ----------------------------------
 * score (n,1,h,w) = 1.0 where 9 contiguous pixels of the radius-3 circle (replicate padding) are all
 * >= centre + threshold or all <= centre - threshold, else 0.0.  Bit-identical to the reference.
 * ---- detector/dog.py:100-142  DoGDetector.forward ---------------------------------------------------
 * out (n, num_scales-1, h, w) = differences of consecutive Gaussian blurs of the replicate-padded
 * image.  weights_1d (num_scales, kernel_size): the row sums of the module's normalised 2-D kernels
 * (their exact 1-D factors).  2 <= num_scales <= 8, kernel_size odd <= 49.
 * score (n,1,h,w), optional: max over scales of |DoG| (DoGDetectorWithScore.forward, dog.py:182-204);
 * out or score may be NULL, not both. */
MI_API int mi_fast_score(const float *image, int n, int h, int w, float threshold, float *score, mi_stream_t stream);
MI_API int mi_dog_responses(const float *image, int n, int h, int w, const float *weights_1d, int num_scales,
                     int kernel_size, float *out, float *score, mi_stream_t stream);

/* ---- feature_detection/match_extraction_wrapper.py:82-113 over shi_tomasi_sparse_bad_sinkhorn.py:79-182
 * The whole path for `batch` image pairs in one call: image1[b] vs image2[b], (batch,1,h,w) f32 each ->
 * keypoints1/2 (batch,K,2) as (y,x), matched1/2 (batch,max_matches,2), match_scores (batch,max_matches),
 * match_valid (batch,max_matches) bytes, match_ij (batch,max_matches,2) int32 or NULL.  Hard-binarised
 * descriptors, L2 cost, matches straight from the Sinkhorn duals (P is never written); K <= 1024.
 * It sequences mi_corner_response, mi_nms_candidates, mi_topk_keypoints, mi_sparse_bad (twice each),
 * mi_cost_dots_bits, mi_sinkhorn_dots and mi_mnn_from_duals_dots on `stream`, with every intermediate in
 * `workspace` (mi_match_pairs_workspace_bytes, 16-byte aligned): nothing is allocated, nothing synchronises.
 * Results are bit-identical to calling those entry points one by one (what the Python modules do).
 * pair_geom / pair_thr / bad_plan: device pointers as for mi_sparse_bad (bad_plan may be NULL). */
typedef struct mi_match_params {
  int block_size;            /* ShiTomasiScore(block_size), 3 in the export CLI */
  int nms_radius;            /* apply_nms_maxpool radius */
  int max_keypoints;         /* K */
  float score_threshold;     /* select_topk_keypoints */
  int border_margin;         /* select_topk_keypoints; the matcher's default is the descriptor's max radius (7) */
  int num_pairs;             /* BAD pairs P: 256 or 512 with the reference tables */
  const uint32_t *pair_geom; /* device, P words */
  const float *pair_thr;     /* device, P floats */
  const void *bad_plan;      /* device, mi_bad_plan_build output, or NULL */
  int normalize_descriptors; /* SparseBAD(normalize_descriptors=...) */
  double epsilon;            /* SinkhornMatcher */
  double unused_score;
  int sinkhorn_iterations;
  int max_matches;           /* MutualNearestNeighborMatcher */
  float match_threshold;
  int flags;                 /* MI_SOLVER_DEFAULT or an OR of MI_SOLVER_MULTI_LAUNCH ("co-residency" in the conventions)
                                and MI_SOLVER_NO_FORK */
} mi_match_params;
MI_API size_t mi_match_pairs_workspace_bytes(int batch, int h, int w, const mi_match_params *params);
MI_API int mi_match_pairs(const float *image1, const float *image2, int batch, int h, int w,
                   const mi_match_params *params, float *keypoints1, float *keypoints2, float *matched1,
                   float *matched2, float *match_scores, uint8_t *match_valid, int32_t *match_ij,
                   void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* u8 ingest form of mi_match_pairs: uint8 frames (batch,1,h,w), same workspace, identical results. */
MI_API int mi_match_pairs_u8(const uint8_t *image1, const uint8_t *image2, int batch, int h, int w,
                      const mi_match_params *params, float *keypoints1, float *keypoints2, float *matched1,
                      float *matched2, float *match_scores, uint8_t *match_valid, int32_t *match_ij,
                      void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- pointcloud/voxel_downsampling.py:16-104  VoxelDownsampling.forward, for a batch of ragged clouds ---------------
 * points (total, d) float32, d >= 3, the clouds packed back to back: cloud b is rows offsets[b] .. offsets[b+1]-1
 * (offsets: batch+1 int64 on the device, offsets[0] = 0, non-decreasing, offsets[batch] = total); leaf: one float32 per
 * cloud on the device.  Per cloud, as the reference: c = floor(p / leaf) (IEEE division) as int64 over columns 0-2,
 * c -= c.min(0), key = c0*d1*d2 + c1*d2 + c2 with d1 = max(c1)+1, d2 = max(c2)+1 in wrapping int64 arithmetic, voxels
 * in ascending SIGNED key order (a wrapped key sorts negative, as the reference's argsort sorts it); each voxel's mean
 * of all d columns.  Cloud b's output block is rows offsets[b] .. offsets[b+1]-1 of out_points (total, d) and out_mask
 * (total bytes): its M_b voxel means first, then zero rows; out_mask is 1 exactly on the first M_b rows;
 * out_counts[b] = M_b (int64).  Means are (float)(fp64 sum / count), one rounding, summed in an order that depends only
 * on the voxel's rows within its cloud: bitwise reproducible, and a cloud's block is the same whatever else is in the
 * batch.  The reference forms each mean as the difference of two global float32 cumsums, which is off by up to 0.125
 * (about 1.3e5 ulps) on 200 000 points of 3*randn + 10 at leaf 0.05: the voxel set, order, counts and mask are the
 * reference's exactly, the means are the exact means rounded once and are NOT its cumsum differences.
 * Preconditions: finite points, finite leaf > 0, |p / leaf| < 2^62; outside them the results are unspecified but every
 * address still comes from indices, the (clamped) offsets and scan results, never from a key or a coordinate.
 * total < 2^31 (MI_E_SHAPE otherwise, or for d < 3, batch < 1); points / out_points / out_mask may be NULL when
 * total = 0.  workspace: mi_voxel_downsample_workspace_bytes(batch, total, d) bytes (~24.5 per point), 16-byte aligned,
 * of any content (MI_E_CAPACITY when short).  Radix sort (8-bit digits, only as many key passes as the batch's keys
 * have significant bits, decided on the device) and segmented fp64 sums: nothing synchronises, the call can be
 * captured into a hipGraph. */
MI_API size_t mi_voxel_downsample_workspace_bytes(int batch, int64_t total, int d);
MI_API int mi_voxel_downsample(const float *points, const int64_t *offsets, int batch, int64_t total, int d,
                               const float *leaf, float *out_points, uint8_t *out_mask, int64_t *out_counts,
                               void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- depth/depth2pointcloud.py:5-24  DepthToPointCloud.forward and depth/depth2pointcloud_with_normal.py:7-33
 * DepthToPointCloudWithNormal.forward, for a batch of frames in one launch ---------------------------------------------
 * depth (batch, h, w): float32 (depth_is_u16 = 0) or uint16 sensor counts (1; converted exactly).  u_tab (w) and v_tab (h)
 * float32 on the device: u_tab[x] = ((float(x) - cx) / fx) * scale, v_tab[y] = ((float(y) - cy) / fy) * scale, and
 * z_scale = 1.0f * scale, all float32 with IEEE division -- the three columns of the reference's `uv` buffer.
 * out_points (batch, h, w, 3) = depth * (u_tab[x], v_tab[y], z_scale): one float32 product each, the reference's bits.
 * out_normals (batch, h, w, 3), or NULL for points only (the points are the same bits either way):
 *     s = X + Y + Z of a point;  dx, dy = the cross-correlation of s with [[1,0,-1],[2,0,-2],[1,0,-1]] and
 *     [[1,2,1],[0,0,0],[-1,-2,-1]], zero outside the frame (the reference's two conv2d over the three channels, padding 1);
 *     n = (dx, dy, -1) / sqrt(dx^2 + dy^2 + 1).
 * The normals are computed from the 3x3 depth neighbourhood and the tables (the point image is not read back); the 18
 * products of a tap sum are added in a fixed order, the reference's convolution adds them in an order its backend
 * chooses: they agree to 18 * eps * (sum of |weight * coordinate| over the taps) + 4 * eps, not bit for bit.
 * batch, h, w >= 1 and batch * h * w < 2^31 (MI_E_SHAPE otherwise); no workspace; capturable into a hipGraph. */
MI_API int mi_depth_to_points(const void *depth, int depth_is_u16, int batch, int h, int w, const float *u_tab,
                              const float *v_tab, float z_scale, float *out_points, float *out_normals,
                              mi_stream_t stream);

/* ---- depth/depth_align.py:63-116  DepthAlignment.forward, for a batch of frames --------------------------------------
 * Re-renders depth (batch, h, w; float32 or uint16 as above; u_tab / v_tab / z_scale of the DEPTH camera) in the colour
 * camera's frame: out (batch, h, w) float32.  rotation (3, 3) row-major, used as p @ rotation, and translation (3):
 * float32 on the device.  Per source pixel (x, y) with raw depth d, float32, in exactly this order:
 *     X = d * u_tab[x];  Y = d * v_tab[y];  Z = d * z_scale
 *     q_j = ((X * R[0][j] + Y * R[1][j]) + Z * R[2][j]) + t[j]                    j = 0, 1, 2
 *     px = q_0 / q_2 * rgb_fx + rgb_cx;  py = q_1 / q_2 * rgb_fy + rgb_cy;  px = py = 0 if q_2 == 0
 *     x0 = trunc(px - 0.5), x1 = trunc(px + 0.5), y0, y1 likewise; the source offers d to the targets
 *     (y0, x0) (y0, x1) (y1, x0) (y1, x1)
 * which is the reference's arithmetic.  Where the reference is undefined or broken this entry defines:
 *   - a target receives the MINIMUM over all sources that write it (the nearest surface wins), 0 if none.  The reference
 *     forms min(align0..3) of four images filled by non-accumulating index_put_ with duplicate indices: which duplicate
 *     survives depends on the thread schedule (1 and 8 CPU threads differ); the minimum over all writers is the one
 *     resolution that does not depend on order, and it is never larger than what the reference returns;
 *   - a source that projects out of frame (px < 0, px >= w, py < 0, py >= h) writes nothing (the reference sends every
 *     such source to pixel (0, 0)); a NaN projection has no pixel and writes nothing either;
 *   - a source whose depth is 0, negative, NaN or >= 10000.0 writes nothing: 0 is "no measurement", and the reference's
 *     fill value 10000 turns any larger value into 0 anyway.  The comparison is on the RAW depth value, before scale: with
 *     millimetre counts (scale 0.001) everything beyond 9999 counts is silenced too, as in the reference;
 *   - a target with x1 == w or y1 == h is dropped (the reference raises IndexError for any source that lands in
 *     [w - 0.5, w) or [h - 0.5, h), i.e. on ordinary camera pairs with similar fields of view).
 * At every target written by at most one source per splat image and by none of the silenced ones the result equals the
 * single-threaded reference bit for bit.  Positive floats order as their bit patterns, so the z-buffer is a uint32
 * atomicMin on `out` itself (filled with a sentinel first, the sentinel replaced by 0 afterwards; `out` may hold
 * anything on entry), taken behind a tile-local z-buffer in LDS that resolves most collisions on chip: integer atomics
 * only, bitwise reproducible, a frame's result is the same alone or in a batch.
 * Three launches, no workspace, capturable.  Shape rules as for mi_depth_to_points. */
MI_API int mi_depth_align(const void *depth, int depth_is_u16, int batch, int h, int w, const float *u_tab,
                          const float *v_tab, float z_scale, float rgb_cx, float rgb_cy, float rgb_fx, float rgb_fy,
                          const float *rotation, const float *translation, float *out, mi_stream_t stream);

/* ---- threshold/otsu.py:5-48  OtsuThreshold and threshold/multi_otsu.py:6-70  MultiOtsuThreshold, for a batch of frames ---
 * The reference builds BINS x BINS masks (Otsu) and an (n_class, C(BINS-1, n_class-1), BINS) mask (multi-Otsu); here the
 * histogram, an int64 prefix sum over the bins and an O(1) score per candidate do the same search.  Four entries:
 * histogram -> threshold search (Otsu or multi-Otsu) -> apply; thresholds are int32 in device memory from the search to
 * the apply, nothing is read back, every entry is capturable into a hipGraph and takes outputs and workspace of any prior
 * content.  Frames: (batch, pixels) of uint8, uint16, int32 or float32 (MI_PIX_*), frame b at element b * pixels, aligned
 * to the element size; batch >= 1, pixels >= 1 (MI_E_SHAPE), 1 <= bins <= MI_THRESHOLD_MAX_BINS.
 * Divergences from the reference:
 *   - min_val is honoured: bin i holds the value min_val + i (the reference indexes its histogram by the raw value and
 *     weights bin i with min_val + i: consistent for min_val = 0 only, where the results here are the reference's);
 *   - values outside [min_val, min_val + bins), NaN and floats beyond the int32 range are NOT counted (the reference
 *     raises from scatter_add; nothing here synchronises to raise);
 *   - a histogram handed to the searches is int64 counts (the reference's multi-Otsu takes float32);
 *   - multi-Otsu scores in fp64 in a fixed order (the reference sums float32 products in an order its backend chooses). */
enum { MI_PIX_U8 = 0, MI_PIX_U16 = 1, MI_PIX_I32 = 2, MI_PIX_F32 = 3 };
#define MI_THRESHOLD_MAX_BINS 65536
#define MI_THRESHOLD_MAX_CLASSES 5

/* hist (batch, bins) int64: hist[b][i] = number of pixels of frame b whose integer value v has v - min_val == i; float32 is
 * truncated toward zero first (the reference's .to(torch.int64)).  hist is cleared by the call.  bins <= 4096: workgroup-
 * private LDS sub-histograms (replicated up to 8 times, runs of equal neighbouring values pre-aggregated) flushed with
 * 64-bit integer atomics; above: the pre-aggregated runs go to global memory directly.  Integer atomics only: the counts
 * are exact and bitwise reproducible.  Two launches. */
MI_API int mi_histogram(const void *frames, int dtype, int batch, long long pixels, int min_val, int bins, int64_t *hist,
                        mi_stream_t stream);

/* Otsu's threshold of each histogram (batch, bins), bins = max_val - min_val + 1: thresh[b] int32.  For every bin t, from
 * exact int64 prefix sums: num_bk = sum_{i<=t} hist[i], fc_bk = sum_{i<=t} (min_val + i) * hist[i], num_wh = N - num_bk,
 * fc_wh = F - fc_bk; then in float32, IEEE division, no contraction, in this order (the reference's own op sequence):
 *     mean_bk = (float)fc_bk / (float)num_bk;  mean_wh = (float)fc_wh / (float)num_wh;  d = mean_bk - mean_wh
 *     var = (float)(num_bk * num_wh) * (d * d)          the int64 product first, rounded once;  NaN -> 0
 * thresh = min_val + the FIRST index of the maximum: the reference's value exactly (for min_val = 0).  The int64 product
 * wraps beyond 3.0e9 pixels per frame, as the reference's does.  One workgroup per frame, one launch. */
MI_API int mi_otsu_threshold(const int64_t *hist, int batch, int bins, int min_val, int32_t *thresh, mi_stream_t stream);

/* Multi-Otsu: the n_class - 1 thresholds of each histogram (batch, bins), bins = max_val - min_val (max_val exclusive, as
 * in the reference): thresholds (batch, n_class - 1) int32.  Candidates: the C(bins-1, n_class-1) tuples
 * 1 <= th_1 < ... < th_{n-1} <= bins-1 in lexicographic order (itertools.combinations); class i holds the bins
 * [th_i, th_{i+1}) with th_0 = 0, th_n = bins; n_i and S_i = sum (min_val + bin) * hist[bin] exact int64.  Score, fp64:
 *     m_i = (double)S_i / (double)n_i;  V = 0.0;  for (i, j) in (0,1), (0,2), ..., (n-2,n-1):
 *         d = m_i - m_j;  V = V + ((double)n_i * (double)n_j) * (d * d);      V = 0 if any n_i == 0 (the reference's NaN -> 0)
 * Result: the candidate with the largest V, the smallest rank among equal V (torch.argmax's first maximum; empty bins make
 * exact ties); returned as min_val + th_k - 1, the inclusive upper bound of class k - 1 (the reference's threshold_indices).
 * 2 <= n_class <= MI_THRESHOLD_MAX_CLASSES (MI_E_PARAM); n_class <= bins <= MI_THRESHOLD_MAX_BINS and
 * C(bins-1, n_class-1) <= 2^31 - 1 (MI_E_SHAPE; mi_multi_otsu_workspace_bytes returns 0 for such a request).  The
 * workspace (8-byte aligned, any content) holds the prefix sums and one partial per workgroup of the sweep; a shorter one
 * is MI_E_CAPACITY.  Three launches; no floating-point atomics, no cross-workgroup waits; bitwise reproducible. */
MI_API size_t mi_multi_otsu_workspace_bytes(int batch, int bins, int n_class);
MI_API int mi_multi_otsu_threshold(const int64_t *hist, int batch, int bins, int min_val, int n_class, int32_t *thresholds,
                                   void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* One pass over the frames with thresholds (batch, n_thresh) int32 read from the device, 1 <= n_thresh <= 4.
 * binary = 0: out uint8 (out_dtype must be MI_PIX_U8), label = number of thresholds t_k with v > t_k.
 * binary = 1 (n_thresh must be 1): out = low where v <= t_0 and high elsewhere (NaN: high, as torch.where(img <= thresh)),
 *     in out_dtype MI_PIX_U8, MI_PIX_I32 or MI_PIX_F32 (low and high converted to it): OtsuThreshold's bin_img with
 *     low = min_val, high = max_val.
 * The comparison is made in the input's type: float32 pixels against (float)t_k; integer pixels exactly (which is the
 * reference's own-type comparison whenever t_k is representable in that type).  MI_E_PARAM for any other combination. */
MI_API int mi_threshold_apply(const void *frames, int dtype, int batch, long long pixels, const int32_t *thresholds,
                              int n_thresh, int out_dtype, int binary, int low, int high, void *out, mi_stream_t stream);

/* ---- relative pose (K15): vo/pose_estimation.py:53-162  estimate_pose_ransac and triangulate_points, for a batch of pairs --
 * The reference does this step on the host with OpenCV, one pair at a time: cv2.findEssentialMat(RANSAC) (:87-94),
 * cv2.recoverPose (:102-108) and cv2.triangulatePoints (:143-160).  Five entries here, batched over pairs, every one a
 * pure function of its arguments: no allocation, no synchronisation, no memset, one stream, no atomics, every sum in a
 * fixed order -- the same inputs and seed give the same bits, and every entry can be captured into a hipGraph.  Outputs
 * and workspace may hold anything on entry; every output element is written.
 * Correspondence i of pair b is pts1[b][i] <-> pts2[b][i], (batch, n, 2) float32 in NORMALISED image coordinates (x, y)
 * as mi_normalise_keypoints writes them; `valid` / `mask` (batch, n) bytes select rows (non-zero = use; valid may be NULL:
 * every row).  Rows that are not selected are never read for their coordinates.  1 <= n <= MI_POSE_MAX_N (the staged
 * correspondences of a pair live in 36 KB of LDS), batch <= 65535 (MI_E_PARAM beyond; < 1: MI_E_SHAPE).
 *
 * Divergences from OpenCV, all deliberate:
 *   - minimal samples are 8 correspondences solved linearly (Hartley-normalised 8-point + projection onto the essential
 *     manifold), not Nister's 5-point solver: one candidate per sample, no polynomial roots;
 *   - the best hypothesis is the one of minimum truncated cost sum min(d^2, thr^2) (MSAC), not of maximum inlier count;
 *   - a fixed number of hypotheses, no adaptive stop from `prob`;
 *   - the sampler is a stateless counter-based hash, not cv::RNG: results do not depend on call history;
 *   - refinement is refine_rounds rounds of linear refit on the inliers (local optimisation), where OpenCV stops at the
 *     best minimal solution;
 *   - recover_pose takes a point's depths from the two-view linear equations instead of a DLT triangulation per
 *     candidate (the same sign and magnitude for consistent correspondences).
 *
 * Sampling.  mix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16 (uint32, wrapping).
 *   draw(seed, b, h, s) = mix(mix(mix(seed + 0x9E3779B9) + b) + (8 h + s)).
 *   Let nv be the number of valid rows of pair b, ranked 0 .. nv-1 in index order.  For slot s = 0 .. 7 in turn:
 *   r = draw(seed, b, h, s) mod (nv - s); then for every rank q already taken, in ASCENDING order of q: if r >= q then
 *   r = r + 1.  Slot s takes rank r (eight distinct ranks; the modulo bias is below nv / 2^32).
 * Solve.  Per image the sample's centroid c and scale sqrt(2) / sqrt(mean |p - c|^2); rows
 *   [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] of normalised points; Gauss-Jordan elimination with complete pivoting
 *   (the first maximum of |a| in (row, column) order); the sample is RANK-DEFICIENT when a pivot is not above 1e-5 times the
 *   first pivot (or a point set has zero spread); null vector scaled to unit norm = E_hat row-major; E = T2^T E_hat T1;
 *   projection onto singular values (s, s, 0), s the mean of the two largest (csrc/essential_math.h, shared with
 *   mi_essential_matrix).  E is defined up to sign and satisfies x2^T E x1 = 0.
 * Scoring.  For every valid row, with X1 = (x1, y1, 1), X2 = (x2, y2, 1): d^2 = (X2^T E X1)^2 /
 *   ((E X1)_0^2 + (E X1)_1^2 + (E^T X2)_0^2 + (E^T X2)_1^2), +inf where the denominator is 0; inlier: d^2 <= thr^2.
 *   count = number of inliers, cost = sum over the valid rows in index order of min(d^2, thr^2), float32.
 * Degenerate: fewer than 8 valid rows, a rank-deficient sample or a non-finite result give cost = +inf, count = 0 and a
 * zero matrix. */
#define MI_POSE_MAX_N 2048
#define MI_POSE_MAX_HYPOTHESES 65536
#define MI_POSE_MAX_REFINE_ROUNDS 8

/* H = num_hypotheses hypotheses per pair, generated and scored: e_h (batch, H, 3, 3), cost (batch, H) float32,
 * count (batch, H) int32.  H < 1: MI_E_SHAPE; H > MI_POSE_MAX_HYPOTHESES, threshold <= 0 or not finite: MI_E_PARAM.
 * threshold is in the units of the points (pixels / mean focal length).  One launch: ceil(H / 64) x batch waves, a lane
 * per hypothesis. */
MI_API int mi_essential_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                   int num_hypotheses, float threshold, uint32_t seed, float *e_h, float *cost,
                                   int32_t *count, mi_stream_t stream);

/* E (batch, 3, 3) from the rows with mask != 0 (mask is required): Hartley normalisation over those rows, the 9x9 normal
 * equations M = A^T A of the rows above, the eigenvector of M's smallest eigenvalue (6 steps of inverse iteration on the
 * Cholesky factor of M + 2e-6 trace(M) I from the all-ones vector), denormalisation and manifold projection as above.
 * ok (batch) bytes: 0 and a zero E for a mask with fewer than 8 rows (or no finite result), else 1.  One wave per pair. */
MI_API int mi_essential_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *e,
                              uint8_t *ok, mi_stream_t stream);

/* The whole estimator: mi_essential_hypotheses into the workspace, then per pair the hypothesis of minimum cost (the
 * lowest h among equals; h = 0 when every cost is +inf) and refine_rounds rounds r = 0 .. R-1 of local optimisation:
 * take the inliers of the best E so far at k_r * threshold, k_r = 1 + (R - 1 - r) / 2 (R = 3: 2, 1.5, 1), refit as
 * mi_essential_refit, score at `threshold`; the refit replaces the best E only when its cost is strictly lower (costs
 * inside this step are summed lanes-strided, so the hypothesis' own cost is re-summed that way first).  A round whose
 * inlier set has fewer than 8 rows changes nothing.
 * e (batch, 3, 3); inlier (batch, n) bytes: d^2 <= threshold^2 under e, 0 for rows that are not valid; best_h (batch) the
 * selected hypothesis; count (batch) = number of inlier bytes set.  A pair without a usable hypothesis gives a zero e, no
 * inliers, count 0.  With refine_rounds = 0, e / count are exactly e_h[best_h] / count[best_h] of mi_essential_hypotheses.
 * 0 <= refine_rounds <= MI_POSE_MAX_REFINE_ROUNDS (MI_E_PARAM).  workspace: mi_essential_ransac_workspace_bytes(batch, n,
 * H) bytes (0 for an unsupported request), 16-byte aligned (MI_E_ALIGN), any content; shorter: MI_E_CAPACITY.  Two launches. */
MI_API size_t mi_essential_ransac_workspace_bytes(int batch, int n, int num_hypotheses);
MI_API int mi_essential_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                               int num_hypotheses, float threshold, int refine_rounds, uint32_t seed, float *e,
                               uint8_t *inlier, int32_t *best_h, int32_t *count, void *workspace, size_t workspace_bytes,
                               mi_stream_t stream);

/* cv2.recoverPose (:102-108): r (batch, 3, 3), t (batch, 3) with x2 ~ r x1 + t, det r = +1, |t| = 1, from e (any scale
 * and sign) and the rows with mask != 0 (NULL: every row).  E is scaled to Frobenius norm sqrt(2); t = the normalised
 * cross product of largest norm among the column pairs (0,1), (0,2), (1,2) of E, the first among equals (the left null
 * vector); Ra = cof(E) - [t]x E and Rb = cof(E) + [t]x E (cof: the matrix of cofactors), each followed by one step
 * R (3 I - R^T R) / 2 towards the nearest rotation.  Candidates in this order: 0 (Ra, t), 1 (Rb, t), 2 (Ra, -t),
 * 3 (Rb, -t).  Under a candidate a row PASSES when, with a = X2 x (R X1), c = X2 x t: z1 = -(a.c) / (a.a) (the depth in
 * camera 1 that best satisfies X2 x (z1 R X1 + t) = 0) and z2 = z1 (R X1)_2 + t_2 are both positive and both below
 * distance_threshold (> 0; OpenCV's recoverPose default is 50).  The candidate with the most passing rows wins, the first
 * among equals.  pose_mask (batch, n): the rows that pass under the winner (a subset of mask); count (batch): their
 * number; ok (batch) bytes: 1 when count >= 5 (the reference's cut at :109), else 0 with r = identity and t = 0.  A zero
 * or non-finite e gives count 0.  One wave per pair. */
MI_API int mi_recover_pose(const float *e, const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n,
                           float distance_threshold, float *r, float *t, uint8_t *pose_mask, int32_t *count, uint8_t *ok,
                           mi_stream_t stream);

/* cv2.triangulatePoints and the tail of triangulate_points (:143-160): proj1, proj2 (batch, 3, 4), pts1, pts2
 * (batch, n, 2) as (x, y) in the units the projection matrices expect (pixels for K [R | t]); any n >= 1.  Per point the
 * rows x P[2] - P[0], y P[2] - P[1] of both views, each scaled to unit norm (conditioning; OpenCV does not), and the unit
 * right singular vector X of the smallest singular value (one-sided Jacobi, 6 sweeps).  points (batch, n, 3) = X[:3] / X[3]
 * where |X[3]| > 1e-9 and the quotient is finite, else zeros; finite (batch, n) bytes say which.  A system of rank < 3 --
 * the second smallest singular value not above 1e-5 times the largest: identical rays under identical cameras, where
 * every point of the ray is a solution -- also gives zeros and finite = 0.  One thread per point. */
MI_API int mi_triangulate(const float *proj1, const float *proj2, const float *pts1, const float *pts2, int batch, int n,
                          float *points, uint8_t *finite, mi_stream_t stream);

/* ---- frame ingest (K16): sample/visual_odometry.py:65-92 load_image_from_array, sample/image_matching.py ------------
 * What the reference's hosts do to every camera frame on the CPU before the model sees it -- cv2.cvtColor(BGR2GRAY),
 * cv2.resize(..., (w, h), INTER_LINEAR), astype(float32) -- in one kernel on the device: the front door of the `_u8`
 * entry points above (uint8 output) and of the float32 ones (float32 output).
 *
 * src: `batch` frames of src_h x src_w pixels of `channels` interleaved bytes (1, 3 or 4: HWC, as cameras and decoders
 * deliver them), rows row_pitch bytes apart, frames frame_pitch bytes apart (a cropped view or a padded camera buffer
 * goes in without a copy).  No alignment is required of src or of the pitches.  channel_order: MI_INGEST_BGR or
 * MI_INGEST_RGB; the 4th of 4 channels is ignored, with 1 channel the order is ignored and the byte is the gray value.
 * dst: (batch, 1, h, w) contiguous, uint8 or -- dst_is_f32 != 0 -- float32 holding exactly the uint8 values.  Only
 * the bytes of src that belong to pixels are used, but the kernel reads whole aligned 16-byte blocks around them.
 *
 * THE ARITHMETIC, in integers (C's >> on non-negative int32; everything fits int32):
 *   gray   g = (3735 B + 19235 G + 9798 R + 16384) >> 15
 *   taps   along each axis, for destination index d, with scale = (double)src / (double)dst:
 *            f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s;        (f: float32)
 *            if (s < 0) { s = 0; f = 0; }    if (s >= src - 1) { s = src - 1; f = 0; }
 *            second tap min(s + 1, src - 1);  w1 = rint(f * 2048), w0 = rint((1 - f) * 2048)
 *            (float32 products, round to nearest even; nothing fused)
 *   rows   r = g[s] * a0 + g[s + 1] * a1                       (horizontal pass, weights a of the x axis)
 *   out    = (((b0 * (r_top >> 4)) >> 16) + ((b1 * (r_bot >> 4)) >> 16) + 2) >> 2      (weights b of the y axis)
 * Gray is taken at the taps only, which equals gray-then-resize.  With src == dst sizes the formula is the identity on
 * the gray image, and the kernel skips the blend there.
 *
 * This is OpenCV 4's 8-bit path (cvtColor's fixed-point BGR2GRAY, resize's INTER_LINEAR with 11-bit weights) restated
 * from its sources AS REMEMBERED: no cv2 build was available to compare against, so agreement with cv2 is UNMEASURED.
 * One known difference: OpenCV switches an exact 2x INTER_LINEAR downscale to its area path (the mean of 2 x 2 pixels);
 * this entry keeps the formula above at every ratio.  The contract is the arithmetic stated here, not cv2.
 *
 * Checks before any launch: NULL src / dst -> MI_E_NULL; batch, src_h, src_w, h, w < 1 -> MI_E_SHAPE; channels not in
 * {1, 3, 4}, channel_order not one of the two, any of the five extents > MI_INGEST_MAX_DIM, row_pitch < src_w * channels,
 * row_pitch > 2^40, frame_pitch < row_pitch * src_h or frame_pitch > 2^48 -> MI_E_PARAM.  One launch; no allocation, no
 * memset, no host synchronisation, no coefficient table copied to the device (the taps are computed in the kernel):
 * capturable like the rest of the library. */
enum { MI_INGEST_BGR = 0, MI_INGEST_RGB = 1 };
#define MI_INGEST_MAX_DIM 16384
MI_API int mi_ingest_frames(const uint8_t *src, int batch, int src_h, int src_w, int channels, long long row_pitch,
                            long long frame_pitch, int channel_order, void *dst, int dst_is_f32, int h, int w,
                            mi_stream_t stream);

/* ---- metric RGB-D pose (K17): matched keypoints + aligned depth -> the rigid motion between two frames, in the depth's units --
 * K15 ends at a translation of unit length.  With a depth frame per image (aligned to the colour camera, mi_depth_align)
 * the matched keypoints lift to 3-D points, and the motion X2 = R X1 + t follows with its scale from three correspondences.
 * The reference has no such step (its odometry sample sums unit translations).  Five entries, batched over pairs, under the
 * contract of the K15 section: pure functions of their arguments, no allocation, no synchronisation, no memset, one stream,
 * no atomics, every sum in a fixed order (the same inputs and seed give the same bits), capturable into a hipGraph; outputs
 * and workspace may hold anything on entry and every output element is written; MI_E_* before any launch.
 * Row i of pair b is pts1[b][i] <-> pts2[b][i], (batch, n, 3) float32 points in the two camera frames; `valid` / `mask`
 * (batch, n) bytes select rows (non-zero = use; valid may be NULL: every row).  Rows that are not selected are never read for
 * their coordinates.  1 <= n <= MI_RIGID_MAX_N (a staged row is 24 bytes: 48 KB of rows and 4 KB of indices in LDS, three
 * one-wave workgroups per CU for mi_rigid_hypotheses and mi_rigid_refit; the second kernel of mi_rigid_ransac adds 4 KB of
 * flags and holds two), batch <= 65535 (MI_E_PARAM beyond; < 1: MI_E_SHAPE).
 *
 * Divergences from the usual host implementations (Open3D's RANSAC registration, OpenCV's estimateAffine3D), all deliberate:
 *   - the model is a rotation and a translation (no scale, no shear), solved in closed form by Horn's unit-quaternion method;
 *     the eigenvector is taken by a FIXED number of cyclic Jacobi sweeps, not by an iterative LAPACK routine;
 *   - the best hypothesis is the one of minimum truncated cost sum min(d^2, thr^2) (MSAC), not of maximum inlier count;
 *   - a fixed number of hypotheses, no adaptive stop; the sampler is K15's stateless counter-based hash;
 *   - refinement is refine_rounds rounds of refit on the inliers (local optimisation), no ICP, no per-point weights;
 *   - depth is read at the NEAREST pixel, never interpolated (interpolating across an occlusion edge invents surfaces).
 *
 * Sampling.  K15's draw(seed, b, h, s), unchanged (the counter is still 8 h + s), for the slots s = 0, 1, 2, with the same
 *   without-replacement rule over the ranks of the valid rows: three distinct ranks.
 * Solve.  For the sample's rows a_k (frame 1), b_k (frame 2), k = 0, 1, 2: centroids ca = ((a_0 + a_1) + a_2) / 3, cb
 *   likewise; S[i][j] = sum over k in order of (a_k - ca)_i (b_k - cb)_j; Horn's symmetric matrix
 *       N = [ Sxx+Syy+Szz   Syz-Szy        Szx-Sxz        Sxy-Syx     ]
 *           [     .         Sxx-Syy-Szz    Sxy+Syx        Szx+Sxz     ]
 *           [     .             .         -Sxx+Syy-Szz    Syz+Szy     ]
 *           [     .             .              .         -Sxx-Syy+Szz ]
 *   the unit eigenvector q = (q0, qx, qy, qz) of N's largest eigenvalue by cyclic Jacobi: 6 sweeps over the pairs (0,1) (0,2)
 *   (0,3) (1,2) (1,3) (2,3) in this order, each pair rotated by the angle that zeroes its off-diagonal element (skipped when
 *   that element is exactly 0), the eigenvalue lambda_m being the first maximum of the final diagonal and q column m of the
 *   accumulated rotations V (the kernels' arithmetic run on the CPU returns the same bits for 4 to 12 sweeps on the test
 *   scenes; 3 sweeps leave 0.18 deg).  Then ONE correction against N itself: w = N q - lambda_m q with float64 products,
 *   q = q + sum over j != m of ((v_j . w) / (lambda_m - lambda_j)) v_j.  Three points span a plane, so N's eigenvalues come
 *   in +- pairs and the two largest of a slim triangle lie within a percent of each other; the rotations' accumulated
 *   roundings (a few eps |N|) then turn into 4e-3 deg, which this step takes back to 3.5e-4 deg, the level of LAPACK's
 *   float32 eigh (3.1e-4 deg on the same 192 samples).  q is scaled to unit length and negated when q0 < 0; R is the
 *   rotation matrix of q; t = cb - R ca.
 * Degenerate sample.  With e1 = p_1 - p_0 and e2 = p_2 - p_0, a sample is degenerate in a frame when
 *   |e1 x e2|^2 <= 1e-6 |e1|^2 |e2|^2 (collinear or repeated points).  Degeneracy in either frame, fewer than 3 valid rows
 *   or a non-finite result give cost = +inf, count = 0 and zeros in rt_h.
 * Score.  For every valid row u = ((R X1) + t) - X2, each component ((R_j0 x + R_j1 y) + R_j2 z) + t_j - X2_j in this order,
 *   d^2 = (u_0^2 + u_1^2) + u_2^2; inlier: d^2 <= thr^2; count = number of inliers, cost = sum over the valid rows in index
 *   order of min(d^2, thr^2), float32. */
#define MI_RIGID_MAX_N 2048

/* keypoints (batch, n, 2) pixel (y, x) + depth (batch, h, w) -> points (batch, n, 3) float32 in the camera frame and valid
 * (batch, n) bytes; one thread per keypoint.  depth: float32 (depth_is_u16 = 0) or uint16 counts (1; converted exactly), as
 * in mi_depth_to_points, ALREADY aligned to the camera of k_inv (3x3 row-major inverse camera matrix, device memory).
 *     xn = (x k_inv[0] + y k_inv[1]) + k_inv[2];  yn = (x k_inv[3] + y k_inv[4]) + k_inv[5]      mi_normalise_keypoints' bits
 *     px = floorf(x + 0.5f);  py = floorf(y + 0.5f);  d = depth[b][py][px];  Z = d * z_scale       one float32 product
 *     point = (xn * Z, yn * Z, Z)
 * A row is valid when valid_in (batch, n; NULL: every row) is non-zero, the keypoint is finite, 0 <= px < w, 0 <= py < h,
 * d is finite and min_depth <= Z <= max_depth.  Invalid rows get a zero point and a zero byte; their depth is not read
 * when the pixel is outside the frame.  batch, n, h, w < 1: MI_E_SHAPE; min_depth <= 0, max_depth < min_depth or not
 * finite, z_scale <= 0 or not finite: MI_E_PARAM.  One launch. */
MI_API int mi_lift_keypoints(const float *keypoints, const void *depth, int depth_is_u16, int batch, int n, int h, int w,
                             const float *k_inv, float z_scale, float min_depth, float max_depth, const uint8_t *valid_in,
                             float *points, uint8_t *valid, mi_stream_t stream);

/* H = num_hypotheses hypotheses per pair, generated and scored: rt_h (batch, H, 12) = R row-major, then t; cost (batch, H)
 * float32, count (batch, H) int32.  H < 1: MI_E_SHAPE; H > MI_POSE_MAX_HYPOTHESES, threshold <= 0 or not finite:
 * MI_E_PARAM.  threshold is in the units of the points.  One launch: ceil(H / 64) x batch waves, a lane per hypothesis. */
MI_API int mi_rigid_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                               int num_hypotheses, float threshold, uint32_t seed, float *rt_h, float *cost, int32_t *count,
                               mi_stream_t stream);

/* r (batch, 3, 3), t (batch, 3) from the rows with mask != 0 (mask is required), in two passes: the centroids ca, cb (sums
 * lanes-strided, then / m for m rows), then the centred products S = sum (a - ca)(b - cb)^T, Ca = sum (a - ca)(a - ca)^T and
 * Cb likewise; the solve of the section above from S.  The set is DEGENERATE when the second largest eigenvalue of Ca or of
 * Cb (cyclic Jacobi as above on the 3x3 matrix, pairs (0,1) (0,2) (1,2)) is not above 1e-6 times the largest: the points
 * of that frame lie on a line or in one place.  ok (batch) bytes: 0 with r = identity and t = 0 for fewer than 3 rows, a
 * degenerate set or a non-finite result, else 1.  One wave per pair. */
MI_API int mi_rigid_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *r, float *t,
                          uint8_t *ok, mi_stream_t stream);

/* The whole estimator: mi_rigid_hypotheses into the workspace, then per pair the hypothesis of minimum cost (the lowest h
 * among equals; h = 0 when every cost is +inf) and refine_rounds rounds r = 0 .. R-1 of local optimisation: take the
 * inliers of the best motion so far at k_r * threshold, k_r = 1 + (R - 1 - r) / 2, refit as mi_rigid_refit, score at
 * `threshold`; the refit replaces the best motion only when its cost is strictly lower.  Inside this step a
 * cost is held as (number of valid rows beyond the threshold, float32 sum of the inliers' d^2, summed lanes-strided) and
 * compared as k thr^2 + s in float64, the hypothesis' own cost re-formed that way first: in one float32 sum a handful of
 * truncated rows (thr^2 each) absorbs any improvement of a small inlier residual (0.0325 + 1e-11 == 0.0325), and the
 * refit of clean data would never replace its minimal sample.  A round whose inlier set has fewer than 3 rows
 * (or is degenerate) changes nothing.
 * r (batch, 3, 3), t (batch, 3); inlier (batch, n) bytes: d^2 <= threshold^2 under (r, t), 0 for rows that are not valid;
 * best_h (batch) the selected hypothesis; count (batch) = number of inlier bytes set; rmse (batch) float32 = sqrt of the
 * mean d^2 over the inliers (summed lanes-strided); ok (batch) bytes = 1 when a usable hypothesis exists and count >= 3.
 * Where ok = 0: r = identity, t = 0, no inliers, count = 0, rmse = 0.  With refine_rounds = 0 and ok = 1, r / t / count are
 * exactly rt_h[best_h] / count[best_h] of mi_rigid_hypotheses.
 * 0 <= refine_rounds <= MI_POSE_MAX_REFINE_ROUNDS (MI_E_PARAM).  workspace: mi_rigid_ransac_workspace_bytes(batch, n, H)
 * bytes (0 for an unsupported request), 16-byte aligned (MI_E_ALIGN), any content; shorter: MI_E_CAPACITY.  Two launches. */
MI_API size_t mi_rigid_ransac_workspace_bytes(int batch, int n, int num_hypotheses);
MI_API int mi_rigid_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                           float threshold, int refine_rounds, uint32_t seed, float *r, float *t, uint8_t *inlier,
                           int32_t *best_h, int32_t *count, float *rmse, uint8_t *ok, void *workspace, size_t workspace_bytes,
                           mi_stream_t stream);

/* ---- dense RGB-D refinement (K18): two aligned depth frames + a starting pose -> the pose refined against every pixel -------
 * K17's pose rests on a few hundred matches, each reading depth at one pixel.  This section refines such a pose (or the
 * identity, for a frame with too few matches) by projective point-to-plane ICP over the whole of both depth frames, and
 * returns the 6x6 information matrix of the result.  Four entries, batched over pairs, under the contract of the K15 / K17
 * sections: pure functions of their arguments, no allocation, no synchronisation, no memset, one stream, no atomics, every
 * sum in a fixed order, capturable into a hipGraph; outputs and workspace may hold anything on entry and every output
 * element is written; MI_E_* before any launch.  A pair's result is the same bits alone or inside a batch, and from run to
 * run.  Motion convention: X2 = R X1 + t.  Per-pixel arithmetic is float32 with nothing fused, the solve and the pose float64.
 *
 * Surfel maps (mi_surfel_maps), per frame: two records of 4 float32 per pixel, (batch, h, w, 4) each.
 *   vertex  (vx, vy, vz, f): for the integer pixel (x, y): xn = (x k_inv[0] + y k_inv[1]) + k_inv[2], yn = (x k_inv[3] +
 *     y k_inv[4]) + k_inv[5] (mi_lift_keypoints' ray), Z = d * z_scale, v = (xn * Z, yn * Z, Z); valid (f = 1) when d is finite
 *     and min_depth <= Z <= max_depth, else zeros.
 *   normal  (nx, ny, nz, f): a = v(x+1, y) - v(x-1, y), b = v(x, y+1) - v(x, y-1), m = a x b with each component as
 *     a_i b_j - a_j b_i, |m|^2 = (m_0^2 + m_1^2) + m_2^2, n = m / sqrt(|m|^2), negated when (n_0 v_0 + n_1 v_1) + n_2 v_2 > 0
 *     (it faces the camera).  Valid (f = 1) only when the centre and all four neighbours are valid and in the frame, every
 *     neighbour's |Z - Z_centre| <= normal_max_jump, and |m|^2 is positive and finite; else zeros.  Border pixels have none.
 *   These are surface normals; the normals of mi_depth_to_points_normals are the reference's Sobel-of-(X+Y+Z) maps.
 *
 * One linearisation at pose (R, t), float32, and source stride s: over the pixels (y, x) of frame 1 with y % s == 0 and
 *   x % s == 0 whose normal is valid, with v1, n1 of frame 1:
 *     q_j = ((R_j0 v1_0 + R_j1 v1_1) + R_j2 v1_2) + t_j;   m_j = (R_j0 n1_0 + R_j1 n1_1) + R_j2 n1_2
 *     u = fx * (q_0 / q_2) + cx, v = fy * (q_1 / q_2) + cy;  px = floorf(u + 0.5f), py = floorf(v + 0.5f)   (nearest pixel:
 *     no interpolation, by K17's argument about occlusion edges)
 *   rejected when q_2 <= 0, (px, py) is outside the frame, frame 2 has no valid normal there, or with v2, n2 of that pixel
 *   and e = q - v2:  (e_0^2 + e_1^2) + e_2^2 > distance_threshold^2  or  (m_0 n2_0 + m_1 n2_1) + m_2 n2_2 < cos(angle_threshold)
 *   (the cosine taken in float64 on the host and rounded to float32).  For a survivor r = (n2_0 e_0 + n2_1 e_1) + n2_2 e_2 and
 *   J = [q x n2, n2] (the cross product's components as q_i n2_j - q_j n2_i).  29 sums: the 21 entries of the upper triangle
 *   of A = sum J^T J in row-major order, the 6 of b = sum J r, sum r^2, the count.
 *   Order of the sums.  The sampled pixels are numbered row-major over the ceil(h / s) x ceil(w / s) grid and cut into slabs
 *   of 2048 consecutive numbers: a function of (h, w, s) alone.  Inside a slab, lane l of 256 adds its samples l, l + 256, ...
 *   in this order in float32 (a rejected pixel adds zeros); each of the 4 waves folds its 64 lanes by wave_sum_dpp's tree
 *   (csrc/common.h); the 4 wave totals are added in wave order in float64; the slabs are added in slab order in float64.
 *   The count is an integer sum.
 *
 * Step.  A x = -b in float64 by LDL^T without pivoting.  The pair is DEGENERATE when count < min_correspondences, when a
 *   pivot is not above 1e-6 * max diag(A), or when a sum, the solution or the new pose is not finite.  Otherwise, with
 *   x = (omega, tau): R <- Exp(omega) R, t <- Exp(omega) t + tau, Exp by Rodrigues in float64 (I + [omega]x below
 *   |omega| = 1e-8).  The pose lives in float64 in the workspace between iterations; each linearisation reads it rounded
 *   to float32, and the outputs are that rounding.  A degenerate pair is FROZEN: its pose stays the one before the failed
 *   solve, later iterations do nothing for it (the kernels read a per-pair state word and return), ok = 0.
 * Schedule.  stages (1 .. MI_ICP_MAX_STAGES) of (stride in {1, 2, 4, 8}, iterations >= 0), at most MI_ICP_MAX_ITERATIONS
 *   iterations in all, run as given: no adaptive stop.  After the last update ONE more linearisation at the last stage's
 *   stride, for every pair (frozen ones at their frozen pose), gives count, rmse = sqrt(sum r^2 / count) (0 for count = 0)
 *   and information = A as a full symmetric 6x6 in (omega, tau) order.  ok = 1 when no solve failed and that count is at
 *   least min_correspondences.  With no iterations at all the result is the initial pose (its bits) with those statistics. */
#define MI_ICP_MAX_STAGES 4
#define MI_ICP_MAX_ITERATIONS 64

/* depth (batch, h, w), float32 (depth_is_u16 = 0) or uint16 counts (1), ALREADY aligned to the camera of k_inv (3x3
 * row-major inverse camera matrix, device memory) -> vertex_out, normal_out (batch, h, w, 4) float32, 16-byte aligned
 * (MI_E_ALIGN).  batch < 1, h or w < 3, batch * h * w >= 2^31: MI_E_SHAPE; batch > 65535, min_depth <= 0, max_depth <
 * min_depth or not finite, z_scale or normal_max_jump <= 0 or not finite: MI_E_PARAM.  One launch, one thread per pixel. */
MI_API int mi_surfel_maps(const void *depth, int depth_is_u16, int batch, int h, int w, const float *k_inv, float z_scale,
                          float min_depth, float max_depth, float normal_max_jump, float *vertex_out, float *normal_out,
                          mi_stream_t stream);

/* bytes of workspace for mi_icp_linearise / mi_icp_refine (0 for an unsupported shape): the float64 poses, the state and
 * step words and one 256-byte record of partial sums per slab of the stride-1 grid and pair. */
MI_API size_t mi_icp_workspace_bytes(int batch, int h, int w);

/* One linearisation: the maps of both frames, r (batch, 3, 3) and t (batch, 3) float32 per pair -> sums (batch, 29)
 * float64 in the order above (the count as a float64).  stride not in {1, 2, 4, 8}, fx or fy or distance_threshold <= 0 or
 * not finite, cx or cy not finite, angle_threshold (radians) outside (0, pi]: MI_E_PARAM; maps or workspace not 16-byte
 * aligned: MI_E_ALIGN; workspace shorter than mi_icp_workspace_bytes: MI_E_CAPACITY.  Two launches. */
MI_API int mi_icp_linearise(const float *vertex1, const float *normal1, const float *vertex2, const float *normal2,
                            const float *r, const float *t, int batch, int h, int w, float fx, float fy, float cx, float cy,
                            int stride, float distance_threshold, float angle_threshold, double *sums, void *workspace,
                            size_t workspace_bytes, mi_stream_t stream);

/* The whole refinement from r0 (batch, 3, 3), t0 (batch, 3).  strides / iterations: HOST arrays of `stages` entries, read
 * before the call returns.  Outputs: r (batch, 3, 3), t (batch, 3), information (batch, 36) float32, rmse (batch) float32,
 * count (batch) int32, steps (batch) int32 = the number of updates applied, ok (batch) bytes.  The checks of
 * mi_icp_linearise, and stages outside 1 .. MI_ICP_MAX_STAGES, an iteration count below 0, more than
 * MI_ICP_MAX_ITERATIONS in all, min_correspondences < 1: MI_E_PARAM.  1 + 2 (iterations + 1) launches, enqueued back to back. */
MI_API int mi_icp_refine(const float *vertex1, const float *normal1, const float *vertex2, const float *normal2,
                         const float *r0, const float *t0, int batch, int h, int w, float fx, float fy, float cx, float cy,
                         const int32_t *strides, const int32_t *iterations, int stages, float distance_threshold,
                         float angle_threshold, int min_correspondences, float *r, float *t, float *information, float *rmse,
                         int32_t *count, int32_t *steps, uint8_t *ok, void *workspace, size_t workspace_bytes,
                         mi_stream_t stream);

/* ---- direct RGB-D refinement (K21): a photometric term joined to K18's point-to-plane system --------------------------------
 * K18 uses depth alone, so a scene of one plane (a wall, a floor, a table top) leaves three directions free and freezes
 * the pair.  This section adds the intensity residual of direct RGB-D odometry, taken on the gray model frames of
 * mi_ingest_frames: texture pins what geometry leaves free.  The term is a WEIGHTED OPTION: texture seen past an occlusion
 * edge biases it, so on a scene that K18 already constrains well the joint result can be further from the truth than
 * K18's.  Four entries, batched over pairs, under the contract of the K15 / K17 / K18 sections: pure functions of their
 * arguments, no allocation, no synchronisation, no memset, one stream, no atomics, every sum in a fixed order, capturable
 * into a hipGraph; outputs and workspace may hold anything on entry and every output element is written; MI_E_* before any
 * launch.  A pair's result is the same bits alone or inside a batch, and from run to run.  Per-pixel arithmetic is float32
 * with nothing fused, the joint system, the solve and the pose float64.  K18's entries, kernels and bits are untouched.
 *
 * Intensity maps (mi_intensity_maps), per frame: one record of 4 float32 per pixel, (batch, h, w, 4): (I, gx, gy, f) with
 *   I the gray value as float32, gx = 0.5f * (I(x+1, y) - I(x-1, y)), gy = 0.5f * (I(x, y+1) - I(x, y-1)); valid (f = 1) for an
 *   interior pixel (1 <= x <= w - 2, 1 <= y <= h - 2) whose five values are finite, else zeros.  Border pixels have none.
 *
 * One photometric linearisation at pose (R, t), float32, and source stride s: over the pixels of frame 1 on the stride's
 *   grid whose VERTEX record and intensity record are valid (no normal is needed), with v1 and I1 of frame 1:
 *     q, u, v, px, py exactly as in K18;  x0 = floorf(u), y0 = floorf(v), a = u - x0, b = v - y0
 *   rejected when q_2 <= 0, the footprint (x0 .. x0 + 1, y0 .. y0 + 1) is not inside the frame, one of its four intensity
 *   records in frame 2 is invalid, frame 2's vertex record at the NEAREST pixel (px, py) is invalid, or |q_2 - v2_2| >
 *   distance_threshold (the occlusion check).  I2, gx, gy are the bilinear blends of the four records c00 c01 (row y0) and
 *   c10 c11 (row y0 + 1), each as top = c00 + a * (c01 - c00), bot = c10 + a * (c11 - c10), top + b * (bot - top).
 *   r = I2 - I1; rejected when |r| > intensity_threshold.  For a survivor
 *     c = ((fx * gx) / q_2, (fy * gy) / q_2, -((c_0 * q_0 + c_1 * q_1) / q_2))   and   J = [q x c, c]
 *   (the cross product's components as q_i c_j - q_j c_i).  29 sums in K18's layout: the 21 entries of the upper triangle of
 *   sum J^T J in row-major order, the 6 of sum J r, sum r^2, the count.  The order of the sums is K18's, word for word: the
 *   same slabs of 2048 sampled pixels, lanes, wave tree and float64 folding.
 *
 * Joint step.  With w = photo_weight (the depth's unit per gray level) as float64 and the geometric sums g of K18's
 *   linearisation and the photometric sums p at the same pose and stride: s_k = g_k + (w * w) * p_k for the 21 + 6 + 1
 *   entries of A, b and sum r^2, and the count count_g + count_p.  K18's step is applied to s: the same solve, the same
 *   rules of degeneracy (the joint count below min_correspondences, a pivot, anything not finite), the same update,
 *   freezing and schedule.  The final linearisation reports both counts, rmse = sqrt(g_27 / count_g) and rmse_photo =
 *   sqrt(p_27 / count_p) (0 for a count of 0) and information = the joint A; ok = 1 when no solve failed and count_g +
 *   count_p is at least min_correspondences.  photo_weight == 0 launches nothing photometric, s = g, count_photo = 0,
 *   rmse_photo = 0: every other output has mi_icp_refine's bits. */

/* gray (batch, h, w), uint8 (gray_is_u8 = 1) or float32 (0): the two outputs of mi_ingest_frames -> intensity_out
 * (batch, h, w, 4) float32, 16-byte aligned (MI_E_ALIGN).  Shape limits of mi_surfel_maps.  One launch, one thread per pixel. */
MI_API int mi_intensity_maps(const void *gray, int gray_is_u8, int batch, int h, int w, float *intensity_out, mi_stream_t stream);

/* bytes of workspace for mi_photo_linearise / mi_rgbd_refine (0 for an unsupported shape): mi_icp_workspace_bytes' content
 * with a second array of slab records. */
MI_API size_t mi_rgbd_workspace_bytes(int batch, int h, int w);

/* One photometric linearisation: the vertex and intensity maps of both frames, r (batch, 3, 3) and t (batch, 3) float32 per
 * pair -> sums (batch, 29) float64 in the order above.  The checks of mi_icp_linearise (no angle), and intensity_threshold
 * <= 0 or not finite: MI_E_PARAM.  Two launches. */
MI_API int mi_photo_linearise(const float *vertex1, const float *intensity1, const float *vertex2, const float *intensity2,
                              const float *r, const float *t, int batch, int h, int w, float fx, float fy, float cx, float cy,
                              int stride, float distance_threshold, float intensity_threshold, double *sums, void *workspace,
                              size_t workspace_bytes, mi_stream_t stream);

/* The joint refinement from r0, t0: mi_icp_refine's arguments, the two intensity maps, photo_weight and
 * intensity_threshold; mi_icp_refine's outputs (count, rmse: the geometric term's) and rmse_photo (batch) float32,
 * count_photo (batch) int32.  The checks of mi_icp_refine, and photo_weight < 0 or not finite, intensity_threshold <= 0 or
 * not finite: MI_E_PARAM.  1 + 3 (iterations + 1) launches (2 (iterations + 1) for photo_weight == 0), enqueued back to back. */
MI_API int mi_rgbd_refine(const float *vertex1, const float *normal1, const float *intensity1, const float *vertex2,
                          const float *normal2, const float *intensity2, const float *r0, const float *t0, int batch, int h,
                          int w, float fx, float fy, float cx, float cy, const int32_t *strides, const int32_t *iterations,
                          int stages, float distance_threshold, float angle_threshold, float photo_weight,
                          float intensity_threshold, int min_correspondences, float *r, float *t, float *information,
                          float *rmse, int32_t *count, float *rmse_photo, int32_t *count_photo, int32_t *steps, uint8_t *ok,
                          void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- TSDF fusion (K19): depth frames -> a fused signed distance volume -> a synthetic surfel map for K18 -----------------------
 * K17 and K18 estimate each pose against ONE noisy depth frame.  This section accumulates depth frames into a truncated
 * signed distance volume and raycasts the volume, at a predicted pose, into a surfel map in exactly mi_surfel_maps' record
 * layout and validity convention, which mi_icp_linearise / mi_icp_refine take as `vertex1` / `normal1` unchanged: frame-to-model
 * tracking.  The reference has no counterpart.  Four entries, batched over volumes, under the contract of the K15 / K17 / K18
 * sections: pure functions of their arguments, no allocation, no synchronisation, no memset, no atomics, one stream,
 * capturable into a hipGraph; every output element is written whatever the buffers held on entry; MI_E_* before any launch;
 * a volume's result is the same bits alone or inside a batch, and from run to run.  Per-voxel and per-sample arithmetic is
 * float32 with nothing fused.
 *
 * Volume.  (batch, nz, ny, nx) voxels, x fastest; a voxel is a record of two float32 (tsdf, weight), 8 bytes; the base is
 *   16-byte aligned (MI_E_ALIGN).  origin (x, y, z), voxel_size and truncation are host parameters shared by the batch.  The
 *   centre of voxel (i, j, k) is ((i + 0.5f) * voxel_size) + origin_x, and likewise for j, k with origin_y, origin_z.  An empty
 *   voxel is (1, 0).  Poses are world (the volume's frame) to camera, X_c = R X_w + t: K17 / K18's X2 = R X1 + t with the volume
 *   as frame 1.
 * Checks common to the volume entries: batch < 1, a dimension < 2, batch * nz * ny * nx >= 2^31: MI_E_SHAPE; batch > 65535,
 *   an origin component not finite, voxel_size or truncation <= 0 or not finite: MI_E_PARAM.
 *
 * Integration, per voxel with centre p, for the frames f = 0 .. frames-1 in order (a frame whose `active` byte is 0 is left out):
 *     q_j = ((R_j0 p_0 + R_j1 p_1) + R_j2 p_2) + t_j                                      skip when q_2 <= 0
 *     px = floorf((fx * (q_0 / q_2) + cx) + 0.5f), py = floorf((fy * (q_1 / q_2) + cy) + 0.5f)   skip outside the w x h frame
 *     d = depth[py][px], Z = d * z_scale                         skip unless d is finite and min_depth <= Z <= max_depth
 *     sdf = Z - q_2                                              skip when sdf < -truncation
 *     f = fminf(1, sdf / truncation);  tsdf <- (tsdf * weight + f) / (weight + 1);  weight <- fminf(weight + 1, max_weight)
 *   The volume makes ONE pass through memory however many frames: a voxel is read once, updated in registers by every frame,
 *   written once (8 bytes in, 8 bytes out).  Frames given in one call and the same frames given one per call give the same bits.
 *
 * Raycast, per integer pixel (x, y): xn = (x k_inv[0] + y k_inv[1]) + k_inv[2], yn = (x k_inv[3] + y k_inv[4]) + k_inv[5], the
 *   ray of mi_surfel_maps.  Samples lie on a FIXED grid of camera depths s_k = ((float)k * step) + min_depth, step =
 *   step_fraction * truncation (one float32 product), k = 0 .. ceilf((max_depth - min_depth) / step) (float32).  A kernel may
 *   leave out ranges of k whose samples lie outside the volume's box (they are invalid); it may not move the grid.
 *   Sample at depth s: c = (xn * s - t_0, yn * s - t_1, s - t_2); X_w,j = (R_0j c_0 + R_1j c_1) + R_2j c_2 (R^T c);
 *     g_j = (X_w,j - origin_j) / voxel_size - 0.5f, the grid coordinate (voxel centres at the integers).  With b = floorf(g) and
 *     a = g - b per axis the sample is the trilinear interpolation of tsdf over the eight corners b + {0, 1}^3, along x, then y,
 *     then z, each step as u + a * (v - u).  It is VALID only when the eight corners exist (0 <= b_j <= n_j - 2 on every axis)
 *     and all eight have weight > 0.
 *   The march ends at the first valid sample with f <= 0; it is a HIT only if the sample before it on the grid (k - 1) was valid
 *     with f_prev > 0: s* = s_prev + step * (f_prev / (f_prev - f)), vertex = (xn * s*, yn * s*, s*, 1).
 *   Normal: with g* the grid coordinate of the depth s* (formed as for a sample), G_j = F(g* + e_j) - F(g* - e_j) for the three
 *     axes, F the trilinear sample and e_j one voxel (the coordinate g*_j + 1.0f or g*_j - 1.0f); all six samples must be valid.
 *     m_j = (R_j0 G_0 + R_j1 G_1) + R_j2 G_2, |m|^2 = (m_0^2 + m_1^2) + m_2^2, n = m / sqrt(|m|^2), negated when
 *     (n_0 v_0 + n_1 v_1) + n_2 v_2 > 0; normal = (n, 1) when |m|^2 is positive and finite, else zeros (the vertex stays).
 *   No hit: both records are zeros. */

/* (1, 0) into every voxel of volume (batch, nz, ny, nx, 2).  One launch. */
MI_API int mi_tsdf_reset(float *volume, int batch, int nz, int ny, int nx, mi_stream_t stream);

/* depth (batch, frames, h, w), float32 (depth_is_u16 = 0) or uint16 counts (1), ALREADY aligned to the camera (fx, fy, cx, cy);
 * r (batch, frames, 3, 3), t (batch, frames, 3) float32; active (batch, frames) bytes in device memory, read by the kernel
 * (non-zero = integrate; NULL: every frame), so that a tracker's `ok` gates the integration without a host synchronisation.
 * frames < 1, h or w < 3, batch * frames * h * w >= 2^31: MI_E_SHAPE; max_weight, fx, fy or z_scale <= 0 or not finite, cx or
 * cy not finite, min_depth <= 0, max_depth < min_depth or not finite: MI_E_PARAM.  One launch, a wave per x-row of the volume. */
MI_API int mi_tsdf_integrate(float *volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y, float origin_z,
                             float voxel_size, float truncation, float max_weight, const void *depth, int depth_is_u16, int frames,
                             int h, int w, float fx, float fy, float cx, float cy, float z_scale, float min_depth, float max_depth,
                             const float *r, const float *t, const uint8_t *active, mi_stream_t stream);

/* volume + one pose per volume, r (batch, 3, 3), t (batch, 3) -> vertex_out, normal_out (batch, h, w, 4) float32, 16-byte
 * aligned (MI_E_ALIGN), in the camera frame.  k_inv: 3x3 row-major inverse camera matrix, device memory.  h or w < 3,
 * batch * h * w >= 2^31: MI_E_SHAPE; step_fraction <= 0, > 1 or not finite, min_depth <= 0, max_depth < min_depth or not finite,
 * 2^24 or more samples on a ray: MI_E_PARAM.  One launch, a wave per 8 x 8 pixel tile. */
MI_API int mi_tsdf_raycast(const float *volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y, float origin_z,
                           float voxel_size, float truncation, float step_fraction, const float *r, const float *t, int h, int w,
                           const float *k_inv, float min_depth, float max_depth, float *vertex_out, float *normal_out,
                           mi_stream_t stream);

/* (ra, ta) o (rb, tb) per item: r = ra rb, t = ra tb + ta, (batch, 3, 3) and (batch, 3) float32.  Every product in float64,
 * every sum as (a + b) + c (+ ta_i) in float64, rounded once to float32: composing the identity returns the other pose's bits.
 * A tracked pose (mi_icp_refine's result onto the prediction) then needs no host arithmetic and stays capturable.  The outputs
 * may not alias the inputs.  batch < 1: MI_E_SHAPE.  One launch. */
MI_API int mi_pose_compose(const float *ra, const float *ta, const float *rb, const float *tb, int batch, float *r, float *t,
                           mi_stream_t stream);

/* ---- TSDF surface extraction (K20): the fused volume -> an indexed triangle mesh with normals, or a point cloud --------------------
 * The zero level set of a K19 volume by marching tetrahedra over the Kuhn split of every cell (no ambiguous faces: the mesh is
 * closed wherever the volume is observed), what KinectFusion-style systems call extraction (Open3D: extract_triangle_mesh,
 * extract_point_cloud).  The reference has no counterpart.  One pass over the volume, batched over volumes under the contract of
 * the K19 section: no allocation, no synchronisation, no memset, no atomics, one stream, capturable; every output element is
 * written; MI_E_* before any launch; a volume's result is the same bits alone or inside a batch, from run to run and under graph
 * replay.  Arithmetic is float32 with nothing fused.  The volume, its origin and voxel_size are K19's.
 *
 * Observed and inside.  A voxel is OBSERVED iff weight >= min_weight (min_weight > 0; 1 is K19's weight > 0 for integrated
 *   volumes).  An observed voxel is INSIDE iff !(tsdf > 0): the raycast's f <= 0, and NaN counts as inside.
 * Cells and corners.  Cell (i, j, k), 0 <= i <= nx-2 and likewise j, k, has corners m = 0..7; corner m is voxel
 *   (i + (m & 1), j + ((m >> 1) & 1), k + ((m >> 2) & 1)).
 * Tetrahedra.  A cell is six tetrahedra around the diagonal 0-7, in this order, the corners of each in this path order
 *   (t0, t1, t2, t3):  (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7).
 * Edges.  Every tetrahedron edge joins corners p < q with q = p | e; e = q - p in 1..7 is the edge's class (1 = x, 2 = y, 3 = xy,
 *   4 = z, 5 = xz, 6 = yz, 7 = xyz).  The edge is owned by the voxel at its lower end p: a voxel owns at most seven edges.
 * Vertices.  A vertex exists on an edge iff both end voxels are observed and exactly one of them is inside (the two ends only:
 *   neighbouring cells agree).  Its id is its rank in the order (owner's linear index (k ny + j) nx + i, then class ascending)
 *   within its volume.  With f_p, f_q the ends' tsdf, a = f_p / (f_p - f_q).  The position is in the WORLD frame (the volume's):
 *   on each axis the edge moves along, ((index_p + 0.5f) * voxel_size + origin) + a * voxel_size, on the others the centre of
 *   index_p itself; the record is (x, y, z, 1).
 * Normals.  At the grid coordinate g = ((float)index_p + a on the axes the edge moves along, (float)index_p on the others):
 *   G_j = F(g + e_j) - F(g - e_j), F K19's trilinear sample (valid only over eight corners of weight > 0), all six samples valid;
 *   len = sqrtf((G_0^2 + G_1^2) + G_2^2); the record is (G / len, 1), or zeros where a sample is invalid or len is not positive
 *   and finite.  The normal points to the positive (free-space) side; it is not flipped.
 * Triangles.  A tetrahedron emits triangles iff all four corners are observed; its case is the mask with bit s set iff t_s is
 *   inside.  One corner s on its own side (1 or 3 inside): one triangle on the edges (s,u1), (s,u2), (s,u3), u1 < u2 < u3 the
 *   other path positions.  Two inside, A < B, two outside, C < D (positions): (AC, AD, BD) then (AC, BD, BC).  Orientation: with
 *   every vertex at its edge's midpoint in the unit cell, a triangle whose (v1 - v0) x (v2 - v0) points from the inside corners'
 *   mean towards the outside corners' mean stays as it is; otherwise its last two vertices are swapped.  That is a fixed 6 x 16
 *   table (csrc/surface_math.h generates it from this rule at compile time).  Triangles are ordered by (cell linear index
 *   (k (ny-1) + j) (nx-1) + i, tetrahedron 0..5, triangle 0..1); each is three int32 vertex ids.
 *   A node whose tsdf is exactly 0 gives a = 0 or 1 on its edges: their vertices coincide and the triangles between them have
 *   zero area.  They are kept, so that the topology does not depend on it.
 *
 * Outputs, per volume: vertex_out (max_vertices, 4) float32; normal_out likewise, or NULL; triangle_out (max_triangles, 3) int32,
 *   or NULL with max_triangles = 0 (a point cloud: no triangle is formed); counts_out (2) int32 = the TRUE totals (vertices,
 *   triangles), even where they exceed the capacities.  Only vertices with id < max_vertices and triangles with ordinal <
 *   max_triangles are written, the triangles with the true ids: a caller compares counts with capacities to detect an incomplete
 *   mesh.  Rows from the count up to the capacity are written too: zeros for vertices and normals, (-1, -1, -1) for triangles.
 *   With both capacities 0 the call is a sizing pass that writes the counts only: every output may be NULL, and an output
 *   pointer that is given all the same (normal_out included) is checked for alignment and otherwise left alone. */

/* bytes of workspace for mi_tsdf_surface (0 for a shape it refuses): one byte per voxel and 16 bytes per x-row. */
MI_API size_t mi_tsdf_surface_workspace_bytes(int batch, int nz, int ny, int nx);

/* volume (batch, nz, ny, nx, 2) -> vertex_out, normal_out (batch, max_vertices, 4), triangle_out (batch, max_triangles, 3),
 * counts_out (batch, 2).  volume, vertex_out, normal_out and workspace 16-byte aligned, triangle_out and counts_out 4-byte
 * (MI_E_ALIGN).  NULL volume, counts_out or workspace, NULL vertex_out with max_vertices != 0, NULL triangle_out with
 * max_triangles != 0: MI_E_NULL.  K19's volume checks, 12 * nz * ny * nx >= 2^31 (ids must fit int32), batch * max_vertices or
 * batch * max_triangles >= 2^31: MI_E_SHAPE.  batch > 65535, min_weight or voxel_size <= 0 or not finite, an origin component
 * not finite, a capacity < 0: MI_E_PARAM.  workspace shorter than mi_tsdf_surface_workspace_bytes, of any content:
 * MI_E_CAPACITY.  normal_out is optional at any capacity.  Three launches (two for the sizing pass). */
MI_API int mi_tsdf_surface(const float *volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y, float origin_z,
                           float voxel_size, float min_weight, int max_vertices, int max_triangles, float *vertex_out,
                           float *normal_out, int32_t *triangle_out, int32_t *counts_out, void *workspace, size_t workspace_bytes,
                           mi_stream_t stream);

/* ---- TSDF intensity (K22): gray values in the fused model -> direct frame-to-model tracking, gray per mesh vertex -----------------
 * K19's volume holds (tsdf, weight) alone, so its raycast gives K18 a surfel map and nothing photometric: on a textured wall,
 * floor or table top model tracking freezes, as K18 does between two frames.  This section keeps a SECOND volume of gray
 * values beside K19's, fuses it from gray frames in the same pass as the depth, and gathers it at given points: at the
 * raycast's vertex map it yields a record map in mi_intensity_maps' layout, (I, 0, 0, f).  mi_photo_linearise /
 * mi_rgbd_refine read only I and f of FRAME 1's intensity record (the gradients are frame 2's, the live frame), so that map
 * is a legitimate `intensity1` and K21 is unchanged.  At the world vertices of mi_tsdf_surface it yields gray per vertex.
 * The reference has no counterpart.  Three entries, batched over volumes, under the contract of the K19 section: no
 * allocation, no synchronisation, no memset, no atomics, one stream, capturable; every output element is written; MI_E_*
 * before any launch; a volume's result is the same bits alone or inside a batch, and from run to run.  Per-voxel and
 * per-sample arithmetic is float32 with nothing fused.  K19's entries, kernels and bits are untouched.
 *
 * Intensity volume.  (batch, nz, ny, nx) records of two float32 (gray, gweight), 8 bytes, x fastest: K19's layout, alignment
 *   (16 bytes, MI_E_ALIGN), origin, voxel_size and shape checks.  An empty record is (0, 0).
 *
 * Integration, per voxel, for the frames in order (a frame whose `active` byte is 0 is left out): K19's update of (tsdf, weight),
 *   step for step, with its q, (px, py), d, Z and sdf = Z - q_2.  Where that update HAPPENED (no skip), and sdf <= truncation,
 *   and g = gray[py][px] (the depth sample's own pixel; uint8 converted to float32) is finite:
 *     gray <- (gray * gweight + g) / (gweight + 1);   gweight <- fminf(gweight + 1, max_weight)
 *   So only voxels inside the band |sdf| <= truncation around a seen surface ever hold a gray value.  The written `volume` has
 *   mi_tsdf_integrate's bits.  One pass over both volumes however many frames; frames given in one call and the same frames
 *   given one per call give the same bits in both volumes.
 *
 * Sampling, per point record (x, y, z, f) with f != 0 and x, y, z finite (any other point is invalid):
 *   with a pose (world to camera, the point is in the camera's frame): c = (x - t_0, y - t_1, z - t_2),
 *     X_w,j = (R_0j c_0 + R_1j c_1) + R_2j c_2: the raycast's operations, so for its vertex (xn s*, yn s*, s*) the grid coordinate
 *     below has the raycast's own bits.  Without a pose the point is X_w.
 *   g_a = (X_w,a - origin_a) / voxel_size - 0.5f per axis; invalid unless 0 <= g_a <= n_a - 1 on every axis (NaN fails).
 *   b_a = fminf(floorf(g_a), n_a - 2), a_a = g_a - b_a: the last layer of voxels is reached with a = 1.
 *   Over the corners m = 0..7 of cell b IN THAT ORDER (corner m is voxel b + (m & 1, (m >> 1) & 1, (m >> 2) & 1)), with
 *     w_m = (wx * wy) * wz, wx = a_x where m & 1 else 1.0f - a_x, and likewise wy, wz with bits 1 and 2:
 *     num and den start at 0 and, for every corner with gweight_m > 0, num <- num + w_m * gray_m, den <- den + w_m.
 *   Valid iff den > 0: I = num / den, the record (I, 0, 0, 1); else zeros.  This is the weight-normalised blend over the OBSERVED
 *   corners: a vertex at the rim of the observed band still gets the gray of what was seen. */

/* (0, 0) into every record of intensity_volume (batch, nz, ny, nx, 2).  One launch. */
MI_API int mi_tsdf_gray_reset(float *intensity_volume, int batch, int nz, int ny, int nx, mi_stream_t stream);

/* mi_tsdf_integrate with a gray frame beside every depth frame: gray (batch, frames, h, w), float32 (gray_is_u8 = 0) or uint8
 * (1), in the depth's camera.  mi_tsdf_integrate's checks; NULL intensity_volume or gray: MI_E_NULL; intensity_volume not
 * 16-byte aligned: MI_E_ALIGN.  One launch, a wave per x-row; a voxel's intensity record is read and written only if a frame
 * updates it. */
MI_API int mi_tsdf_integrate_gray(float *volume, float *intensity_volume, int batch, int nz, int ny, int nx, float origin_x,
                                  float origin_y, float origin_z, float voxel_size, float truncation, float max_weight,
                                  const void *depth, int depth_is_u16, const void *gray, int gray_is_u8, int frames, int h, int w,
                                  float fx, float fy, float cx, float cy, float z_scale, float min_depth, float max_depth,
                                  const float *r, const float *t, const uint8_t *active, mi_stream_t stream);

/* intensity_volume + points (batch, n, 4) float32 + an optional pose per volume, r (batch, 3, 3) and t (batch, 3), both given
 * or both NULL (one without the other: MI_E_NULL) -> intensity_out (batch, n, 4) float32.  The volume's checks (no truncation);
 * n < 1, batch * n >= 2^31: MI_E_SHAPE; intensity_volume, points and intensity_out 16-byte aligned (MI_E_ALIGN).  One launch, one
 * thread per point. */
MI_API int mi_tsdf_sample_gray(const float *intensity_volume, int batch, int nz, int ny, int nx, float origin_x, float origin_y,
                               float origin_z, float voxel_size, const float *points, int n, const float *r, const float *t,
                               float *intensity_out, mi_stream_t stream);

/* ---- absolute pose (K23): 3-D points + the pixels they are seen at -> the camera pose, batched P3P RANSAC ----------------------
 * K15 estimates a motion from 2-D to 2-D matches (unit translation), K17 from 3-D to 3-D matches (depth in both frames).
 * This section takes 3-D points on one side and pixels on the other: matches whose depth is missing in the second frame, a
 * colour frame against the points of a TSDF volume, a new frame against triangulated landmarks.  The host call users would
 * reach for is cv2.solvePnPRansac.  Four entries, batched over pairs, under the contract of the K15 / K17 sections: pure
 * functions of their arguments, no allocation, no synchronisation, no memset, one stream, no atomics, every sum in a fixed
 * order (the same inputs and seed give the same bits), capturable into a hipGraph; outputs and workspace may hold anything
 * on entry and every output element is written; MI_E_* before any launch.
 * Row i of pair b is pts3[b][i] <-> pts2[b][i]: pts3 (batch, n, 3) float32 points X in the model frame, pts2 (batch, n, 2)
 * float32 NORMALISED image points (u, v) = (x, y) as mi_normalise_keypoints writes them; `valid` / `mask` (batch, n) bytes
 * select rows (non-zero = use; valid may be NULL: every row).  Rows that are not selected are never read for their
 * coordinates.  The pose is X_c = R X + t, the camera looking along +z.  Thresholds are in normalised units (pixels / mean
 * focal length), as in K15.  1 <= n <= MI_PNP_MAX_N (a staged row is 20 bytes: 40 KB of rows and 4 KB of indices in LDS;
 * the second kernel of mi_pnp_ransac adds 4 KB of flags), batch <= 65535 (MI_E_PARAM beyond; < 1: MI_E_SHAPE).
 *
 * Divergences from cv2.solvePnPRansac, all deliberate:
 *   - a fixed number of hypotheses, no adaptive stop from `confidence`; the sampler is K15's stateless counter-based hash,
 *     not cv::RNG: results do not depend on call history;
 *   - the best hypothesis is the one of minimum truncated cost sum min(d^2, thr^2) (MSAC), not of maximum inlier count;
 *   - the minimal solver is stated below (OpenCV's default inside RANSAC is EPnP on 5 points, or P3P/AP3P on request);
 *   - refinement is refine_rounds rounds of a FIXED number of Gauss-Newton iterations on the inliers (local optimisation),
 *     where OpenCV runs Levenberg-Marquardt to a tolerance on the final inlier set;
 *   - no camera matrix and no distortion coefficients: the image points arrive normalised and undistorted.
 *
 * Sampling.  K15's draw(seed, b, h, s), unchanged (the counter is still 8 h + s), for the slots s = 0 .. 3, with the same
 *   without-replacement rule over the ranks of the valid rows: four distinct ranks.  Slots 0 .. 2 are the minimal sample,
 *   slot 3 picks among its solutions.
 * Solve (float32; only + - * / and sqrt, every loop of a fixed length; csrc/pnp_math.h).  With X_k, (u_k, v_k), k = 0, 1, 2:
 *   1. bearings f_k = (u, v, 1) / sqrt((u^2 + v^2) + 1); c12 = f_0 . f_1, c13 = f_0 . f_2, c23 = f_1 . f_2 (each
 *      (x x' + y y') + z z'); a12 = |X_0 - X_1|^2, a13 = |X_0 - X_2|^2, a23 = |X_1 - X_2|^2.  The depths l_k along the
 *      bearings satisfy l_i^2 + l_j^2 - 2 c_ij l_i l_j = a_ij, i.e. L^T M_ij L = a_ij for L = (l_1, l_2, l_3).
 *   2. D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 give L^T D1 L = L^T D2 L = 0.  det(D1 + g D2) is a cubic in g:
 *      c0 = det D1, c3 = det D2, c1 = sum_ij cof(D1)_ij D2_ij, c2 = sum_ij cof(D2)_ij D1_ij; divided by c3 it is
 *      g^3 + b g^2 + c g + d.
 *   3. One real root g by 24 Newton steps g <- g - p(g) / p'(g) (a step with p'(g) = 0 is skipped) from a start beyond the
 *      outer stationary point: with v = sqrt(b^2 - 3 c) real, t1 = (-b - v) / 3; if p(t1) > 0 the start is
 *      t1 - sqrt(-p(t1) / (3 t1 + b)), else with t2 = (-b + v) / 3 it is t2 + sqrt(-p(t2) / (3 t2 + b)); without stationary
 *      points the start is the inflection -b / 3.  From there Newton's iteration is monotone.
 *   4. D0 = D1 + g D2 is singular.  Its eigen-decomposition by K17's cyclic Jacobi (6 sweeps, pairs (0,1) (0,2) (1,2)); the
 *      eigenvalue of smallest magnitude (the first among equals) is dropped, the other two, sigma_p > 0 > sigma_q with unit
 *      eigenvectors e_p, e_q (no solution when their product is not negative), factor the form:
 *      L^T D0 L = (n+ . L)(n- . L) with n+- = sqrt(sigma_p) e_p +- sqrt(-sigma_q) e_q.
 *   5. Candidate c = 0 .. 3: the plane n = n+ for c < 2 and n- for c >= 2 gives l_1 = w0 l_2 + w1 l_3 with w0 = -n_1 / n_0,
 *      w1 = -n_2 / n_0; substituted into a13 L^T M12 L - a12 L^T M13 L = 0 and divided by l_2^2 this is qa tau^2 + qb tau
 *      + qc = 0 for tau = l_3 / l_2, with
 *          qa = ((a13 - a12) w1^2 + 2 a12 c13 w1) - a12
 *          qb = (2 a12 c13 w0 - 2 a13 c12 w1) - 2 w0 w1 (a12 - a13)
 *          qc = ((a13 - a12) w0^2 - 2 a13 c12 w0) + a13;
 *      no candidate when qb^2 - 4 qa qc < 0; q = -(qb + sign(qb) sqrt(qb^2 - 4 qa qc)) / 2 (sign(0) = +1); tau = q / qa for
 *      even c and qc / q for odd c; no candidate unless tau > 0.  l_2 = sqrt(a23 / (tau (tau - 2 c23) + 1)), l_3 = tau l_2,
 *      l_1 = w0 l_2 + w1 l_3; no candidate unless all three are positive and finite.
 *   6. Polish: 2 Gauss-Newton steps L <- L - J^-1 r on the three equations of step 1 (J^-1 by the adjugate; a step with
 *      det J = 0 is skipped); afterwards the depths must again be positive and finite.
 *   7. (R, t) of the candidate: K17's minimal solve (Horn, "metric RGB-D pose": Solve) with a_k = X_k, b_k = l_k f_k,
 *      including its degeneracy test of both triangles and its finiteness test.
 *   8. The candidate with the smallest d^2 (Score, below) on the slot-3 row wins; the first candidate that exists is taken
 *      whatever its d^2, a later one replaces it only with a strictly smaller d^2.
 * Refusals.  Fewer than 4 valid rows; the three model points, or the three bearings, degenerate under K17's test
 *   (|e1 x e2|^2 <= 1e-6 |e1|^2 |e2|^2); no candidate; a non-finite result or cost: cost = +inf, count = 0, zeros in rt_h.
 * Score.  For every valid row (x, y, z) = (R X) + t, each component ((R_j0 X_0 + R_j1 X_1) + R_j2 X_2) + t_j;
 *   d^2 = (x / z - u)^2 + (y / z - v)^2; a row with z <= 0 or a non-finite d^2 has d^2 = +inf (beyond any threshold).
 *   inlier: d^2 <= thr^2; count = number of inliers, cost = sum over the valid rows in index order of min(d^2, thr^2), float32.
 * Refit.  Gauss-Newton on the reprojection error under K18's left perturbation (omega, tau): R <- Exp(omega) R,
 *   t <- Exp(omega) t + tau.  A row with z > 0 gives, with xn = x / z, yn = y / z, iz = 1 / z (float32),
 *       J_u = [-(xn yn), 1 + xn^2, -yn, iz, 0, -(xn iz)]   r_u = xn - u
 *       J_v = [-(1 + yn^2), xn yn, xn, 0, iz, -(yn iz)]    r_v = yn - v
 *   and rows with z <= 0 are skipped.  The 29 sums have K18's layout (21 of A = J^T J's upper triangle, 6 of b = J^T r, r^2,
 *   and the number of ROWS used), each row adding its u line, then its v line; lanes stride over the rows and
 *   wave_sum_dpp folds the 64 partial sums.  K18's solve of A x = -b (float64 LDL^T, pivot ratio 1e-6) and pose update
 *   (float64 pose, rounded to float32 for the next linearisation).  3 iterations, then one more linearisation at the
 *   result, whose A is `info`.  Any of these 4 systems unusable -- fewer than 4 rows, a pivot ratio at or below 1e-6, a
 *   non-finite value -- stops the refit: ok = 0, (r, t) = (r0, t0), info = 0. */
#define MI_PNP_MAX_N 2048

/* H = num_hypotheses hypotheses per pair, generated and scored: rt_h (batch, H, 12) = R row-major, then t; cost (batch, H)
 * float32, count (batch, H) int32.  H < 1: MI_E_SHAPE; H > MI_POSE_MAX_HYPOTHESES, threshold <= 0 or not finite:
 * MI_E_PARAM.  One launch: ceil(H / 64) x batch waves, a lane per hypothesis. */
MI_API int mi_pnp_hypotheses(const float *pts3, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                             float threshold, uint32_t seed, float *rt_h, float *cost, int32_t *count, mi_stream_t stream);

/* The refit of the section above over the rows with mask != 0 (mask is required) from the pose r0 (batch, 3, 3), t0
 * (batch, 3): r (batch, 3, 3), t (batch, 3), info (batch, 6, 6) float32 (the full symmetric A in (omega, tau) order),
 * ok (batch) bytes.  One wave per pair. */
MI_API int mi_pnp_refit(const float *pts3, const float *pts2, const uint8_t *mask, const float *r0, const float *t0, int batch,
                        int n, float *r, float *t, float *info, uint8_t *ok, mi_stream_t stream);

/* The whole estimator, K17's point for point: mi_pnp_hypotheses into the workspace, then per pair the hypothesis of minimum
 * cost (the lowest h among equals; h = 0 when every cost is +inf) and refine_rounds rounds r = 0 .. R-1 of local
 * optimisation: take the inliers of the best pose so far at k_r * threshold, k_r = 1 + (R - 1 - r) / 2, refit from that
 * pose as mi_pnp_refit, score at `threshold`; the refit replaces the best pose only when its cost is strictly lower.  Inside
 * this step a cost is held as (number of valid rows beyond the threshold, float32 sum of the inliers' d^2, summed
 * lanes-strided) and compared as k thr^2 + s in float64, the hypothesis' own cost re-formed that way first (K17 says why).
 * A round whose refit is not ok changes nothing.
 * r (batch, 3, 3), t (batch, 3); inlier (batch, n) bytes: d^2 <= threshold^2 under (r, t), 0 for rows that are not valid;
 * best_h (batch) the selected hypothesis; count (batch) = number of inlier bytes set; rmse (batch) float32 = sqrt of the
 * mean d^2 over the inliers (normalised units); info (batch, 6, 6) float32 = A of the Refit linearisation at (r, t) over
 * the inliers; ok (batch) bytes = 1 when a usable hypothesis exists and count >= 4.  Where ok = 0: r = identity, t = 0, no
 * inliers, count = 0, rmse = 0, info = 0.  With refine_rounds = 0 and ok = 1, r / t / count are exactly rt_h[best_h] /
 * count[best_h] of mi_pnp_hypotheses.
 * 0 <= refine_rounds <= MI_POSE_MAX_REFINE_ROUNDS (MI_E_PARAM).  workspace: mi_pnp_ransac_workspace_bytes(batch, n, H) bytes
 * (0 for an unsupported request), 16-byte aligned (MI_E_ALIGN), any content; shorter: MI_E_CAPACITY.  Two launches. */
MI_API size_t mi_pnp_ransac_workspace_bytes(int batch, int n, int num_hypotheses);
MI_API int mi_pnp_ransac(const float *pts3, const float *pts2, const uint8_t *valid, int batch, int n, int num_hypotheses,
                         float threshold, int refine_rounds, uint32_t seed, float *r, float *t, uint8_t *inlier,
                         int32_t *best_h, int32_t *count, float *rmse, float *info, uint8_t *ok, void *workspace,
                         size_t workspace_bytes, mi_stream_t stream);

/* ---- planar two-view pose (K24): 2-D to 2-D matches on a plane or under a pure rotation -> homography, pose, model choice ------
 * K15 solves for E linearly from 8 correspondences.  That system is degenerate when the matched points lie on a plane and
 * when the camera only rotates; with pixel noise its rank test still passes and K15 returns a confident, wrong pose.  In
 * both cases the two views are related by a homography x2 ~ H x1, H = R + T N^T for the plane N . X1 = 1 (T in units of the
 * plane's distance to camera 1; T = 0 for a pure rotation).  The host calls users would reach for are cv2.findHomography
 * (RANSAC) and cv2.decomposeHomographyMat; the choice between the two models is ORB-SLAM's initialiser's.  Six entries,
 * batched over pairs, under the contract of the K15 section: pure functions of their arguments, no allocation, no
 * synchronisation, no memset, one stream, no atomics, every sum in a fixed order (the same inputs and seed give the same
 * bits), capturable into a hipGraph; outputs and workspace may hold anything on entry and every output element is written;
 * MI_E_* before any launch.  Points, `valid` / `mask`, n and batch are K15's: (batch, n, 2) float32 NORMALISED (x, y),
 * 1 <= n <= MI_POSE_MAX_N, batch <= 65535 (MI_E_PARAM beyond; < 1: MI_E_SHAPE); thresholds are in normalised units.
 *
 * Divergences from OpenCV, all deliberate: K15's (a fixed number of hypotheses, MSAC, the counter-based sampler, refit
 * rounds in place of Levenberg-Marquardt), and: the error is the SYMMETRIC transfer error (findHomography scores the
 * forward error alone); the decomposition is Ma, Soatto, Kosecka and Sastry's ("An Invitation to 3-D Vision", 5.3.3), not
 * Malis and Vargas'; its four candidates are returned sorted by a depth test instead of unsorted.
 *
 * Model.  18 floats: H row-major, then G = adj(H) (G H = det(H) I), negated when det H < 0: a positive multiple of H^-1.
 *   Both are scaled to unit Frobenius norm, H first, G computed from the scaled H.  Only H is written out.
 * Sampling.  K15's draw(seed, b, h, s), unchanged (the counter is still 8 h + s), for the slots s = 0 .. 3: four distinct
 *   ranks, K23's.
 * Solve.  tri(a, b, c) = (b_x - a_x)(c_y - a_y) - (b_y - a_y)(c_x - a_x).
 *   1. Refusal: a triple (a, b, c) of points is COLLINEAR under K17's rule, with e1 = b - a, e2 = c - a, when
 *      (e1 x e2)^2 <= 1e-6 |e1|^2 |e2|^2.  The sample is refused when any of the triples (0,1,2) (0,1,3) (0,2,3) (1,2,3) is
 *      collinear in either image.
 *   2. Per image Hartley's rule over the four points: centroid c = (((p0 + p1) + p2) + p3) / 4, scale s = sqrt(2) /
 *      sqrt(sum |p - c|^2 / 4) (refused when the sum is 0), p^ = (p - c) s, i.e. T = [s 0 -s c_x; 0 s -s c_y; 0 0 1].
 *   3. Per image the projective basis of the normalised points: [p0 p1 p2] l = p3 by cofactors, l0 = tri(p3, p1, p2),
 *      l1 = tri(p0, p3, p2), l2 = tri(p0, p1, p3) (the common denominator tri(p0, p1, p2) scales the result and is left
 *      out); B = [l0 p0, l1 p1, l2 p2] with columns l_k (x_k, y_k, 1).
 *   4. H^ = B2 adj(B1), row i of adj(B1) being (column i+1) x (column i+2) of B1, indices mod 3; H = T2^-1 H^ T1.
 *   5. Sign and completion: H is negated when (H X1)_2 < 0 at sample point 0, X1 = (x1, y1, 1); scaled; G as above.
 *      Refused when det H = 0, when anything is not finite, or when (H X1)_2 > 0 fails at any of the four sample points
 *      (the sample straddles the line H sends to infinity).
 * Score.  For every valid row, with (hx, hy, hw) = H X1 and (gx, gy, gw) = G X2, each component (M_j0 x + M_j1 y) + M_j2:
 *   d^2 = (((x2 - hx / hw)^2 + (y2 - hy / hw)^2) + (x1 - gx / gw)^2) + (y1 - gy / gw)^2, the symmetric transfer error;
 *   d^2 = +inf when hw <= 0 or gw <= 0.  inlier: d^2 <= thr^2; count = number of inliers, cost = sum over the valid rows in
 *   index order of min(d^2, thr^2), float32.
 * Degenerate: fewer than 4 valid rows or a refused sample give cost = +inf, count = 0 and a zero matrix. */

/* H = num_hypotheses hypotheses per pair, generated and scored: h_h (batch, H, 3, 3), cost (batch, H) float32, count
 * (batch, H) int32.  H < 1: MI_E_SHAPE; H > MI_POSE_MAX_HYPOTHESES, threshold <= 0 or not finite: MI_E_PARAM.  One launch:
 * ceil(H / 64) x batch waves, a lane per hypothesis, the sample solved in registers. */
MI_API int mi_homography_hypotheses(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                    int num_hypotheses, float threshold, uint32_t seed, float *h_h, float *cost,
                                    int32_t *count, mi_stream_t stream);

/* h (batch, 3, 3) from the rows with mask != 0 (mask is required): Hartley's rule over those rows (centroids from
 * lanes-strided sums, / m for m rows; scale sqrt(2) / sqrt(sum |p - c|^2 / m)); per row, with u = (x1, y1, 1) of the
 * normalised points, the two DLT lines [u, 0, -x2 u] and [0, u, -y2 u]; the 9x9 normal equations M = A^T A, which consist
 * of the blocks S0 = sum u u^T (twice on the diagonal), -Sx = -sum x2 u u^T, -Sy = -sum y2 u u^T and Sr = sum (x2^2 + y2^2)
 * u u^T and are formed from those 24 sums; the eigenvector of M's smallest eigenvalue by K15's inverse iteration
 * (mi_essential_refit: 6 steps on the Cholesky factor of M + 2e-6 trace(M) I from the all-ones vector; one code) = H^
 * row-major; H = T2^-1 H^ T1; negated when (H X1)_2 < 0 at the centroid of the first image's rows; completed as in Solve 5.
 * ok (batch) bytes: 0 and a zero h for fewer than 4 rows, a point set without spread, det H = 0 or a non-finite result,
 * else 1.  One wave per pair. */
MI_API int mi_homography_refit(const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n, float *h,
                               uint8_t *ok, mi_stream_t stream);

/* The whole estimator, K17's point for point: mi_homography_hypotheses into the workspace, then per pair the hypothesis of
 * minimum cost (the lowest h among equals; h = 0 when every cost is +inf) and refine_rounds rounds r = 0 .. R-1 of local
 * optimisation: take the inliers of the best model so far at k_r * threshold, k_r = 1 + (R - 1 - r) / 2, refit as
 * mi_homography_refit, score at `threshold`; the refit replaces the best model only when its cost is strictly lower, costs
 * held as (rows beyond the threshold, float32 sum of the inliers' d^2, summed lanes-strided) and compared as k thr^2 + s in
 * float64, the hypothesis' own cost re-formed that way first (K17 says why).  A round whose refit is not ok changes nothing.
 * h (batch, 3, 3); inlier (batch, n) bytes: d^2 <= threshold^2 under the model, 0 for rows that are not valid; best_h
 * (batch) the selected hypothesis; count (batch) = number of inlier bytes set; cost (batch) float32 = the final model's MSAC
 * cost over the valid rows, k thr^2 + s of the paragraph above rounded to float32.  A pair without a usable hypothesis
 * gives a zero h, no inliers, count 0 and cost = +inf.  With refine_rounds = 0, h / count / inlier are exactly those of
 * hypothesis best_h of mi_homography_hypotheses.
 * 0 <= refine_rounds <= MI_POSE_MAX_REFINE_ROUNDS (MI_E_PARAM).  workspace: mi_homography_ransac_workspace_bytes(batch, n,
 * H) bytes (0 for an unsupported request), 16-byte aligned (MI_E_ALIGN), any content; shorter: MI_E_CAPACITY.  Two launches. */
MI_API size_t mi_homography_ransac_workspace_bytes(int batch, int n, int num_hypotheses);
MI_API int mi_homography_ransac(const float *pts1, const float *pts2, const uint8_t *valid, int batch, int n,
                                int num_hypotheses, float threshold, int refine_rounds, uint32_t seed, float *h,
                                uint8_t *inlier, int32_t *best_h, int32_t *count, float *cost, void *workspace,
                                size_t workspace_bytes, mi_stream_t stream);

/* cv2.decomposeHomographyMat for normalised points, with the candidates tested and sorted: from h (batch, 3, 3; any scale
 * and sign) and the rows with mask != 0 (NULL: every row), four candidates per pair: r (batch, 4, 3, 3), t (batch, 4, 3),
 * normal (batch, 4, 3), count (batch, 4) int32, with x2 ~ (r + t normal^T) x1.  t is T in units of the plane's distance to
 * camera 1 (NOT of unit length); normal is of unit length and points from camera 1 towards the plane.
 *   1. H is scaled to unit Frobenius norm and negated when X2^T H X1 > 0 holds on fewer than half of the masked rows.
 *   2. The eigen-decomposition of H^T H by K17's cyclic Jacobi (6 sweeps, pairs (0,1) (0,2) (1,2)); eigenvalues sorted
 *      w1 >= w2 >= w3 (the lower index first among equals) with unit eigenvectors v1, v2, v3, each negated when its
 *      component of largest magnitude (the first among equals) is negative.  H is divided by sqrt(w2), the w by w2.
 *   3. u+- = (sqrt(1 - w3) v1 +- sqrt(w1 - 1) v3) / sqrt(w1 - w3) (a negative radicand counts as 0); N = v2 x u;
 *      U = [v2, u, N], W = [H v2, H u, H v2 x H u] (columns); R = W U^T followed by one step R (3 I - R^T R) / 2 towards
 *      the nearest rotation, as in mi_recover_pose; T = (H - R) N.  Candidates: 0 (R+, T+, N+), 1 (R-, T-, N-),
 *      2 (R+, -T+, -N+), 3 (R-, -T-, -N-).
 *   4. A masked row PASSES under a candidate when N . X1 > 0 and ((R X1)_2 / (N . X1)) + T_2 > 0: its depths in the two
 *      cameras, in units of the plane's distance, are positive.
 *   5. The candidates are written sorted by passing count, descending; equal counts by the larger trace of R, then by
 *      candidate index.  count holds the passing counts; pose_mask (batch, n) the rows that pass under slot 0.  Two
 *      candidates generally pass every row of a plane in front of both cameras; which of them is the scene's cannot be
 *      told from one pair.
 *   6. rotation_only (batch) bytes: 1 when w1 - w3 <= 5.9e-6 (HG_ROTATION_TOL, csrc/homography_math.h, where its
 *      measurement is written down).  Slot 0 is then (H (H^T H)^(-1/2) through the eigen-decomposition, followed by the
 *      step of 3; t = 0; normal = 0) with every masked row passing, and slots 1 .. 3 are copies of it.
 *   7. ok (batch) bytes: 0 when slot 0 passes fewer than 4 rows or h is zero or not finite; then every r is the identity
 *      and t, normal, count, pose_mask and rotation_only are zero.
 * One wave per pair. */
MI_API int mi_homography_pose(const float *h, const float *pts1, const float *pts2, const uint8_t *mask, int batch, int n,
                              float *r, float *t, float *normal, int32_t *count, uint8_t *pose_mask, uint8_t *rotation_only,
                              uint8_t *ok, mi_stream_t stream);

/* The choice between K15's essential matrix e and the homography h (both (batch, 3, 3), any scale) of each pair:
 * score_M = sum over the valid rows of max(0, 1 - d^2_M / thr_M^2), float32, lanes striding over the rows (lane l sums rows
 * l, l + 64, .. in order; wave_sum_dpp folds the 64 partial sums), with d^2_E K15's Sampson distance under e and d^2_H the
 * transfer error of the section above under (h, G = adj(h) sign-matched and scaled to unit Frobenius norm; h is taken as
 * it comes).  A row with d^2 = +inf adds 0; a zero or singular model scores 0.  score_e, score_h (batch) float32; choice
 * (batch) bytes: 1 (homography) when score_h > cut * (score_e + score_h), else 0 (also when both scores are 0).
 * ORB-SLAM's published cut is 0.45.  thr_e, thr_h <= 0 or not finite, cut outside [0, 1]: MI_E_PARAM.  One wave per pair. */
MI_API int mi_two_view_select(const float *e, const float *h, const float *pts1, const float *pts2, const uint8_t *valid,
                              int batch, int n, float thr_e, float thr_h, float cut, float *score_e, float *score_h,
                              uint8_t *choice, mi_stream_t stream);

/* ---- windowed bundle adjustment (K25): the poses of a window of frames and their shared landmarks, refined jointly -------------
 * Every pose of the sections above comes from two frames.  This section couples them: Levenberg-Marquardt on the
 * reprojection error of a window, the landmarks eliminated (Schur complement), `batch` independent windows per call, one
 * workgroup each.  The host calls users would reach for are g2o, Ceres or cv2.detail.BundleAdjusterReproj.  Four entries
 * under the contract of the K15 / K23 sections: pure functions of their arguments, no allocation, no synchronisation, no
 * memset, one stream, no atomics, every sum in a fixed order (the same inputs give the same bits, alone or inside a batch),
 * capturable into a hipGraph; outputs and workspace may hold anything on entry, every output element is written and outputs
 * alias nothing; MI_E_* before any launch.
 *
 * State.  F frames with poses r (batch, F, 3, 3), t (batch, F, 3), X_c = R X + t (K23's convention), and L landmarks points
 *   (batch, L, 3) in the model frame, all float32.  Observations: obs (batch, F, L, 2) float32 NORMALISED (u, v) as
 *   mi_normalise_keypoints writes them, vis (batch, F, L) bytes, non-zero = seen; an entry that is not seen is never read for
 *   its coordinates.  2 <= F <= MI_BA_MAX_FRAMES, 1 <= L <= MI_BA_MAX_LANDMARKS (below: MI_E_SHAPE, as batch < 1; above:
 *   MI_E_PARAM, as batch > 65535).  Frames 0 .. num_fixed - 1 are held (the gauge: 1 for metric input, 2 to pin a monocular
 *   scale, F for structure only); num_fixed outside 1 .. F: MI_E_PARAM.  huber < 0 or not finite: MI_E_PARAM.
 * Active.  A landmark is ACTIVE when at least 2 of its F vis bytes are set -- a function of vis alone.  An inactive landmark
 *   adds nothing anywhere and is returned unchanged.  "Observation" below means a seen entry of an active landmark.
 * Threads.  256 per window.  Thread tid owns the landmarks l = tid, tid + 256, ...  A sum "over the landmarks" is: each
 *   thread's float32 partial sum over its landmarks in that order, wave_sum_dpp over the 64 lanes of each wave, then the four
 *   waves' sums added in wave order in float64 starting from 0.
 * Residual (float32).  (x, y, z), d^2 = e2 of K23's Score; an observation with z <= 0 or a non-finite e2 has e2 = +inf.
 *   e = sqrt(e2).  With huber > 0 and e > huber: rho = (2 huber) e - huber huber and w = huber / e; otherwise rho = e2, w = 1.
 *   rho = +inf where e2 = +inf.
 * Cost.  Each thread adds rho over its landmarks, and for one landmark over the frames in index order; summed over the
 *   landmarks (above) it is a float64, returned rounded to float32.  Nothing active: 0.
 * Lines (float32).  An observation with e2 = +inf adds nothing below.  Otherwise with K23's xn, yn, iz: J_u, J_v, r_u, r_v
 *   of K23's Refit, and the point lines X_u[j] = J_u[3] R_0j + J_u[5] R_2j, X_v[j] = J_v[4] R_1j + J_v[5] R_2j (the rows of
 *   [[iz, 0, -xn iz], [0, iz, -yn iz]] R).  Per landmark, over its frames in index order, with V kept as (00 01 02 11 12 22):
 *       V_ij += (w X_u[i]) X_u[j], then V_ij += (w X_v[i]) X_v[j];  h_i += (w X_u[i]) r_u, then h_i += (w X_v[i]) r_v.
 *   Fixed frames add here too.  W_fl (6 x 3) = [(w J_u[i]) X_u[c] + (w J_v[i]) X_v[c]].
 * Inverse.  m = V with the diagonal V_ii + lambda V_ii (lambda rounded to float32); cofactors c as in K23's step 2
 *   (pnp_cof), det = (m00 c00 + m01 c01) + m02 c02, Vi = c / det.  Pivots p0 = m00, p1 = c22 / m00, p2 = det / c22.  The
 *   landmark is FROZEN for this step -- Vi = 0: it acts as a fixed point -- unless max(m00, m11, m22) > 0, min(p0, p1, p2) >
 *   1e-6 max(m00, m11, m22) and every Vi element is finite.
 * Reduced system, n = 6 (F - num_fixed) unknowns, free frame f at offset 6 (f - num_fixed).  For every free f, over the
 *   landmarks seen in f: Y = W_fl Vi with Y_ic = (W_i0 Vi_0c + W_i1 Vi_1c) + W_i2 Vi_2c;
 *       U_ij += (w J_u[i]) J_u[j], then += (w J_v[i]) J_v[j] (i <= j);  g_i += (w J_u[i]) r_u, then += (w J_v[i]) r_v;
 *       Q_ij += (Y_i0 W_j0 + Y_i1 W_j1) + Y_i2 W_j2 (i <= j);  q_i += (Y_i0 h_0 + Y_i1 h_1) + Y_i2 h_2.
 *   The 54 sums over the landmarks are float64: S_ff = (U + lambda diag U) - Q, b_f = g - q.  For every pair f < f' of free
 *   frames, over the landmarks seen in both: Q_ij += (Y_i0 W'_j0 + Y_i1 W'_j1) + Y_i2 W'_j2 with Y of f and W' of f';
 *   S_ff' = -Q.
 * Solve.  S dp = -b in float64 by LDL^T without pivoting on the packed upper triangle: for column j = 0 .. n - 1 the pivot
 *   d_j = S_jj (after the updates of the earlier columns), l_ij = S_ji / d_j, S_rc -= (l_rj l_cj) d_j for j < r <= c; then
 *   y = -b, y_k -= l_ki y_i for i ascending; x_k = y_k / d_k, x_k -= l_ik x_i for i descending.  K18's rule for n unknowns:
 *   unusable when max diag S <= 0, a pivot is not above 1e-6 max diag S (the diagonal before elimination), or an x is not
 *   finite.  n = 0 is usable.
 * Step.  Poses: K18's update of the float64 pose with dp_f, rounded to float32 for every line.  Points (float32, dp
 *   rounded to float32): s = h; over the FREE frames seen, in index order, su = J_u . dp_f, sv = J_v . dp_f (each
 *   ((((a0 + a1) + a2) + a3) + a4) + a5), s_a += (w X_u[a]) su, then s_a += (w X_v[a]) sv;
 *   X_a <- X_a + -((Vi_a0 s_0 + Vi_a1 s_1) + Vi_a2 s_2).
 * Loop.  lambda = 1e-4 (float64).  `iterations` times: linearise at the state with lambda, solve, step to a candidate,
 *   evaluate its cost; when the system was usable and the candidate's cost is finite and strictly lower (float64 sums
 *   compared), the candidate becomes the state and lambda <- max(lambda / 10, 1e-9); otherwise lambda <- min(10 lambda, 1e6).
 *   Never stops early.  Refusal: the initial cost is not finite, or no landmark is active. */
#define MI_BA_MAX_FRAMES 16
#define MI_BA_MAX_LANDMARKS 2048
#define MI_BA_MAX_ITERATIONS 32

/* Cost alone, the outlier test between rounds: e2 (batch, F, L) float32, the observation's e2 (+inf behind the camera) and
 * 0 where the entry is not seen or the landmark inactive; cost (batch) float32; active (batch, L) bytes.  One launch. */
MI_API int mi_ba_cost(const float *r, const float *t, const float *points, const float *obs, const uint8_t *vis, int batch,
                      int frames, int landmarks, float huber, float *e2, float *cost, uint8_t *active, mi_stream_t stream);

/* Workspace of mi_ba_linearise and mi_ba_refine: 13 floats per landmark (Vi, h, the active flag, the candidate point), L
 * rounded up to a multiple of 4; 0 for an unsupported shape.  16-byte aligned (MI_E_ALIGN), any content; shorter:
 * MI_E_CAPACITY.  The alignment is reserved: with it each of a window's 13 arrays starts on a 16-byte boundary, which
 * four-wide accesses would need; the kernels as built read and write the workspace one float at a time. */
MI_API size_t mi_ba_workspace_bytes(int batch, int frames, int landmarks);

/* One undamped (lambda = 0) linearisation at the given state: s (batch, 6F, 6F) float32, the full symmetric reduced system
 * -- the marginal information of the window's poses -- with zero rows and columns for the fixed frames; b (batch, 6F)
 * float32, zero for the fixed frames; cost (batch).  An observation with e2 = +inf is skipped (and cost = +inf).  One launch. */
MI_API int mi_ba_linearise(const float *r, const float *t, const float *points, const float *obs, const uint8_t *vis, int batch,
                           int frames, int landmarks, int num_fixed, float huber, float *s, float *b, float *cost,
                           void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* The whole loop in one launch.  1 <= iterations <= MI_BA_MAX_ITERATIONS (MI_E_PARAM).  r (batch, F, 3, 3), t (batch, F, 3),
 * points (batch, L, 3): the final state (fixed frames and inactive landmarks are their inputs' bits); point_ok (batch, L)
 * bytes: 1 for an active landmark of a window that was not refused; cost0, cost (batch) float32: the cost at the input and
 * at the result; accepted (batch) int32: the number of accepted steps; info (batch, 6F, 6F): s of mi_ba_linearise at the
 * result, bit for bit; ok (batch) bytes.  A refused window: ok = 0, the outputs equal the inputs, point_ok = 0, accepted = 0,
 * info = 0, cost0 = cost = +inf (0 when no landmark is active). */
MI_API int mi_ba_refine(const float *r0, const float *t0, const float *points0, const float *obs, const uint8_t *vis, int batch,
                        int frames, int landmarks, int num_fixed, int iterations, float huber, float *r, float *t, float *points,
                        uint8_t *point_ok, float *cost0, float *cost, int32_t *accepted, float *info, uint8_t *ok,
                        void *workspace, size_t workspace_bytes, mi_stream_t stream);

/* ---- loop-closure retrieval (K26): which of the keyframes already seen is this frame? ------------------------------------------
 * Every section above is handed the two frames, or the window, that belong together.  This one finds them: a brute-force,
 * exact vote of a query frame's packed descriptors against every keyframe of a database, the first step of loop closure and
 * of relocalisation; a host would use a bag-of-words index (DBoW2) and cv2.BFMatcher.knnMatch with Lowe's ratio test.  Two
 * entries under the contract of the K15 / K23 / K25 sections: pure functions of their arguments, no allocation, no
 * synchronisation, no memset, no atomics, one stream, exactly one thread writes each output element, capturable into a
 * hipGraph; outputs may hold anything on entry, every element is written and outputs alias nothing; MI_E_* before any launch.
 * All arithmetic is on integers (one float32 multiply and compare in the vote), so the results do not depend on any order.
 *
 * Descriptors.  The packed hard bits of mi_sparse_bad / mi_sparse_bad_oriented: num_bits in {256, 512} (every other value:
 *   MI_E_PARAM), W = num_bits / 32 words each.  hamming(a, b) = popcount(a xor b).  ABSENT = num_bits + 1.
 * One query frame q against one keyframe f.  Query descriptors 0 .. kq - 1 with validity bytes q_valid (q, kq), database
 *   descriptors 0 .. kd - 1 with db_valid (n, kd); non-zero = valid, a NULL mask = all valid.  1 <= kq, kd <=
 *   MI_PLACE_MAX_DESCRIPTORS.  For a valid query descriptor i: the key of column j is hamming << 16 | j over the VALID j;
 *   key1 is the smallest key -- the nearest descriptor, the lowest index on a tie --, key2 the smallest among the other
 *   columns.  d1 = key1 >> 16, j1 = key1 & 0xffff (ABSENT and -1 with no valid column); d2 = key2 >> 16 (ABSENT with fewer
 *   than two valid columns).  i VOTES for f iff d1 <= max_distance and (float)d1 < ratio * (float)d2: one float32 multiply,
 *   one compare.  An invalid query row never votes and reports j1 = -1, d1 = ABSENT.  votes[q, f] = the number of voting rows.
 *   0 <= max_distance <= num_bits and 0 < ratio <= 1 (MI_E_PARAM otherwise, NaN included).
 * Extents.  n, kd, q, kq, slots < 1: MI_E_SHAPE; n > MI_PLACE_MAX_KEYFRAMES, kd or kq > MI_PLACE_MAX_DESCRIPTORS, q > 65535:
 *   MI_E_PARAM.  db_bits 16-byte aligned, the 32-bit arrays 4-byte aligned (MI_E_ALIGN).
 *
 * mi_place_votes.  db_bits (n, kd, W), q_bits (q, kq, W) uint32.  frame_index NULL: slots must equal n (MI_E_SHAPE) and slot s
 *   is keyframe s.  Otherwise frame_index (q, slots) int32 and slot s of query q scores keyframe frame_index[q, s]; a slot of
 *   -1 (any negative value) gives votes 0, nn_index -1, nn_distance ABSENT, nn_vote 0; an index >= n is the caller's error and
 *   is not detected.  votes (q, slots) int32.  nn_index, nn_distance (q, slots, kq) int32 and nn_vote (q, slots, kq) bytes: j1,
 *   d1 and the vote of every query row -- all three or none (a mixture: MI_E_NULL).  One launch; no distance matrix exists in
 *   memory and a keyframe's descriptors are read once per (query, slot). */
#define MI_PLACE_MAX_DESCRIPTORS 1024
#define MI_PLACE_MAX_KEYFRAMES 65536
#define MI_PLACE_MAX_CANDIDATES 64
MI_API int mi_place_votes(const uint32_t *db_bits, const uint8_t *db_valid, int n, int kd, const uint32_t *q_bits,
                          const uint8_t *q_valid, int q, int kq, const int32_t *frame_index, int slots, int num_bits,
                          int max_distance, float ratio, int32_t *votes, int32_t *nn_index, int32_t *nn_distance,
                          uint8_t *nn_vote, mi_stream_t stream);

/* Selection, per query.  votes (q, n) int32.  Keyframe f is ELIGIBLE when votes[q, f] >= min_votes and f lies outside
 * [excl_lo[q], excl_hi[q]) -- the temporal neighbours of the query; excl_lo, excl_hi (q) int32, both NULL (nothing is
 * excluded) or both given (one of them: MI_E_NULL).  The eligible keyframes ordered by (votes descending, index ascending):
 * the first num_candidates go to cand_index (q, num_candidates) and cand_votes (q, num_candidates) int32; empty places hold -1
 * and 0.  1 <= num_candidates <= MI_PLACE_MAX_CANDIDATES and n <= MI_PLACE_MAX_KEYFRAMES (MI_E_PARAM); q, n < 1: MI_E_SHAPE.
 * One launch, one workgroup per query. */
MI_API int mi_place_select(const int32_t *votes, int q, int n, const int32_t *excl_lo, const int32_t *excl_hi, int min_votes,
                           int num_candidates, int32_t *cand_index, int32_t *cand_votes, mi_stream_t stream);

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
#endif /* MI355X_MATCH_H */
